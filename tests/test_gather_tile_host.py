"""k_gather_augment_u8's tile index math, run on the host: the kernel's two
phases are plain functions in csrc/gather_augment.h, and
tests/host/gather_tile_check.cpp runs them for every thread of every tile
on canary-fenced buffers, all 16 codes, ten shapes (tails, sub-tile,
non-square, multi-tile). Needs only a C++ compiler, no GPU."""

import shutil
import subprocess
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent


def _cxx():
    for name in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(name)
        if path:
            return path
    raise AssertionError("no C++ compiler found (the extension build "
                         "needs one too)")


def test_gather_tile_phases_on_host(tmp_path):
    exe = tmp_path / "gather_tile_check"
    build = subprocess.run(
        [_cxx(), "-std=c++17", "-O1",
         "-I", str(REPO / "waternet_amd" / "csrc"),
         str(REPO / "tests" / "host" / "gather_tile_check.cpp"),
         "-o", str(exe)],
        capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("OK ")
