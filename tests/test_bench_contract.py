"""Driver-contract guards: bench.py's flags and its recorded JSON line
must keep the exact schema the driver parses (BASELINE metric/config)."""

import json
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent

REQUIRED_KEYS = {
    "metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
    "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
}


def test_bench_args_defaults():
    import sys

    import bench

    argv = sys.argv
    sys.argv = ["bench.py"]  # no flags: driver default invocation
    try:
        a = bench.parse_args()
    finally:
        sys.argv = argv
    assert a.gpus == 1 and a.steps == 30 and a.warmup == 10
    assert a.batch_size == 16 and a.height == 112 and a.width == 112
    assert a.mode == "train"


def _parse(argv):
    import sys

    import bench

    saved = sys.argv
    sys.argv = ["bench.py", *argv]
    try:
        return bench.parse_args()
    finally:
        sys.argv = saved


def test_bench_full_and_dump_flags():
    """A plain run neither dumps nor runs extras; both are opt-in."""
    a = _parse([])
    assert a.full is False and a.dump_outputs is None
    a = _parse(["--full", "--dump-outputs", "some/dir", "--steps", "7"])
    assert a.full is True and a.dump_outputs == "some/dir" and a.steps == 7


def test_dump_outputs_writes_float_npy(tmp_path):
    """dump_outputs stores every array as float32, keeping float64."""
    import numpy as np
    import torch

    import bench

    out = tmp_path / "nested" / "dump"
    bench.dump_outputs(str(out), {
        "u8": np.arange(6, dtype=np.uint8).reshape(2, 3),
        "bf16": torch.tensor([1.5, -2.0], dtype=torch.bfloat16),
        "f64": torch.tensor([0.1], dtype=torch.float64),
    })
    assert sorted(p.name for p in out.iterdir()) == [
        "bf16.npy", "f64.npy", "u8.npy"]
    u8, bf, f64 = (np.load(out / f"{n}.npy") for n in ("u8", "bf16", "f64"))
    assert u8.dtype == np.float32 and u8.shape == (2, 3)
    assert np.array_equal(u8.ravel(), np.arange(6))
    assert bf.dtype == np.float32 and bf.tolist() == [1.5, -2.0]
    assert f64.dtype == np.float64 and f64[0] == 0.1


@pytest.mark.gpu
def test_bench_dump_outputs_gpu(tmp_path, monkeypatch, capsys):
    """Two tiny runs with the same arguments: --steps sets the timed-step
    count, the result line carries ms_per_step, --dump-outputs leaves the
    last step's params/grads/metric sums as finite float arrays within
    64 MB, and the two dumps agree to rounding.

    Bound: the last timed step starts from the same state and batch in
    both runs, so the only difference is the order of the fp32 atomic
    accumulations (relative 6e-8 per add) and, through it, a bf16 rounding
    (2^-8) flipping in isolated activations; one flipped element among the
    >1e5 feeding a reduction moves it by <4e-3/sqrt(1e5) ~ 1e-5. 1e-4
    relative L2 leaves room for several and is far below what a changed
    kernel or a drifting state (>1e-3 after 25 steps) produces."""
    import sys

    import numpy as np

    import bench

    dumps = []
    for run in ("a", "b"):
        out = tmp_path / run
        monkeypatch.setattr(sys, "argv", [
            "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1",
            "--batch-size", "2", "--height", "64", "--width", "64",
            "--dump-outputs", str(out)])
        bench.main()
        rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert REQUIRED_KEYS <= set(rec.keys())
        assert rec["steps"] == 3 and rec["ms_per_step"] > 0
        assert abs(rec["value"] * rec["ms_per_step"] / 1000.0 - 2) < 1e-6

        params = np.load(out / "params.npy")
        grads = np.load(out / "grads.npy")
        sums = np.load(out / "metric_sums.npy")
        assert params.dtype == np.float32 and grads.dtype == np.float32
        assert params.shape == grads.shape and params.ndim == 1
        assert sums.dtype == np.float64 and sums.shape == (5,)
        assert np.isfinite(params).all() and np.isfinite(grads).all()
        assert np.isfinite(sums).all() and np.abs(grads).max() > 0
        total = sum(p.stat().st_size for p in out.iterdir())
        assert total <= 64 * 1024 * 1024
        dumps.append((params, grads, sums))

    for name, x, y in zip(("params", "grads", "metric_sums"), *dumps):
        x, y = x.astype(np.float64), y.astype(np.float64)
        rel = np.linalg.norm(x - y) / np.linalg.norm(x)
        print(f"{name}: run-to-run relative L2 {rel:.3e}")
        assert rel < 1e-4, (name, rel)


def test_recorded_bench_line_schema():
    rec = json.loads((REPO / "profiles" / "r02_bench_final.json").read_text())
    assert REQUIRED_KEYS <= set(rec.keys()), REQUIRED_KEYS - set(rec.keys())
    assert rec["metric"].startswith("train images/sec")
    assert rec["higher_is_better"] is True
    assert rec["scaling"] == "weak"
    assert rec["dtype"] == "bf16"
    assert rec["data"] == "synthetic"
    assert rec["config"]["model"] == "waternet"
    assert rec["config"]["im_size"] == "112x112"
    assert rec["config"]["global_batch"] == rec["n_gpus"] * 16
    assert abs(rec["vs_baseline"] - rec["value"] / 12.8) < 1e-6
    # whole-job aggregate sanity: value == total images / elapsed
    assert abs(rec["value"] * rec["ms_per_step"] / 1000.0
               - rec["n_gpus"] * 16) < 1e-6


def test_bench_requires_gpu_clear_exit():
    """On a CPU-only box bench.py exits with a clear message (the driver
    only runs it on GPU boxes; anything else must not half-run)."""
    import os
    import subprocess
    import sys

    # hide every GPU from the child so this holds on a GPU box too
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1",
               CUDA_VISIBLE_DEVICES="-1")
    out = subprocess.run(
        [sys.executable, str(REPO / "bench.py"), "--steps", "1"],
        capture_output=True, text=True, timeout=600, env=env,
    )
    assert out.returncode != 0
    assert "requires a ROCm GPU" in out.stderr
