"""Epoch throughput of train.py on PNG files, with and without
--device-cache, next to the --synthetic rate of the same session.

Writes a UIEB-shaped directory under --workdir (890 PNG pairs in raw-890/
and reference-890/, smooth seeded ~640x480 images so the files are
realistically sized), then runs train.py on it for a few epochs per mode:

  png        DataLoader path: decode + resize + augment per sample per epoch
  png_cache  --device-cache: decode once, gather + augment on the GPU
  synthetic  --synthetic 800: the in-memory path the headline numbers use

Each run is a fresh child process with its own timeout; modes alternate
and the tool stops at the first non-zero exit. The per-epoch
"[fast] epoch train wall ... img/s" lines are parsed, each run's first
epoch (graph capture, worker start-up) is dropped, and every run is
appended to a JSONL file.

    python tools/realdata_epoch_bench.py --workdir /tmp/uieb_like \\
        --repeats 3 --epochs 4 --out profiles/realdata_epoch_bench.jsonl
"""

import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
N_PAIRS = 890
EPOCH_RE = re.compile(r"\[fast\] epoch train wall ([0-9.]+)s = ([0-9]+) img/s")
CACHE_RE = re.compile(
    r"\[cache\] ([0-9]+) pairs ([0-9]+)x([0-9]+), ([0-9.]+) MB, "
    r"built in ([0-9.]+) s")


def _write_pair(job):
    """One smooth raw/ref pair: low-res noise bilinearly upsampled plus a
    little fine noise (natural-image-like, so PNG neither collapses to
    nothing nor stores white noise)."""
    from PIL import Image

    root, i = job
    rng = np.random.default_rng(1_000_003 + i)
    w, h = 640 + 8 * int(rng.integers(-4, 5)), 480 + 8 * int(rng.integers(-4, 5))
    low = rng.integers(0, 256, size=(h // 32 + 1, w // 32 + 1, 3),
                       dtype=np.uint8)
    raw = np.asarray(Image.fromarray(low).resize((w, h), Image.BILINEAR),
                     dtype=np.int16)
    raw = raw + rng.integers(-3, 4, size=raw.shape)
    # the reference is a colour-corrected variant of the raw image
    ref = raw * np.array([1.15, 1.0, 0.9]) + np.array([12, 0, -6])
    for d, arr in (("raw-890", raw), ("reference-890", ref)):
        Image.fromarray(np.clip(arr, 0, 255).astype(np.uint8)).save(
            Path(root) / d / f"{i:04d}.png")
    return i


def make_dataset(root, procs):
    root = Path(root)
    dirs = [root / "raw-890", root / "reference-890"]
    if all(d.is_dir() and len(list(d.glob("*.png"))) == N_PAIRS
           for d in dirs):
        return 0.0
    for d in dirs:
        d.mkdir(parents=True, exist_ok=True)
    t0 = time.time()
    import multiprocessing as mp

    with mp.get_context("spawn").Pool(procs) as pool:
        pool.map(_write_pair, [(str(root), i) for i in range(N_PAIRS)],
                 chunksize=16)
    return time.time() - t0


def run_mode(mode, args, data_root, rundir):
    cmd = [sys.executable, str(REPO / "train.py"),
           "--epochs", str(args.epochs), "--batch-size", str(args.batch_size),
           "--height", str(args.height), "--width", str(args.width),
           "--engine", "fast"]
    if mode == "synthetic":
        cmd += ["--synthetic", "800"]
    else:
        cmd += ["--data-root", str(data_root)]
    if mode == "png_cache":
        cmd += ["--device-cache"]
    if args.num_workers is not None:
        cmd += ["--num-workers", str(args.num_workers)]
    env = dict(os.environ, WATERNET_TRAINING_DIR=str(rundir))
    t0 = time.time()
    res = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True,
                         text=True, timeout=args.timeout)
    wall = time.time() - t0
    rates = [int(m.group(2)) for m in EPOCH_RE.finditer(res.stdout)]
    caches = [{"pairs": int(m.group(1)), "mb": float(m.group(4)),
               "build_s": float(m.group(5))}
              for m in CACHE_RE.finditer(res.stdout)]
    rec = {
        "mode": mode, "returncode": res.returncode,
        "height": args.height, "width": args.width,
        "batch_size": args.batch_size, "epochs": args.epochs,
        "epoch_img_s": rates,
        "steady_img_s": rates[1:],  # first epoch: capture + start-up
        "steady_median_img_s": (statistics.median(rates[1:])
                                if len(rates) > 1 else None),
        "cache_builds": caches, "process_wall_s": round(wall, 2),
    }
    if res.returncode != 0:
        rec["stderr_tail"] = res.stderr[-2000:]
    return rec


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--workdir", required=True)
    p.add_argument("--out", default=str(REPO / "profiles" /
                                        "realdata_epoch_bench.jsonl"))
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--epochs", type=int, default=4)
    p.add_argument("--height", type=int, default=112)
    p.add_argument("--width", type=int, default=112)
    p.add_argument("--batch-size", type=int, default=16)
    p.add_argument("--num-workers", type=int, default=None,
                   help="passed to train.py (its default: 4)")
    p.add_argument("--modes", default="png,png_cache,synthetic")
    p.add_argument("--timeout", type=int, default=600,
                   help="seconds per child process")
    p.add_argument("--gen-procs", type=int, default=8)
    args = p.parse_args(argv)
    if args.epochs < 2:
        p.error("--epochs must be >= 2 (the first epoch is dropped)")

    work = Path(args.workdir)
    data_root = work / "uieb_like"
    gen_s = make_dataset(data_root, args.gen_procs)
    n_bytes = sum(f.stat().st_size for f in data_root.rglob("*.png"))
    print(f"[bench] dataset {data_root}: {N_PAIRS} pairs, "
          f"{n_bytes / 1e6:.0f} MB of PNG, generated in {gen_s:.1f} s",
          flush=True)

    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    modes = [m for m in args.modes.split(",") if m]
    for rep in range(args.repeats):
        for mode in modes:  # alternate modes within each repeat
            rec = run_mode(mode, args, data_root, work / "runs")
            rec["repeat"] = rep
            with open(out, "a") as f:
                f.write(json.dumps(rec) + "\n")
            print(f"[bench] rep {rep} {mode:10s} epochs {rec['epoch_img_s']}"
                  f" img/s, steady median {rec['steady_median_img_s']}, "
                  f"cache {rec['cache_builds']}", flush=True)
            if rec["returncode"] != 0:
                print(rec.get("stderr_tail", ""), file=sys.stderr)
                raise SystemExit(
                    f"{mode} run exited {rec['returncode']}; stopping")


if __name__ == "__main__":
    main()
