"""Cost of temporally smoothed statistics on the 1080p video engine: fps of
the plain engine and of one with temporal_alpha set, measured in the same
process in alternating runs (as tools/infer_stability.py measures the plain
engine alone), so clock drift hits both alike. Prints one JSON line;
--out also writes it to a file."""

import argparse
import json
import pathlib
import sys
import time

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

import numpy as np
import torch

from waternet_amd.engine.inferencer import InferenceEngine
from waternet_amd.models.waternet import WaterNet

H, W = 1088, 1920


def timed(eng, frames, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        eng.infer_frame(frames[i % len(frames)])
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--alpha", type=float, default=0.3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    torch.manual_seed(0)
    model = WaterNet().to("cuda:0")
    engines = {
        "plain": InferenceEngine(model, H, W, device="cuda:0"),
        "temporal": InferenceEngine(model, H, W, device="cuda:0",
                                    temporal_alpha=args.alpha),
    }
    rng = np.random.default_rng(0)
    frames = [rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
              for _ in range(4)]
    for eng in engines.values():
        timed(eng, frames, 10)  # capture + warm-up
    fps = {k: [] for k in engines}
    for r in range(args.runs):
        for k, eng in engines.items():
            fps[k].append(timed(eng, frames, args.frames))
            print(f"run {r} {k}: {fps[k][-1]:.2f} fps", flush=True)

    def p50(v):
        return sorted(v)[len(v) // 2]

    result = {
        "shape": f"{H}x{W}", "frames_per_run": args.frames,
        "alpha": args.alpha, "fps": fps,
        "graph": {k: e._graph is not None for k, e in engines.items()},
        "fps_p50_plain": p50(fps["plain"]),
        "fps_p50_temporal": p50(fps["temporal"]),
        "spread_pct_plain": 100.0 * (max(fps["plain"]) - min(fps["plain"]))
        / max(fps["plain"]),
        "slowdown_pct": 100.0 * (1.0 - p50(fps["temporal"])
                                 / p50(fps["plain"])),
        "counters": engines["temporal"].temporal_counters(),
    }
    line = json.dumps(result)
    print(line)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
