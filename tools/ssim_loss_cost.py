"""Step-time cost of the opt-in SSIM loss term (train.py --ssim-weight).

bench.py measures the default step and must not grow options, so this tool
times the same BenchTrainer step with and without the term:

  python tools/ssim_loss_cost.py --pairs 5 --out cost.jsonl
      alternates fresh child processes, ssim_weight 0 / W / 0 / W ..., each
      timing --steps graph-replayed steps after --warmup, and appends every
      run to the JSONL (one line per run, `ms_per_step`).
  python tools/ssim_loss_cost.py --child W [--no-graph]
      one such run in this process (also the command to put behind
      `rocprofv3 --kernel-trace --stats --` for the kernels' own times).
  python tools/ssim_loss_cost.py --calls
      device-event time of the three extension calls at the step's shape,
      back to back: ssim_sum_nhwc (the metric), ssim_fwd_save_nhwc,
      ssim_bwd_nhwc. A call is its kernel plus the allocations and, for the
      two forwards, the partial-sum reduction; it is not a kernel time.
"""

import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
if str(REPO) not in sys.path:
    sys.path.insert(0, str(REPO))


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--child", type=float, default=None, metavar="W",
                   help="time one run at ssim_weight W in this process")
    p.add_argument("--calls", action="store_true")
    p.add_argument("--ssim-weight", type=float, default=50.0)
    p.add_argument("--pairs", type=int, default=5)
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--batch-size", type=int, default=16)
    p.add_argument("--height", type=int, default=112)
    p.add_argument("--width", type=int, default=112)
    p.add_argument("--no-graph", action="store_true")
    p.add_argument("--out", type=str, default=None)
    return p.parse_args()


def run_child(args):
    import torch

    from waternet_amd.engine.fast import BenchTrainer

    if not torch.cuda.is_available():
        raise SystemExit("ssim_loss_cost.py requires a ROCm GPU")
    tr = BenchTrainer(batch_size=args.batch_size, height=args.height,
                      width=args.width, device="cuda:0", seed=1234,
                      use_graph=not args.no_graph, ssim_weight=args.child)
    for _ in range(max(args.warmup, 1)):
        tr.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        tr.step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    m = tr.metrics()
    print(json.dumps({
        "ssim_weight": args.child, "ms_per_step": dt / args.steps * 1e3,
        "steps": args.steps, "warmup": args.warmup,
        "graph": tr._graph is not None, "batch_size": args.batch_size,
        "im_size": f"{args.height}x{args.width}",
        "loss": m["loss"], "ssim": m["ssim"],
    }))


def run_calls(args):
    import torch

    from waternet_amd.ops import ext

    e = ext()
    shape = (args.batch_size, args.height, args.width, 16)
    g = torch.Generator().manual_seed(0)
    a = torch.rand(shape, generator=g).bfloat16().cuda()
    b = torch.rand(shape, generator=g).bfloat16().cuda()
    gs = torch.full((1,), 1e-6, device="cuda")
    _, dmaps = e.ssim_fwd_save_nhwc(a, b, 3, 1.0, 0.01, 0.03)
    calls = {
        "ssim_sum_nhwc": lambda: e.ssim_sum_nhwc(a, b, 3, 1.0, 0.01, 0.03),
        "ssim_fwd_save_nhwc": lambda: e.ssim_fwd_save_nhwc(a, b, 3, 1.0,
                                                            0.01, 0.03),
        "ssim_bwd_nhwc": lambda: e.ssim_bwd_nhwc(a, b, dmaps, gs, 3),
    }
    n = 500
    out = {"shape": list(shape), "clog": 3, "calls_per_timing": n}
    for name, fn in calls.items():
        for _ in range(20):
            fn()
        reps = []
        for _ in range(5):
            start = torch.cuda.Event(enable_timing=True)
            stop = torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(n):
                fn()
            stop.record()
            torch.cuda.synchronize()
            reps.append(start.elapsed_time(stop) / n * 1e3)
        out[name + "_us_per_call"] = reps
    print(json.dumps(out))


def main():
    args = parse_args()
    if args.child is not None:
        run_child(args)
        return
    if args.calls:
        run_calls(args)
        return
    runs = {0.0: [], args.ssim_weight: []}
    for _ in range(args.pairs):
        for w in runs:
            cmd = [sys.executable, str(Path(__file__).resolve()), "--child",
                   str(w), "--steps", str(args.steps), "--warmup",
                   str(args.warmup), "--batch-size", str(args.batch_size),
                   "--height", str(args.height), "--width", str(args.width)]
            if args.no_graph:
                cmd.append("--no-graph")
            res = subprocess.run(cmd, capture_output=True, text=True,
                                 timeout=600)
            if res.returncode != 0:
                # a failed run ends the measurement: nothing more is started
                raise SystemExit(f"child failed ({res.returncode}):\n"
                                 f"{res.stderr[-2000:]}")
            line = res.stdout.strip().splitlines()[-1]
            rec = json.loads(line)
            runs[w].append(rec["ms_per_step"])
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
    med = {w: statistics.median(v) for w, v in runs.items()}
    summary = {
        "summary": True,
        "median_ms_per_step": {str(w): m for w, m in med.items()},
        "spread_ms": {str(w): max(v) - min(v) for w, v in runs.items()},
        "added_us_per_step": (med[args.ssim_weight] - med[0.0]) * 1e3,
    }
    print(json.dumps(summary))
    if args.out:
        with open(args.out, "a") as f:
            f.write(json.dumps(summary) + "\n")


if __name__ == "__main__":
    main()
