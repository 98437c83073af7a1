"""Per-shape A/B of conv2d_fwd (bias + ReLU) on the deep k3 VGG layers: the
tile-resident tier (k_conv_tile) against the tier each shape ran on before.

WN_CONV_TILE and its companions are read once per process, so every timing
comes from a fresh child. The driver alternates the configurations REPS
times and writes one JSON line per child:
  {"config", "rep", "env", "rows": [{"shape", "plan", "us": [...]}, ...]}
"us" are the means of WINDOWS timed windows of ITERS back-to-back calls each
(device events), after WARMUP calls.

Run (GPU box):  python tools/conv_tile_ab.py out.jsonl [config ...]
"""

import json
import os
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent

CONFIGS = {
    "off": {"WN_CONV_TILE": "0"},
    "tile128": {"WN_CONV_TILE": "1", "WN_CONV_TILE_CC": "128"},
    "tile64": {"WN_CONV_TILE": "1", "WN_CONV_TILE_CC": "64"},
    "default": {},
}
KNOBS = ("WN_CONV_TILE", "WN_CONV_TILE_CC")

# (N, H=W, cin, cout): bs 16 at 112^2 (56, 28, 14, 7) and at 256^2 (128, 64,
# 32, 16: no multiples of 14, so those rows stay on their tier)
SHAPES = [(16, 56, 128, 128),
          (16, 28, 128, 256), (16, 28, 256, 128), (16, 28, 256, 256),
          (16, 14, 256, 512), (16, 14, 512, 256), (16, 14, 512, 512),
          (16, 7, 512, 512),
          (16, 128, 128, 128), (16, 64, 256, 256), (16, 32, 512, 512),
          (16, 16, 512, 512)]
REPS, WARMUP, ITERS, WINDOWS = 3, 20, 100, 3


def child():
    sys.path.insert(0, str(REPO))
    import torch

    from waternet_amd.ops import ext as _ext

    ext = _ext()
    rows = []
    for n, hw, cin, cout in SHAPES:
        torch.manual_seed(0)
        x = torch.randn(n, hw, hw, cin, device="cuda").bfloat16()
        w = torch.randn(cout, cin, 3, 3, device="cuda") / (9 * cin) ** 0.5
        b = torch.randn(cout, device="cuda")
        wp = ext.pack_weight_fwd(w.contiguous(), cout, cin)
        run = lambda: ext.conv2d_fwd(x, wp, b, 3, cout, cout, 1)
        for _ in range(WARMUP):
            run()
        us = []
        for _ in range(WINDOWS):
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(ITERS):
                run()
            e1.record()
            torch.cuda.synchronize()
            us.append(round(e0.elapsed_time(e1) * 1e3 / ITERS, 2))
        plan = list(ext.conv2d_fwd_plan(n, hw, hw, cin, cout, 3))
        rows.append({"shape": f"{n}x{hw}x{hw} {cin}->{cout}", "plan": plan,
                     "us": us})
    print("ROWS " + json.dumps(rows))


def main():
    out = Path(sys.argv[1])
    configs = sys.argv[2:] or list(CONFIGS)
    base = {k: v for k, v in os.environ.items() if k not in KNOBS}
    with open(out, "a") as f:
        for rep in range(REPS):
            for cfg in configs:
                r = subprocess.run(
                    [sys.executable, str(Path(__file__).resolve()), "--child"],
                    env={**base, **CONFIGS[cfg]}, cwd=REPO,
                    capture_output=True, text=True, timeout=300)
                if r.returncode != 0:
                    sys.exit(f"{cfg} rep {rep}: exit {r.returncode}\n"
                             + r.stderr[-3000:])
                line = [l for l in r.stdout.splitlines()
                        if l.startswith("ROWS ")][-1]
                rec = {"config": cfg, "rep": rep, "env": CONFIGS[cfg],
                       "rows": json.loads(line[5:])}
                f.write(json.dumps(rec) + "\n")
                f.flush()
                print(cfg, rep, [(r_["shape"], r_["plan"][0], min(r_["us"]))
                                 for r_ in rec["rows"]], flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child()
    else:
        main()
