"""Per-shape wgrad kernel timing, A/B between k_conv_wgrad
(WN_WGRAD_PATCH=0) and k_conv_wgrad_patch (WN_WGRAD_PATCH=1). The switch is
read once per process, so each side runs in a fresh child process; the
parent prints both per shape, with the bytes each launch stages through LDS
(computed from the shapes, zero-buffer pad slots included) and the
resulting global->LDS rate next to TF/s.

    python tools/wgrad_bench.py            # A/B, shapes at bs=16 112^2
    WG_N=16 WG_HW=256 python tools/wgrad_bench.py
    WN_WGRAD_PATCH=1 python tools/wgrad_bench.py --child   # one side only

Shapes = the WaterNet training layers that reach the MFMA wgrad kernels.
"""

import json
import os
import subprocess
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

SHAPES = [  # (ks, C, K, label)
    (7, 12, 128, "cmg.conv1"),
    (5, 128, 128, "cmg.conv2"),
    (3, 128, 128, "cmg.conv3"),
    (1, 128, 64, "cmg.conv4"),
    (7, 64, 64, "cmg.conv5"),
    (5, 64, 64, "cmg.conv6"),
    (3, 64, 64, "cmg.conv7"),
    (7, 6, 32, "refiner.conv1(x3)"),
    (5, 32, 32, "refiner.conv2(x3)"),
    # K <= 4: k_wgrad_smallk on both sides (WN_WGRAD_PATCH does not apply)
    (3, 64, 3, "cmg.conv8"),
    (3, 32, 3, "refiner.conv3(x3)"),
    # instantiated patch-kernel classes no WaterNet layer uses (not in TOTAL)
    (7, 128, 128, "extra k7 128"),
    (5, 64, 128, "extra k5 64-128"),
    (3, 32, 32, "extra k3 32"),
    (7, 32, 32, "extra k7 32"),
    (5, 12, 64, "extra k5 16-64"),
    (3, 12, 128, "extra k3 16-128"),
]


def pow2(c):
    p = 16
    while p < c:
        p *= 2
    return p


def patch_class(ks, Cp, Kp):
    """Channel class k_conv_wgrad_patch is instantiated for (0 = none);
    mirrors conv2d_wgrad in csrc/conv_wgrad.hip."""
    if ks < 3:
        return 0
    if Cp % 64 == 0 and Kp % 64 == 0:
        return 64
    if Cp == 32 and Kp == 32:
        return 32
    if Cp == 16 and (Kp == 32 or Kp % 64 == 0):
        return 16  # k_conv_wgrad_patch16 (tap pairs)
    return 0


def patch_chunk(cls, W):
    if cls not in (64, 16):
        return 64
    forced = int(os.environ.get("WN_WGRAD_PATCH_CH", "0"))
    if forced in (64, 112):
        return forced
    pad64, pad112 = -(-W // 64) * 64, -(-W // 112) * 112
    return 112 if pad112 < pad64 else 64


def staged_bytes(ks, Cp, Kp, N, H, W, patch):
    """Bytes one launch moves global->LDS (every glds slot, pads included)."""
    cls = patch_class(ks, Cp, Kp) if patch else 0
    if Kp == 16:  # k_wgrad_smallk reads global memory directly
        return 0
    if cls == 0:  # k_conv_wgrad: 64-row chunks, BK x 128 tiles
        BK = min(Kp, 128)
        cpk = (64 // 4 * 72 + 16) // 8
        sa = -(-(BK // 16) * cpk // 256)
        sb = -(-8 * cpk // 256)
        gx, gy = -(-Kp // BK), -(-ks * ks * Cp // 128)
        chunks = -(-N * H * W // 64)
        return chunks * (sa + sb) * 4096 * gx * gy
    CH = patch_chunk(cls, W)
    nseg = -(-W // CH)
    pad = ks // 2
    rows = sum(N * max(0, H - abs(d - pad)) for d in range(ks))
    if cls == 16:  # Patch16Geo: BK 32/64, images padded to whole k-steps
        BK = 32 if Kp == 32 else 64
        pxa = -(-CH // 16 // (128 // BK)) * (128 // BK) * 16
        sa = -(-pxa * (BK // 8) // 256)
        sb = -(-(pxa + ks) * 2 // 256)
        return rows * nseg * (sa + sb) * 4096 * (Kp // BK)
    sa = -(-CH * (cls // 8) // 256)
    sb = -(-(CH + ks - 1) * (cls // 8) // 256)
    return rows * nseg * (sa + sb) * 4096 * (Kp // cls) * (Cp // cls)


def child():
    import torch

    from waternet_amd.ops import ext

    e = ext()
    N = int(os.environ.get("WG_N", "16"))
    H = W = int(os.environ.get("WG_HW", "112"))
    torch.manual_seed(0)
    for ks, C, K, label in SHAPES:
        Cp, Kp = pow2(C), pow2(K)
        dy = torch.randn(N, H, W, Kp, device="cuda",
                         dtype=torch.bfloat16).contiguous()
        x = torch.randn(N, H, W, Cp, device="cuda",
                        dtype=torch.bfloat16).contiguous()
        dw = torch.zeros(K, C, ks, ks, device="cuda", dtype=torch.float32)
        for _ in range(3):
            e.conv2d_wgrad(dy, x, dw, ks)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        iters = 20
        for _ in range(iters):
            e.conv2d_wgrad(dy, x, dw, ks)
        torch.cuda.synchronize()
        us = (time.perf_counter() - t0) / iters * 1e6
        print(json.dumps({"label": label, "us": us}), flush=True)


def main():
    N = int(os.environ.get("WG_N", "16"))
    H = W = int(os.environ.get("WG_HW", "112"))
    us = {}
    for patch in (0, 1):
        env = dict(os.environ, WN_WGRAD_PATCH=str(patch))
        out = subprocess.run([sys.executable, __file__, "--child"], env=env,
                             check=True, capture_output=True, text=True)
        us[patch] = {r["label"]: r["us"] for r in
                     map(json.loads, out.stdout.strip().splitlines())}
    print(f"N={N} HW={H}  old = WN_WGRAD_PATCH=0, new = WN_WGRAD_PATCH=1 "
          f"(old kernel where the patch kernel has no instance)")
    print(f"  {'layer':18s} {'shape':>14s} | {'old us':>8s} {'TF/s':>6s} "
          f"{'MB':>6s} {'TB/s':>5s} | {'new us':>8s} {'TF/s':>6s} "
          f"{'MB':>6s} {'TB/s':>5s} | new/old")
    tot = {0: 0.0, 1: 0.0}
    for ks, C, K, label in SHAPES:
        Cp, Kp = pow2(C), pow2(K)
        flops = 2.0 * N * H * W * K * C * ks * ks
        mult = 3 if "x3" in label else 0 if "extra" in label else 1
        row = f"  {label:18s} {f'k{ks} {C}->{K}':>14s} |"
        for patch in (0, 1):
            t = us[patch][label]
            b = staged_bytes(ks, Cp, Kp, N, H, W, patch)
            tot[patch] += t * mult
            row += (f" {t:8.1f} {flops / t / 1e6:6.1f} {b / 1e6:6.0f} "
                    f"{b / t / 1e6:5.2f} |")
        row += f" {us[1][label] / us[0][label]:5.2f}"
        print(row)
    print(f"  TOTAL per step (x3 refiners counted): old {tot[0]:.0f} us, "
          f"new {tot[1]:.0f} us")


if __name__ == "__main__":
    if "--child" in sys.argv:
        child()
    else:
        main()
