"""k_conv_wgrad_patch16 (Cp = 16: two dx taps per MFMA, phantom tap dropped)
against an fp32 unfold-matmul reference, bitwise on integer data.

Laid out like test_gpu_wgrad_patch.py: WN_WGRAD_PATCH is read once per
process, so one child process (this file executed as a script) runs every
case with WN_WGRAD_PATCH=1 and writes one .npz; the tests only compare.
Inputs are rebuilt from the case id on both sides.

Integers in [-3, 3]: every partial sum is an integer below
9 * N*H*W <= 10350 < 2^24, so fp32 accumulation is exact in any order and dW
must equal the fp32 reference bitwise.
"""

import os
import subprocess
import sys
import zlib
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
N = 2
H = 5   # k7's dy halo leaves the image on both sides
# C = 16 leaves no zero pad channel: a wrong half -> tap mapping cannot hide
CS = [3, 12, 16]
# Kp = 16 (no patch16 instance: k_conv_wgrad), 32 (BK 32), 64 / 128 (BK 64)
KS_OUT = [5, 32, 64, 128]
KSS = [3, 5, 7]
# (W, forced chunk length or 0): 16 = one exact k-step; 19 = tail k-step;
# 67 / 115 = CH + 3 for both chunk lengths (two segments per row; the halo
# and the phantom-tap pixel cross the seam)
WS = [(16, 0), (19, 0), (67, 64), (115, 112)]
# split-m block count forced for these widths: every block owns <= 1 chunk
MANY_BLOCKS = {19: 100000, 115: 100000}
ACC = [(3, 12, 128, 19, 0), (5, 3, 32, 19, 0), (7, 16, 64, 19, 0),
       (7, 12, 128, 115, 112), (7, 3, 32, 67, 64)]
# X non-zero in the last image column only
LASTCOL = [(3, 16, 32, 16), (5, 16, 64, 19), (7, 16, 32, 16),
           (7, 16, 128, 19)]


def pow2(c):
    p = 16
    while p < c:
        p *= 2
    return p


def int_id(ks, C, K, W, ch):
    return f"int-k{ks}-c{C}-k{K}-w{W}-ch{ch}"


def acc_id(ks, C, K, W, ch):
    return f"acc-k{ks}-c{C}-k{K}-w{W}-ch{ch}"


def last_id(ks, C, K, W):
    return f"last-k{ks}-c{C}-k{K}-w{W}"


def make_inputs(cid, C, K, W, lastcol=False):
    """dy (N,H,W,K), x (N,H,W,C) fp32 integers in [-3, 3]."""
    rng = np.random.default_rng(zlib.crc32(cid.encode()))
    x = rng.integers(-3, 4, size=(N, H, W, C)).astype(np.float32)
    dy = rng.integers(-3, 4, size=(N, H, W, K)).astype(np.float32)
    if lastcol:
        x[:, :, :-1] = 0
        x[:, :, -1] = np.where(x[:, :, -1] == 0, 2, x[:, :, -1])
    return dy, x


def make_dw0(cid, ks, C, K):
    rng = np.random.default_rng(zlib.crc32(cid.encode()) ^ 0x5A5A)
    return rng.integers(-5, 6, size=(K, C, ks, ks)).astype(np.float32)


def reference(dy, x, ks):
    """dW[k,c,r,s] = sum_m dY[m,k] * X[m shifted by (r-PAD, s-PAD), c]."""
    n, h, w, C = x.shape
    K = dy.shape[3]
    pad = ks // 2
    xp = np.zeros((n, h + 2 * pad, w + 2 * pad, C), dtype=np.float32)
    xp[:, pad:pad + h, pad:pad + w] = x
    dyf = dy.reshape(-1, K)
    dw = np.zeros((K, C, ks, ks), dtype=np.float32)
    for r in range(ks):
        for s in range(ks):
            dw[:, :, r, s] = dyf.T @ xp[:, r:r + h, s:s + w].reshape(-1, C)
    return dw


# ---------------------------------------------------------------------------
# child process: run every case on the GPU, save the results
# ---------------------------------------------------------------------------

def _run_case(ext, dy, x, ks, C, K, ch, dw0=None):
    Cp, Kp = pow2(C), pow2(K)
    n, h, w, _ = x.shape
    xg = torch.zeros(n, h, w, Cp, dtype=torch.bfloat16, device="cuda")
    xg[..., :C] = torch.from_numpy(x).cuda().bfloat16()
    dyg = torch.zeros(n, h, w, Kp, dtype=torch.bfloat16, device="cuda")
    dyg[..., :K] = torch.from_numpy(dy).cuda().bfloat16()
    if dw0 is None:
        dw = torch.zeros(K, C, ks, ks, dtype=torch.float32, device="cuda")
    else:
        dw = torch.from_numpy(dw0).cuda().contiguous()
    # both knobs are read per call by conv2d_wgrad
    for var, val in (("WN_WGRAD_PATCH_CH", ch),
                     ("WN_WGRAD_PATCH_BLOCKS", MANY_BLOCKS.get(w, 0))):
        if val:
            os.environ[var] = str(val)
        else:
            os.environ.pop(var, None)
    ext.conv2d_wgrad(dyg, xg, dw, ks)
    torch.cuda.synchronize()
    return dw.cpu().numpy()


def _child(out_path):
    sys.path.insert(0, str(REPO))
    from waternet_amd.ops import ext as _ext

    ext = _ext()
    res = {}
    for ks in KSS:
        for C in CS:
            for K in KS_OUT:
                for W, ch in WS:
                    cid = int_id(ks, C, K, W, ch)
                    dy, x = make_inputs(cid, C, K, W)
                    res[cid] = _run_case(ext, dy, x, ks, C, K, ch)
    for ks, C, K, W, ch in ACC:
        cid = acc_id(ks, C, K, W, ch)
        dy, x = make_inputs(cid, C, K, W)
        res[cid] = _run_case(ext, dy, x, ks, C, K, ch,
                             make_dw0(cid, ks, C, K))
    for ks, C, K, W in LASTCOL:
        cid = last_id(ks, C, K, W)
        dy, x = make_inputs(cid, C, K, W, lastcol=True)
        res[cid] = _run_case(ext, dy, x, ks, C, K, 0)
    np.savez(out_path, **res)


if __name__ == "__main__":
    _child(sys.argv[1])
    sys.exit(0)


# ---------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def got(tmp_path_factory):
    out = tmp_path_factory.mktemp("wgc16") / "wgrad_c16.npz"
    env = dict(os.environ, WN_WGRAD_PATCH="1")
    env.pop("WN_WGRAD_PATCH_CH", None)
    env.pop("WN_WGRAD_PATCH_BLOCKS", None)
    r = subprocess.run(
        [sys.executable, str(Path(__file__).resolve()), str(out)],
        env=env, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return dict(np.load(out))


def _assert_same(have, want):
    bad = np.argwhere(have != want)
    assert bad.size == 0, (
        f"{len(bad)} of {want.size} differ; first (k,c,r,s)={bad[0]} "
        f"got {have[tuple(bad[0])]} want {want[tuple(bad[0])]}")


@pytest.mark.parametrize("W,ch", WS)
@pytest.mark.parametrize("K", KS_OUT)
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("ks", KSS)
def test_exact_integer(got, ks, C, K, W, ch):
    cid = int_id(ks, C, K, W, ch)
    dy, x = make_inputs(cid, C, K, W)
    _assert_same(got[cid], reference(dy, x, ks))


@pytest.mark.parametrize("ks,C,K,W,ch", ACC)
def test_accumulates_into_dw(got, ks, C, K, W, ch):
    """A pre-filled dW comes back as dW0 + grad."""
    cid = acc_id(ks, C, K, W, ch)
    dy, x = make_inputs(cid, C, K, W)
    _assert_same(got[cid], make_dw0(cid, ks, C, K) + reference(dy, x, ks))


@pytest.mark.parametrize("ks,C,K,W", LASTCOL)
def test_last_column_only(got, ks, C, K, W):
    """X is non-zero only in the last image column, and non-zero everywhere
    there: the phantom tap dx = KS reads that column for the output pixels
    left of it and must not leak into tap KS-1 (or anywhere)."""
    cid = last_id(ks, C, K, W)
    dy, x = make_inputs(cid, C, K, W, lastcol=True)
    assert (x[:, :, -1] != 0).all() and not x[:, :, :-1].any()
    _assert_same(got[cid], reference(dy, x, ks))
