"""k_wgrad_smallk (K <= 4 weight gradient, U rows in flight per thread with
a branch-free masked tail) against an fp32 unfold-matmul reference, bitwise
on integer data.

Integers in [-3, 3]: every partial sum is an integer below
9 * N*H*W <= 4608 < 2^24, so fp32 accumulation is exact in any order.
(N,H,W) = (1,1,3) and (2,5,19) give M = 3 and 190 rows — fewer than the
unroll times the m-rows a block covers, so the masked tail does the work;
(2,16,16) runs full iterations too.
"""

import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KOUT = [1, 3, 4]
CPS = [16, 32, 64]
KSS = [1, 3, 5]
NHW = [(1, 1, 3), (2, 5, 19), (2, 16, 16)]


@pytest.fixture(scope="module")
def ext():
    from waternet_amd.ops import ext as _ext

    return _ext()


def make_inputs(cid, n, h, w, C, K):
    rng = np.random.default_rng(zlib.crc32(cid.encode()))
    x = rng.integers(-3, 4, size=(n, h, w, C)).astype(np.float32)
    dy = rng.integers(-3, 4, size=(n, h, w, K)).astype(np.float32)
    return dy, x


def reference(dy, x, ks):
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


def run(ext, dy, x, ks, Cp, dw0=None):
    n, h, w, C = x.shape
    K = dy.shape[3]
    xg = torch.zeros(n, h, w, Cp, dtype=torch.bfloat16, device="cuda")
    xg[..., :C] = torch.from_numpy(x).cuda().bfloat16()
    dyg = torch.zeros(n, h, w, 16, dtype=torch.bfloat16, device="cuda")
    dyg[..., :K] = torch.from_numpy(dy).cuda().bfloat16()
    if dw0 is None:
        dw = torch.zeros(K, C, ks, ks, dtype=torch.float32, device="cuda")
    else:
        dw = torch.from_numpy(dw0).cuda().contiguous()
    ext.conv2d_wgrad(dyg, xg, dw, ks)
    torch.cuda.synchronize()
    return dw.cpu().numpy()


@pytest.mark.parametrize("n,h,w", NHW)
@pytest.mark.parametrize("ks", KSS)
@pytest.mark.parametrize("Cp", CPS)
@pytest.mark.parametrize("K", KOUT)
def test_exact_integer(ext, K, Cp, ks, n, h, w):
    # C = Cp - 1: the last channel octet is partly pad, all others are live
    C = Cp - 1
    cid = f"smallk-k{K}-cp{Cp}-ks{ks}-{n}x{h}x{w}"
    dy, x = make_inputs(cid, n, h, w, C, K)
    want = reference(dy, x, ks)
    have = run(ext, dy, x, ks, Cp)
    bad = np.argwhere(have != want)
    assert bad.size == 0, (
        f"{len(bad)} of {want.size} differ; first (k,c,r,s)={bad[0]} "
        f"got {have[tuple(bad[0])]} want {want[tuple(bad[0])]}")


def test_accumulates_into_dw(ext):
    K, Cp, ks, (n, h, w) = 3, 32, 3, (2, 5, 19)
    cid = "smallk-acc"
    dy, x = make_inputs(cid, n, h, w, Cp, K)
    rng = np.random.default_rng(7)
    dw0 = rng.integers(-5, 6, size=(K, Cp, ks, ks)).astype(np.float32)
    have = run(ext, dy, x, ks, Cp, dw0.copy())
    assert np.array_equal(have, dw0 + reference(dy, x, ks))
