"""Inputs and the CPU reference shared by the exact weight-gradient tests
(test_gpu_wgrad_patch.py, test_gpu_wgrad_generic.py). Both sides of a test,
the GPU child process and the comparing parent, rebuild the inputs from the
case id."""

import zlib

import numpy as np
import torch


def pow2(c):
    p = 16
    while p < c:
        p *= 2
    return p


def make_inputs(cid, C, K, H, W, integer, n=2):
    """dy (n,H,W,K), x (n,H,W,C) fp32, exactly representable in bf16."""
    rng = np.random.default_rng(zlib.crc32(cid.encode()))
    if integer:  # asymmetric by construction: iid integers in [-3, 3]
        x = rng.integers(-3, 4, size=(n, H, W, C)).astype(np.float32)
        dy = rng.integers(-3, 4, size=(n, H, W, K)).astype(np.float32)
    else:
        x = rng.random((n, H, W, C), dtype=np.float32)
        dy = rng.standard_normal((n, H, W, K), dtype=np.float32)
    x = torch.from_numpy(x).bfloat16().float().numpy()
    dy = torch.from_numpy(dy).bfloat16().float().numpy()
    return dy, x


def make_dw0(cid, ks, C, K):
    rng = np.random.default_rng(zlib.crc32(cid.encode()) ^ 0x5A5A)
    return rng.integers(-5, 6, size=(K, C, ks, ks)).astype(np.float32)


def reference(dy, x, ks, dtype):
    """dW[k,c,r,s] = sum_m dY[m,k] * X[m shifted by (r-PAD, s-PAD), c]."""
    n, H, W, C = x.shape
    K = dy.shape[3]
    pad = ks // 2
    xp = np.zeros((n, H + 2 * pad, W + 2 * pad, C), dtype=dtype)
    xp[:, pad:pad + H, pad:pad + W] = x
    dyf = dy.reshape(-1, K).astype(dtype)
    dw = np.zeros((K, C, ks, ks), dtype=dtype)
    for r in range(ks):
        for s in range(ks):
            dw[:, :, r, s] = dyf.T @ xp[:, r:r + H, s:s + W].reshape(-1, C)
    return dw
