"""Shared reference of the SSIM-loss tests (test_gpu_ssim_loss.py,
test_ssim_loss_cpu.py): seeded cases, the float64 autograd gradient of
`_ssim_torch`, and the closed-form gradient the HIP kernels implement,
evaluated in any torch dtype on the CPU.

Closed form, per window q with gaussian-weighted sums sx, sy, sxx, syy, sxy:
    A1 = 2 sx sy + c1          A2 = 2 (sxy - sx sy) + c2
    B1 = sx^2 + sy^2 + c1      B2 = (sxx - sx^2) + (syy - sy^2) + c2
    S  = A1 A2 / (B1 B2)
    D1 = dS/dsx  = 2 sy (A2 - A1)/(B1 B2) - 2 sx S (1/B1 - 1/B2)
    D2 = dS/dsxx = -S / B2
    D3 = dS/dsxy = 2 A1 / (B1 B2)
and per pixel p, with T(.) the transposed (full) window correlation,
    dx(p) = g/count * [T(D1) + 2 x T(D2) + y T(D3)](p).
"""

import functools
import zlib

import torch
import torch.nn.functional as F

from waternet_amd.utils.metrics import _gaussian_kernel2d, _ssim_torch

DATA_RANGE, K1, K2 = 1.0, 0.01, 0.03

# (N, H, W, Cp, Clog): one window; ragged window tiles (OH 17, OW 33) and
# ragged pixel tiles (27x43); one channel, W = one LDS patch; Clog == Cp
SHAPES = [(1, 11, 11, 16, 3), (2, 27, 43, 16, 3), (1, 16, 26, 16, 1),
          (2, 12, 37, 4, 4)]
KINDS = ["random", "flat"]
UPSTREAM = [1.0, -0.37]


@functools.lru_cache(maxsize=None)
def images(shape, kind):
    """Two related (N,Clog,H,W) fp32 images in [0,1], exact in bf16. `flat`
    is the near-constant pair 0.5 + 0.01 * rand, where sxx - sx^2 cancels."""
    n, h, w, _, clog = shape
    g = torch.Generator()
    g.manual_seed(zlib.crc32(repr(("ssim_loss", shape, kind)).encode()))
    if kind == "flat":
        a = 0.5 + 0.01 * torch.rand(n, clog, h, w, generator=g)
        b = 0.5 + 0.01 * torch.rand(n, clog, h, w, generator=g)
    else:
        a = torch.rand(n, clog, h, w, generator=g)
        b = (a * 0.7 + 0.3 * torch.rand(n, clog, h, w, generator=g))
        b = b.clamp(0, 1)
    return a.bfloat16().float(), b.bfloat16().float()


def to_nhwc(x, cp, seed):
    """(N,C,H,W) fp32 -> (N,H,W,Cp) bf16 with non-zero garbage in the pad
    channels, so a kernel that reads or copies them is caught."""
    n, c, h, w = x.shape
    g = torch.Generator()
    g.manual_seed(seed)
    full = (torch.rand(n, h, w, cp, generator=g) + 1).bfloat16()
    full[..., :c] = x.permute(0, 2, 3, 1).bfloat16()
    return full


@functools.lru_cache(maxsize=None)
def autograd_f64(shape, kind):
    """(mean SSIM, d mean SSIM / da) in float64 by torch autograd."""
    a, b = images(shape, kind)
    a64 = a.double().requires_grad_(True)
    s = _ssim_torch(a64, b.double(), DATA_RANGE, 11, 1.5, K1, K2)
    (grad,) = torch.autograd.grad(s, a64)
    return s.detach(), grad


def formula_grad(a, b, dtype):
    """d mean SSIM / da by the closed form above, all arithmetic in
    `dtype`."""
    a, b = a.to(dtype), b.to(dtype)
    n, c, h, w = a.shape
    kern = _gaussian_kernel2d(11, 1.5, a.device, dtype)
    kern = kern.expand(c, 1, 11, 11).contiguous()

    def filt(x):
        return F.conv2d(x, kern, groups=c)

    def filt_t(x):
        return F.conv_transpose2d(x, kern, groups=c)

    sx, sy = filt(a), filt(b)
    sxx, syy, sxy = filt(a * a), filt(b * b), filt(a * b)
    c1, c2 = (K1 * DATA_RANGE) ** 2, (K2 * DATA_RANGE) ** 2
    a1 = 2 * sx * sy + c1
    a2 = 2 * (sxy - sx * sy) + c2
    b1 = sx * sx + sy * sy + c1
    b2 = (sxx - sx * sx) + (syy - sy * sy) + c2
    s = a1 * a2 / (b1 * b2)
    d1 = 2 * sy * (a2 - a1) / (b1 * b2) - 2 * sx * s * (1 / b1 - 1 / b2)
    d2 = -s / b2
    d3 = 2 * a1 / (b1 * b2)
    count = n * c * (h - 10) * (w - 10)
    return (filt_t(d1) + 2 * a * filt_t(d2) + b * filt_t(d3)) / count


@functools.lru_cache(maxsize=None)
def fp32_formula_eps(shape, kind):
    """max |fp32 closed form - float64 autograd| / max |float64 autograd|:
    what fp32 arithmetic alone costs on this case."""
    _, ref = autograd_f64(shape, kind)
    got = formula_grad(*images(shape, kind), torch.float32).double()
    return ((got - ref).abs().max() / ref.abs().max()).item()
