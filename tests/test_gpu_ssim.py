"""ssim_sum (NCHW fp32) and ssim_sum_nhwc (padded NHWC bf16) against
`_ssim_torch` in float64 on bf16-exact data, at the sizes where the 16x16
tiling changes: 11x11 is a single window, 26x27 and 27x26 put one column /
one row of windows into a second tile. Two images, so blockIdx.z decodes
both an image and a channel.

Tolerance 1e-3 absolute on the mean, the one test_gpu_ops.py uses for the
fp32 kernel. The two entries run the same arithmetic on the same partial
layout, so on equal values they return the same bits; that is asserted too.
"""

import zlib

import pytest
import torch

from waternet_amd.utils.metrics import _ssim_torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ATOL = 1e-3
HW = [(11, 11), (26, 27), (27, 26)]
N = 2
ARGS = (1.0, 0.01, 0.03)  # data_range, k1, k2


@pytest.fixture(scope="module")
def ext():
    from waternet_amd.ops import ext as _ext

    return _ext()


def images(C, hw):
    """Two related (N,C,H,W) images in [0,1], exact in bf16."""
    g = torch.Generator()
    g.manual_seed(zlib.crc32(repr(("ssim", C, hw)).encode()))
    a = torch.rand(N, C, *hw, generator=g)
    b = (a * 0.7 + 0.3 * torch.rand(N, C, *hw, generator=g)).clamp(0, 1)
    return a.bfloat16().float(), b.bfloat16().float()


def to_nhwc(x, Cp, g=None):
    """(N,C,H,W) fp32 -> (N,H,W,Cp) bf16; pad channels hold non-zero
    garbage when a generator is given, else there are none to fill."""
    n, c, h, w = x.shape
    if g is None:
        assert c == Cp
        full = torch.empty(n, h, w, Cp, dtype=torch.bfloat16)
    else:
        full = (torch.rand(n, h, w, Cp, generator=g) + 1).bfloat16()
    full[..., :c] = x.permute(0, 2, 3, 1).bfloat16()
    return full


def want_mean(a, b):
    return _ssim_torch(a.double(), b.double(), ARGS[0], 11, 1.5,
                       *ARGS[1:]).item()


def count(C, hw):
    return N * C * (hw[0] - 10) * (hw[1] - 10)


@pytest.mark.parametrize("hw", HW)
def test_ssim_sum_nchw(ext, hw):
    a, b = images(3, hw)
    s = ext.ssim_sum(a.to(DEV), b.to(DEV), *ARGS)
    assert s.dtype == torch.float64 and s.dim() == 0
    got, want = s.item() / count(3, hw), want_mean(a, b)
    print(f"nchw {hw}: got {got!r} want {want!r} diff {abs(got - want):.3e}")
    assert abs(got - want) <= ATOL


@pytest.mark.parametrize("hw", HW)
@pytest.mark.parametrize("Clog", [3, 16])
def test_ssim_sum_nhwc(ext, Clog, hw):
    a, b = images(Clog, hw)
    g = torch.Generator()
    g.manual_seed(5)
    pads = g if Clog < 16 else None
    an, bn = to_nhwc(a, 16, pads), to_nhwc(b, 16, pads)
    if pads is not None:
        assert an[..., Clog:].float().abs().min() >= 1
        assert not torch.equal(an[..., Clog:], bn[..., Clog:])
    s = ext.ssim_sum_nhwc(an.to(DEV), bn.to(DEV), Clog, *ARGS)
    assert s.dtype == torch.float64 and s.dim() == 0
    got, want = s.item() / count(Clog, hw), want_mean(a, b)
    print(f"nhwc Clog={Clog} {hw}: got {got!r} want {want!r} "
          f"diff {abs(got - want):.3e}")
    assert abs(got - want) <= ATOL


@pytest.mark.parametrize("hw", HW)
def test_ssim_entries_agree_bitwise(ext, hw):
    a, b = images(3, hw)
    g = torch.Generator()
    g.manual_seed(6)
    s0 = ext.ssim_sum(a.to(DEV), b.to(DEV), *ARGS)
    s1 = ext.ssim_sum_nhwc(to_nhwc(a, 16, g).to(DEV),
                           to_nhwc(b, 16, g).to(DEV), 3, *ARGS)
    print(f"{hw}: nchw {s0.item()!r} nhwc {s1.item()!r}")
    assert torch.equal(s0, s1)


def test_ssim_strided_inputs_are_copied(ext):
    a, b = images(3, (12, 13))
    an = to_nhwc(a, 16, torch.Generator().manual_seed(7)).to(DEV)
    wide = torch.zeros(N, 12, 13, 32, dtype=torch.bfloat16, device=DEV)
    wide[..., ::2] = an
    assert torch.equal(ext.ssim_sum_nhwc(wide[..., ::2], an, 3, *ARGS),
                       ext.ssim_sum_nhwc(an, an, 3, *ARGS))
    ap = a.to(DEV).permute(0, 1, 3, 2)  # non-contiguous NCHW
    assert torch.equal(ext.ssim_sum(ap, ap.contiguous(), *ARGS),
                       ext.ssim_sum(ap.contiguous(), ap.contiguous(), *ARGS))


def expect_raises(op, name, good, bad):
    op(*good.values())  # the baseline the bad cases are derived from is valid
    for case, change in bad.items():
        with pytest.raises(RuntimeError, match=name):
            op(*{**good, **change}.values())
            pytest.fail(f"case '{case}' was accepted")


def test_ssim_host_checks(ext):
    x = torch.ones(2, 12, 13, 16, dtype=torch.bfloat16, device=DEV)
    good = dict(a=x, b=x, Clog=3, data_range=1.0, k1=0.01, k2=0.03)
    expect_raises(ext.ssim_sum_nhwc, "ssim_sum_nhwc", good, {
        "b dtype": dict(b=x.float()),
        "b on cpu": dict(b=x.cpu()),
        "a dtype": dict(a=x.float()),
        "sizes": dict(b=x[:, :11].contiguous()),
        "rank": dict(a=x[0], b=x[0]),
        "Clog > Cp": dict(Clog=17),
        "Clog < 1": dict(Clog=0),
        "below the window": dict(a=x[:, :10].contiguous(),
                                 b=x[:, :10].contiguous()),
    })
    f = torch.ones(2, 3, 12, 13, device=DEV)
    good = dict(a=f, b=f, data_range=1.0, k1=0.01, k2=0.03)
    expect_raises(ext.ssim_sum, "ssim_sum", good, {
        "b on cpu": dict(b=f.cpu()),
        "b dtype": dict(b=f.double()),
        "a dtype": dict(a=f.bfloat16()),
        "sizes": dict(b=f[:, :2].contiguous()),
        "below the window": dict(a=f[:, :, :10].contiguous(),
                                 b=f[:, :, :10].contiguous()),
    })


def test_ssim_empty_batch(ext):
    s = ext.ssim_sum_nhwc(
        torch.ones(0, 12, 13, 16, dtype=torch.bfloat16, device=DEV),
        torch.ones(0, 12, 13, 16, dtype=torch.bfloat16, device=DEV), 3, *ARGS)
    assert s.dtype == torch.float64 and s.item() == 0.0
    s = ext.ssim_sum(torch.ones(0, 3, 12, 13, device=DEV),
                     torch.ones(0, 3, 12, 13, device=DEV), *ARGS)
    assert s.dtype == torch.float64 and s.item() == 0.0
