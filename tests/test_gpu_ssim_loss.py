"""SSIM as a training loss: ssim_fwd_save_nhwc / ssim_bwd_nhwc and the
SsimNhwc autograd op against float64 CPU autograd of `_ssim_torch` on the
bf16-rounded inputs (ssim_loss_ref.py holds the cases and the reference).

Gradient tolerance, per element:
    |dx - ref| <= 2^-8 |ref| + eps * max|ref|
The first term is for the bf16 rounding of the output. bf16 keeps 8
significant bits, so rounding to nearest costs up to 2^-8 |dx| just above a
power of two (2^-9 just below one): the term has no slack there, and the
fp32 error of the kernels has to fit into the second term. eps is 4 x the
error of the same closed form evaluated in fp32 torch on the CPU against
that float64 reference, measured per case by fp32_formula_eps (the kernels
sum the 121 taps in another order than torch's convolutions). The measured
values are recorded in docs/KERNELS.md.
"""

import pytest
import torch

from ssim_loss_ref import (DATA_RANGE, K1, K2, KINDS, SHAPES, UPSTREAM,
                           autograd_f64, fp32_formula_eps, images, to_nhwc)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ARGS = (DATA_RANGE, K1, K2)


@pytest.fixture(scope="module")
def ext():
    from waternet_amd.ops import ext as _ext

    return _ext()


def nhwc_pair(shape, kind):
    a, b = images(shape, kind)
    cp = shape[3]
    return to_nhwc(a, cp, 5).to(DEV), to_nhwc(b, cp, 6).to(DEV)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_saving_forward_equals_metric(ext, shape, kind):
    """Same body, same partials, same f64 sum: the same bits."""
    an, bn = nhwc_pair(shape, kind)
    n, h, w, cp, clog = shape
    s0 = ext.ssim_sum_nhwc(an, bn, clog, *ARGS)
    s1, dmaps = ext.ssim_fwd_save_nhwc(an, bn, clog, *ARGS)
    print(f"{shape} {kind}: metric {s0.item()!r} saving {s1.item()!r}")
    assert s1.dtype == torch.float64 and s1.dim() == 0
    assert torch.equal(s0, s1)
    assert dmaps.dtype == torch.float32
    assert dmaps.shape == (n, clog, 3, h - 10, w - 10)
    assert torch.isfinite(dmaps).all()
    want, _ = autograd_f64(shape, kind)
    count = n * clog * (h - 10) * (w - 10)
    assert abs(s1.item() / count - want.item()) <= 1e-3  # test_gpu_ssim's


@pytest.mark.parametrize("g", UPSTREAM)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_gradient_parity(shape, kind, g):
    from waternet_amd.ops.ssim import ssim_loss_nhwc, ssim_nhwc

    an, bn = nhwc_pair(shape, kind)
    n, h, w, cp, clog = shape
    an.requires_grad_(True)
    bn.requires_grad_(True)  # the target is a constant: no gradient
    s = ssim_loss_nhwc(an, bn, clog, DATA_RANGE)
    assert s.dtype == torch.float32 and s.dim() == 0
    assert torch.equal(s.detach(),
                       ssim_nhwc(an.detach(), bn.detach(), clog, DATA_RANGE))
    (s * g).backward()
    dx = an.grad
    assert bn.grad is None
    assert dx.dtype == torch.bfloat16 and dx.shape == an.shape
    assert dx.is_contiguous()
    if cp > clog:
        assert dx[..., clog:].float().abs().max().item() == 0.0

    _, ref = autograd_f64(shape, kind)
    ref = ref * g
    got = dx[..., :clog].permute(0, 3, 1, 2).double().cpu()
    eps1 = fp32_formula_eps(shape, kind)
    eps = 4.0 * eps1
    rmax = ref.abs().max().item()
    err = (got - ref).abs()
    tol = 2.0 ** -8 * ref.abs() + eps * rmax
    worst = (err / tol).max().item()
    print(f"{shape} {kind} g={g}: fp32-formula eps {eps1:.3e}, max|ref| "
          f"{rmax:.3e}, max err {err.max().item():.3e} "
          f"({err.max().item() / rmax:.3e} of max|ref|), worst err/tol "
          f"{worst:.3f}")
    assert (err <= tol).all()


def test_strided_inputs_are_copied(ext):
    an, bn = nhwc_pair(SHAPES[0], "random")
    gs = torch.full((1,), 0.25, device=DEV)
    wide = torch.zeros(1, 11, 11, 32, dtype=torch.bfloat16, device=DEV)
    wide[..., ::2] = an
    s0, d0 = ext.ssim_fwd_save_nhwc(an, bn, 3, *ARGS)
    s1, d1 = ext.ssim_fwd_save_nhwc(wide[..., ::2], bn, 3, *ARGS)
    assert torch.equal(s0, s1) and torch.equal(d0, d1)
    assert torch.equal(ext.ssim_bwd_nhwc(wide[..., ::2], bn, d0, gs, 3),
                       ext.ssim_bwd_nhwc(an, bn, d0, gs, 3))


def expect_raises(op, name, good, bad):
    op(*good.values())  # the baseline the bad cases are derived from is valid
    for case, change in bad.items():
        with pytest.raises(RuntimeError, match=name):
            op(*{**good, **change}.values())
            pytest.fail(f"case '{case}' was accepted")


def test_host_checks(ext):
    x = torch.ones(2, 12, 13, 16, dtype=torch.bfloat16, device=DEV)
    small = x[:, :10].contiguous()
    narrow = x[:, :, :10].contiguous()
    good = dict(a=x, b=x, Clog=3, data_range=1.0, k1=0.01, k2=0.03)
    expect_raises(ext.ssim_fwd_save_nhwc, "ssim_fwd_save_nhwc", good, {
        "a dtype": dict(a=x.float()),
        "b dtype": dict(b=x.float()),
        "b on cpu": dict(b=x.cpu()),
        "sizes": dict(b=x[:, :11].contiguous()),
        "rank": dict(a=x[0], b=x[0]),
        "Clog > Cp": dict(Clog=17),
        "Clog < 1": dict(Clog=0),
        "a and b on cpu": dict(a=x.cpu(), b=x.cpu()),
        "H below the window": dict(a=small, b=small),
        "W below the window": dict(a=narrow, b=narrow),
    })
    _, dmaps = ext.ssim_fwd_save_nhwc(x, x, 3, 1.0, 0.01, 0.03)
    gs = torch.ones(1, device=DEV)
    good = dict(a=x, b=x, dmaps=dmaps, gscale=gs, Clog=3)
    expect_raises(ext.ssim_bwd_nhwc, "ssim_bwd_nhwc", good, {
        "a dtype": dict(a=x.float()),
        "b on cpu": dict(b=x.cpu()),
        "sizes": dict(b=x[:, :11].contiguous()),
        "rank": dict(a=x[0], b=x[0]),
        "Clog > Cp": dict(Clog=17),
        "Clog < 1": dict(Clog=0),
        "Clog not the maps'": dict(Clog=4),
        "a and b on cpu": dict(a=x.cpu(), b=x.cpu()),
        "H below the window": dict(a=small, b=small),
        "W below the window": dict(a=narrow, b=narrow),
        "dmaps dtype": dict(dmaps=dmaps.double()),
        "dmaps shape": dict(dmaps=dmaps[..., :-1].contiguous()),
        "dmaps strided": dict(dmaps=dmaps.transpose(3, 4)),
        "dmaps on cpu": dict(dmaps=dmaps.cpu()),
        "gscale dtype": dict(gscale=gs.double()),
        "gscale on cpu": dict(gscale=gs.cpu()),
        "gscale empty": dict(gscale=gs[:0]),
    })


def test_empty_batch(ext):
    x = torch.ones(0, 12, 13, 16, dtype=torch.bfloat16, device=DEV)
    s, dmaps = ext.ssim_fwd_save_nhwc(x, x, 3, *ARGS)
    assert s.dtype == torch.float64 and s.item() == 0.0
    assert dmaps.shape == (0, 3, 3, 2, 3)
    dx = ext.ssim_bwd_nhwc(x, x, dmaps, torch.ones(1, device=DEV), 3)
    assert dx.shape == x.shape and dx.dtype == torch.bfloat16
