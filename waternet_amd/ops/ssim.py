"""Native HIP SSIM — the reference's torchmetrics
StructuralSimilarityIndexMeasure call site (train.py:44-47, SURVEY.md §2.2
K21), same 11x11/sigma-1.5 gaussian-window semantics. ssim_nhwc and
ssim_native are the metric path (no autograd); ssim_loss_nhwc is the same
value with a HIP backward, for the opt-in `1 - SSIM` training-loss term."""

import torch

from waternet_amd.ops import ext


def ssim_nhwc(preds, target, clog, data_range, k1=0.01, k2=0.03):
    """SSIM over NHWC bf16 tensors (clog logical channels) — the full-NHWC
    metric path (11x11 gaussian, sigma 1.5, torchmetrics semantics)."""
    a = preds.contiguous()
    b = target.contiguous()
    s = ext().ssim_sum_nhwc(a, b, clog, float(data_range), k1, k2)
    n, h, w, _ = a.shape
    count = n * clog * (h - 10) * (w - 10)
    return (s / count).to(torch.float32)


class SsimNhwc(torch.autograd.Function):
    """Mean SSIM over NHWC bf16 tensors with a grad path to `preds` (the
    training-loss twin of ssim_nhwc). The forward also stores dS/dsx,
    dS/dsxx, dS/dsxy of every window as fp32 maps; the backward is one
    transposed window correlation of those maps (csrc/ssim.hip). `target`
    is the reference image and is treated as a constant: its gradient is
    None even when it requires one."""

    @staticmethod
    def forward(ctx, preds, target, clog, data_range, k1, k2):
        a = preds.contiguous()
        b = target.contiguous()
        s, dmaps = ext().ssim_fwd_save_nhwc(a, b, clog, float(data_range),
                                            k1, k2)
        n, h, w, _ = a.shape
        ctx.save_for_backward(a, b, dmaps)
        ctx.clog = clog
        ctx.count = n * clog * (h - 10) * (w - 10)
        return (s / ctx.count).to(torch.float32)

    @staticmethod
    def backward(ctx, g):
        a, b, dmaps = ctx.saved_tensors
        # device scalar, so the launch replays inside a captured graph
        gscale = (g.to(torch.float32) / ctx.count).reshape(1).contiguous()
        da = ext().ssim_bwd_nhwc(a, b, dmaps, gscale, ctx.clog)
        return da, None, None, None, None, None


def ssim_loss_nhwc(preds, target, clog, data_range, k1=0.01, k2=0.03):
    """ssim_nhwc as a differentiable loss term: the mean SSIM as an fp32
    scalar whose backward reaches `preds` (use `1 - ssim_loss_nhwc(...)`).
    The forward value is bit-identical to ssim_nhwc on the same inputs."""
    return SsimNhwc.apply(preds, target, clog, data_range, k1, k2)


def ssim_native(preds, target, data_range, kernel_size=11, sigma=1.5,
                k1=0.01, k2=0.03):
    if kernel_size != 11 or abs(sigma - 1.5) > 1e-9:
        from waternet_amd.utils.metrics import _ssim_torch

        return _ssim_torch(preds, target, data_range, kernel_size, sigma, k1,
                           k2)
    a = preds.float().contiguous()
    b = target.float().contiguous()
    s = ext().ssim_sum(a, b, float(data_range), k1, k2)
    n, c, h, w = a.shape
    count = n * c * (h - kernel_size + 1) * (w - kernel_size + 1)
    return (s / count).to(torch.float32)
