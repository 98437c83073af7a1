"""Training losses: VGG-perceptual + MSE composite.

Replicates train.py:110-127: ImageNet-normalize both images, run the VGG19
perceptual model on each, perceptual = mean(square(255*(f(x)-f(y)))),
mse = mean(square(255*(out-ref))), loss = 0.05*perceptual + mse.

Beyond the reference: ssim_weight > 0 adds ssim_weight * (1 - SSIM) (the
eager twin of FastStepEngine's HIP SSIM loss term).
"""

import torch

from waternet_amd.models.vgg import normalize_imagenet

PERCEPTUAL_WEIGHT = 0.05


def perceptual_loss(out, ref, vgg_model) -> torch.Tensor:
    fx = vgg_model(normalize_imagenet(out))
    with torch.no_grad():
        fy = vgg_model(normalize_imagenet(ref))
    d = 255.0 * (fx - fy)
    return torch.mean(d * d)


def mse_loss(out, ref) -> torch.Tensor:
    d = 255.0 * (out - ref)
    return torch.mean(d * d)


def composite_loss(out, ref, vgg_model, ssim_weight=0.0):
    """Returns (loss, perceptual, mse). ssim_weight > 0 adds
    ssim_weight * (1 - SSIM(out, ref)), data_range 1, to the loss only (in
    the unit of mse); 0 computes exactly the reference loss."""
    p = perceptual_loss(out, ref, vgg_model)
    m = mse_loss(out, ref)
    loss = PERCEPTUAL_WEIGHT * p + m
    if ssim_weight > 0:
        from waternet_amd.utils.metrics import _ssim_torch

        loss = loss + ssim_weight * (1.0 - _ssim_torch(out, ref, 1.0))
    return loss, p, m
