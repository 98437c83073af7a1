"""The opt-in SSIM loss term on the CPU/eager path: composite_loss, the
trainer, the train.py flag, and the closed-form gradient that the GPU tests
use to size their tolerance (ssim_loss_ref.py)."""

import json

import pytest
import torch

from ssim_loss_ref import (KINDS, SHAPES, autograd_f64, formula_grad,
                           fp32_formula_eps, images)


def test_composite_loss_adds_weighted_term():
    from waternet_amd.engine.losses import PERCEPTUAL_WEIGHT, composite_loss
    from waternet_amd.models.vgg import PerceptualModel
    from waternet_amd.utils.metrics import _ssim_torch

    torch.manual_seed(0)
    vgg = PerceptualModel()
    out = torch.rand(2, 3, 32, 32, requires_grad=True)
    ref = (out.detach() * 0.8 + 0.2 * torch.rand(2, 3, 32, 32)).clamp(0, 1)
    w = 50.0
    base = composite_loss(out, ref, vgg)
    got = composite_loss(out, ref, vgg, ssim_weight=w)
    assert len(base) == 3 and len(got) == 3
    loss0, p0, m0 = base
    loss, p, m = got
    assert torch.equal(p, p0) and torch.equal(m, m0)
    assert torch.equal(loss0, PERCEPTUAL_WEIGHT * p0 + m0)
    term = w * (1.0 - _ssim_torch(out, ref, 1.0))
    assert term.item() > 0
    # fp32: one rounding of the sum beyond the term's own
    assert abs((loss - loss0).item() - term.item()) <= 2.0 ** -22 * loss.item()
    # the term carries gradient: d loss - d loss0 = -w dSSIM
    (g,) = torch.autograd.grad(loss, out, retain_graph=True)
    (g0,) = torch.autograd.grad(loss0, out, retain_graph=True)
    (gs,) = torch.autograd.grad(_ssim_torch(out, ref, 1.0), out)
    assert gs.abs().max() > 0
    assert torch.allclose(g - g0, -w * gs, rtol=1e-3,
                          atol=1e-5 * g.abs().max().item())


def test_flag_parses_with_default_zero():
    import train as train_cli

    assert train_cli.parse_args([]).ssim_weight == 0.0
    assert train_cli.parse_args(["--ssim-weight", "2.5"]).ssim_weight == 2.5
    with pytest.raises(SystemExit):
        train_cli.main(["--ssim-weight", "-1", "--synthetic", "4"])


def test_train_cli_eager_ssim_weight(tmp_path, monkeypatch):
    import train as train_cli

    monkeypatch.setenv("WATERNET_TRAINING_DIR", str(tmp_path))
    args = ["--engine", "eager", "--epochs", "1", "--batch-size", "2",
            "--height", "32", "--width", "32", "--synthetic", "4"]
    train_cli.main(args + ["--ssim-weight", "50"])
    train_cli.main(args)
    cfg = json.loads((tmp_path / "0" / "config.json").read_text())
    assert cfg["ssim_weight"] == 50
    cfg0 = json.loads((tmp_path / "1" / "config.json").read_text())
    assert "ssim_weight" not in cfg0
    rows = (tmp_path / "0" / "metrics-train.csv").read_text().splitlines()
    assert rows[0] == "mse,ssim,psnr,perceptual_loss,loss"
    mse, _, _, perceptual, loss = (float(v) for v in rows[1].split(","))
    # the eager trainer's SSIM metric infers its data range, the loss term
    # uses 1.0, so only the term's range is checked here: 0 < 1 - SSIM < 2
    extra = loss - (0.05 * perceptual + mse)
    assert 1e-3 < extra < 100.0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_closed_form_is_the_autograd_gradient(shape, kind):
    """In float64 the closed form that the kernels implement equals
    autograd to rounding; in fp32 it is what sizes the GPU tolerance."""
    _, ref = autograd_f64(shape, kind)
    got = formula_grad(*images(shape, kind), torch.float64)
    rel = ((got - ref).abs().max() / ref.abs().max()).item()
    eps = fp32_formula_eps(shape, kind)
    print(f"{shape} {kind}: f64 closed form {rel:.3e}, fp32 closed form "
          f"{eps:.3e} of max|grad|")
    assert rel <= 1e-11
    assert 0.0 < eps <= 1e-3
