"""The opt-in SSIM loss term through the model, FastStepEngine and train.py
on the GPU, at 32x32, batch 2, seeded."""

import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
W_SSIM = 50.0


def q(x):
    return x.bfloat16().float()


def test_model_grads_through_ssim_loss_native_vs_eager():
    """WaterNet native forward -> ssim_loss_nhwc -> backward against the
    eager fp32 composition with `_ssim_torch`; the criterion of
    test_model_backward_native_vs_eager (max err / max |ref| < 0.08)."""
    from waternet_amd.engine.native import waternet_forward_from_inputs
    from waternet_amd.models.waternet import WaterNet
    from waternet_amd.ops import ext
    from waternet_amd.ops.ssim import ssim_loss_nhwc
    from waternet_amd.utils.metrics import _ssim_torch

    torch.manual_seed(9)
    model = WaterNet().to(DEV)
    x = q(torch.rand(2, 3, 32, 32, device=DEV))
    ref = q((x * 0.8 + 0.2 * torch.rand_like(x)).clamp(0, 1))

    e = ext()
    inputs = e.build_inputs(x, x, x, x)
    out_nhwc = waternet_forward_from_inputs(model, *inputs)
    s = ssim_loss_nhwc(out_nhwc, e.nchw_to_nhwc(ref, 16), 3, 1.0)
    s.backward()
    native = {n: p.grad.clone() for n, p in model.named_parameters()}
    model.zero_grad()

    os.environ["WATERNET_AMD_EAGER"] = "1"
    try:
        s_ref = _ssim_torch(model(x, x, x, x), ref, 1.0)
        s_ref.backward()
    finally:
        os.environ.pop("WATERNET_AMD_EAGER")
    print(f"ssim native {s.item()!r} eager {s_ref.item()!r}")
    for n, p in model.named_parameters():
        g, r = native[n], p.grad
        scale = r.abs().max().item() + 1e-8
        err = (g - r).abs().max().item() / scale
        print(f"{n}: rel err {err:.4f} (max |ref| {scale:.3e})")
        assert err < 0.08, f"{n}: rel err {err}"


@pytest.fixture(scope="module")
def engine_runs():
    """3 steps on identical data, eager body and captured graph."""
    from waternet_amd.engine.fast import BenchTrainer

    out = {}
    for name, graph in (("eager", False), ("graph", True)):
        tr = BenchTrainer(batch_size=2, height=32, width=32, device=DEV,
                          use_graph=graph, seed=7, ssim_weight=W_SSIM)
        for _ in range(3):
            tr.step()
        torch.cuda.synchronize()
        out[name] = (tr.metrics(), tr._graph is not None)
    return out


def test_engine_graph_matches_eager(engine_runs):
    """Tolerance of test_bench_trainer_graph_matches_eager."""
    (me, _), (mg, captured) = engine_runs["eager"], engine_runs["graph"]
    print(f"eager {me}\ngraph {mg}")
    assert captured, "the step with the SSIM term was not captured"
    for k in me:
        assert abs(me[k] - mg[k]) / (abs(me[k]) + 1e-6) < 5e-2, (k, me, mg)


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_engine_loss_is_sum_of_reported_terms(engine_runs, mode):
    """loss = 0.05 perceptual + mse255 + W (1 - ssim) per step, so also for
    the step means. The engine forms it in fp32 with 6 roundings (0.05
    itself, two products, 1 - ssim, two sums), each at most 2^-24 of a value
    no larger than the sum of the terms' magnitudes: 6 * 2^-24 of that sum
    bounds the difference from the float64 evaluation, 8 * 2^-24 is
    asserted."""
    m, _ = engine_runs[mode]
    terms = [0.05 * m["perceptual"], m["mse255"], W_SSIM * (1.0 - m["ssim"])]
    want = sum(terms)
    bound = 8 * 2.0 ** -24 * sum(abs(t) for t in terms)
    print(f"{mode}: loss {m['loss']!r} want {want!r} diff "
          f"{abs(m['loss'] - want):.3e} bound {bound:.3e} terms {terms}")
    assert 0.0 < 1.0 - m["ssim"] < 2.0
    assert abs(m["loss"] - want) <= bound


def test_zero_weight_is_the_reference_loss():
    from waternet_amd.engine.fast import BenchTrainer

    tr = BenchTrainer(batch_size=2, height=32, width=32, device=DEV,
                      use_graph=False, seed=7)
    tr.step()
    torch.cuda.synchronize()
    m = tr.metrics()
    want = 0.05 * m["perceptual"] + m["mse255"]
    assert abs(m["loss"] - want) <= 8 * 2.0 ** -24 * want
    with pytest.raises(ValueError, match="ssim_weight"):
        BenchTrainer(batch_size=2, height=32, width=32, device=DEV,
                     use_graph=False, ssim_weight=-1.0)


def _train(tmp_path, name, extra):
    import train as train_cli

    os.environ["WATERNET_TRAINING_DIR"] = str(tmp_path / name)
    try:
        # --num-workers 0: the 8 loader workers train.py would fork by
        # default cost 15 s per run late in a full-suite process
        train_cli.main(["--synthetic", "8", "--epochs", "1", "--batch-size",
                        "2", "--height", "32", "--width", "32",
                        "--num-workers", "0"] + extra)
    finally:
        os.environ.pop("WATERNET_TRAINING_DIR", None)
    savedir = tmp_path / name / "0"
    cfg = json.loads((savedir / "config.json").read_text())
    rows = (savedir / "metrics-train.csv").read_text().splitlines()
    assert rows[0] == "mse,ssim,psnr,perceptual_loss,loss"
    return cfg, [float(v) for v in rows[1].split(",")]


def test_train_cli_ssim_weight(tmp_path):
    cfg, (mse, ssim, _, perceptual, loss) = _train(
        tmp_path, "with", ["--ssim-weight", "50"])
    assert cfg["ssim_weight"] == 50
    want = 0.05 * perceptual + mse + 50 * (1 - ssim)
    # the CSV keeps 6 decimals of each value; fp32 sum as in the test above
    assert abs(loss - want) <= 0.5e-6 * (0.05 + 1 + 50 + 1) \
        + 8 * 2.0 ** -24 * want
    cfg0, (mse0, _, _, perceptual0, loss0) = _train(tmp_path, "without", [])
    assert "ssim_weight" not in cfg0
    want0 = 0.05 * perceptual0 + mse0
    assert abs(loss0 - want0) <= 0.5e-6 * (0.05 + 1 + 1) \
        + 8 * 2.0 ** -24 * want0
