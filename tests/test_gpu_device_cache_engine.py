"""GPU tests of the device-resident dataset cache above the kernel:
FastStepEngine.load_batch_cached (eager and under hipGraph replay),
train.py --device-cache end to end, and build_cache on PNG files."""

import json
import os

import numpy as np
import pytest
import torch

from waternet_amd.data.device_cache import (
    DeviceEpochSource,
    apply_code,
    build_cache,
    identity_pair,
)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H = W = 64


def _smooth_images(n, h, w, seed):
    """Spatially-correlated uint8 images (low-res noise upsampled)."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, size=(n, h // 8, w // 8, 3)).astype(np.uint8)
    up = base.repeat(8, axis=1).repeat(8, axis=2).astype(np.int32)
    fine = rng.integers(-12, 13, size=up.shape)
    return np.clip(up + fine, 0, 255).astype(np.uint8)


def _expected(cache_np, idx, codes):
    return np.stack([apply_code(cache_np[i], c) for i, c in zip(idx, codes)])


@pytest.mark.parametrize("use_graph", [False, True])
def test_load_batch_cached_fills_static_buffers(use_graph):
    from waternet_amd.engine.fast import FastStepEngine
    from waternet_amd.models.waternet import WaterNet

    torch.manual_seed(4)
    eng = FastStepEngine(WaterNet().to(DEV), batch_size=4, height=H,
                         width=W, device=DEV, use_graph=use_graph)
    raw_np, ref_np = _smooth_images(6, H, W, 1), _smooth_images(6, H, W, 2)
    craw, cref = torch.from_numpy(raw_np).to(DEV), \
        torch.from_numpy(ref_np).to(DEV)

    # two consecutive steps with different indices and codes: a stale
    # static buffer (or a replay that skipped the gather) would show
    for idx, codes in (([5, 0, 3, 3], [0, 7, 12, 4]),
                       ([1, 4, 2, 0], [9, 2, 14, 5])):
        got = eng.load_batch_cached(
            craw, cref, torch.tensor(idx, dtype=torch.int32, device=DEV),
            torch.tensor(codes, dtype=torch.int32, device=DEV))
        assert got[0] is eng.raw_static and got[1] is eng.ref_static
        eng.step()
        torch.cuda.synchronize()
        assert np.array_equal(eng.raw_static.cpu().numpy(),
                              _expected(raw_np, idx, codes))
        assert np.array_equal(eng.ref_static.cpu().numpy(),
                              _expected(ref_np, idx, codes))
    assert (eng._graph is not None) == use_graph
    m = eng.metrics()
    assert all(np.isfinite(v) for v in m.values()), m

    # short batch: tail-sized temporaries, static buffers left alone
    before = eng.raw_static.clone()
    raw_t, ref_t = eng.load_batch_cached(
        craw, cref, torch.tensor([2, 5], dtype=torch.int32, device=DEV),
        torch.tensor([6, 13], dtype=torch.int32, device=DEV))
    assert raw_t.shape == (2, H, W, 3)
    eng.step_batch(raw_t, ref_t)
    eng.eval_batch(raw_t, ref_t)
    torch.cuda.synchronize()
    assert np.array_equal(raw_t.cpu().numpy(),
                          _expected(raw_np, [2, 5], [6, 13]))
    assert np.array_equal(ref_t.cpu().numpy(),
                          _expected(ref_np, [2, 5], [6, 13]))
    assert torch.equal(before, eng.raw_static)
    assert all(np.isfinite(v) for v in eng.metrics().values())
    assert all(np.isfinite(v) for v in eng.eval_metrics().values())


def test_train_cli_device_cache(tmp_path, capsys):
    """Same artefacts as the DataLoader path's CLI test; 22 train / 2 val
    at batch 8 runs the ragged-tail branch and the validation gather."""
    import train as train_cli

    os.environ["WATERNET_TRAINING_DIR"] = str(tmp_path)
    try:
        train_cli.main([
            "--epochs", "2", "--batch-size", "8", "--height", "64",
            "--width", "64", "--synthetic", "24", "--device-cache",
            "--full-state",
        ])
    finally:
        os.environ.pop("WATERNET_TRAINING_DIR", None)
    out = capsys.readouterr().out
    assert "[cache] 22 pairs 64x64" in out and "[cache] 2 pairs 64x64" in out
    assert out.count("[fast] epoch train wall") == 2
    savedir = tmp_path / "0"
    sd = torch.load(savedir / "last.pt", map_location="cpu")
    from waternet_amd.models.waternet import WaterNet

    m = WaterNet()
    m.load_state_dict(sd)
    assert len(sd) == 34
    assert all(torch.isfinite(v).all() for v in sd.values())
    train_csv = (savedir / "metrics-train.csv").read_text().splitlines()
    assert train_csv[0] == "mse,ssim,psnr,perceptual_loss,loss"
    assert len(train_csv) == 3  # header + 2 epochs
    val_csv = (savedir / "metrics-val.csv").read_text().splitlines()
    assert val_csv[0] == "mse,ssim,psnr,perceptual_loss"
    assert len(val_csv) == 3
    rows = np.loadtxt(savedir / "metrics-train.csv", delimiter=",",
                      skiprows=1)
    assert np.isfinite(rows).all()
    assert np.isfinite(np.loadtxt(savedir / "metrics-val.csv",
                                  delimiter=",", skiprows=1)).all()
    cfg = json.loads((savedir / "config.json").read_text())
    assert cfg["batch_size"] == 8
    assert cfg["device_cache"] is True
    assert (savedir / "last-trainstate.pt").exists()


def test_build_cache_from_png_files_and_train(tmp_path, capsys):
    from PIL import Image

    from waternet_amd.data.dataset import UIEBDataset
    from waternet_amd.engine.fast import FastStepEngine
    from waternet_amd.models.waternet import WaterNet

    raw_dir, ref_dir = tmp_path / "raw-890", tmp_path / "reference-890"
    raw_dir.mkdir()
    ref_dir.mkdir()
    raws, refs = _smooth_images(8, 80, 80, 5), _smooth_images(8, 80, 80, 6)
    for i in range(8):
        Image.fromarray(raws[i]).save(raw_dir / f"{i:03d}.png")
        Image.fromarray(refs[i]).save(ref_dir / f"{i:03d}.png")
    ds = UIEBDataset(raw_dir, ref_dir, im_height=H, im_width=W,
                     transform=identity_pair, raw_mode=True)

    craw, cref = build_cache(ds, DEV, num_workers=0, batch_size=3)
    assert "[cache] 8 pairs 64x64, 0.2 MB, built in" in capsys.readouterr().out
    assert craw.shape == (8, H, W, 3) and craw.dtype == torch.uint8
    assert craw.device == torch.device(DEV) == cref.device
    host_raw = np.stack([ds[i]["raw"].numpy() for i in range(8)])
    host_ref = np.stack([ds[i]["ref"].numpy() for i in range(8)])
    assert np.array_equal(craw.cpu().numpy(), host_raw)
    assert np.array_equal(cref.cpu().numpy(), host_ref)
    assert not np.array_equal(host_raw, host_ref)

    src = DeviceEpochSource(craw, cref, batch_size=4, shuffle=True,
                            augment=True, seed=3, rank=0)
    torch.manual_seed(6)
    eng = FastStepEngine(WaterNet().to(DEV), batch_size=4, height=H,
                         width=W, device=DEV, use_graph=False)
    seen = []
    for idx, codes, n in src.epoch(0):
        assert n == 4 and idx.device == craw.device
        eng.load_batch_cached(craw, cref, idx, codes)
        eng.step()
        i_h, c_h = idx.cpu().tolist(), codes.cpu().tolist()
        assert np.array_equal(eng.raw_static.cpu().numpy(),
                              _expected(host_raw, i_h, c_h))
        assert np.array_equal(eng.ref_static.cpu().numpy(),
                              _expected(host_ref, i_h, c_h))
        seen += i_h
    assert sorted(seen) == list(range(8))
    assert eng._steps == 2
    assert all(np.isfinite(v) for v in eng.metrics().values())


def test_build_cache_refuses_when_too_large():
    class Huge(torch.utils.data.Dataset):
        def __len__(self):
            return 1 << 40

        def __getitem__(self, i):
            z = torch.zeros((8, 8, 3), dtype=torch.uint8)
            return {"raw": z, "ref": z}

    with pytest.raises(RuntimeError, match="more than half"):
        build_cache(Huge(), DEV)
