"""CPU tests of the device-resident dataset cache's host layer
(waternet_amd/data/device_cache.py): the augmentation-code semantics, the
draw-order parity with PairedAugment, the epoch source, and the CLI guard.
The HIP gather itself is covered by test_gpu_gather_augment.py."""

import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from waternet_amd.data.augment import PairedAugment
from waternet_amd.data.device_cache import (
    DeviceEpochSource,
    apply_code,
    gather_augment,
    sample_codes,
)

REPO = Path(__file__).resolve().parent.parent


def _pattern(h, w, n=0):
    y, x, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(3),
                          indexing="ij")
    return (((y * w + x) * 3 + c + 17 * n) % 251).astype(np.uint8)


def _closed_form(img, code):
    """The issue's per-pixel closed form, written out literally."""
    h, w = img.shape[:2]
    k = (code >> 2) & 3
    oh, ow = (w, h) if k & 1 else (h, w)
    out = np.empty((oh, ow, 3), dtype=img.dtype)
    for oy in range(oh):
        for ox in range(ow):
            if k == 0:
                y, x = oy, ox
            elif k == 1:
                y, x = ox, w - 1 - oy
            elif k == 2:
                y, x = h - 1 - oy, w - 1 - ox
            else:
                y, x = h - 1 - ox, oy
            if code & 2:
                y = h - 1 - y
            if code & 1:
                x = w - 1 - x
            out[oy, ox] = img[y, x]
    return out


def _rot90_composition(img, code):
    if code & 1:
        img = img[:, ::-1]
    if code & 2:
        img = img[::-1]
    return np.ascontiguousarray(np.rot90(img, (code >> 2) & 3))


@pytest.mark.parametrize("code", range(16))
def test_apply_code_all_codes(code):
    sq = _pattern(6, 6)
    assert np.array_equal(apply_code(sq, code), _closed_form(sq, code))
    assert np.array_equal(apply_code(sq, code), _rot90_composition(sq, code))
    if not (code >> 2) & 1:  # even k keeps the shape of a non-square image
        ns = _pattern(5, 7)
        got = apply_code(ns, code)
        assert got.shape == ns.shape
        assert np.array_equal(got, _closed_form(ns, code))
        assert np.array_equal(got, _rot90_composition(ns, code))


def test_sixteen_codes_eight_images():
    sq = _pattern(6, 6)
    distinct = {apply_code(sq, c).tobytes() for c in range(16)}
    assert len(distinct) == 8


def test_draw_order_parity_with_paired_augment():
    n = 64
    aug = PairedAugment(rng=np.random.default_rng(123))
    codes = sample_codes(np.random.default_rng(123), n, square=True)
    assert codes.dtype == np.int32 and codes.shape == (n,)
    for i in range(n):
        raw, ref = _pattern(6, 6, i), _pattern(6, 6, 100 + i)
        a_raw, a_ref = aug(image=raw, mask=ref)
        assert np.array_equal(apply_code(raw, codes[i]), a_raw), i
        assert np.array_equal(apply_code(ref, codes[i]), a_ref), i
    assert len(set(codes.tolist())) > 4  # the stream really varies


def test_sample_codes_non_square_same_draws():
    sq = sample_codes(np.random.default_rng(5), 200, square=True)
    ns = sample_codes(np.random.default_rng(5), 200, square=False)
    assert np.array_equal(ns, sq & ~4)  # same draws, k -> k & 2
    assert (sq & 4).any()


def _cpu_cache(n, h, w):
    raw = torch.from_numpy(np.stack([_pattern(h, w, i) for i in range(n)]))
    ref = torch.from_numpy(
        np.stack([_pattern(h, w, 50 + i) for i in range(n)]))
    return raw, ref


def _collect(src, e):
    batches = list(src.epoch(e))
    idx = torch.cat([b[0] for b in batches]).numpy()
    codes = torch.cat([b[1] for b in batches]).numpy()
    return batches, idx, codes


def test_epoch_source_batches_and_determinism():
    raw, ref = _cpu_cache(22, 8, 8)
    src = DeviceEpochSource(raw, ref, batch_size=8, shuffle=True,
                            augment=True, seed=7, rank=0)
    assert len(src) == 3
    batches, idx, codes = _collect(src, 3)
    assert [b[2] for b in batches] == [8, 8, 6]
    assert [b[0].shape[0] for b in batches] == [8, 8, 6]
    assert all(b[0].dtype == torch.int32 and b[1].dtype == torch.int32
               for b in batches)
    assert sorted(idx.tolist()) == list(range(22))
    assert not np.array_equal(idx, np.arange(22))  # shuffled

    _, idx2, codes2 = _collect(src, 3)
    assert np.array_equal(idx, idx2) and np.array_equal(codes, codes2)
    again = DeviceEpochSource(raw, ref, 8, shuffle=True, augment=True,
                              seed=7, rank=0)
    _, idx3, codes3 = _collect(again, 3)
    assert np.array_equal(idx, idx3) and np.array_equal(codes, codes3)

    _, idx_e, codes_e = _collect(src, 4)
    assert not np.array_equal(codes, codes_e)
    assert not np.array_equal(idx, idx_e)
    other_rank = DeviceEpochSource(raw, ref, 8, shuffle=True, augment=True,
                                   seed=7, rank=1)
    _, _, codes_r = _collect(other_rank, 3)
    assert not np.array_equal(codes, codes_r)
    assert ((codes >= 0) & (codes < 16)).all()
    assert (codes & 4).any()  # square cache: odd k does occur


def test_epoch_source_plain_order_and_no_augment():
    raw, ref = _cpu_cache(22, 8, 8)
    src = DeviceEpochSource(raw, ref, batch_size=8, shuffle=False,
                            augment=False, seed=1, rank=0)
    _, idx, codes = _collect(src, 0)
    assert np.array_equal(idx, np.arange(22))
    assert not codes.any()


def test_epoch_source_non_square_never_odd_k():
    raw, ref = _cpu_cache(22, 8, 16)
    src = DeviceEpochSource(raw, ref, batch_size=8, shuffle=True,
                            augment=True, seed=0, rank=0)
    seen = set()
    for e in range(8):
        _, _, codes = _collect(src, e)
        assert not (codes & 4).any()
        seen |= set(codes.tolist())
    assert len(seen) > 4


def test_out_of_range_index_rejected_on_host():
    raw, ref = _cpu_cache(22, 8, 8)
    src = DeviceEpochSource(raw, ref, batch_size=8)
    for bad in (22, -1, 2 ** 32):  # 2**32 would wrap to 0 as int32
        order = np.arange(22, dtype=np.int64)
        order[5] = bad
        with pytest.raises(IndexError, match="out of range"):
            src.epoch(0, order=order)
    with pytest.raises(IndexError, match="out of range"):
        gather_augment(raw, ref, torch.tensor([0, 22], dtype=torch.int32),
                       torch.zeros(2, dtype=torch.int32),
                       torch.empty((2, 8, 8, 3), dtype=torch.uint8),
                       torch.empty((2, 8, 8, 3), dtype=torch.uint8))


def test_cpu_gather_matches_apply_code():
    raw, ref = _cpu_cache(7, 8, 8)
    idx = torch.tensor([3, 0, 6, 3, 1, 6, 6, 2, 5], dtype=torch.int32)
    codes = torch.tensor([0, 5, 15, 9, 2, 12, 7, 14, 4], dtype=torch.int32)
    out_raw = torch.full((9, 8, 8, 3), 0xAB, dtype=torch.uint8)
    out_ref = torch.full_like(out_raw, 0xAB)
    gather_augment(raw, ref, idx, codes, out_raw, out_ref)
    for b in range(9):
        i, c = int(idx[b]), int(codes[b])
        assert np.array_equal(out_raw[b].numpy(),
                              apply_code(raw[i].numpy(), c)), b
        assert np.array_equal(out_ref[b].numpy(),
                              apply_code(ref[i].numpy(), c)), b

    # non-square: odd k acts as k & 2
    raw, ref = _cpu_cache(3, 8, 16)
    idx = torch.tensor([2, 0], dtype=torch.int32)
    codes = torch.tensor([4 | 1, 12 | 2], dtype=torch.int32)
    out_raw = torch.empty((2, 8, 16, 3), dtype=torch.uint8)
    out_ref = torch.empty_like(out_raw)
    gather_augment(raw, ref, idx, codes, out_raw, out_ref)
    assert np.array_equal(out_raw[0].numpy(), apply_code(raw[2].numpy(), 1))
    assert np.array_equal(out_ref[1].numpy(),
                          apply_code(ref[0].numpy(), 8 | 2))


def test_build_cache_on_cpu_subset(capsys):
    from waternet_amd.data.dataset import SyntheticUIEBDataset
    from waternet_amd.data.device_cache import build_cache

    ds = SyntheticUIEBDataset(n_images=7, im_height=8, im_width=16,
                              raw_mode=True)
    sub = torch.utils.data.Subset(ds, [4, 1, 6, 2, 0])
    raw, ref = build_cache(sub, "cpu", num_workers=0, batch_size=2)
    assert raw.shape == ref.shape == (5, 8, 16, 3)
    assert raw.dtype == torch.uint8
    for j, i in enumerate([4, 1, 6, 2, 0]):
        assert torch.equal(raw[j], ds[i]["raw"])
        assert torch.equal(ref[j], ds[i]["ref"])
    assert "[cache] 5 pairs 8x16, 0.0 MB, built in" in capsys.readouterr().out
    with pytest.raises(ValueError, match="raw-mode"):
        build_cache(SyntheticUIEBDataset(n_images=2, im_height=8,
                                         im_width=8, run_transforms=False),
                    "cpu")


def test_device_cache_needs_fast_engine(tmp_path):
    import os

    env = dict(os.environ, WATERNET_TRAINING_DIR=str(tmp_path / "runs"),
               HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    out = subprocess.run(
        [sys.executable, str(REPO / "train.py"), "--device-cache",
         "--engine", "eager", "--synthetic", "24", "--epochs", "1",
         "--batch-size", "8", "--height", "32", "--width", "32"],
        cwd=tmp_path, capture_output=True, text=True, timeout=600, env=env,
    )
    assert out.returncode != 0
    assert "--device-cache requires the fast engine" in out.stderr
    assert not (tmp_path / "runs").exists()  # refused before any output
