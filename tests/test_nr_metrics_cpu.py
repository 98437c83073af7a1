"""CPU tests for the no-reference quality metrics (UIQM, UCIQE): closed
forms, an independent pixel-loop UISM, the trimmed mean by sort against the
one by histogram, block anchoring, and the two CLI entry points."""

import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from waternet_amd.utils import nr_metrics as nrm

REPO = Path(__file__).resolve().parent.parent


def _no_gpu_env():
    import os

    return dict(os.environ, HIP_VISIBLE_DEVICES="-1",
                CUDA_VISIBLE_DEVICES="-1")


def _save_weights(tmp_path):
    import torch

    from waternet_amd.models.waternet import WaterNet

    torch.manual_seed(0)
    ckpt = tmp_path / "w.pt"
    torch.save(WaterNet().state_dict(), ckpt)
    return ckpt


@pytest.mark.parametrize("grey", [0, 97, 255])
def test_constant_image_is_all_zero(grey):
    """A constant (grey) image has no colour, no edges, no contrast and no
    chroma: all five values are exactly 0."""
    img = np.full((19, 21, 3), grey, dtype=np.uint8)
    m = nrm.nr_metrics(img)
    assert m.shape == (1, 5) and m.dtype == np.float64
    assert np.array_equal(m, np.zeros((1, 5)))


def test_too_small_image_refused():
    with pytest.raises(ValueError, match="at least 8x8"):
        nrm.nr_metrics(np.zeros((7, 20, 3), dtype=np.uint8))
    with pytest.raises(ValueError, match="at least 8x8"):
        nrm.uiqm(np.zeros((20, 7, 3), dtype=np.uint8))


def test_uicm_closed_form_constant_opponents():
    """R-G = d and YB constant everywhere: both variances vanish and
    UICM == -0.0268*sqrt(d^2 + YB^2), whatever the pixels look like."""
    rng = np.random.default_rng(0)
    d, yb2 = 37, -51                       # YB = yb2/2 = -25.5
    # R = G + d, B = (R + G - yb2)/2 = G + (d - yb2)/2 = G + 44
    g = rng.integers(0, 200, size=(16, 24)).astype(np.int64)
    img = np.stack([g + d, g, g + (d - yb2) // 2], axis=-1)
    assert img.min() >= 0 and img.max() <= 255
    img = img.astype(np.uint8)
    assert nrm.uicm(img) == -0.0268 * math.sqrt(d * d + (yb2 / 2.0) ** 2)


def test_uiconm_closed_form():
    """Every block holds max M and min m: UIConM = -(t/s)*ln(t/s)."""
    M, m = 200, 40
    rng = np.random.default_rng(1)
    img = rng.integers(m, M + 1, size=(24, 32, 3), dtype=np.uint8)
    img[0::8, 0::8, 0] = M
    img[1::8, 1::8, 2] = m
    q = (M - m) / (M + m)
    assert nrm.uiconm(img) == pytest.approx(-q * math.log(q), rel=1e-14)


def _uism_loops(img):
    """Independent UISM: per-pixel Sobel with clamped indices, per-block
    max/min, python ints throughout."""
    H, W = img.shape[:2]
    k2, k1 = H // 8, W // 8
    weights = (0.299, 0.587, 0.114)
    total = 0.0
    for c in range(3):
        ch = [[int(v) for v in row] for row in img[..., c]]

        def px(y, x):
            return ch[min(max(y, 0), H - 1)][min(max(x, 0), W - 1)]

        acc = 0.0
        for by in range(k2):
            for bx in range(k1):
                mx, mn = None, None
                for y in range(by * 8, by * 8 + 8):
                    for x in range(bx * 8, bx * 8 + 8):
                        gx = (px(y - 1, x + 1) + 2 * px(y, x + 1)
                              + px(y + 1, x + 1) - px(y - 1, x - 1)
                              - 2 * px(y, x - 1) - px(y + 1, x - 1))
                        gy = (px(y + 1, x - 1) + 2 * px(y + 1, x)
                              + px(y + 1, x + 1) - px(y - 1, x - 1)
                              - 2 * px(y - 1, x) - px(y - 1, x + 1))
                        e2 = (gx * gx + gy * gy) * px(y, x) ** 2
                        mx = e2 if mx is None else max(mx, e2)
                        mn = e2 if mn is None else min(mn, e2)
                if mn > 0:
                    acc += 0.5 * math.log(mx / mn)
        total += weights[c] * (2.0 / (k1 * k2)) * acc
    return total


@pytest.mark.parametrize("shape", [(16, 24), (19, 21)])
def test_uism_matches_pixel_loop(shape):
    rng = np.random.default_rng(shape[0])
    img = rng.integers(0, 256, size=shape + (3,), dtype=np.uint8)
    assert nrm.uism(img) == pytest.approx(_uism_loops(img), rel=1e-12)


def test_uism_zero_min_blocks_contribute_nothing():
    """A flat block has min E2 == 0 and adds 0, not -inf or nan."""
    rng = np.random.default_rng(5)
    img = rng.integers(1, 256, size=(16, 16, 3), dtype=np.uint8)
    img[:8, :8] = 100
    v = nrm.uism(img)
    assert np.isfinite(v) and v == pytest.approx(_uism_loops(img), rel=1e-12)


def _trimmed_mean_hist(x, lo_val, hi_val):
    """The trimmed mean the way the kernel computes it: walk a histogram."""
    n = x.size
    t_l, t_r = (n + 9) // 10, n // 10
    hist = np.bincount(x.ravel() - lo_val, minlength=hi_val - lo_val + 1)
    cum, tsum = 0, 0
    for v, cnt in enumerate(hist.tolist()):
        take = min(cum + cnt, n - t_r) - max(cum, t_l)
        if take > 0:
            tsum += take * (v + lo_val)
        cum += cnt
    return tsum / (n - t_l - t_r)


@pytest.mark.parametrize("n", [30, 1485])
def test_trimmed_mean_sort_equals_histogram(n):
    """N=30 is where ceil(0.1*N) goes wrong in floating point; N=1485 has
    T_L=149 != T_R=148."""
    rng = np.random.default_rng(n)
    x = rng.integers(-255, 256, size=n).astype(np.int64)
    t_l, t_r = (n + 9) // 10, n // 10
    assert t_l == math.ceil(n / 10) and t_r == n // 10
    if n == 1485:
        assert t_l != t_r
    assert nrm.trimmed_mean(x) == _trimmed_mean_hist(x, -255, 255)
    assert nrm.trimmed_mean(x) == np.sort(x)[t_l:n - t_r].mean()


def test_uiconm_ignores_remainder_pixels():
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, size=(19, 21, 3), dtype=np.uint8)
    assert nrm.uiconm(img) == nrm.uiconm(img[:16, :16])


def test_uiqm_is_the_weighted_sum_and_batch_shape():
    rng = np.random.default_rng(2)
    x = rng.integers(0, 256, size=(2, 16, 24, 3), dtype=np.uint8)
    m = nrm.nr_metrics(x)
    assert m.shape == (2, 5)
    for i in range(2):
        assert m[i, 3] == 0.0282 * m[i, 0] + 0.2953 * m[i, 1] \
            + 3.5753 * m[i, 2]
        assert m[i, 3] == nrm.uiqm(x[i])
        assert m[i, 4] == nrm.uciqe(x[i])
    assert np.array_equal(nrm.nr_metrics(x[1]), m[1:2])


def test_uciqe_constant_chroma_has_zero_sigma():
    """Pure red: chroma is constant, L is constant: UCIQE = 0.2576*c/l
    exactly, with no sqrt(rounding noise) from the variance."""
    from waternet_amd.data.transforms import rgb2lab_u8

    img = np.zeros((16, 24, 3), dtype=np.uint8)
    img[..., 0] = 255
    L8, A8, B8 = (int(v) for v in rgb2lab_u8(img)[0, 0])
    c = math.sqrt((A8 - 128) ** 2 + (B8 - 128) ** 2) / 255.0
    assert nrm.uciqe(img) == pytest.approx(0.2576 * c / (L8 / 255.0),
                                           rel=1e-14)


def test_inference_cli_report_quality_cpu(tmp_path):
    """--report-quality on the CPU path: one printed line, quality.csv with
    the specified header and one row, *_before equal to nr_metrics of the
    source at %.6f; without the flag no quality.csv appears."""
    from PIL import Image

    ckpt = _save_weights(tmp_path)
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, size=(16, 24, 3), dtype=np.uint8)
    src = tmp_path / "x.png"
    Image.fromarray(img).save(src)

    cmd = [sys.executable, str(REPO / "inference.py"), "--source", str(src),
           "--weights", str(ckpt)]
    out = subprocess.run(cmd + ["--name", "q", "--report-quality"],
                         cwd=tmp_path, capture_output=True, text=True,
                         timeout=600, env=_no_gpu_env())
    assert out.returncode == 0, out.stderr
    assert "x.png: UIQM " in out.stdout
    lines = (tmp_path / "output" / "q" / "quality.csv").read_text() \
        .splitlines()
    assert lines[0] == (
        "source,frames,uiqm_before,uiqm_after,uciqe_before,uciqe_after,"
        "uicm_before,uicm_after,uism_before,uism_after,uiconm_before,"
        "uiconm_after")
    assert len(lines) == 2
    row = dict(zip(lines[0].split(","), lines[1].split(",")))
    assert row["source"] == "x.png" and row["frames"] == "1"
    m = nrm.nr_metrics(img)[0]
    with Image.open(tmp_path / "output" / "q" / "x.png") as im:
        m_after = nrm.nr_metrics(np.asarray(im.convert("RGB")))[0]
    for i, key in enumerate(nrm.KEYS):
        assert row[f"{key}_before"] == "%.6f" % m[i], key
        assert row[f"{key}_after"] == "%.6f" % m_after[i], key

    out = subprocess.run(cmd + ["--name", "plain"], cwd=tmp_path,
                         capture_output=True, text=True, timeout=600,
                         env=_no_gpu_env())
    assert out.returncode == 0, out.stderr
    assert "UIQM" not in out.stdout
    assert sorted(p.name for p in (tmp_path / "output" / "plain").iterdir()) \
        == ["x.png"]


def test_score_cli_no_ref(tmp_path):
    """score.py --no-ref needs no weights or dataset and prints the mean
    UIQM / UCIQE and the image count."""
    import ast

    from PIL import Image

    rng = np.random.default_rng(6)
    d = tmp_path / "imgs"
    d.mkdir()
    imgs = [rng.integers(0, 256, size=s + (3,), dtype=np.uint8)
            for s in ((16, 24), (19, 21))]
    for i, im in enumerate(imgs):
        Image.fromarray(im).save(d / f"{i}.png")
    (d / "notes.txt").write_text("not an image")
    out = subprocess.run(
        [sys.executable, str(REPO / "score.py"), "--no-ref", str(d)],
        cwd=tmp_path, capture_output=True, text=True, timeout=600,
        env=_no_gpu_env())
    assert out.returncode == 0, out.stderr
    got = ast.literal_eval(out.stdout.strip())
    m = nrm.nr_metrics(imgs[0]) + nrm.nr_metrics(imgs[1])
    assert got["images"] == 2
    assert got["uiqm"] == pytest.approx(m[0, 3] / 2, rel=1e-12)
    assert got["uciqe"] == pytest.approx(m[0, 4] / 2, rel=1e-12)
