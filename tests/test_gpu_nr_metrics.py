"""GPU tests for the no-reference quality kernels (csrc/nr_metrics.hip)
against the NumPy float64 definitions in waternet_amd/utils/nr_metrics.py.

Tolerance rtol=1e-9, atol=1e-9 is derived, not measured: the inputs of every
log/sqrt are exact integers on both sides, so what remains is double rounding
over at most ~1.5e5 summed terms (<= N*2^-53 ~ 2e-11 relative) plus a few
ulp of log. UCIQE is defined on the project's 8-bit LAB, so the GPU value is
compared against uciqe_from_lab of the bytes k_rgb2lab produced, and those
bytes against the CPU LAB separately (<= 1 count)."""

import functools

import numpy as np
import pytest
import torch

from waternet_amd.data.transforms import rgb2lab_u8
from waternet_amd.utils import nr_metrics as nrm

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RTOL = ATOL = 1e-9

SHAPES = [
    (1, 8, 8),       # one block
    (3, 24, 40),     # 3x5 blocks, H != W, image stride
    (2, 19, 21),     # remainder pixels; Sobel at column 15 reads column 16
    (1, 9, 67),      # 201-byte rows: unaligned
    (1, 33, 45),     # N % 10 != 0
    (1, 272, 520),   # 2210 blocks, several histogram partials
]
CONTENTS = ["random", "narrow", "black", "white", "red", "step", "stripes"]


@functools.lru_cache(maxsize=None)
def make_input(shape, content):
    n, h, w = shape
    rng = np.random.default_rng(1000 * h + w)
    x = np.zeros((n, h, w, 3), dtype=np.uint8)
    if content == "random":
        x = rng.integers(0, 256, size=x.shape, dtype=np.uint8)
    elif content == "narrow":
        x = rng.integers(100, 104, size=x.shape, dtype=np.uint8)
    elif content == "white":
        x[:] = 255
    elif content == "red":
        x[..., 0] = 255
    elif content == "step":      # 0/255 vertical steps, 4 columns per period
        x[:, :, (np.arange(w) // 2) % 2 == 1] = 255
    elif content == "stripes":   # 1/255, every column next to an edge
        x[:] = 1
        x[:, :, ((np.arange(w) + 1) // 2) % 2 == 1] = 255
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(shape, content):
    """NumPy [uicm, uism, uiconm, uiqm] per image, computed once."""
    x = make_input(shape, content)
    ref = np.array([[nrm.uicm(im), nrm.uism(im), nrm.uiconm(im),
                     nrm.uiqm(im)] for im in x])
    ref.setflags(write=False)
    return ref


def _block_extrema(img):
    e2 = np.stack([nrm.sobel_energy(img[..., c]) for c in range(3)])
    k2, k1 = img.shape[0] // 8, img.shape[1] // 8
    b = e2[:, :k2 * 8, :k1 * 8].reshape(3, k2, 8, k1, 8)
    return b.max(axis=(2, 4)), b.min(axis=(2, 4))


def test_inputs_reach_the_intended_paths():
    """The narrow-range image has blocks with min E2 == 0 and blocks with
    min E2 > 0; the step pattern's largest E2 needs more than 32 bits, and
    the striped one has such blocks with a non-zero minimum, so the 64-bit
    maximum reaches a logarithm."""
    mx, mn = _block_extrema(make_input((1, 272, 520), "narrow")[0])
    assert (mn == 0).any() and (mn > 0).any()
    mx, mn = _block_extrema(make_input((1, 272, 520), "step")[0])
    assert mx.max() > 2 ** 32
    mx, mn = _block_extrema(make_input((3, 24, 40), "stripes")[0])
    assert ((mx > 2 ** 32) & (mn > 0)).any()


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_nr_metrics_matches_numpy(shape, content):
    from waternet_amd.ops import ext

    x = make_input(shape, content)
    xg = torch.from_numpy(np.array(x)).to(DEV)

    lab = ext().rgb2lab_u8(xg).cpu().numpy()
    lab_cpu = np.stack([rgb2lab_u8(im) for im in x])
    lab_diff = np.abs(lab.astype(int) - lab_cpu.astype(int)).max()
    print(f"{shape} {content}: max LAB diff {lab_diff}")
    assert lab.shape == x.shape and lab.dtype == np.uint8
    assert lab_diff <= 1

    out = nrm.nr_metrics(xg)
    assert out.shape == (shape[0], 5) and out.dtype == torch.float64
    assert out.device.type == "cuda"
    got = out.cpu().numpy()
    ref = reference(shape, content)
    ref_uciqe = np.array([nrm.uciqe_from_lab(im) for im in lab])
    print("got", got.tolist())
    print("ref", ref.tolist(), ref_uciqe.tolist())
    print("max abs diff", np.abs(got[:, :4] - ref).max(),
          np.abs(got[:, 4] - ref_uciqe).max())
    np.testing.assert_allclose(got[:, :4], ref, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(got[:, 4], ref_uciqe, rtol=RTOL, atol=ATOL)
    if content in ("black", "white"):
        assert np.array_equal(got, np.zeros_like(got))

    again = nrm.nr_metrics(xg).cpu().numpy()
    assert got.tobytes() == again.tobytes(), "second call differs in bits"


def test_nr_metrics_noncontiguous_and_refusals():
    x = make_input((3, 24, 40), "random")
    xg = torch.from_numpy(np.array(x)).to(DEV)
    full = nrm.nr_metrics(xg)
    crop = nrm.nr_metrics(xg[1:, :19, :21])  # a strided view
    want = nrm.nr_metrics(xg[1:, :19, :21].contiguous())
    assert torch.equal(crop, want)
    assert not torch.equal(crop, full[1:])
    with pytest.raises(RuntimeError, match="at least 8x8"):
        nrm.nr_metrics(xg[:, :7])
    with pytest.raises(RuntimeError, match="uint8"):
        nrm.nr_metrics(xg.float())
    with pytest.raises(TypeError):
        nrm.nr_metrics(xg.cpu())
