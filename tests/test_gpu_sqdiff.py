"""sqdiff255_sum (k_sqdiff255_flat / k_sqdiff255_pix: capped grid-stride
grid, fp32 per thread, f64 block reduction, one atomic per block) against a
float64 torch reference on the same bf16 inputs.

Values in [0, 1] as the loss sees them. Relative tolerance 1e-6: a term
(255*(a-b))^2 carries three fp32 roundings (<= 3 * 2^-24 = 1.8e-7
relative), a thread adds at most 9 such non-negative terms at these sizes
(<= 8 * 2^-24 = 4.8e-7 more, worst case), and everything above the thread
is f64.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL = 1e-6


@pytest.fixture(scope="module")
def ext():
    from waternet_amd.ops import ext as _ext

    return _ext()


def pair(shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    a = torch.rand(shape, generator=g).bfloat16().cuda()
    b = torch.rand(shape, generator=g).bfloat16().cuda()
    return a, b


def ref_sum(a, b):
    d = 255.0 * (a.double() - b.double())
    return (d * d).sum().item()


@pytest.mark.parametrize("n", [1, 65, 4097, 16 * 7 * 7 * 512])
def test_flat(ext, n):
    # Clog == Cp selects the flat kernel; one long row makes numel = n for
    # sizes that are no multiple of the 8-element vector
    a, b = pair((1, 1, 1, n), n)
    got = ext.sqdiff255_sum(a, b, n).item()
    want = ref_sum(a, b)
    print(f"flat n={n}: got {got!r} want {want!r} "
          f"rel {abs(got - want) / want:.3e}")
    assert abs(got - want) <= RTOL * want


def test_flat_nhwc_shape(ext):
    # the shape the perceptual loss uses: (16, 7, 7, 512)
    a, b = pair((16, 7, 7, 512), 3)
    got = ext.sqdiff255_sum(a, b, 512).item()
    want = ref_sum(a, b)
    assert abs(got - want) <= RTOL * want


# 16 * 112 * 112 pixels need more blocks than the grid cap: grid-stride path
@pytest.mark.parametrize("nhw", [1, 190, 12544, 16 * 112 * 112])
def test_pix(ext, nhw):
    # Clog 3 of Cp 16: the 13 pad channels hold non-zero values on purpose
    # and must not be counted
    a, b = pair((1, 1, nhw, 16), 100 + nhw)
    got = ext.sqdiff255_sum(a, b, 3).item()
    want = ref_sum(a[..., :3], b[..., :3])
    print(f"pix nhw={nhw}: got {got!r} want {want!r} "
          f"rel {abs(got - want) / want:.3e}")
    assert abs(got - want) <= RTOL * want
