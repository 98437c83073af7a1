"""GPU tests of k_gather_augment_u8 (csrc/elementwise.hip): every
comparison is bitwise against the NumPy reference apply_code. Images hold
an asymmetric pattern, so a swapped axis, a wrong mirror or a wrong cache
entry cannot pass by accident."""

import numpy as np
import pytest
import torch

from waternet_amd.data.device_cache import apply_code

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FILL = 0xAB
GUARD = 4096  # bytes around each output view; a multiple of 4


def _pattern(n, h, w, salt=0):
    i, y, x, c = np.meshgrid(np.arange(n), np.arange(h), np.arange(w),
                             np.arange(3), indexing="ij")
    return (((y * w + x) * 3 + c + 17 * i + salt) % 251).astype(np.uint8)


def _caches(nc, h, w):
    return _pattern(nc, h, w), _pattern(nc, h, w, salt=101)


def _guarded(b, h, w):
    """(B,H,W,3) uint8 view into a 0xAB-filled buffer with guards."""
    n = b * h * w * 3
    buf = torch.full((GUARD + n + GUARD,), FILL, dtype=torch.uint8,
                     device=DEV)
    return buf, buf[GUARD:GUARD + n].view(b, h, w, 3)


def _run(raw_np, ref_np, idx, codes, allow_transpose):
    from waternet_amd.ops import ext

    b = len(idx)
    h, w = raw_np.shape[1:3]
    craw = torch.from_numpy(raw_np).to(DEV)
    cref = torch.from_numpy(ref_np).to(DEV)
    buf_a, out_raw = _guarded(b, h, w)
    buf_b, out_ref = _guarded(b, h, w)
    ext().gather_augment_u8(
        craw, cref,
        torch.tensor(idx, dtype=torch.int32, device=DEV),
        torch.tensor(codes, dtype=torch.int32, device=DEV),
        out_raw, out_ref, allow_transpose)
    torch.cuda.synchronize()
    for buf in (buf_a, buf_b):
        host = buf.cpu().numpy()
        assert (host[:GUARD] == FILL).all(), "wrote before the output"
        assert (host[-GUARD:] == FILL).all(), "wrote past the output"
    return out_raw.cpu().numpy(), out_ref.cpu().numpy()


def _check(raw_np, ref_np, idx, codes, allow_transpose, expect_codes=None):
    got_raw, got_ref = _run(raw_np, ref_np, idx, codes, allow_transpose)
    expect_codes = codes if expect_codes is None else expect_codes
    for b, (i, c) in enumerate(zip(idx, expect_codes)):
        assert np.array_equal(got_raw[b], apply_code(raw_np[i], c)), \
            (b, i, c, "raw")
        assert np.array_equal(got_ref[b], apply_code(ref_np[i], c)), \
            (b, i, c, "ref")


def test_all_codes_tile_plus_tail():
    """40 = one full 32-pixel tile + an 8-pixel tail, both directions."""
    raw, ref = _caches(7, 40, 40)
    idx = [3, 0, 6, 6, 1, 5, 2, 3, 0, 4, 6, 1, 1, 5, 2, 0]
    _check(raw, ref, idx, list(range(16)), True)


def test_smaller_than_a_tile():
    raw, ref = _caches(3, 8, 8)
    _check(raw, ref, [2], [13], True)
    # B=5 then B=3: together one code for each of the 8 distinct
    # transforms (k in 0..3, with and without hflip)
    _check(raw, ref, [1, 0, 2, 2, 1], [0, 4, 8, 12, 1], True)
    _check(raw, ref, [0, 2, 1], [5, 9, 13], True)


def test_non_square_even_k_and_k_masking():
    raw, ref = _caches(4, 24, 56)
    even = [0, 1, 2, 3, 8, 9, 10, 11]
    _check(raw, ref, [3, 1, 0, 2, 2, 0, 1, 3], even, False)
    odd = [4, 5, 6, 7, 12, 13, 14, 15]
    _check(raw, ref, [0, 3, 2, 1, 1, 2, 3, 0], odd, False,
           expect_codes=[c & ~4 for c in odd])
    # a square cache with the flag clear masks k the same way
    raw, ref = _caches(2, 40, 40)
    _check(raw, ref, [1, 0, 1], [4, 12, 7], False, expect_codes=[0, 8, 3])


def test_interior_tile_boundaries_under_transposes():
    raw, ref = _caches(3, 64, 64)
    _check(raw, ref, [2, 0, 1], [4, 12, 7], True)


def test_every_output_byte_overwritten():
    """Outputs start as 0xAB everywhere and the caches here hold no 0xAB
    byte, so any output byte still 0xAB was not written."""
    raw, ref = _caches(5, 40, 40)
    raw[raw == FILL] = 0
    ref[ref == FILL] = 1
    idx = [4, 0, 3, 3, 1, 2, 0, 4]
    codes = [0, 5, 6, 15, 8, 12, 3, 10]
    got_raw, got_ref = _run(raw, ref, idx, codes, True)
    assert not (got_raw == FILL).any() and not (got_ref == FILL).any()
    for b, (i, c) in enumerate(zip(idx, codes)):
        assert np.array_equal(got_raw[b], apply_code(raw[i], c))
        assert np.array_equal(got_ref[b], apply_code(ref[i], c))


def test_index_clamp_value():
    """The kernel clamps idx with an unsigned min, so the read stays inside
    the cache by construction: Nc+3 and -1 (0xFFFFFFFF) both give the last
    entry."""
    nc = 4
    raw, ref = _caches(nc, 16, 16)
    idx = [nc + 3, -1, 1]
    clamped = np.minimum(np.array(idx, dtype=np.int32).view(np.uint32),
                         nc - 1).tolist()
    assert clamped == [3, 3, 1]
    got_raw, got_ref = _run(raw, ref, idx, [0, 6, 13], True)
    for b, (i, c) in enumerate(zip(clamped, [0, 6, 13])):
        assert np.array_equal(got_raw[b], apply_code(raw[i], c))
        assert np.array_equal(got_ref[b], apply_code(ref[i], c))


def test_python_wrapper_defaults_allow_transpose():
    from waternet_amd.data.device_cache import gather_augment

    for h, w, expect in ((16, 16, [4, 15]), (8, 24, [0, 11])):
        raw, ref = _caches(2, h, w)
        craw, cref = torch.from_numpy(raw).to(DEV), \
            torch.from_numpy(ref).to(DEV)
        out_raw = torch.empty((2, h, w, 3), dtype=torch.uint8, device=DEV)
        out_ref = torch.empty_like(out_raw)
        gather_augment(craw, cref,
                       torch.tensor([1, 0], dtype=torch.int32, device=DEV),
                       torch.tensor([4, 15], dtype=torch.int32, device=DEV),
                       out_raw, out_ref)
        for b, (i, c) in enumerate(zip([1, 0], expect)):
            assert np.array_equal(out_raw[b].cpu().numpy(),
                                  apply_code(raw[i], c))
            assert np.array_equal(out_ref[b].cpu().numpy(),
                                  apply_code(ref[i], c))


def test_host_checks_raise_without_launching():
    from waternet_amd.ops import ext

    op = ext().gather_augment_u8

    def u8(*shape, device=DEV):
        return torch.zeros(shape, dtype=torch.uint8, device=device)

    def i32(n, device=DEV):
        return torch.zeros(n, dtype=torch.int32, device=device)

    out_raw, out_ref = u8(2, 16, 16, 3), u8(2, 16, 16, 3)
    good = dict(cache_raw=u8(3, 16, 16, 3), cache_ref=u8(3, 16, 16, 3),
                idx=i32(2), codes=i32(2), out_raw=out_raw, out_ref=out_ref,
                allow_transpose=True)
    op(**good)  # the baseline the bad cases are derived from is valid
    assert not out_raw.any() and not out_ref.any()  # zeros gathered

    bad = {
        "H % 8": dict(cache_raw=u8(3, 12, 16, 3), cache_ref=u8(3, 12, 16, 3),
                      out_raw=u8(2, 12, 16, 3), out_ref=u8(2, 12, 16, 3),
                      allow_transpose=False),
        "W % 8": dict(cache_raw=u8(3, 16, 20, 3), cache_ref=u8(3, 16, 20, 3),
                      out_raw=u8(2, 16, 20, 3), out_ref=u8(2, 16, 20, 3),
                      allow_transpose=False),
        "cache dtype": dict(cache_raw=u8(3, 16, 16, 3).to(torch.int8)),
        "out dtype": dict(out_ref=u8(2, 16, 16, 3).float()),
        "idx dtype": dict(idx=torch.zeros(2, dtype=torch.int64, device=DEV)),
        "codes dtype": dict(codes=torch.zeros(2, dtype=torch.uint8,
                                              device=DEV)),
        "idx on cpu": dict(idx=i32(2, device="cpu")),
        "cache on cpu": dict(cache_ref=u8(3, 16, 16, 3, device="cpu")),
        "cache shapes": dict(cache_ref=u8(4, 16, 16, 3)),
        "out batch": dict(out_raw=u8(3, 16, 16, 3)),
        "out size": dict(out_raw=u8(2, 16, 8, 3), out_ref=u8(2, 16, 8, 3)),
        "codes length": dict(codes=i32(3)),
        "channels": dict(cache_raw=u8(3, 16, 16, 4),
                         cache_ref=u8(3, 16, 16, 4)),
        "non-contiguous": dict(
            cache_raw=u8(3, 16, 16, 6)[..., ::2]),
        "transpose non-square": dict(
            cache_raw=u8(3, 16, 24, 3), cache_ref=u8(3, 16, 24, 3),
            out_raw=u8(2, 16, 24, 3), out_ref=u8(2, 16, 24, 3),
            allow_transpose=True),
    }
    out_raw.fill_(FILL)
    out_ref.fill_(FILL)
    for name, change in bad.items():
        with pytest.raises(RuntimeError, match="gather_augment_u8"):
            op(**{**good, **change})
            pytest.fail(f"case '{name}' was accepted")
    torch.cuda.synchronize()
    # nothing was launched: the valid outputs are untouched
    assert (out_raw == FILL).all() and (out_ref == FILL).all()
