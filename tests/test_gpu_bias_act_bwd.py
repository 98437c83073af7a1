"""bias_grad, act_bwd and act_bwd_bias against CPU references, exactly.

bias_grad (k_bias_grad + k_bias_grad_reduce) runs on integer dy in [-3, 3]:
every partial sum is an integer of magnitude <= 3 * M < 2^24, so fp32 is
exact in any order and db must equal db0 + the fp64 column sum.

act_bwd / act_bwd_bias (k_act_bwd, k_act_bwd_bias + k_abb_reduce): dpre is
compared with a CPU fp32 recompute, each step rounded to fp32 and the result
rounded to bf16 (round to nearest even). ReLU is y > 0 ? dy : 0; sigmoid is
(dy * y) * (1 - y) in that order. No step can contract into an FMA, so
equality is expected. The db of the fused kernel is exact on crafted data:
integer dy in [-3, 3] and, for sigmoid, y in {0.25, 0.5, 0.75}, so every
derivative is a multiple of 1/16 and every sum stays exact in fp32.
"""

import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RELU, SIGMOID = 1, 2


@pytest.fixture(scope="module")
def ext():
    from waternet_amd.ops import ext as _ext

    return _ext()


def rng_of(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def int_dy(rng, nhw, Kp):
    """Integers in [-3, 3] on every one of the Kp columns (the pad columns
    too: what is summed into db is decided by K alone)."""
    return torch.from_numpy(
        rng.integers(-3, 4, size=(*nhw, Kp)).astype(np.float32)).bfloat16()


# ---------------------------------------------------------------------------
# bias_grad
# ---------------------------------------------------------------------------

def bias_launch(M, Kp):
    """The launch shape of bias_grad's host rule, to pin what a case
    reaches: (gx, msplit, MR, rows per slice, empty trailing slices)."""
    ngrp = Kp // 8
    kgr = min(ngrp, 32)
    gx = -(-ngrp // kgr)
    mr = 256 // kgr
    msplit = min(max(1, 448 // gx), -(-M // mr))
    rows = -(-M // msplit)
    empty = sum(1 for y in range(msplit) if y * rows >= M)
    return gx, msplit, mr, rows, empty


# (N, H, W), Kp
BIAS_CASES = [
    ((1, 1, 1), 16),
    ((1, 1, 127), 16),       # below MR = 128
    ((1, 3, 5), 128),
    ((2, 30, 50), 64),
    ((2, 60, 60), 128),      # msplit 448, rows 17, 24 empty trailing slices,
                             # the reduce loop runs twice
    ((1, 1, 1801), 512),     # gx = 2, msplit 224, 23 empty slices
    ((3, 5, 3823), 16),      # M = 57,345: msplit 448 at MR 128
]


def test_bias_case_table_reaches_what_it_claims():
    assert bias_launch(127, 16) == (1, 1, 128, 127, 0)
    assert bias_launch(7200, 128) == (1, 448, 16, 17, 24)
    assert bias_launch(1801, 512) == (2, 224, 8, 9, 23)
    assert bias_launch(57345, 16)[:3] == (1, 448, 128)
    assert bias_launch(57345, 16)[3] * 448 > 57345  # ragged last slice


@pytest.mark.parametrize("full_k", [True, False], ids=["K=Kp", "K<Kp"])
@pytest.mark.parametrize("nhw,Kp", BIAS_CASES)
def test_bias_grad_exact(ext, nhw, Kp, full_k):
    """db0 + column sums, bitwise, with db a slice of a larger pre-filled
    buffer (the gradient arena): nothing outside db[:K] changes, so the
    columns >= K of a Kp-long view at db's address keep their values."""
    K = Kp if full_k else (3 if Kp == 16 else Kp - 5)
    rng = rng_of("bias", nhw, Kp, K)
    dy = int_dy(rng, nhw, Kp)
    M = dy.numel() // Kp
    assert 3 * M < 2 ** 24
    off = 8
    arena0 = torch.from_numpy(
        rng.integers(-9, 10, size=off + Kp + 24).astype(np.float32))
    arena = arena0.clone().to(DEV)
    db = arena[off:off + K]
    ext.bias_grad(dy.to(DEV), db)
    torch.cuda.synchronize()
    want = arena0.clone()
    col = dy.double().reshape(M, Kp).sum(0)[:K]
    want[off:off + K] = (arena0[off:off + K].double() + col).float()
    got = arena.cpu()
    bad = (got != want).nonzero().flatten().tolist()
    assert not bad, (f"arena indices {bad[:8]} differ (db = [{off}, "
                     f"{off + K})): got {got[bad[:8]]} want {want[bad[:8]]}")


# ---------------------------------------------------------------------------
# act_bwd / act_bwd_bias
# ---------------------------------------------------------------------------

# Kp, K, act, (N, H, W)
ACT_CASES = [
    (128, 128, RELU, (1, 1, 1)),        # n8 = 16: one partial block
    (64, 64, RELU, (3, 9, 7)),
    (64, 60, SIGMOID, (3, 9, 7)),
    (128, 128, RELU, (2, 72, 60)),      # n8 = 138,240 > 512 * 256: the
                                        # grid-stride loop runs, ragged second
                                        # pass; 512 slabs = two reduce passes
    (16, 3, SIGMOID, (2, 192, 176)),    # n8 = 135,168: the same regime at
                                        # the narrowest Kp
    (32, 32, RELU, (1, 1, 32769)),      # n8 = 131,076: just above 512 * 256
    (32, 20, SIGMOID, (1, 1, 32769)),
]


def test_act_case_table_reaches_what_it_claims():
    n8 = {c: c[3][0] * c[3][1] * c[3][2] * c[0] // 8 for c in ACT_CASES}
    loop = 512 * 256  # rows of 8 one pass of the capped grid covers
    assert n8[ACT_CASES[0]] == 16
    assert n8[ACT_CASES[3]] == 138240 and loop < 138240 < 2 * loop
    assert n8[ACT_CASES[4]] == 135168 > loop
    assert n8[ACT_CASES[5]] == loop + 4


def act_ref(dy, y, act):
    """CPU fp32 recompute of dY * act'(Y): the unrounded fp32 derivative."""
    g, v = dy.float(), y.float()
    if act == RELU:
        return torch.where(v > 0, g, torch.zeros_like(g))
    return (g * v) * (1.0 - v)


def random_pair(rng, nhw, Kp, act):
    """Random bf16 dy and post-activation y. ReLU outputs include 0, -0.0
    and negative values; sigmoid outputs lie in (0, 1)."""
    shape = (*nhw, Kp)
    dy = torch.from_numpy(
        rng.standard_normal(shape, dtype=np.float32)).bfloat16()
    if act == RELU:
        y = rng.standard_normal(shape, dtype=np.float32)
        y[rng.random(shape) < 0.2] = 0.0
        y[rng.random(shape) < 0.1] = -0.0
    else:
        y = 1.0 / (1.0 + np.exp(-3.0 * rng.standard_normal(
            shape, dtype=np.float32)))
    return dy, torch.from_numpy(y.astype(np.float32)).bfloat16()


def crafted_pair(rng, nhw, Kp, act):
    """Integer dy in [-3, 3]; y in {-1, -0.0, 0, 0.5, 2} for ReLU and in
    {0.25, 0.5, 0.75} for sigmoid: every derivative is a multiple of 1/16
    of magnitude <= 3, exact in bf16, and every column sum is exact in
    fp32."""
    shape = (*nhw, Kp)
    dy = int_dy(rng, nhw, Kp)
    vals = (np.array([-1.0, -0.0, 0.0, 0.5, 2.0], dtype=np.float32)
            if act == RELU else
            np.array([0.25, 0.5, 0.75], dtype=np.float32))
    y = torch.from_numpy(vals[rng.integers(0, len(vals), size=shape)])
    return dy, y.bfloat16()


def assert_same(got, want, what):
    """Equality of every element (as values: -0.0 == 0.0)."""
    got, want = got.float().flatten(), want.float().flatten()
    bad = (got != want).nonzero().flatten()
    assert bad.numel() == 0, (
        f"{what}: {bad.numel()} of {want.numel()} differ; first at "
        f"{bad[0].item()}: got {got[bad[0]].item()} want "
        f"{want[bad[0]].item()}")


@pytest.mark.parametrize("Kp,K,act,nhw", ACT_CASES)
def test_act_bwd_exact(ext, Kp, K, act, nhw):
    rng = rng_of("act", Kp, act, nhw)
    dy, y = random_pair(rng, nhw, Kp, act)
    got = ext.act_bwd(dy.to(DEV), y.to(DEV), act)
    assert_same(got.cpu(), act_ref(dy, y, act).bfloat16(), "dpre")


@pytest.mark.parametrize("act", [RELU, SIGMOID])
def test_act_bwd_past_the_grid_cap(ext, act):
    """2x192x176x128: n8 = 1,081,344 rows of 8 against the 4096 x 256
    threads of the capped grid, so the grid-stride loop runs a ragged second
    pass."""
    nhw, Kp = (2, 192, 176), 128
    assert 4096 * 256 < 2 * 192 * 176 * Kp // 8 < 2 * 4096 * 256
    rng = rng_of("act-big", act)
    dy, y = random_pair(rng, nhw, Kp, act)
    got = ext.act_bwd(dy.to(DEV), y.to(DEV), act)
    assert_same(got.cpu(), act_ref(dy, y, act).bfloat16(), "dpre")


@pytest.mark.parametrize("Kp,K,act,nhw", ACT_CASES)
def test_act_bwd_bias_exact(ext, Kp, K, act, nhw):
    """Crafted data: dpre and db0 + column sums of the derivative, both
    exact; db is a slice of a larger pre-filled buffer and nothing outside
    db[:K] changes. Random data: dpre against the fp32 recompute."""
    rng = rng_of("abb", Kp, K, act, nhw)
    dy, y = crafted_pair(rng, nhw, Kp, act)
    d = act_ref(dy, y, act)
    M = dy.numel() // Kp
    assert torch.equal(d * 16, (d * 16).round()) and 16 * 3 * M < 2 ** 24
    off = 8
    arena0 = torch.from_numpy(
        rng.integers(-9, 10, size=off + Kp + 24).astype(np.float32))
    arena = arena0.clone().to(DEV)
    got = ext.act_bwd_bias(dy.to(DEV), y.to(DEV), act, arena[off:off + K])
    torch.cuda.synchronize()
    assert_same(got.cpu(), d.bfloat16(), "dpre (crafted)")
    want = arena0.clone()
    col = d.double().reshape(M, Kp).sum(0)[:K]
    want[off:off + K] = (arena0[off:off + K].double() + col).float()
    assert_same(arena.cpu(), want, f"arena around db = [{off}, {off + K})")

    dy, y = random_pair(rng, nhw, Kp, act)
    db = torch.zeros(K, device=DEV)
    got = ext.act_bwd_bias(dy.to(DEV), y.to(DEV), act, db)
    assert_same(got.cpu(), act_ref(dy, y, act).bfloat16(), "dpre (random)")


# ---------------------------------------------------------------------------
# host checks: a tensor the kernels would misread raises before any launch
# ---------------------------------------------------------------------------

def bf16(*shape, device=DEV):
    return torch.ones(shape, dtype=torch.bfloat16, device=device)


def strided(*shape):
    """A non-contiguous bf16 view of `shape` (every other channel)."""
    return bf16(*shape[:-1], 2 * shape[-1])[..., ::2]


def test_act_bwd_host_checks(ext):
    good = dict(dy=bf16(2, 3, 5, 16), y=bf16(2, 3, 5, 16), act=RELU)
    assert ext.act_bwd(*good.values()).shape == (2, 3, 5, 16)
    bad = {
        "strided dy": dict(dy=strided(2, 3, 5, 16)),
        "strided y": dict(y=strided(2, 3, 5, 16)),
        "sizes": dict(y=bf16(2, 3, 5, 32)),
        "dtype": dict(y=bf16(2, 3, 5, 16).float()),
        "cpu": dict(dy=bf16(2, 3, 5, 16, device="cpu")),
        "act": dict(act=0),
    }
    for name, change in bad.items():
        with pytest.raises(RuntimeError, match="act_bwd"):
            ext.act_bwd(*{**good, **change}.values())
            pytest.fail(f"case '{name}' was accepted")


def test_act_bwd_bias_host_checks(ext):
    db = torch.full((16,), 7.0, device=DEV)
    good = dict(dy=bf16(2, 3, 5, 16), y=bf16(2, 3, 5, 16), act=RELU, db=db)
    ext.act_bwd_bias(*good.values())
    assert (db == 7.0 + 30.0).all()  # the baseline is valid: 30 rows of ones
    db.fill_(7.0)
    bad = {
        "strided dy": dict(dy=strided(2, 3, 5, 16)),
        "strided y": dict(y=strided(2, 3, 5, 16)),
        "sizes": dict(y=bf16(2, 3, 10, 16)),
        "dtype": dict(y=bf16(2, 3, 5, 16).half()),
        "cpu": dict(y=bf16(2, 3, 5, 16, device="cpu")),
        "act": dict(act=3),
        "Kp > 128": dict(dy=bf16(1, 1, 2, 256), y=bf16(1, 1, 2, 256)),
        "Kp not a power of two": dict(dy=bf16(1, 1, 2, 48),
                                      y=bf16(1, 1, 2, 48)),
        "db longer than Kp": dict(db=torch.zeros(17, device=DEV)),
        "db dtype": dict(db=torch.zeros(16, device=DEV).double()),
        "db strided": dict(db=torch.zeros(32, device=DEV)[::2]),
        "db on cpu": dict(db=torch.zeros(16)),
    }
    for name, change in bad.items():
        with pytest.raises(RuntimeError, match="act_bwd_bias"):
            ext.act_bwd_bias(*{**good, **change}.values())
            pytest.fail(f"case '{name}' was accepted")
    torch.cuda.synchronize()
    assert (db == 7.0).all()  # nothing was launched


def test_bias_grad_host_checks(ext):
    db = torch.full((16,), 7.0, device=DEV)
    good = dict(dy=bf16(2, 3, 5, 16), db=db)
    ext.bias_grad(*good.values())
    assert (db == 7.0 + 30.0).all()
    db.fill_(7.0)
    bad = {
        "strided dy": dict(dy=strided(2, 3, 5, 16)),
        "dtype": dict(dy=bf16(2, 3, 5, 16).float()),
        "rank": dict(dy=bf16(30, 16)),
        "cpu": dict(dy=bf16(2, 3, 5, 16, device="cpu")),
        "db longer than Kp": dict(db=torch.zeros(17, device=DEV)),
        "db dtype": dict(db=torch.zeros(16, device=DEV).bfloat16()),
        "db strided": dict(db=torch.zeros(32, device=DEV)[::2]),
        "db on cpu": dict(db=torch.zeros(16)),
    }
    for name, change in bad.items():
        with pytest.raises(RuntimeError, match="bias_grad"):
            ext.bias_grad(*{**good, **change}.values())
            pytest.fail(f"case '{name}' was accepted")
    torch.cuda.synchronize()
    assert (db == 7.0).all()  # nothing was launched
