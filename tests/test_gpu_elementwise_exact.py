"""The layout bridges, gated fusion, 2x2 max pooling and the squared-diff
backward, each exactly against a CPU reference.

Every input is chosen so that the exact result is representable in the
output type, so the comparison needs no tolerance:
  - bridges move bf16-exact values;
  - fusion maps and refined images take values in {0, 1/4, 1/2, 3/4, 1} and
    dout holds integers in [-3, 3], so every product and every 3-term sum is
    exact in bf16 (with or without FMA contraction);
  - max pooling moves values in {-1, 0, 1}, so ties are everywhere and the
    kernel's rule decides: scan (0,0), (0,1), (1,0), (1,1) with strict >,
    the first maximum wins;
  - sqdiff255_bwd is bf16(fp32(gscale * sign) * fp32(a - b)) with
    quarter-valued a and b: a - b is exact, one fp32 product, one rounding
    to bf16.
Comparisons are by value (-0.0 == 0.0).
"""

import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GRID_CAP = 4096 * 256  # threads of the capped 1-D grids


@pytest.fixture(scope="module")
def ext():
    from waternet_amd.ops import ext as _ext

    return _ext()


def gen(*key):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(repr(key).encode()))
    return g


def assert_same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    g, w = got.float().flatten(), want.float().flatten()
    bad = (g != w).nonzero().flatten()
    assert bad.numel() == 0, (
        f"{what}: {bad.numel()} of {w.numel()} differ; first at "
        f"{bad[0].item()}: got {g[bad[0]].item()} want {w[bad[0]].item()}")


# ---------------------------------------------------------------------------
# NCHW fp32 <-> NHWC bf16 bridges
# ---------------------------------------------------------------------------

# 1 / 255 / 257 pixels: one partial 256-pixel block, one pixel short of a
# block, one pixel into the second; 3 x 9 x 10: a block straddles two images
BRIDGE_NHW = [(1, 1, 1), (1, 15, 17), (1, 1, 257), (3, 9, 10)]
BRIDGE_C = [(3, 16), (100, 128), (512, 512)]


@pytest.mark.parametrize("nhw", BRIDGE_NHW)
@pytest.mark.parametrize("C,Cp", BRIDGE_C)
def test_bridges_exact(ext, C, Cp, nhw):
    n, h, w = nhw
    g = gen("bridge", C, Cp, nhw)
    x = torch.randn(n, C, h, w, generator=g).bfloat16().float()
    y = ext.nchw_to_nhwc(x.to(DEV), Cp)
    want = torch.zeros(n, h, w, Cp, dtype=torch.bfloat16)
    want[..., :C] = x.permute(0, 2, 3, 1).bfloat16()
    assert_same(y.cpu(), want, "nchw_to_nhwc")
    assert not y[..., C:].any(), "pad channels must be exactly 0"
    # the round trip is the identity
    assert_same(ext.nhwc_to_nchw(y, C).cpu(), x, "round trip")
    # nhwc_to_nchw slices the logical channels whatever the pad ones hold
    z = torch.randn(n, h, w, Cp, generator=g).bfloat16()
    assert_same(ext.nhwc_to_nchw(z.to(DEV), C).cpu(),
                z[..., :C].permute(0, 3, 1, 2).float().contiguous(),
                "nhwc_to_nchw")


# ---------------------------------------------------------------------------
# gated fusion
# ---------------------------------------------------------------------------

def quarters(g, *shape):
    return (torch.randint(0, 5, shape, generator=g).float() / 4).bfloat16()


def fusion_ref(dout, maps, rs):
    """fp32 reference of forward and backward over the 3 logical channels;
    every value is exact, so the order of the sums does not matter."""
    m = maps[..., :3].float()
    r = [t[..., :3].float() for t in rs]
    g = dout[..., :3].float()
    out = r[0] * m[..., 0:1] + r[1] * m[..., 1:2] + r[2] * m[..., 2:3]
    dm = torch.stack([(g * ri).sum(-1) for ri in r], dim=-1)
    dr = [g * m[..., i:i + 1] for i in range(3)]

    def pad(t):
        full = torch.zeros(*t.shape[:-1], 16, dtype=torch.bfloat16)
        full[..., :3] = t.bfloat16()
        assert torch.equal(full[..., :3].float(), t), "not exact in bf16"
        return full

    return pad(out), [pad(dm)] + [pad(t) for t in dr]


# 1 x 1032 x 1024 = 1,056,768 pixels: past the capped grid's one pass
FUSION_NHW = [(1, 1, 1), (1, 15, 17), (1, 1, 257), (1, 1032, 1024)]


@pytest.mark.parametrize("nhw", FUSION_NHW)
def test_fusion_exact(ext, nhw):
    """Forward and all four backward outputs. The pad channels 3..15 of the
    inputs hold non-zero values: they must not be read, and the pad channels
    of all five outputs must be 0."""
    if nhw == FUSION_NHW[-1]:
        assert nhw[0] * nhw[1] * nhw[2] > GRID_CAP
    g = gen("fusion", nhw)
    maps = quarters(g, *nhw, 16)
    rs = [quarters(g, *nhw, 16) for _ in range(3)]
    dout = torch.randint(-3, 4, (*nhw, 16), generator=g).float().bfloat16()
    want_out, want_grads = fusion_ref(dout, maps, rs)
    dev = [t.to(DEV) for t in (maps, *rs)]
    out = ext.fusion_fwd(*dev)
    assert_same(out.cpu(), want_out, "out")
    grads = ext.fusion_bwd(dout.to(DEV), *dev)
    assert len(grads) == 4
    for name, got, want in zip(("dmaps", "drwb", "drce", "drgc"), grads,
                               want_grads):
        assert_same(got.cpu(), want, name)
        assert not got[..., 3:].any(), f"{name}: pad channels must be 0"
    assert not out[..., 3:].any(), "out: pad channels must be 0"


# ---------------------------------------------------------------------------
# 2x2 max pooling
# ---------------------------------------------------------------------------

def maxpool_ref(x, dy):
    """NumPy reference with the kernel's rule: scan (0,0), (0,1), (1,0),
    (1,1) with strict >, so the first maximum wins. Odd H / W: the last row
    / column is dropped and dx is 0 there."""
    n, H, W, C = x.shape
    oh, ow = H // 2, W // 2
    cand = [x[:, dy_:2 * oh:2, dx_:2 * ow:2] for dy_ in (0, 1)
            for dx_ in (0, 1)]
    m = cand[0].copy()
    a = np.zeros(m.shape, dtype=np.uint8)
    for i in (1, 2, 3):
        win = cand[i] > m
        m[win] = cand[i][win]
        a[win] = i
    dx = np.zeros_like(x)
    for i in range(4):
        view = dx[:, (i >> 1):2 * oh:2, (i & 1):2 * ow:2]
        view[a == i] = dy[a == i]
    return m, a, dx


# odd H and W at both channel widths; 2 x 66 x 66 x 512: 1,115,136 outputs,
# past the capped grid's one pass
POOL_SHAPES = [(2, 7, 9, 64), (1, 5, 6, 512), (3, 2, 3, 64), (2, 66, 66, 512)]


@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_maxpool_exact(ext, shape):
    n, H, W, C = shape
    if shape == POOL_SHAPES[-1]:
        assert n * (H // 2) * (W // 2) * C > GRID_CAP
    g = gen("pool", shape)
    x = torch.randint(-1, 2, shape, generator=g).float()
    # non-zero gradients, so a gradient that lands on the wrong input shows
    dy = torch.randint(1, 4, (n, H // 2, W // 2, C), generator=g).float()
    dy *= torch.randint(0, 2, dy.shape, generator=g).float() * 2 - 1
    m, a, dx = maxpool_ref(x.numpy(), dy.numpy())
    y, idx = ext.maxpool2x2_fwd(x.bfloat16().to(DEV))
    assert_same(y.cpu(), torch.from_numpy(m).bfloat16(), "y")
    assert idx.dtype == torch.uint8
    assert np.array_equal(idx.cpu().numpy(), a), "argmax index"
    got = ext.maxpool2x2_bwd(dy.bfloat16().to(DEV), idx, H, W)
    assert_same(got.cpu(), torch.from_numpy(dx).bfloat16(), "dx")
    if H % 2:
        assert not got[:, H - 1].any(), "dropped last row must get 0"
    if W % 2:
        assert not got[:, :, W - 1].any(), "dropped last column must get 0"


# ---------------------------------------------------------------------------
# sqdiff255_bwd
# ---------------------------------------------------------------------------

# 2 x 96 x 96 x 64 = 1,179,648 elements: past the capped grid's one pass
SQD_SHAPES = [(1, 3, 5, 16), (2, 96, 96, 64)]


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("shape", SQD_SHAPES)
def test_sqdiff255_bwd_exact(ext, shape, sign):
    if shape == SQD_SHAPES[-1]:
        assert int(np.prod(shape)) > GRID_CAP
    g = gen("sqd", shape)
    a, b = quarters(g, *shape), quarters(g, *shape)
    # grad * 2 * 255^2 / numel for grad = 0.7, numel = 3000: the products
    # with quarters need rounding to bf16
    gscale = torch.tensor([0.7 * 2.0 * 255.0 * 255.0 / 3000.0],
                          dtype=torch.float32)
    gs = gscale * torch.tensor(sign, dtype=torch.float32)  # exact
    want = (gs * (a.float() - b.float())).bfloat16()
    assert not torch.equal(want.float(), gs * (a.float() - b.float()))
    got = ext.sqdiff255_bwd(a.to(DEV), b.to(DEV), gscale.to(DEV), sign)
    assert_same(got.cpu(), want, "da")


# ---------------------------------------------------------------------------
# host checks: a tensor the kernels would misread raises before any launch
# ---------------------------------------------------------------------------

def bf16(*shape, device=DEV):
    return torch.ones(shape, dtype=torch.bfloat16, device=device)


def strided(*shape):
    """A non-contiguous bf16 view of `shape` (every other channel)."""
    return bf16(*shape[:-1], 2 * shape[-1])[..., ::2]


def expect_raises(op, name, good, bad):
    op(*good.values())  # the baseline the bad cases are derived from is valid
    for case, change in bad.items():
        with pytest.raises(RuntimeError, match=name):
            op(*{**good, **change}.values())
            pytest.fail(f"case '{case}' was accepted")


def test_fusion_fwd_host_checks(ext):
    s = (2, 3, 5, 16)
    good = dict(maps=bf16(*s), rwb=bf16(*s), rce=bf16(*s), rgc=bf16(*s))
    expect_raises(ext.fusion_fwd, "fusion_fwd", good, {
        "strided maps": dict(maps=strided(*s)),
        "strided rce": dict(rce=strided(*s)),
        "sizes": dict(rgc=bf16(2, 3, 4, 16)),
        "Cp != 16": {k: bf16(2, 3, 5, 32) for k in good},
        "dtype": dict(rwb=bf16(*s).float()),
        "cpu": dict(rwb=bf16(*s, device="cpu")),
    })


def test_fusion_bwd_host_checks(ext):
    s = (2, 3, 5, 16)
    good = dict(dout=bf16(*s), maps=bf16(*s), rwb=bf16(*s), rce=bf16(*s),
                rgc=bf16(*s))
    expect_raises(ext.fusion_bwd, "fusion_bwd", good, {
        "strided dout": dict(dout=strided(*s)),
        "strided rgc": dict(rgc=strided(*s)),
        "sizes": dict(dout=bf16(2, 3, 6, 16)),
        "Cp != 16": {k: bf16(2, 3, 5, 32) for k in good},
        "dtype": dict(dout=bf16(*s).float()),
        "cpu": dict(maps=bf16(*s, device="cpu")),
    })


def test_sqdiff255_bwd_host_checks(ext):
    s = (2, 3, 5, 16)
    good = dict(a=bf16(*s), b=bf16(*s),
                gscale=torch.ones(1, device=DEV), sign=1.0)
    expect_raises(ext.sqdiff255_bwd, "sqdiff255_bwd", good, {
        "strided a": dict(a=strided(*s)),
        "strided b": dict(b=strided(*s)),
        "sizes": dict(b=bf16(2, 3, 5, 32)),
        "dtype": dict(a=bf16(*s).float()),
        "gscale dtype": dict(gscale=torch.ones(1, device=DEV).double()),
        "gscale on cpu": dict(gscale=torch.ones(1)),
        "gscale size": dict(gscale=torch.ones(2, device=DEV)),
    })


def test_maxpool2x2_fwd_host_checks(ext):
    good = dict(x=bf16(2, 4, 6, 64))
    expect_raises(ext.maxpool2x2_fwd, "maxpool2x2_fwd", good, {
        "strided": dict(x=strided(2, 4, 6, 64)),
        "dtype": dict(x=bf16(2, 4, 6, 64).float()),
        "rank": dict(x=bf16(4, 6, 64)),
        "cpu": dict(x=bf16(2, 4, 6, 64, device="cpu")),
    })


def test_maxpool2x2_bwd_host_checks(ext):
    idx = torch.zeros(2, 2, 3, 64, dtype=torch.uint8, device=DEV)
    good = dict(dy=bf16(2, 2, 3, 64), idx=idx, H=5, W=6)
    expect_raises(ext.maxpool2x2_bwd, "maxpool2x2_bwd", good, {
        "strided dy": dict(dy=strided(2, 2, 3, 64)),
        "strided idx": dict(idx=torch.zeros(2, 2, 3, 128, dtype=torch.uint8,
                                            device=DEV)[..., ::2]),
        "idx sizes": dict(idx=idx[:, :1].contiguous()),
        "idx dtype": dict(idx=idx.int()),
        "idx on cpu": dict(idx=idx.cpu()),
        "H too large": dict(H=6),
        "W too small": dict(W=5),
    })
