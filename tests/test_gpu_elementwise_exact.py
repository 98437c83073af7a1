"""The layout bridges, gated fusion, 2x2 max pooling, the squared-diff
backward and the RGB pixel maps (uint8 / planar fp32 / padded NHWC bf16
bridges, input builders, normalize, uint8 postprocess), each exactly against
a CPU reference.

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
  - the pixel maps are compared with a CPU fp32 recompute of the kernel's
    own arithmetic: float(byte) * fp32(1/255) (a multiply; / 255 differs for
    126 of the 256 bytes in fp32), (v - mean_c) / std_c and g / std_c with
    correctly rounded fp32 division, trunc(clip(v, 0, 1) * 255); one
    rounding to the output type. Pad channels that are inputs hold non-zero
    values, pad channels that are outputs must be exactly 0.
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
# pixel maps: u8 / planar fp32 / padded NHWC bf16 -> the same, three logical
# values per pixel through a per-channel op, and the two input builders
# ---------------------------------------------------------------------------

# 1 pixel; 257: one pixel into a second block; 1 x 1032 x 1024: the second
# pass of the capped grid-stride loop
PIX_NHW = [(1, 1, 1), (1, 1, 257), (1, 1032, 1024)]
# (nhw, Cp) for the kernels with a padded side
PIX_NHW_CP = [(PIX_NHW[0], 16), (PIX_NHW[1], 16), (PIX_NHW[1], 32),
              (PIX_NHW[2], 16)]
# the kernels' constant 1.f / 255.f; they multiply by it, and x * S255
# differs from x / 255 in fp32 for 126 of the 256 bytes
S255 = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(
    255.0, dtype=torch.float32)
MEAN = torch.tensor([0.485, 0.456, 0.406], dtype=torch.float32)
STD = torch.tensor([0.229, 0.224, 0.225], dtype=torch.float32)
# fp32 division is correctly rounded on both sides, so the normalize kernels
# are compared bit for bit; 1 would allow the one differing rounding a
# division can cause
NORMALIZE_ULPS = 0


def u8_ramp(nhw, mul, off):
    """(N,H,W,3) bytes (i * mul + off) mod 256 over the flat index: with an
    odd `mul` every 256 consecutive elements hold all 256 byte values."""
    n = nhw[0] * nhw[1] * nhw[2] * 3
    if nhw == PIX_NHW[-1]:
        assert n // 3 > GRID_CAP
    x = ((torch.arange(n, dtype=torch.int64) * mul + off) % 256).to(
        torch.uint8).reshape(*nhw, 3)
    if n >= 256:
        assert x.flatten().bincount(minlength=256).min() > 0
    return x


def garbage_pads(g, logical, Cp):
    """(..., 3) bf16 -> (..., Cp) with non-zero values in channels 3..Cp-1."""
    full = (torch.rand(*logical.shape[:-1], Cp, generator=g) + 1).bfloat16()
    full[..., :3] = logical
    assert full[..., 3:].float().abs().min() >= 1
    return full


def padded(logical, Cp):
    full = torch.zeros(*logical.shape[:-1], Cp, dtype=logical.dtype)
    full[..., :logical.shape[-1]] = logical
    return full


def to_planar(x):
    return x.permute(0, 3, 1, 2).contiguous()


def assert_ulps(got, want, what, ulps):
    """`got` within `ulps` representable values of `want` (same dtype, all
    finite); ulps = 0 is assert_same."""
    if ulps == 0:
        return assert_same(got, want, what)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    as_int = torch.int16 if got.dtype == torch.bfloat16 else torch.int32

    def key(t):  # monotone integer image of the float order
        i = t.contiguous().view(as_int).to(torch.int64)
        return torch.where(i < 0, -(i & (2 ** (8 * t.element_size() - 1) - 1)),
                           i)

    d = (key(got) - key(want)).abs().max().item()
    print(f"{what}: max distance {d} ulp")
    assert d <= ulps, f"{what}: {d} ulp apart"


@pytest.mark.parametrize("nhw,Cp", PIX_NHW_CP)
def test_u8_to_nhwc_exact(ext, nhw, Cp):
    x = u8_ramp(nhw, 7, 11)
    y = ext.u8_to_nhwc(x.to(DEV), Cp)
    assert_same(y.cpu(), padded((x.float() * S255).bfloat16(), Cp),
                "u8_to_nhwc")
    assert not y[..., 3:].any(), "pad channels must be exactly 0"


@pytest.mark.parametrize("nhw", PIX_NHW)
def test_u8_to_nchw_exact(ext, nhw):
    x = u8_ramp(nhw, 5, 3)
    assert_same(ext.u8_to_nchw(x.to(DEV)).cpu(), to_planar(x.float() * S255),
                "u8_to_nchw")


def check_built_inputs(outs, srcs):
    """cmg_in = [raw wb ce gc 0000], r*_in = [raw src 0...]: every output and
    every 3-channel slot of it against its own source."""
    assert len(outs) == 4
    names = ("raw", "wb", "ce", "gc")
    cmg = outs[0].cpu()
    for i, name in enumerate(names):
        assert_same(cmg[..., 3 * i:3 * i + 3], srcs[i], f"cmg_in <- {name}")
    assert not outs[0][..., 12:].any(), "cmg_in: pad channels must be 0"
    for i in (1, 2, 3):
        r = outs[i].cpu()
        assert_same(r[..., 0:3], srcs[0], f"r{names[i]}_in <- raw")
        assert_same(r[..., 3:6], srcs[i], f"r{names[i]}_in <- {names[i]}")
        assert not outs[i][..., 6:].any(), f"r{names[i]}_in: pads must be 0"


@pytest.mark.parametrize("nhw", PIX_NHW)
def test_build_inputs_u8_exact(ext, nhw):
    xs = [u8_ramp(nhw, m, o) for m, o in ((1, 0), (3, 64), (5, 128), (7, 192))]
    outs = ext.build_inputs_u8(*[x.to(DEV) for x in xs])
    check_built_inputs(outs, [(x.float() * S255).bfloat16() for x in xs])


@pytest.mark.parametrize("nhw", PIX_NHW)
def test_build_inputs_exact(ext, nhw):
    g = gen("build_inputs", nhw)
    xs = [torch.randn(*nhw, 3, generator=g).bfloat16() for _ in range(4)]
    outs = ext.build_inputs(*[to_planar(x.float()).to(DEV) for x in xs])
    check_built_inputs(outs, xs)


@pytest.mark.parametrize("nhw,Cp", PIX_NHW_CP)
def test_out_to_u8_exact(ext, nhw, Cp):
    g = gen("out_to_u8", nhw, Cp)
    v = (torch.rand(*nhw, 3, generator=g) * 2 - 0.5).bfloat16()
    special = torch.tensor([0.0, 1.0, 1.0 / 256], dtype=torch.bfloat16)
    v.view(-1)[:3] = special
    assert v.float().min() >= -0.5 and v.float().max() <= 1.5
    want = (v.float().clamp(0, 1) * 255).to(torch.uint8)  # truncates
    assert want.view(-1)[:3].tolist() == [0, 255, 0]
    got = ext.out_to_u8(garbage_pads(g, v, Cp).to(DEV))
    assert got.dtype == torch.uint8 and got.shape == want.shape
    assert torch.equal(got.cpu(), want), "out_to_u8"


@pytest.mark.parametrize("nhw,Cp", PIX_NHW_CP)
def test_normalize_nhwc_exact(ext, nhw, Cp):
    g = gen("normalize_nhwc", nhw, Cp)
    x = torch.rand(*nhw, 3, generator=g).bfloat16()
    y = ext.normalize_nhwc_fwd(garbage_pads(g, x, Cp).to(DEV))
    assert_ulps(y.cpu(), padded(((x.float() - MEAN) / STD).bfloat16(), Cp),
                "normalize_nhwc_fwd", NORMALIZE_ULPS)
    assert not y[..., 3:].any(), "fwd: pad channels must be exactly 0"
    dy = torch.randn(*nhw, 3, generator=g).bfloat16()
    dx = ext.normalize_nhwc_bwd(garbage_pads(g, dy, Cp).to(DEV))
    assert_ulps(dx.cpu(), padded((dy.float() / STD).bfloat16(), Cp),
                "normalize_nhwc_bwd", NORMALIZE_ULPS)
    assert not dx[..., 3:].any(), "bwd: pad channels must be exactly 0"


@pytest.mark.parametrize("nhw,Cp", PIX_NHW_CP)
def test_normalize_vgg_exact(ext, nhw, Cp):
    g = gen("normalize_vgg", nhw, Cp)
    x = torch.rand(*nhw, 3, generator=g)
    y = ext.normalize_vgg_fwd(to_planar(x).to(DEV), Cp)
    assert_ulps(y.cpu(), padded(((x - MEAN) / STD).bfloat16(), Cp),
                "normalize_vgg_fwd", NORMALIZE_ULPS)
    assert not y[..., 3:].any(), "fwd: pad channels must be exactly 0"
    dy = torch.randn(*nhw, 3, generator=g).bfloat16()
    dx = ext.normalize_vgg_bwd(garbage_pads(g, dy, Cp).to(DEV), 3)
    assert_ulps(dx.cpu(), to_planar(dy.float() / STD), "normalize_vgg_bwd",
                NORMALIZE_ULPS)


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


def u8(*shape, device=DEV):
    return torch.ones(shape, dtype=torch.uint8, device=device)


def f32(*shape, device=DEV):
    return torch.ones(shape, dtype=torch.float32, device=device)


def test_build_inputs_host_checks(ext):
    s = (2, 3, 4, 5)
    good = dict(raw=f32(*s), wb=f32(*s), ce=f32(*s), gc=f32(*s))
    expect_raises(ext.build_inputs, "build_inputs", good, {
        "raw channels": dict(raw=f32(2, 4, 4, 5)),
        "wb smaller": dict(wb=f32(2, 3, 4, 4)),
        "ce smaller": dict(ce=f32(1, 3, 4, 5)),
        "gc rank": dict(gc=f32(3, 4, 5)),
        "wb dtype": dict(wb=f32(*s).double()),
        "gc on cpu": dict(gc=f32(*s, device="cpu")),
    })
    s = (2, 4, 5, 3)
    good = dict(raw=u8(*s), wb=u8(*s), ce=u8(*s), gc=u8(*s))
    expect_raises(ext.build_inputs_u8, "build_inputs_u8", good, {
        "raw channels": dict(raw=u8(2, 4, 5, 4)),
        "wb smaller": dict(wb=u8(2, 4, 4, 3)),
        "ce smaller": dict(ce=u8(1, 4, 5, 3)),
        "gc smaller": dict(gc=u8(2, 3, 5, 3)),
        "ce dtype": dict(ce=u8(*s).float()),
        "wb on cpu": dict(wb=u8(*s, device="cpu")),
    })


def test_sqdiff255_sum_host_checks(ext):
    s = (2, 3, 5, 16)
    good = dict(a=bf16(*s), b=bf16(*s), Clog=3)
    expect_raises(ext.sqdiff255_sum, "sqdiff255_sum", good, {
        "a dtype": dict(a=bf16(*s).float()),
        "b dtype": dict(b=bf16(*s).float()),
        "b on cpu": dict(b=bf16(*s, device="cpu")),
        "strided a": dict(a=strided(*s)),
        "strided b": dict(b=strided(*s)),
        "sizes": dict(b=bf16(2, 3, 4, 16)),
        "rank": dict(a=bf16(3, 5, 16), b=bf16(3, 5, 16)),
        "Clog > Cp": dict(Clog=17),
        "Clog < 1": dict(Clog=0),
    })


def test_adam_step_host_checks(ext):
    n = 40
    good = dict(p=f32(n), g=f32(n), m=f32(n), v=f32(n), lr_buf=f32(1),
                b1=0.9, b2=0.999, eps=1e-8,
                step_buf=torch.zeros(1, dtype=torch.int32, device=DEV))
    expect_raises(ext.adam_step, "adam_step", good, {
        "g shorter": dict(g=f32(n - 1)),
        "m shorter": dict(m=f32(n - 1)),
        "v shorter": dict(v=f32(n - 1)),
        "g dtype": dict(g=f32(n).double()),
        "m on cpu": dict(m=f32(n, device="cpu")),
        "strided v": dict(v=f32(2 * n)[::2]),
        "lr_buf on cpu": dict(lr_buf=f32(1, device="cpu")),
        "step_buf on cpu": dict(step_buf=torch.zeros(1, dtype=torch.int32)),
        "lr_buf dtype": dict(lr_buf=f32(1).double()),
        "step_buf dtype": dict(step_buf=torch.zeros(1, dtype=torch.int64,
                                                    device=DEV)),
        "lr_buf empty": dict(lr_buf=f32(0)),
    })
    assert good["step_buf"].item() == 1, "a refused call must not tick"


def test_three_channel_host_checks(ext):
    """The wrappers that touch channels 0..2 of a padded NHWC tensor."""
    expect_raises(ext.u8_to_nhwc, "u8_to_nhwc", dict(x=u8(2, 4, 5, 3), Cp=16), {
        "Cp < 3": dict(Cp=2),
        "channels": dict(x=u8(2, 4, 5, 4)),
        "dtype": dict(x=u8(2, 4, 5, 3).float()),
        "cpu": dict(x=u8(2, 4, 5, 3, device="cpu")),
    })
    expect_raises(ext.u8_to_nchw, "u8_to_nchw", dict(x=u8(2, 4, 5, 3)), {
        "channels": dict(x=u8(2, 4, 5, 4)),
        "rank": dict(x=u8(4, 5, 3)),
        "cpu": dict(x=u8(2, 4, 5, 3, device="cpu")),
    })
    for name in ("normalize_nhwc_fwd", "normalize_nhwc_bwd", "out_to_u8"):
        expect_raises(getattr(ext, name), name, dict(x=bf16(2, 4, 5, 16)), {
            "Cp < 3": dict(x=bf16(2, 4, 5, 2)),
            "dtype": dict(x=bf16(2, 4, 5, 16).float()),
            "rank": dict(x=bf16(4, 5, 16)),
            "cpu": dict(x=bf16(2, 4, 5, 16, device="cpu")),
        })


def test_bridge_host_checks(ext):
    expect_raises(ext.nchw_to_nhwc, "nchw_to_nhwc",
                  dict(x=f32(2, 3, 4, 5), Cp=16), {
        "Cp % 16": dict(Cp=24),
        "Cp = 0": dict(Cp=0),
        "C > Cp": dict(x=f32(2, 17, 4, 5)),
        "dtype": dict(x=f32(2, 3, 4, 5).bfloat16()),
        "cpu": dict(x=f32(2, 3, 4, 5, device="cpu")),
    })
    expect_raises(ext.nhwc_to_nchw, "nhwc_to_nchw",
                  dict(x=bf16(2, 4, 5, 16), C=3), {
        "Cp % 16": dict(x=bf16(2, 4, 5, 24)),
        "C > Cp": dict(C=17),
        "C < 0": dict(C=-1),
        "dtype": dict(x=bf16(2, 4, 5, 16).float()),
        "cpu": dict(x=bf16(2, 4, 5, 16, device="cpu")),
    })


def test_normalize_vgg_host_checks(ext):
    expect_raises(ext.normalize_vgg_fwd, "normalize_vgg_fwd",
                  dict(x=f32(2, 3, 4, 5), Cp=16), {
        "channels": dict(x=f32(2, 4, 4, 5)),
        "rank": dict(x=f32(3, 4, 5)),
        "dtype": dict(x=f32(2, 3, 4, 5).bfloat16()),
        "cpu": dict(x=f32(2, 3, 4, 5, device="cpu")),
        "Cp < 3": dict(Cp=2),
    })
    expect_raises(ext.normalize_vgg_bwd, "normalize_vgg_bwd",
                  dict(dy=bf16(2, 4, 5, 16), C=3), {
        "dtype": dict(dy=bf16(2, 4, 5, 16).float()),
        "cpu": dict(dy=bf16(2, 4, 5, 16, device="cpu")),
        "rank": dict(dy=bf16(4, 5, 16)),
        "Cp < 3": dict(dy=bf16(2, 4, 5, 2)),
        "C != 3": dict(C=4),
    })


def test_empty_inputs_return_empty(ext):
    """N = 0: the right shapes come back and nothing is launched (a launch
    with a zero grid is an error)."""
    e4 = [u8(0, 4, 5, 3)] * 4
    assert [tuple(t.shape) for t in ext.build_inputs_u8(*e4)] == \
        [(0, 4, 5, 16)] * 4
    assert [tuple(t.shape) for t in ext.build_inputs(*[f32(0, 3, 4, 5)] * 4)] \
        == [(0, 4, 5, 16)] * 4
    assert ext.u8_to_nhwc(u8(0, 4, 5, 3), 16).shape == (0, 4, 5, 16)
    assert ext.u8_to_nchw(u8(0, 4, 5, 3)).shape == (0, 3, 4, 5)
    assert ext.out_to_u8(bf16(0, 4, 5, 16)).shape == (0, 4, 5, 3)
    assert ext.normalize_nhwc_fwd(bf16(0, 4, 5, 16)).shape == (0, 4, 5, 16)
    assert ext.normalize_nhwc_bwd(bf16(0, 4, 5, 16)).shape == (0, 4, 5, 16)
    assert ext.normalize_vgg_fwd(f32(0, 3, 4, 5), 16).shape == (0, 4, 5, 16)
    assert ext.normalize_vgg_bwd(bf16(0, 4, 5, 16), 3).shape == (0, 3, 4, 5)
    assert ext.nchw_to_nhwc(f32(0, 3, 4, 5), 16).shape == (0, 4, 5, 16)
    assert ext.nhwc_to_nchw(bf16(0, 4, 5, 16), 3).shape == (0, 3, 4, 5)
    # no logical channel: defined, all zero
    assert ext.nhwc_to_nchw(bf16(2, 4, 5, 16), 0).shape == (2, 0, 4, 5)
    assert not ext.nchw_to_nhwc(f32(2, 0, 4, 5), 16).any()
    s = ext.sqdiff255_sum(bf16(0, 4, 5, 16), bf16(0, 4, 5, 16), 3)
    assert s.dtype == torch.float64 and s.item() == 0.0
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    ext.adam_step(f32(0), f32(0), f32(0), f32(0), f32(1), 0.9, 0.999, 1e-8,
                  step)
    assert step.item() == 0, "nothing launched, the counter included"


def test_strided_inputs_are_copied(ext):
    """The wrappers that accept a non-contiguous tensor and copy it give the
    result of the contiguous copy."""
    x = torch.arange(2 * 4 * 5 * 6, dtype=torch.uint8, device=DEV).reshape(
        2, 4, 5, 6)[..., ::2]
    assert not x.is_contiguous()
    xc = x.contiguous()
    assert torch.equal(ext.u8_to_nhwc(x, 16), ext.u8_to_nhwc(xc, 16))
    assert torch.equal(ext.u8_to_nchw(x), ext.u8_to_nchw(xc))
    for a, b in zip(ext.build_inputs_u8(xc, x, xc, x),
                    ext.build_inputs_u8(xc, xc, xc, xc)):
        assert torch.equal(a, b)
    f = xc.float().permute(0, 3, 1, 2)  # (2,3,4,5), channels-last strides
    assert not f.is_contiguous()
    fc = f.contiguous()
    for a, b in zip(ext.build_inputs(fc, f, fc, f),
                    ext.build_inputs(fc, fc, fc, fc)):
        assert torch.equal(a, b)
    assert torch.equal(ext.normalize_vgg_fwd(f, 16),
                       ext.normalize_vgg_fwd(fc, 16))
    assert torch.equal(ext.nchw_to_nhwc(f, 16), ext.nchw_to_nhwc(fc, 16))
    h = ((torch.arange(2 * 4 * 5 * 32, device=DEV) % 7) / 8).bfloat16().reshape(
        2, 4, 5, 32)[..., ::2]
    assert not h.is_contiguous()
    hc = h.contiguous()
    for name in ("normalize_nhwc_fwd", "normalize_nhwc_bwd", "out_to_u8"):
        op = getattr(ext, name)
        assert torch.equal(op(h), op(hc)), name
    assert torch.equal(ext.normalize_vgg_bwd(h, 3),
                       ext.normalize_vgg_bwd(hc, 3))
    assert torch.equal(ext.nhwc_to_nchw(h, 3), ext.nhwc_to_nchw(hc, 3))
