"""k_conv_tile (the tile-resident conv fwd/dgrad tier for the deep k3 layers),
exact on integer data against a float64 per-tap shifted matmul: the method of
test_gpu_conv_patch_exact.py, whose helpers are copied here.

Data: x in {-1, 0, 1}; weights +-1 with probability
min(2/3, 1000 / (9 * C_in)), else 0; bias an integer in [-8, 8]. Every
partial sum is a small integer, so fp32 accumulation is exact in any order
and |y| <= 256 (asserted on the reference) is exact in bf16: the kernel must
equal the reference bitwise whatever its chunking, and pad channels must be
zero. Sigmoid cases use density 4 / (9 * C_in) and atol = 2^-8 (one bf16 ulp
just below 1.0).

Shapes are the smallest the tier accepts. 14x14 tiles: one tile (N=1, 14x14);
N=2 at 28x14 and N=1 at 14x42 (H != W, tiles at every image edge, an
interior tile, two images); N=3 at 28x28. 7x7 images, four to a tile: N=1 (a
partly filled tile), 4 (a full one), 5 (a full one and a tail). Channels:
Cp 128 / 256 / 512 are 1 / 2 / 4 chunks of 128 (2 / 4 / 8 of 64: the direct
epilogue and k_splitk_finalize<2,4,8>), Kp 128 and 256 (two N blocks).

WN_CONV_TILE is read once per process, and batches this small are off by
default (conv_tile_wins in conv_fwd.hip lists classes measured at N = 16), so
the exact cases run in children: "forced" (WN_CONV_TILE=1: 128-channel chunks
unless the table says otherwise), "cc64" (the bench-only WN_CONV_TILE_CC=64:
64-channel chunks), and "off" (WN_CONV_TILE=0: the present tiers). Every child
asserts the plan per case, runs each case twice and asserts identical bits,
and writes the raw outputs to one .npz; the tests only compare. Two
default-on shapes run in this process as well.

Random-normal data (test_random_within_derived_bound): against a float64 CPU
conv of the bf16-rounded inputs every output must lie within half a bf16 ulp
of the reference value plus the fp32 accumulation bound n * 2^-24 * sum|x*w|
with n = 9 * Cp terms (each of the n - 1 additions and the n products'
roundings contributes at most 2^-24 relative to a partial sum that is at most
sum|x*w|; the slab sums of the finalize pass are among those additions). The
split-K tier (the "off" child) must pass the same check.
"""

import functools
import os
import subprocess
import sys
import zlib
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
DEV = "cuda:0"
ACT_NONE, ACT_RELU, ACT_SIGMOID = 0, 1, 2
ENV_KNOBS = ("WN_CONV_TILE", "WN_CONV_TILE_CC", "WN_CONV_PATCH",
             "WN_IGEMM8_VAR", "WN_IGEMM8_M32", "WN_IGEMM8_MTHRESH")
# The default dispatch of the flagship shapes (bs 16 at 112^2), pinned:
# (N, H, W, Cp, Kp) -> plan. The classes and widths that won the per-shape A/B
# (docs/KERNELS.md, k_conv_tile table); 7^2 lost and keeps split-K.
FLAGSHIP_PLANS = {
    (16, 56, 56, 128, 128): ("tile", 128, 1),
    (16, 28, 28, 128, 256): ("tile", 128, 1),
    (16, 28, 28, 256, 128): ("tile", 128, 4),
    (16, 28, 28, 256, 256): ("tile", 128, 2),
    (16, 14, 14, 256, 512): ("tile", 128, 4),
    (16, 14, 14, 512, 256): ("tile", 128, 8),
    (16, 14, 14, 512, 512): ("tile", 128, 4),
    (16, 7, 7, 512, 512): ("splitk", 128, 16),
}


def pow2(c):
    p = 16
    while p < c:
        p *= 2
    return p


def default_cc(n, h, w, cp, kp):
    """Chunk width the default dispatch runs a shape at, 0 where it keeps its
    tier: read off FLAGSHIP_PLANS (classes are on from N = 16)."""
    plan = FLAGSHIP_PLANS.get((16, h, w, cp, kp), ("", 0, 0))
    return cp // plan[2] if n >= 16 and plan[0] == "tile" else 0


class Case:
    """One conv2d_fwd call, ks = 3. cin -> cout is the kernel's view: for a
    dgrad case cin is the conv's K (channels of dy) and cout the conv's C."""

    ks = 3

    def __init__(self, mode, n, h, w, cin, cout, act=ACT_NONE, bias=False,
                 data="int"):
        self.mode, self.n, self.h, self.w = mode, n, h, w
        self.cin, self.cout, self.act, self.bias = cin, cout, act, bias
        self.data = data
        self.id = (f"{mode}-{n}x{h}x{w}-{cin}to{cout}-a{act}"
                   f"{'b' if bias else ''}{'-rnd' if data != 'int' else ''}")

    @property
    def shape(self):
        return (self.n, self.h, self.w, pow2(self.cin), pow2(self.cout))


S14 = [(1, 14, 14), (2, 28, 14), (1, 14, 42), (3, 28, 28)]
S7 = [(1, 7, 7), (4, 7, 7), (5, 7, 7)]

CASES = []
for _sp in S14 + S7:
    for _cin, _cout in ((128, 128), (256, 256), (512, 128)):
        CASES.append(Case("fwd", *_sp, _cin, _cout))
    CASES.append(Case("dgrad", *_sp, 256, 256))
for _sp in ((3, 28, 28), (5, 7, 7)):
    CASES.append(Case("dgrad", *_sp, 128, 128))
    CASES.append(Case("dgrad", *_sp, 512, 256))
    # ReLU + bias on the direct and on the finalize epilogue
    CASES.append(Case("fwd", *_sp, 128, 128, ACT_RELU, True))
    CASES.append(Case("fwd", *_sp, 512, 128, ACT_RELU, True))
    # cout 100 -> Kp 128: 28 pad channels must be exactly zero; sigmoid(0) =
    # 0.5 would show a missing mask (direct, then finalize epilogue)
    CASES.append(Case("fwd", *_sp, 128, 100, ACT_SIGMOID, True))
    CASES.append(Case("fwd", *_sp, 256, 100, ACT_SIGMOID, True))
    CASES.append(Case("dgrad", *_sp, 256, 100))
# default-on shapes (N = 16): run in this process too; 128-channel chunks
# with finalize<4>, 64-channel chunks with finalize<8>
DEFAULT_ON = [Case("fwd", 16, 14, 14, 512, 512, ACT_RELU, True),
              Case("dgrad", 16, 14, 14, 512, 256)]
CASES += DEFAULT_ON
# random-normal data
RANDOM = [Case("fwd", 2, 14, 14, 512, 512, data="normal"),
          Case("fwd", 2, 28, 28, 256, 256, data="normal")]

BY_ID = {c.id: c for c in CASES + RANDOM}
assert len(BY_ID) == len(CASES) + len(RANDOM)


# ---------------------------------------------------------------------------
# inputs, reference, kernel call
# ---------------------------------------------------------------------------

def make_inputs(case):
    """x (N,H,W,cin) and conv weights (K,C,3,3) as fp32, bias (cout,) or
    None. A dgrad case's weights are (cin, cout, 3, 3)."""
    rng = np.random.default_rng(zlib.crc32(case.id.encode()))
    wshape = ((case.cout, case.cin) if case.mode == "fwd"
              else (case.cin, case.cout)) + (3, 3)
    if case.data == "normal":  # bf16-representable normal draws
        x = rng.standard_normal((case.n, case.h, case.w, case.cin))
        w = rng.standard_normal(wshape) / np.sqrt(9.0 * case.cin)
        rnd = lambda a: torch.from_numpy(a).float().bfloat16().float().numpy()
        return rnd(x), rnd(w), None
    L = 9 * case.cin
    dens = 4.0 / L if case.act == ACT_SIGMOID else min(2.0 / 3.0, 1000.0 / L)
    x = rng.integers(-1, 2, size=(case.n, case.h, case.w, case.cin))
    w = rng.choice([-1, 1], size=wshape) * (rng.random(wshape) < dens)
    b = None
    if case.bias:
        lim = 2 if case.act == ACT_SIGMOID else 8
        b = rng.integers(-lim, lim + 1, size=(case.cout,)).astype(np.float32)
    return x.astype(np.float32), w.astype(np.float32), b


def shifted_matmul(case, x, w, b, dev):
    """Pre-activation y (N,H,W,cout) in float64.
    fwd:   y[n,y,x,k]  = b[k] + sum x[n, y+r-1, x+s-1, c] * w[k,c,r,s]
    dgrad: dx[n,y,x,c] = sum dy[n, y-(r-1), x-(s-1), k] * w[k,c,r,s]"""
    n, h, wd = case.n, case.h, case.w
    xp = torch.zeros(n, h + 2, wd + 2, case.cin, dtype=torch.float64,
                     device=dev)
    xp[:, 1:1 + h, 1:1 + wd] = torch.from_numpy(x).to(dev)
    w64 = torch.from_numpy(w).to(dev).double()
    y = torch.zeros(n, h, wd, case.cout, dtype=torch.float64, device=dev)
    for r in range(3):
        for s in range(3):
            if case.mode == "fwd":
                y += xp[:, r:r + h, s:s + wd] @ w64[:, :, r, s].T
            else:
                y += xp[:, 2 - r:2 - r + h, 2 - s:2 - s + wd] @ w64[:, :, r, s]
    if b is not None:
        y += torch.from_numpy(b).to(dev).double()
    return y


@functools.lru_cache(maxsize=None)
def reference(cid):
    case = BY_ID[cid]
    return shifted_matmul(case, *make_inputs(case), DEV)


def run_kernel(ext, case):
    """The call ops/conv.py makes; returns y (N,H,W,Kp) bf16."""
    x, w, b = make_inputs(case)
    Cp, Kp = pow2(case.cin), pow2(case.cout)
    xg = torch.zeros(case.n, case.h, case.w, Cp, dtype=torch.bfloat16,
                     device=DEV)
    xg[..., :case.cin] = torch.from_numpy(x).to(DEV).bfloat16()
    wg = torch.from_numpy(w).to(DEV).contiguous()
    bg = None if b is None else torch.from_numpy(b).to(DEV)
    if case.mode == "fwd":
        wp = ext.pack_weight_fwd(wg, Kp, Cp)
    else:  # conv's (Kp, Cp) = kernel's (Cp, Kp)
        wp = ext.pack_weight_dgrad(wg, Cp, Kp)
    y = ext.conv2d_fwd(xg, wp, bg, 3, Kp, case.cout, case.act)
    torch.cuda.synchronize()
    return y


def plan_of(ext, case):
    n, h, w, cp, kp = case.shape
    return tuple(ext.conv2d_fwd_plan(n, h, w, cp, kp, 3))


def check(case, y):
    ref = reference(case.id)
    # a condition on the inputs, not on the kernel
    assert ref.abs().max().item() <= 256
    K = case.cout
    assert y.shape == (case.n, case.h, case.w, pow2(K))
    got = y[..., :K].double()
    if case.act == ACT_SIGMOID:
        err = (got - torch.sigmoid(ref)).abs()
        bad = (err > 2.0 ** -8).nonzero()
        what = f"max err {err.max().item():.3g}"
    else:
        want = ref.clamp_min(0) if case.act == ACT_RELU else ref
        bad = (got != want).nonzero()
        what = "exact"
        if len(bad):
            i = tuple(bad[0].tolist())
            what = f"got {got[i].item()} want {want[i].item()}"
        else:
            assert torch.equal(got, want)
    assert len(bad) == 0, (
        f"{case.id}: {len(bad)} of {got.numel()} differ; first "
        f"(n,y,x,k)={tuple(bad[0].tolist())} {what}")
    pad = y[..., K:]
    if pad.numel():
        nz = (pad != 0).nonzero()
        assert len(nz) == 0, (
            f"{case.id}: {len(nz)} pad outputs non-zero; first (n,y,x,k-K)="
            f"{tuple(nz[0].tolist())} = {pad[tuple(nz[0].tolist())].item()}")


# ---------------------------------------------------------------------------
# child process: one knob setting, raw bf16 bits of every output
# ---------------------------------------------------------------------------

# child name -> (environment, its cases, on the tile tier?). A forced shape
# runs at WN_CONV_TILE_CC, else at the table's chunk width, else at 128.
CHILDREN = {
    "forced": ({"WN_CONV_TILE": "1"}, CASES + RANDOM, True),
    "cc64": ({"WN_CONV_TILE": "1", "WN_CONV_TILE_CC": "64"}, CASES, True),
    "off": ({"WN_CONV_TILE": "0"}, DEFAULT_ON + RANDOM, False),
}


def _child(name, out_path):
    sys.path.insert(0, str(REPO))
    from waternet_amd.ops import ext as _ext

    ext = _ext()
    env, cases, tile = CHILDREN[name]
    for k, v in env.items():
        assert os.environ.get(k) == v
    res = {}
    for case in cases:
        plan = plan_of(ext, case)
        if tile:
            cc = (int(env.get("WN_CONV_TILE_CC", 0))
                  or default_cc(*case.shape) or 128)
            assert plan == ("tile", 128, pow2(case.cin) // cc), (case.id, plan)
        else:
            assert plan[0] == "splitk", (case.id, plan)
        y = run_kernel(ext, case).view(torch.int16).cpu().numpy()
        again = run_kernel(ext, case).view(torch.int16).cpu().numpy()
        assert np.array_equal(y, again), f"{case.id}: bits differ on repeat"
        res[case.id] = y
    np.savez(out_path, **res)


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
    sys.exit(0)


_child_cache = {}


def _child_outputs(name):
    """Outputs of the child, started once (a failed child is not started
    again: its error is what every later case reports)."""
    if name not in _child_cache:
        try:
            _child_cache[name] = _run_child(name)
        except BaseException as e:  # noqa: BLE001 - re-raised per case
            _child_cache[name] = e
    res = _child_cache[name]
    if isinstance(res, BaseException):
        raise res
    return res


def _run_child(name):
    import tempfile

    out = Path(tempfile.mkdtemp(prefix="convtile")) / f"{name}.npz"
    env = {k: v for k, v in os.environ.items() if k not in ENV_KNOBS}
    env.update(CHILDREN[name][0])
    r = subprocess.run(
        [sys.executable, str(Path(__file__).resolve()), name, str(out)],
        env=env, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = dict(np.load(out))
    out.unlink()
    out.parent.rmdir()
    return res


def _bf16(bits):
    return torch.from_numpy(bits).to(DEV).view(torch.bfloat16)


# ---------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ext():
    from waternet_amd.ops import ext as _ext

    return _ext()


def _ids(cases):
    return [c.id for c in cases]


def _default_env():
    for k in ENV_KNOBS:
        assert k not in os.environ, f"{k} is set: not the default dispatch"


def test_case_coverage():
    """Every spatial shape x 1 / 2 / 4 chunks forward, dgrad on every spatial
    shape, two N blocks, pad channels and both activations on both
    epilogues."""
    for sp in S14 + S7:
        here = [c for c in CASES if (c.n, c.h, c.w) == sp]
        assert {c.cin for c in here if c.mode == "fwd"} >= {128, 256, 512}
        assert any(c.mode == "dgrad" for c in here)
    assert any(pow2(c.cout) == 256 for c in CASES)
    for cin in (128, 256):  # direct / finalize
        assert {c.act for c in CASES if c.cin == cin and c.cout == 100} >= {2}
    assert {(c.cin > 128) for c in CASES if c.act == ACT_RELU} == {False, True}


def test_ineligible_shapes_keep_their_tier(ext):
    """H or W no multiple of 14, Cp = 64, Kp = 64, KS = 5, a patch-eligible
    shape, batches under 16 and classes that were not measured: not the tile
    tier by default. The plans other test files pin stay."""
    _default_env()
    for n, h, w, cp, kp, ks in ((16, 28, 30, 256, 256, 3),
                                (16, 20, 28, 256, 256, 3),
                                (16, 16, 16, 512, 512, 3),
                                (16, 56, 56, 64, 128, 3),
                                (16, 56, 56, 128, 64, 3),
                                (16, 28, 28, 128, 128, 5),
                                (16, 28, 28, 256, 256, 1),
                                (15, 14, 14, 512, 512, 3),
                                (3, 28, 28, 256, 256, 3),
                                (16, 28, 14, 256, 256, 3),
                                (16, 42, 42, 256, 256, 3),
                                (16, 56, 56, 256, 256, 3),
                                (16, 28, 28, 512, 512, 3),
                                (64, 7, 7, 512, 512, 3)):
        assert ext.conv2d_fwd_plan(n, h, w, cp, kp, ks)[0] != "tile"
    assert tuple(ext.conv2d_fwd_plan(16, 112, 112, 128, 128, 3)) == (
        "patch", 128, 1)
    assert tuple(ext.conv2d_fwd_plan(1, 113, 113, 64, 256, 3)) == (
        "splitk", 128, 2)
    assert tuple(ext.conv2d_fwd_plan(1, 53, 59, 128, 512, 3)) == (
        "splitk", 128, 5)
    assert tuple(ext.conv2d_fwd_plan(2, 96, 96, 64, 128, 3)) == (
        "splitk", 128, 3)


def test_default_plans_follow_the_table(ext):
    """The flagship shapes run the pinned plans, at N = 16 and above; every
    small test case keeps its present tier by default."""
    _default_env()
    for shape, want in FLAGSHIP_PLANS.items():
        assert tuple(ext.conv2d_fwd_plan(*shape, 3)) == want, shape
        if want[0] == "tile":
            big = (32,) + shape[1:]
            assert tuple(ext.conv2d_fwd_plan(*big, 3)) == want, big
    for case in CASES:
        if case not in DEFAULT_ON:
            assert plan_of(ext, case)[0] == "splitk", case.id


@pytest.mark.parametrize("child", ["forced", "cc64"])
@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_tile_exact(case, child):
    """Forced onto the tile tier in a child (which asserts the plan and the
    repeatability per case): exact, pads zero."""
    _default_env()
    bits = _child_outputs(child)[case.id]
    check(case, _bf16(bits))


@pytest.mark.parametrize("case", DEFAULT_ON, ids=_ids(DEFAULT_ON))
def test_tile_default_exact(ext, case):
    """Default-on grids in this process: the tile plan, exact, identical bits
    on a second call, and (exact sums, shared epilogue) the bits of the
    split-K tier (a child with WN_CONV_TILE=0)."""
    _default_env()
    cc = default_cc(*case.shape)
    assert cc and plan_of(ext, case) == ("tile", 128, pow2(case.cin) // cc)
    y = run_kernel(ext, case)
    check(case, y)
    bits = y.view(torch.int16).cpu().numpy()
    assert np.array_equal(
        bits, run_kernel(ext, case).view(torch.int16).cpu().numpy())
    assert np.array_equal(bits, _child_outputs("off")[case.id])


@functools.lru_cache(maxsize=None)
def _random_reference(cid):
    """(ref, bound) on the CPU in float64 from the bf16-rounded inputs."""
    case = BY_ID[cid]
    x, w, _ = make_inputs(case)
    ref = shifted_matmul(case, x, w, None, "cpu")
    mag = shifted_matmul(case, np.abs(x), np.abs(w), None, "cpu")
    n_terms = 9 * pow2(case.cin)
    # half a bf16 ulp (8 significand bits) of the reference value
    half_ulp = torch.exp2(torch.floor(torch.log2(
        ref.abs().clamp_min(2.0 ** -126))) - 8)
    return ref, half_ulp + n_terms * 2.0 ** -24 * mag


@pytest.mark.parametrize("child", ["forced", "off"])
@pytest.mark.parametrize("case", RANDOM, ids=_ids(RANDOM))
def test_random_within_derived_bound(case, child):
    """Random-normal data on the tile tier and, so that the bound is seen
    not to be vacuous, on the split-K tier."""
    _default_env()
    ref, bound = _random_reference(case.id)
    got = _bf16(_child_outputs(child)[case.id]).cpu().double()
    assert got.shape == ref.shape
    err = (got - ref).abs()
    worst = (err / bound).max().item()
    print(f"{case.id} [{child}]: max err {err.max().item():.3g}, "
          f"max err/bound {worst:.3g}")
    assert torch.isfinite(got).all()
    assert worst <= 1.0, f"{case.id} [{child}]: err/bound {worst:.4g}"
