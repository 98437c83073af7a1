"""k_conv_patch (the patch-staged conv fwd/dgrad tier), exact on integer data
against a float64 per-tap shifted matmul: the method of
test_gpu_conv_exact.py, whose helpers are copied here.

Data: x in {-1, 0, 1}; weights +-1 with probability
min(2/3, 1000 / (ks^2 * C_in)), else 0; bias an integer in [-8, 8]. Every
partial sum is a small integer, so fp32 accumulation is exact in any order
and |y| <= 256 (asserted on the reference) is exact in bf16: the kernel must
equal the reference bitwise, and pad channels must be zero. Sigmoid cases use
density 4 / (ks^2 * C_in) and atol = 2^-8 (one bf16 ulp just below 1.0).

Shapes are the smallest the tier accepts: gz == 1 at gy = 1 needs
ceil(M / 128) >= 320. N=3 at 112x144 is 7 x 9 tiles of 16x16 pixels (odd
counts both ways, H != W, three images: a tile-index or image-stride mix-up
shows); N=2 at 144x144 is 9 x 9. With 16-pixel tiles and "same" padding every
edge and corner tile reads its halo from the zero buffer.

WN_CONV_PATCH is read once per process. Classes that are on by default
(DEFAULT_ON, the test's copy of conv_patch_wins in conv_fwd.hip) run in this
process, and once more in a child with WN_CONV_PATCH=0, which must report
igemm8 and produce the same bf16 bits. Classes that are instantiated but off
by default run in a child with WN_CONV_PATCH=1. Each child runs all its cases
and writes the raw outputs to one .npz; the tests only compare.
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
ENV_KNOBS = ("WN_CONV_PATCH", "WN_IGEMM8_VAR", "WN_IGEMM8_M32",
             "WN_IGEMM8_MTHRESH")

# (ks, Cp, Kp) classes the default dispatch sends to k_conv_patch: the same
# list as conv_patch_wins() in conv_fwd.hip.
DEFAULT_ON = frozenset((ks, cp, kp) for ks in (3, 5, 7)
                       for cp in (64, 128) for kp in (64, 128))


def pow2(c):
    p = 16
    while p < c:
        p *= 2
    return p


class Case:
    """One conv2d_fwd call. cin -> cout is the kernel's view: for a dgrad
    case cin is the conv's K (channels of dy) and cout the conv's C."""

    def __init__(self, mode, n, h, w, cin, cout, ks, act=ACT_NONE,
                 bias=False):
        self.mode, self.n, self.h, self.w = mode, n, h, w
        self.cin, self.cout, self.ks = cin, cout, ks
        self.act, self.bias = act, bias
        self.cls = (ks, pow2(cin), pow2(cout))
        self.bn = 128 if pow2(cout) >= 128 else 64
        self.id = (f"{mode}-{n}x{h}x{w}-{cin}to{cout}-k{ks}-a{act}"
                   f"{'b' if bias else ''}")

    def with_act(self, act, bias=True):
        return Case(self.mode, self.n, self.h, self.w, self.cin, self.cout,
                    self.ks, act, bias)


# every instantiated class, fwd and dgrad; Cp = 128 crosses two channel chunks
CASES = []
for _ks in (3, 5, 7):
    for _cin, _cout in ((64, 64), (128, 128), (64, 128), (128, 64)):
        CASES.append(Case("fwd", 3, 112, 144, _cin, _cout, _ks))
        CASES.append(Case("dgrad", 2, 144, 144, _cin, _cout, _ks))
# dgrad of 100->128 k5 (Klog = 100 < Kp = 128): 28 pad channels must be zero
PAD = Case("dgrad", 3, 112, 144, 128, 100, 5)
CASES.append(PAD)
# the epilogue on a shape with pad channels: sigmoid(0) = 0.5 would show a
# missing mask
CASES.append(Case("fwd", 3, 112, 144, 128, 100, 5, ACT_RELU, True))
CASES.append(Case("fwd", 3, 112, 144, 128, 100, 5, ACT_SIGMOID, True))

BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
ON = [c for c in CASES if c.cls in DEFAULT_ON]
FORCED = [c for c in CASES if c.cls not in DEFAULT_ON]


# ---------------------------------------------------------------------------
# inputs, reference, kernel call
# ---------------------------------------------------------------------------

def make_inputs(case):
    """x (N,H,W,cin) and conv weights (K,C,ks,ks) as fp32 integers, bias
    (cout,) or None. A dgrad case's weights are (cin, cout, ks, ks)."""
    rng = np.random.default_rng(zlib.crc32(case.id.encode()))
    L = case.ks * case.ks * case.cin
    dens = 4.0 / L if case.act == ACT_SIGMOID else min(2.0 / 3.0, 1000.0 / L)
    x = rng.integers(-1, 2, size=(case.n, case.h, case.w, case.cin))
    wshape = ((case.cout, case.cin) if case.mode == "fwd"
              else (case.cin, case.cout)) + (case.ks, case.ks)
    w = rng.choice([-1, 1], size=wshape) * (rng.random(wshape) < dens)
    b = None
    if case.bias:
        lim = 2 if case.act == ACT_SIGMOID else 8
        b = rng.integers(-lim, lim + 1, size=(case.cout,)).astype(np.float32)
    return x.astype(np.float32), w.astype(np.float32), b


@functools.lru_cache(maxsize=None)
def reference(cid):
    """Pre-activation y (N,H,W,cout) in float64 on the device.
    fwd:   y[n,y,x,k]  = b[k] + sum x[n, y+r-P, x+s-P, c] * w[k,c,r,s]
    dgrad: dx[n,y,x,c] = sum dy[n, y-(r-P), x-(s-P), k] * w[k,c,r,s]"""
    case = BY_ID[cid]
    x, w, b = make_inputs(case)
    n, h, wd, ks, P = case.n, case.h, case.w, case.ks, case.ks // 2
    xp = torch.zeros(n, h + 2 * P, wd + 2 * P, case.cin, dtype=torch.float64,
                     device=DEV)
    xp[:, P:P + h, P:P + wd] = torch.from_numpy(x).to(DEV)
    w64 = torch.from_numpy(w).to(DEV).double()
    y = torch.zeros(n, h, wd, case.cout, dtype=torch.float64, device=DEV)
    for r in range(ks):
        for s in range(ks):
            if case.mode == "fwd":
                y += xp[:, r:r + h, s:s + wd] @ w64[:, :, r, s].T
            else:
                rr, ss = 2 * P - r, 2 * P - s
                y += xp[:, rr:rr + h, ss:ss + wd] @ w64[:, :, r, s]
    if b is not None:
        y += torch.from_numpy(b).to(DEV).double()
    return y


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
    y = ext.conv2d_fwd(xg, wp, bg, case.ks, Kp, case.cout, case.act)
    torch.cuda.synchronize()
    return y


def assert_plan(ext, case, kernel):
    plan = tuple(ext.conv2d_fwd_plan(case.n, case.h, case.w, pow2(case.cin),
                                     pow2(case.cout), case.ks))
    assert plan == (kernel, case.bn, 1), (
        f"{case.id}: runs on {plan}, meant {kernel}")


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

# child name -> (WN_CONV_PATCH, its cases, the kernel they must run on)
CHILDREN = {"off": ("0", ON, "igemm8"), "forced": ("1", FORCED, "patch")}


def _child(name, out_path):
    sys.path.insert(0, str(REPO))
    from waternet_amd.ops import ext as _ext

    ext = _ext()
    knob, cases, kernel = CHILDREN[name]
    assert os.environ.get("WN_CONV_PATCH") == knob
    res = {}
    for case in cases:
        assert_plan(ext, case, kernel)
        res[case.id] = run_kernel(ext, case).view(torch.int16).cpu().numpy()
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

    out = Path(tempfile.mkdtemp(prefix="convpatch")) / f"{name}.npz"
    env = {k: v for k, v in os.environ.items() if k not in ENV_KNOBS}
    env["WN_CONV_PATCH"] = CHILDREN[name][0]
    r = subprocess.run(
        [sys.executable, str(Path(__file__).resolve()), name, str(out)],
        env=env, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = dict(np.load(out))
    out.unlink()
    out.parent.rmdir()
    return res


# ---------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ext():
    from waternet_amd.ops import ext as _ext

    return _ext()


def _ids(cases):
    return [c.id for c in cases]


def test_case_coverage():
    """fwd and dgrad of every instantiated class, pad channels, both
    activations; every case is in exactly one of the two groups."""
    for mode in ("fwd", "dgrad"):
        got = {c.cls for c in CASES if c.mode == mode and c.act == ACT_NONE}
        assert got >= {(ks, cp, kp) for ks in (3, 5, 7)
                       for cp in (64, 128) for kp in (64, 128)}
    assert {c.act for c in CASES if c.cout < pow2(c.cout)} == {0, 1, 2}
    assert len(ON) + len(FORCED) == len(CASES)


def test_ineligible_shapes_keep_their_tier(ext):
    """H or W no multiple of 16, an uninstantiated class, or a split-K grid:
    not the patch tier, whatever the class."""
    for k in ENV_KNOBS:
        assert k not in os.environ, f"{k} is set: not the default dispatch"
    for n, h, w, cp, kp, ks in ((3, 112, 150, 64, 64, 7),
                                (3, 120, 144, 64, 64, 7),
                                (3, 112, 144, 32, 64, 5),
                                (3, 112, 144, 64, 256, 3),
                                (3, 112, 144, 64, 64, 1),
                                (2, 96, 96, 128, 128, 5)):
        assert ext.conv2d_fwd_plan(n, h, w, cp, kp, ks)[0] != "patch"


@pytest.mark.parametrize("case", ON, ids=_ids(ON))
def test_patch_default_exact(ext, case):
    """Default-on classes: exact in this process, and bit-identical to
    k_conv_igemm8 (a child with WN_CONV_PATCH=0) on the same inputs."""
    for k in ENV_KNOBS:
        assert k not in os.environ, f"{k} is set: not the default dispatch"
    assert_plan(ext, case, "patch")
    y = run_kernel(ext, case)
    check(case, y)
    # the sums are exact on both sides and the epilogue is shared: same bits
    bits = _child_outputs("off")[case.id]
    assert np.array_equal(y.view(torch.int16).cpu().numpy(), bits)


if FORCED:  # today every class is on by default: nothing to force
    @pytest.mark.parametrize("case", FORCED, ids=_ids(FORCED))
    def test_patch_forced_exact(ext, case):
        """Classes that are instantiated but off by default, forced with
        WN_CONV_PATCH=1 in a child (which asserts the patch plan per
        case)."""
        for k in ENV_KNOBS:
            assert k not in os.environ, f"{k} is set: not the default dispatch"
        assert ext.conv2d_fwd_plan(case.n, case.h, case.w, pow2(case.cin),
                                   pow2(case.cout), case.ks)[0] == "igemm8"
        bits = _child_outputs("forced")[case.id]
        check(case, torch.from_numpy(bits).to(DEV).view(torch.bfloat16))
