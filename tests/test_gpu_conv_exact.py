"""conv2d_fwd (forward and dgrad) on every dispatch tier, exact on integer
data against a float64 per-tap shifted matmul.

Tiers: k_conv_igemm (BN 16/32/64/128), its split-K form with
k_splitk_finalize<GZ> for every instantiated GZ, and the 8-wave
k_conv_igemm8 with its env-selected variants. Every case first asserts the
tier it runs on (ext.conv2d_fwd_plan), so a change of the dispatch rule
cannot silently move a case off the kernel it is here for.

Data: x in {-1, 0, 1}; weights +-1 with probability
min(2/3, 1000 / (ks^2 * C_in)), else 0; bias an integer in [-8, 8]. Every
partial sum is a small integer, so fp32 accumulation is exact in any order,
and |y| <= 256 (asserted on the reference) is exact in bf16: the kernel must
equal the reference bitwise. sum ~ N(0, 2/3 * 1000) at the longest K, i.e.
sigma ~ 26, so 256 is ~10 sigma away.

Sigmoid cases use density 4 / (ks^2 * C_in) (pre-activations within about
+-8) and atol = 2^-8: one bf16 ulp just below 1.0, against an error budget of
half an ulp of output rounding plus __expf's ~1e-6.

WN_IGEMM8_VAR / WN_IGEMM8_M32 are read once per process, so each variant
runs in one child process (this file executed as a script) that writes the
raw outputs to one .npz; the tests only compare. Inputs are rebuilt from the
case id on both sides.
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
ENV_KNOBS = ("WN_IGEMM8_VAR", "WN_IGEMM8_M32", "WN_IGEMM8_MTHRESH")


def pow2(c):
    p = 16
    while p < c:
        p *= 2
    return p


class Case:
    """One conv2d_fwd call. cin -> cout is the kernel's view: for a dgrad
    case cin is the conv's K (channels of dy) and cout the conv's C."""

    def __init__(self, mode, n, h, w, cin, cout, ks, plan, act=ACT_NONE,
                 bias=False):
        self.mode, self.n, self.h, self.w = mode, n, h, w
        self.cin, self.cout, self.ks = cin, cout, ks
        self.plan, self.act, self.bias = plan, act, bias
        self.id = (f"{mode}-{n}x{h}x{w}-{cin}to{cout}-k{ks}-a{act}"
                   f"{'b' if bias else ''}")

    def with_act(self, act, bias=True):
        return Case(self.mode, self.n, self.h, self.w, self.cin, self.cout,
                    self.ks, self.plan, act, bias)


def fwd(n, h, w, cin, cout, ks, *plan, **kw):
    return Case("fwd", n, h, w, cin, cout, ks, plan, **kw)


def dgrad(n, h, w, cin, cout, ks, *plan, **kw):
    return Case("dgrad", n, h, w, cin, cout, ks, plan, **kw)


# plan = (kernel, BN, gz). Widths make tiles cross image rows and images and
# leave an M tail that is no multiple of 16.
IGEMM = [
    fwd(2, 23, 29, 3, 16, 3, "igemm", 16, 1),     # nk=5: odd on DK=2, KG%32=16
    fwd(2, 23, 29, 32, 3, 3, "igemm", 16, 1),     # nk=9, 13 pad channels
    fwd(2, 23, 29, 6, 32, 5, "igemm", 32, 1),     # nk=13, odd
    fwd(2, 23, 29, 128, 64, 1, "igemm", 64, 1),   # nk=4
    fwd(2, 23, 29, 32, 64, 3, "igemm", 64, 1),    # nk=9
    # long K on the narrow tile (base=321, nk=196), M tail 107
    dgrad(3, 117, 117, 128, 12, 7, "igemm", 16, 1),
    fwd(3, 117, 117, 32, 32, 5, "igemm", 32, 1),  # base=321, nk=25
    fwd(1, 101, 103, 64, 512, 3, "igemm", 128, 1),  # gy=4, base=328, tail 35
]
IGEMM += [IGEMM[1].with_act(ACT_RELU), IGEMM[4].with_act(ACT_RELU)]

SPLITK = [
    fwd(1, 113, 113, 64, 256, 3, "splitk", 128, 2),  # gy=2
    fwd(2, 95, 97, 32, 64, 5, "splitk", 64, 3),
    fwd(1, 121, 125, 6, 32, 7, "splitk", 32, 4),
    fwd(2, 23, 29, 64, 128, 3, "splitk", 128, 4),    # nk=18: slices 4,5,4,5
    fwd(1, 53, 59, 128, 512, 3, "splitk", 128, 5),   # gy=4
    fwd(3, 57, 59, 64, 128, 5, "splitk", 128, 6),
    fwd(1, 89, 100, 128, 3, 3, "splitk", 16, 7),     # pad zeroed in finalize
    fwd(2, 63, 63, 32, 32, 7, "splitk", 32, 8),
    # nk=36: slices of 3, shorter than the 4-tile prologue
    fwd(2, 43, 47, 128, 64, 3, "splitk", 64, 12),
    fwd(2, 23, 29, 128, 128, 5, "splitk", 128, 16),
    fwd(1, 5, 7, 64, 64, 7, "splitk", 64, 16),       # M=35: one block, tail
    # dgrad of 100->128 k5: finalize zeroes 28 pad channels of Cp=128
    dgrad(2, 23, 29, 128, 100, 5, "splitk", 128, 16),
]
SPLITK += [SPLITK[3].with_act(ACT_RELU), SPLITK[6].with_act(ACT_RELU),
           SPLITK[8].with_act(ACT_RELU)]

IGEMM8 = [
    fwd(3, 73, 75, 32, 64, 1, "igemm8", 64, 1),      # nk=1, M tail 41
    fwd(3, 73, 75, 64, 128, 1, "igemm8", 128, 1),    # nk=2
    fwd(1, 127, 131, 128, 64, 1, "igemm8", 64, 1),   # nk=4, M tail 253
    fwd(3, 73, 75, 32, 64, 3, "igemm8", 64, 1),      # nk=9
    fwd(3, 73, 75, 64, 256, 3, "igemm8", 128, 1),    # gy=2, base=258
    fwd(2, 127, 131, 128, 128, 5, "igemm8", 128, 1),  # base=260, nk=100
    dgrad(2, 127, 131, 128, 128, 5, "igemm8", 128, 1),
    fwd(2, 127, 131, 64, 64, 7, "igemm8", 64, 1),    # nk=98
    dgrad(2, 127, 131, 64, 64, 7, "igemm8", 64, 1),
    fwd(2, 127, 131, 64, 128, 3, "igemm8", 128, 1),  # nk=18
    dgrad(3, 73, 75, 3, 64, 3, "igemm8", 64, 1),     # input Kp=16, nk=5
    # dgrad of 100->128 k5: 28 pad channels zeroed at BN >= 64
    dgrad(2, 127, 131, 128, 100, 5, "igemm8", 128, 1),
]
IGEMM8 += [IGEMM8[3].with_act(ACT_RELU), IGEMM8[4].with_act(ACT_RELU)]

# one per epilogue implementation: plain, finalize, igemm8 (the last two
# with pad channels, where sigmoid(0) = 0.5 would show a missing mask)
SIGMOID = [
    fwd(2, 23, 29, 16, 3, 1, "igemm", 16, 1, act=ACT_SIGMOID, bias=True),
    fwd(1, 89, 100, 128, 3, 3, "splitk", 16, 7, act=ACT_SIGMOID, bias=True),
    fwd(2, 127, 131, 128, 100, 5, "igemm8", 128, 1, act=ACT_SIGMOID,
        bias=True),
]

# igemm8 variants: nk=1, gy=2, long K; each plain and with ReLU + bias
VARIANTS = {"var1": {"WN_IGEMM8_VAR": "1"}, "var2": {"WN_IGEMM8_VAR": "2"},
            "var3": {"WN_IGEMM8_VAR": "3"}, "m32": {"WN_IGEMM8_M32": "1"}}
VARIANT_CASES = [IGEMM8[0], IGEMM8[4], IGEMM8[7]]
VARIANT_CASES += [c.with_act(ACT_RELU) for c in VARIANT_CASES]


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


def assert_plan(ext, case):
    for k in ENV_KNOBS:
        assert k not in os.environ, f"{k} is set: not the default dispatch"
    plan = tuple(ext.conv2d_fwd_plan(case.n, case.h, case.w, pow2(case.cin),
                                     pow2(case.cout), case.ks))
    assert plan == case.plan, f"{case.id}: runs on {plan}, meant {case.plan}"


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
        f"{case.id} {case.plan}: {len(bad)} of {got.numel()} differ; first "
        f"(n,y,x,k)={tuple(bad[0].tolist())} {what}")
    pad = y[..., K:]
    if pad.numel():
        nz = (pad != 0).nonzero()
        assert len(nz) == 0, (
            f"{case.id}: {len(nz)} pad outputs non-zero; first (n,y,x,k-K)="
            f"{tuple(nz[0].tolist())} = {pad[tuple(nz[0].tolist())].item()}")


ALL = IGEMM + SPLITK + IGEMM8 + SIGMOID
BY_ID = {c.id: c for c in ALL + VARIANT_CASES}
assert len({c.id for c in ALL}) == len(ALL)


# ---------------------------------------------------------------------------
# child process: one igemm8 variant, raw bf16 bits of every output
# ---------------------------------------------------------------------------

def _child(out_path):
    sys.path.insert(0, str(REPO))
    from waternet_amd.ops import ext as _ext

    ext = _ext()
    res = {}
    for case in VARIANT_CASES:
        res[case.id] = run_kernel(ext, case).view(torch.int16).cpu().numpy()
    np.savez(out_path, **res)


if __name__ == "__main__":
    _child(sys.argv[1])
    sys.exit(0)


# ---------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ext():
    from waternet_amd.ops import ext as _ext

    return _ext()


def _ids(cases):
    return [c.id for c in cases]


@pytest.mark.parametrize("case", IGEMM, ids=_ids(IGEMM))
def test_igemm_exact(ext, case):
    assert_plan(ext, case)
    check(case, run_kernel(ext, case))


@pytest.mark.parametrize("case", SPLITK, ids=_ids(SPLITK))
def test_splitk_exact(ext, case):
    assert_plan(ext, case)
    check(case, run_kernel(ext, case))


@pytest.mark.parametrize("case", IGEMM8, ids=_ids(IGEMM8))
def test_igemm8_exact(ext, case):
    assert_plan(ext, case)
    check(case, run_kernel(ext, case))


@pytest.mark.parametrize("case", SIGMOID, ids=_ids(SIGMOID))
def test_sigmoid_epilogue(ext, case):
    assert_plan(ext, case)
    check(case, run_kernel(ext, case))


def test_tier_coverage():
    """The tables above reach every tier the dispatch rule can choose."""
    plans = {c.plan for c in ALL if c.act != ACT_SIGMOID}
    assert {("igemm", bn, 1) for bn in (16, 32, 64, 128)} <= plans
    assert ({gz for k, _, gz in plans if k == "splitk"}
            == {2, 3, 4, 5, 6, 7, 8, 12, 16})
    assert {bn for k, bn, _ in plans if k == "splitk"} == {16, 32, 64, 128}
    for mode in ("fwd", "dgrad"):
        assert {c.plan[1] for c in IGEMM8 if c.mode == mode} == {64, 128}
    assert any(pow2(c.cout) > 128 for c in IGEMM8)  # gy = 2


_variant_cache = {}


def _variant_outputs(name):
    """Outputs of the variant's child, started once (a failed child is not
    started again: its error is what every later case reports)."""
    if name not in _variant_cache:
        try:
            _variant_cache[name] = _run_variant_child(name)
        except BaseException as e:  # noqa: BLE001 - re-raised per case
            _variant_cache[name] = e
    res = _variant_cache[name]
    if isinstance(res, BaseException):
        raise res
    return res


def _run_variant_child(name):
    import tempfile

    out = Path(tempfile.mkdtemp(prefix="igemm8var")) / f"{name}.npz"
    env = {k: v for k, v in os.environ.items() if k not in ENV_KNOBS}
    env.update(VARIANTS[name])
    r = subprocess.run(
        [sys.executable, str(Path(__file__).resolve()), str(out)],
        env=env, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = dict(np.load(out))
    out.unlink()
    out.parent.rmdir()
    return res


@pytest.mark.parametrize("case", VARIANT_CASES, ids=_ids(VARIANT_CASES))
@pytest.mark.parametrize("name", list(VARIANTS))
def test_igemm8_variant_exact(ext, name, case):
    """k_conv_igemm8<BN, KS, VAR 1/2/3> and <.., M32>. The children run one
    after another: each is started by the first test that needs it."""
    assert_plan(ext, case)
    bits = _variant_outputs(name)[case.id]
    check(case, torch.from_numpy(bits).to(DEV).view(torch.bfloat16))
