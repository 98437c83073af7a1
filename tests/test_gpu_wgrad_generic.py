"""k_conv_wgrad, the generic MFMA weight-gradient kernel, bitwise against an
fp32 unfold-matmul reference on integer data.

k_conv_wgrad is the default for every k1 layer and for every channel pair
outside the patch classes, and WN_WGRAD_PATCH=0 selects it everywhere. Both
WN_WGRAD_PATCH and WN_WGRAD_M32 are read once per process, so the kernels run
in two child processes (this file executed as a script): child A with
WN_WGRAD_PATCH=0 (32x32x16 MFMA for BK >= 32) and child B with
WN_WGRAD_PATCH=0 WN_WGRAD_M32=0 (16x16x32 MFMA everywhere). Each child runs
its cases once and writes one .npz with every dW and the plan
conv2d_wgrad_plan reported for it; the tests only compare. Every case first
asserts the plan (kernel, BK, gx, gy, gz) it claims to exercise.

Inputs are integers in [-3, 3], so every partial sum is an integer of
magnitude <= 9 * M; the largest M here is 82,944, giving 746,496 < 2^24, so
fp32 accumulation is exact in any order and dW must equal the reference
bitwise.
"""

import functools
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import pytest
import torch

from wgrad_exact import make_dw0, make_inputs, pow2, reference

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
CH = 64  # k_conv_wgrad's m rows per chunk
ENV_ONCE = ("WN_WGRAD_PATCH", "WN_WGRAD_M32")  # read once per process

# Every (KS, BK) with tails. 2x5x19: M = 190 = three chunks with a 62-row
# tail, non-power-of-two divisors for the magic division, and k7's dy halo
# leaves the image on both sides. (C, K, BK, gx); KG = KS^2 * Cp, so the
# 6 -> 12 row has KG = 16 / 144 / 400 / 784 (a partly filled or 16-wide last
# rsc tile) and 32 -> 200 has gx = 2 with the K tail inside the second k-tile.
TAIL_NHW = (2, 5, 19)
TAIL_CK = [(6, 12, 16, 1), (24, 20, 32, 1), (40, 64, 64, 1),
           (128, 128, 128, 1), (32, 200, 128, 2)]
KSS = [1, 3, 5, 7]

# The double-buffered chunk loop: the smallest M at which a block owns two
# and three chunks. (ks, C, K, (N, H, W), split, chunks, chunks per block)
CHUNK = [
    (7, 128, 128, (3, 24, 28), 13, 32, {2, 3}),    # 32-row tail
    (1, 128, 64, (4, 144, 144), 640, 1296, {2, 3}),  # cmg.conv4
    (1, 256, 256, (2, 72, 72), 160, 162, {1, 2}),
    (3, 32, 64, (2, 84, 84), 213, 221, {1, 2}),    # off-class: default generic
    (5, 12, 12, (2, 72, 72), 160, 162, {1, 2}),    # BK = 16
]
CHUNK_B = CHUNK[:2]  # these run on the 16x16x32 path too
DEFAULT_GENERIC = [c for c in CHUNK if c[0] == 1 or (c[1], c[2]) == (32, 64)]

# one partial chunk, image smaller than the kernel
SMALL = (7, 64, 64, (1, 3, 5))

# pre-filled dW comes back as dW0 + grad
ACC = [(1, 128, 64, (2, 5, 19)), (5, 12, 12, (2, 72, 72))]


def cid_of(kind, ks, C, K, nhw):
    return f"{kind}-k{ks}-c{C}-k{K}-n{nhw[0]}h{nhw[1]}w{nhw[2]}"


def child_cases(which):
    """(kind, ks, C, K, nhw) of everything child `which` runs."""
    out = []
    for ks in KSS:
        for C, K, BK, _ in TAIL_CK:
            if which == "A" or BK >= 32:
                out.append(("tail", ks, C, K, TAIL_NHW))
    for ks, C, K, nhw, *_ in (CHUNK if which == "A" else CHUNK_B):
        out.append(("chunk", ks, C, K, nhw))
    if which == "A":
        out.append(("small",) + SMALL)
        out += [("acc",) + a for a in ACC]
    return out


@functools.lru_cache(maxsize=None)
def want(kind, ks, C, K, nhw):
    """The expected dW of a case, computed once and shared by both children's
    tests; treated as read-only."""
    cid = cid_of(kind, ks, C, K, nhw)
    dy, x = make_inputs(cid, C, K, nhw[1], nhw[2], True, n=nhw[0])
    ref = reference(dy, x, ks, np.float32)
    if kind == "acc":
        ref = make_dw0(cid, ks, C, K) + ref
    ref.setflags(write=False)
    return ref


# ---------------------------------------------------------------------------
# child process: run every case on the GPU, save the results
# ---------------------------------------------------------------------------

def _child(out_path, which):
    sys.path.insert(0, str(REPO))
    from waternet_amd.ops import ext as _ext

    ext = _ext()
    t0 = time.perf_counter()
    res = {}
    for kind, ks, C, K, nhw in child_cases(which):
        cid = cid_of(kind, ks, C, K, nhw)
        n, H, W = nhw
        Cp, Kp = pow2(C), pow2(K)
        dy, x = make_inputs(cid, C, K, H, W, True, n=n)
        xg = torch.zeros(n, H, W, Cp, dtype=torch.bfloat16, device="cuda")
        xg[..., :C] = torch.from_numpy(x).cuda().bfloat16()
        dyg = torch.zeros(n, H, W, Kp, dtype=torch.bfloat16, device="cuda")
        dyg[..., :K] = torch.from_numpy(dy).cuda().bfloat16()
        if kind == "acc":
            dw = torch.from_numpy(make_dw0(cid, ks, C, K)).cuda().contiguous()
        else:
            dw = torch.zeros(K, C, ks, ks, dtype=torch.float32, device="cuda")
        plan = ext.conv2d_wgrad_plan(n, H, W, Cp, Kp, K, ks)
        ext.conv2d_wgrad(dyg, xg, dw, ks)
        torch.cuda.synchronize()
        res[cid] = dw.cpu().numpy()
        res[cid + "/kernel"] = np.array(plan[0])
        res[cid + "/grid"] = np.array(plan[1:], dtype=np.int64)
    res["seconds"] = np.array(time.perf_counter() - t0)
    np.savez(out_path, **res)


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
    sys.exit(0)


# ---------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------

# Measured on the MI355X: a child takes CHILD_SECONDS from interpreter start
# to exit, nearly all of it the cold extension load; the limit is 10 x that.
CHILD_SECONDS = 3
CHILD_TIMEOUT = 10 * CHILD_SECONDS


def _spawn(tmp, which):
    out = tmp / f"wgrad_generic_{which}.npz"
    env = dict(os.environ, WN_WGRAD_PATCH="0")
    env.pop("WN_WGRAD_M32", None)
    if which == "B":
        env["WN_WGRAD_M32"] = "0"
    t0 = time.perf_counter()
    r = subprocess.run(
        [sys.executable, str(Path(__file__).resolve()), str(out), which],
        env=env, cwd=REPO, capture_output=True, text=True,
        timeout=CHILD_TIMEOUT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = dict(np.load(out))
    print(f"child {which}: {time.perf_counter() - t0:.1f} s in all, "
          f"{float(got['seconds']):.2f} s in its cases")
    return got


@pytest.fixture(scope="module")
def child_a(tmp_path_factory):
    return _spawn(tmp_path_factory.mktemp("wgg_a"), "A")


@pytest.fixture(scope="module")
def child_b(tmp_path_factory):
    return _spawn(tmp_path_factory.mktemp("wgg_b"), "B")


def chunks_per_block(nhw, gz):
    """Chunks each of the gz split-m blocks runs: block z takes chunks z,
    z + gz, ..."""
    n_chunks = -(-(nhw[0] * nhw[1] * nhw[2]) // CH)
    return {len(range(z, n_chunks, gz)) for z in range(gz)}


def assert_plan(got, which, kind, ks, C, K, nhw, BK, gx, gz):
    """The child launched k_conv_wgrad<ks, BK, 64, M32> on (gx, gy, gz)."""
    cid = cid_of(kind, ks, C, K, nhw)
    m32 = which == "A" and BK >= 32
    assert str(got[cid + "/kernel"]) == ("generic" if m32 else "generic16")
    gy = -(-(ks * ks * pow2(C)) // 128)
    assert got[cid + "/grid"].tolist() == [BK, gx, gy, gz], cid
    return (ks, BK, m32)


def assert_exact(got, kind, ks, C, K, nhw):
    cid = cid_of(kind, ks, C, K, nhw)
    ref = want(kind, ks, C, K, nhw)
    out = got[cid]
    bad = np.argwhere(out != ref)
    assert bad.size == 0, (
        f"{cid}: {len(bad)} of {ref.size} differ; first (k,c,r,s)={bad[0]} "
        f"got {out[tuple(bad[0])]} want {ref[tuple(bad[0])]}")


def test_parent_environment_is_default():
    """The default plans asserted below are those of a process with neither
    once-per-process variable set."""
    for var in ENV_ONCE:
        assert var not in os.environ, var


@pytest.mark.parametrize("C,K,BK,gx", TAIL_CK)
@pytest.mark.parametrize("ks", KSS)
def test_tails_m32(child_a, ks, C, K, BK, gx):
    """Every (KS, BK) of the default path: 32x32x16 MFMA for BK >= 32, the
    16x16x32 path for BK = 16. Three chunks, one per block (split = 3)."""
    assert_plan(child_a, "A", "tail", ks, C, K, TAIL_NHW, BK, gx, 3)
    assert chunks_per_block(TAIL_NHW, 3) == {1}
    assert_exact(child_a, "tail", ks, C, K, TAIL_NHW)


@pytest.mark.parametrize("C,K,BK,gx", [t for t in TAIL_CK if t[2] >= 32])
@pytest.mark.parametrize("ks", KSS)
def test_tails_m16(child_b, ks, C, K, BK, gx):
    """The same for WN_WGRAD_M32=0: the 16x16x32 path at BK >= 32."""
    assert_plan(child_b, "B", "tail", ks, C, K, TAIL_NHW, BK, gx, 3)
    assert_exact(child_b, "tail", ks, C, K, TAIL_NHW)


@pytest.mark.parametrize("ks,C,K,nhw,split,chunks,per_block", CHUNK)
def test_chunk_loop_m32(child_a, ks, C, K, nhw, split, chunks, per_block):
    """Blocks that own two and three chunks: stage(buf ^ 1, next) under the
    MFMAs, the conditional trailing barrier and the buffer flip."""
    assert -(-(nhw[0] * nhw[1] * nhw[2]) // CH) == chunks
    BK = min(pow2(K), 128)
    assert_plan(child_a, "A", "chunk", ks, C, K, nhw, BK, pow2(K) // BK,
                split)
    assert chunks_per_block(nhw, split) == per_block
    assert_exact(child_a, "chunk", ks, C, K, nhw)


@pytest.mark.parametrize("ks,C,K,nhw,split,chunks,per_block", CHUNK_B)
def test_chunk_loop_m16(child_b, ks, C, K, nhw, split, chunks, per_block):
    BK = min(pow2(K), 128)
    assert_plan(child_b, "B", "chunk", ks, C, K, nhw, BK, pow2(K) // BK,
                split)
    assert chunks_per_block(nhw, split) == per_block
    assert_exact(child_b, "chunk", ks, C, K, nhw)


@pytest.mark.parametrize("ks,C,K,nhw,split,chunks,per_block", DEFAULT_GENERIC)
def test_default_plan_is_generic(ks, C, K, nhw, split, chunks, per_block):
    """k1 layers and channel pairs outside the patch classes run
    k_conv_wgrad by default, on the grid the child ran."""
    from waternet_amd.ops import ext

    test_parent_environment_is_default()
    BK = min(pow2(K), 128)
    plan = ext().conv2d_wgrad_plan(*nhw, pow2(C), pow2(K), K, ks)
    assert tuple(plan) == ("generic", BK, pow2(K) // BK,
                           -(-(ks * ks * pow2(C)) // 128), split)


def test_one_partial_chunk_image_smaller_than_kernel(child_a):
    """k7 at 1x3x5: M = 15, one block per tile, every tap's halo leaves the
    image."""
    ks, C, K, nhw = SMALL
    assert_plan(child_a, "A", "small", ks, C, K, nhw, 64, 1, 1)
    assert_exact(child_a, "small", ks, C, K, nhw)


@pytest.mark.parametrize("ks,C,K,nhw", ACC)
def test_accumulates_into_dw(child_a, ks, C, K, nhw):
    """A pre-filled integer dW0 comes back as dW0 + grad."""
    assert str(child_a[cid_of("acc", ks, C, K, nhw) + "/kernel"]) in (
        "generic", "generic16")
    assert_exact(child_a, "acc", ks, C, K, nhw)


def test_tables_cover_every_instantiation(child_a, child_b):
    """The asserted plans reach all 28 k_conv_wgrad<KS, BK, 64, M32>
    instantiations (KS 1/3/5/7 x BK 16/32/64/128 x M32, no M32 at BK = 16),
    and blocks that run 1, 2 and 3 chunks."""
    seen, per_block = set(), set()
    for which, got in (("A", child_a), ("B", child_b)):
        for kind, ks, C, K, nhw in child_cases(which):
            cid = cid_of(kind, ks, C, K, nhw)
            BK, _, _, gz = got[cid + "/grid"].tolist()
            kernel = str(got[cid + "/kernel"])
            assert kernel in ("generic", "generic16"), cid
            seen.add((ks, BK, kernel == "generic"))
            per_block |= chunks_per_block(nhw, gz)
    every = {(ks, BK, m32) for ks in KSS for BK in (16, 32, 64, 128)
             for m32 in (False, True) if BK >= 32 or not m32}
    assert len(every) == 28 and seen == every
    assert {1, 2, 3} <= per_block
