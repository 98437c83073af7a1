"""Temporally smoothed WB/CLAHE statistics on the GPU: the stats/apply split
of the preprocess, k_temporal_blend against the NumPy definition
(waternet_amd/data/temporal.py) bit for bit, and the engine option."""

import numpy as np
import pytest
import torch
from temporal_seq import two_scene_sequence

from waternet_amd.data.temporal import (TemporalStabilizer, TemporalState,
                                        scene_cut_count, temporal_blend)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# 64x64; 40x48: 5x6-pixel tiles, non-square; 37x45: odd, through pad8
SHAPES = [(64, 64), (40, 48), (37, 45)]


@pytest.fixture(scope="module")
def ext():
    from waternet_amd.ops import ext as _ext

    return _ext()


def _padded(frames):
    from waternet_amd.engine.inferencer import pad8

    return [pad8(f)[0] for f in frames]


def _stream_a(h, w):
    """8 frames, the scene cut at index 4."""
    return _padded(two_scene_sequence(h, w, per_scene=4, seed=2))


def _stream_b(h, w):
    """8 other frames, bright scene first, the scene cut at index 3."""
    s = two_scene_sequence(h, w, per_scene=5, seed=7, offsets=(150, 30))
    return _padded(s[2:10])


def _dev(frames):
    return torch.from_numpy(np.stack(frames)).to(DEV)


@pytest.mark.parametrize("hw", SHAPES)
def test_stats_then_apply_is_preprocess_all(ext, hw):
    raw = _dev([_stream_a(*hw)[0], _stream_b(*hw)[5]])  # N=2
    want = ext.preprocess_all(raw)
    params, luts, lab, thists = ext.preprocess_stats(raw)
    got = ext.preprocess_apply(raw, lab, params, luts)
    for g, w_ in zip(got, want):
        assert torch.equal(g, w_)
    n, h, w = raw.shape[:3]
    assert params.shape == (n, 3, 2) and params.dtype == torch.float32
    assert luts.shape == (n, 64, 256) and luts.dtype == torch.uint8
    assert thists.shape == (n, 64, 256) and thists.dtype == torch.int32
    # the tile histograms are still the raw counts after the LUT kernel
    # read them: they sum to the L histogram of the LAB image
    for i in range(n):
        g = thists[i].sum(0).cpu().numpy()
        L = lab[i, :, :, 0].cpu().numpy()
        assert np.array_equal(g, np.bincount(L.ravel(), minlength=256))
        assert np.array_equal(lab[i].cpu().numpy(),
                              ext.rgb2lab_u8(raw[i:i + 1])[0].cpu().numpy())


def _blend_against_numpy(ext, streams, hw, alpha=0.3, scene_cut=0.5):
    """Run k_temporal_blend over the streams' frames on the GPU's own
    per-frame statistics and compare every state tensor, after every frame,
    with the NumPy definition run on those same statistics. Returns the
    cut counts."""
    from waternet_amd.ops.preprocess import new_temporal_state

    n = len(streams)
    hp, wp = streams[0][0].shape[:2]
    cut_count = scene_cut_count(scene_cut, hp, wp)
    state = new_temporal_state(n, DEV)
    ref = [TemporalState() for _ in range(n)]
    for t in range(len(streams[0])):
        raw = _dev([s[t] for s in streams])
        params, luts, _, thists = ext.preprocess_stats(raw)
        ext.temporal_blend(state["wb"], state["lut"], state["lhist"],
                           state["counters"], state["lut_u8"], params, luts,
                           thists, alpha, cut_count)
        got = {k: v.cpu().numpy() for k, v in state.items()}
        p_h, l_h = params.cpu().numpy(), luts.cpu().numpy()
        g_h = thists.cpu().numpy().astype(np.int64).sum(axis=1)
        for i in range(n):
            wb, used = temporal_blend(ref[i], p_h[i], l_h[i], g_h[i], alpha,
                                      cut_count)
            where = (hw, t, i)
            # float32 compared as bits: no tolerance
            assert np.array_equal(got["wb"][i].view(np.uint32),
                                  wb.view(np.uint32)), where
            assert np.array_equal(got["lut"][i].view(np.uint32),
                                  ref[i].lut.view(np.uint32)), where
            assert np.array_equal(got["lhist"][i], ref[i].lhist), where
            assert np.array_equal(got["lut_u8"][i], used), where
            assert got["counters"][i].tolist() == \
                [ref[i].has_state, ref[i].frames, ref[i].cuts], where
    return [r.cuts for r in ref], state


@pytest.mark.parametrize("hw", SHAPES)
def test_blend_kernel_is_the_numpy_definition(ext, hw):
    cuts, state = _blend_against_numpy(ext, [_stream_a(*hw)], hw)
    assert cuts == [1]
    # the smoothing is in effect: the state is no frame's own LUT set
    lut = state["lut"].cpu().numpy()
    assert not np.array_equal(lut, np.rint(lut))


def test_blend_kernel_streams_do_not_interact(ext):
    hw = (40, 48)
    a, b = _stream_a(*hw), _stream_b(*hw)
    cuts, both = _blend_against_numpy(ext, [a, b], hw)
    assert cuts == [1, 1]
    # each stream alone ends in the state it has next to the other
    for i, s in enumerate((a, b)):
        _, alone = _blend_against_numpy(ext, [s], hw)
        for k in both:
            assert torch.equal(both[k][i], alone[k][0]), (k, i)


def test_blend_wrapper_rejects_bad_arguments(ext):
    from waternet_amd.ops.preprocess import new_temporal_state

    raw = _dev([_stream_a(40, 48)[0]])
    params, luts, _, thists = ext.preprocess_stats(raw)
    st = new_temporal_state(1, DEV)

    def call(alpha=0.3, cut_count=10, **over):
        a = dict(st, wb_params=params, luts=luts, tile_hists=thists)
        a.update(over)
        ext.temporal_blend(a["wb"], a["lut"], a["lhist"], a["counters"],
                           a["lut_u8"], a["wb_params"], a["luts"],
                           a["tile_hists"], alpha, cut_count)

    bad = [
        dict(luts=luts.float()),                       # dtype
        dict(tile_hists=thists.long()),
        dict(wb=st["wb"].double()),
        dict(lhist=st["lhist"][:, :255].contiguous()),  # shape
        dict(lut=st["lut"][:, :63].contiguous()),
        dict(counters=st["counters"][:, :2].contiguous()),
        dict(wb_params=params.reshape(1, 2, 3)),
        dict(lut_u8=torch.zeros(2, 64, 256, dtype=torch.uint8, device=DEV)),
        dict(lut=st["lut"].transpose(1, 2)),           # not contiguous
        dict(luts=luts.cpu()),                         # device
        dict(alpha=0.0), dict(alpha=-0.5), dict(alpha=1.5),
        dict(alpha=float("nan")),
        dict(cut_count=-1),
    ]
    for kw in bad:
        with pytest.raises(RuntimeError, match="temporal_blend"):
            call(**kw)
    # nothing was launched: the state is as allocated
    assert all(int(v.abs().sum()) == 0 for v in st.values())
    call()
    assert st["counters"].tolist() == [[1, 1, 0]]
    with pytest.raises(RuntimeError, match="preprocess_apply"):
        ext.preprocess_apply(raw, raw, params.double(), luts)
    with pytest.raises(RuntimeError, match="preprocess_apply"):
        ext.preprocess_apply(raw, raw[:, :8].contiguous(), params, luts)
    with pytest.raises(RuntimeError, match="preprocess_apply"):
        ext.preprocess_apply(raw, raw, params, luts[:, :32].contiguous())


# ---------------------------------------------------------------------------
# Engine
# ---------------------------------------------------------------------------


@pytest.fixture(scope="module")
def model():
    from waternet_amd.models.waternet import WaterNet

    torch.manual_seed(23)
    return WaterNet().to(DEV)


def _engine(model, hw, **kw):
    from waternet_amd.engine.inferencer import InferenceEngine

    return InferenceEngine(model, hw[0], hw[1], device=DEV, **kw)


@pytest.mark.parametrize("hw", [(64, 64), (37, 45)])
def test_engine_alpha_one_is_the_plain_engine(model, hw):
    """alpha = 1 replaces the state by each frame's own statistics
    (s + (x - s) == x: exact within a scene, where clip points stay within a
    factor 2 of each other, and a cut assigns)."""
    frames = _stream_a(*hw)
    php = frames[0].shape[:2]
    plain = _engine(model, php)
    one = _engine(model, php, temporal_alpha=1.0)
    for t, f in enumerate(frames):
        assert np.array_equal(one.infer_frame(f), plain.infer_frame(f)), t
    assert one.temporal_counters() == {"frames": 8, "cuts": 1}
    with pytest.raises(RuntimeError, match="temporal_alpha"):
        plain.temporal_counters()
    plain.reset_temporal()  # a no-op without the option


def test_engine_graph_replays_keep_the_state(model):
    """Graph replays against eager launches, frame by frame: the state
    persists across replays and the capture warm-up leaves none behind.
    Then reset_temporal() starts the same stream over."""
    hw = (64, 64)
    frames = _stream_a(*hw)
    graph = _engine(model, hw, temporal_alpha=0.3)
    eager = _engine(model, hw, temporal_alpha=0.3, use_graph=False)
    plain = _engine(model, hw)
    first = []
    for t, f in enumerate(frames):
        out = graph.infer_frame(f)
        assert np.array_equal(out, eager.infer_frame(f)), t
        assert graph.temporal_counters() == eager.temporal_counters() == \
            {"frames": t + 1, "cuts": int(t >= 4)}
        same = np.array_equal(out, plain.infer_frame(f))
        # frame 0 and the cut frame are per-frame results, the others not
        assert same == (t in (0, 4)), t
        first.append(out)
    assert graph._graph is not None, "the graph engine fell back to eager"
    assert eager._graph is None
    for eng in (graph, eager):
        eng.reset_temporal()
        assert eng.temporal_counters() == {"frames": 0, "cuts": 0}
        for t, f in enumerate(frames):
            assert np.array_equal(eng.infer_frame(f), first[t]), t
        assert eng.temporal_counters() == {"frames": 8, "cuts": 1}


def test_engine_rejects_bad_options(model):
    for kw in (dict(temporal_alpha=0.0), dict(temporal_alpha=1.2),
               dict(temporal_alpha=0.5, scene_cut=-0.1)):
        with pytest.raises(ValueError):
            _engine(model, (64, 64), **kw)


# ---------------------------------------------------------------------------
# GPU pipeline against the CPU path
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("hw", [(64, 64), (40, 48)])
def test_stream_transform_gpu_vs_cpu(ext, hw):
    """The stabilised (wb, gc, he) at alpha = 0.3 over 4 frames with a cut in
    the middle, against TemporalStabilizer, within the bounds
    test_preprocess_gpu_vs_cpu sets for the per-frame transform."""
    from waternet_amd.ops.preprocess import (gpu_transform_stream,
                                             new_temporal_state)

    frames = _stream_a(*hw)[2:6]  # the cut at index 2
    cpu = TemporalStabilizer(0.3, 0.5)
    state = new_temporal_state(1, DEV)
    cut_count = scene_cut_count(0.5, *hw)
    for t, f in enumerate(frames):
        wb_c, gc_c, he_c = cpu.transform(f)
        wb_g, gc_g, he_g = (x[0].cpu().numpy() for x in gpu_transform_stream(
            _dev([f]), state, 0.3, cut_count))
        assert np.array_equal(gc_g, gc_c), "gamma LUT must be exact"
        dwb = np.abs(wb_g.astype(int) - wb_c.astype(int))
        dhe = np.abs(he_g.astype(int) - he_c.astype(int))
        print(f"{hw} frame {t}: wb max {dwb.max()} frac {(dwb > 0).mean():.5f}"
              f" | he mean {dhe.mean():.4f} max {dhe.max()} "
              f"frac>1 {(dhe > 1).mean():.5f}")
        assert dwb.max() <= 1 and (dwb > 0).mean() < 0.01, \
            f"WB mismatch: max {dwb.max()}, frac {(dwb > 0).mean()}"
        assert dhe.mean() < 0.5, f"CLAHE mean diff {dhe.mean()}"
        assert dhe.max() <= 8 and (dhe > 1).mean() < 0.01, \
            f"CLAHE mismatch: max {dhe.max()}, frac>1 {(dhe > 1).mean()}"
    assert state["counters"].tolist() == [[1, 4, 1]]
    assert (cpu.frames, cpu.cuts) == (4, 1)
