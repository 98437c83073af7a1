"""The NumPy definition of temporally smoothed WB/CLAHE statistics
(waternet_amd/data/temporal.py) and its CLI surface on the CPU path.

Byte equality with the per-frame transform() is defined where a frame's
clip points are float32-exact: the state is float32, transform() keeps
float64 clip points, and the stretch truncates (hi-lo) * (255/(hi-lo)) for
every pixel clipped at hi, which lands on 255 or 254.99.. depending on the
last bit of lo and hi. Integer quantiles (the two order statistics around
the quantile position coincide) are exact; the tests below that compare
against transform() check that condition on their inputs first. gc and he
do not depend on it."""

import os
import stat
import sys
from pathlib import Path

import numpy as np
import pytest
from temporal_seq import blob_sequence, two_scene_sequence

from waternet_amd.data.temporal import (TemporalStabilizer, TemporalState,
                                        scene_cut_count, temporal_blend)
from waternet_amd.data.transforms import transform, white_balance_params

REPO = Path(__file__).resolve().parent.parent

# seed 2: the clip points of frame 0 and of the cut frame are float32-exact
# (asserted where it is used)
CUT_SEED = 2


def _f32_exact(frame):
    p = white_balance_params(frame)
    return np.array_equal(p, p.astype(np.float32).astype(np.float64))


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _levels_sequence(n=6, h=64, w=64, seed=5):
    """Changing frames on few grey levels (24 levels, ~170 pixels each):
    every quantile falls inside a level, so every clip point is an
    integer."""
    rng = np.random.default_rng(seed)
    frames = [(rng.integers(0, 24, size=(h, w, 3)) * 8
               + rng.integers(0, 40)).astype(np.uint8) for _ in range(n)]
    assert all(_f32_exact(f) for f in frames), "test input precondition"
    return frames


def test_alpha_one_is_per_frame():
    st = TemporalStabilizer(1.0, 0.5)
    for f in _levels_sequence():
        assert _same(st.transform(f), transform(f))
    assert st.frames == 6


@pytest.mark.parametrize("alpha", [0.05, 0.3, 1.0])
def test_first_frame_is_per_frame(alpha):
    f = _levels_sequence(n=1)[0]
    st = TemporalStabilizer(alpha, 0.5)
    assert _same(st.transform(f), transform(f))
    # ... and again after reset(), whatever came in between
    st.transform(255 - f)
    st.reset()
    assert _same(st.transform(f), transform(f))
    assert (st.frames, st.cuts) == (1, 0)


def test_constant_sequence_is_fixed_point():
    f = two_scene_sequence(64, 64, per_scene=1, seed=CUT_SEED)[0]
    st = TemporalStabilizer(0.3, 0.5)
    first = st.transform(f)
    wb0, lut0 = st.state.wb.copy(), st.state.lut.copy()
    for _ in range(5):
        assert _same(st.transform(f), first)
        assert np.array_equal(st.state.wb, wb0)
        assert np.array_equal(st.state.lut, lut0)
    assert st.cuts == 0 and st.last_d == 0


@pytest.mark.parametrize("hw", [(64, 64), (40, 48), (37, 45)])
def test_scene_cut_detected_at_the_boundary(hw):
    h, w = hw
    frames = two_scene_sequence(h, w, per_scene=6, seed=CUT_SEED)
    st = TemporalStabilizer(0.3, 0.5)
    # the histograms count the frame padded to the 8x8 tile grid
    hp, wp = h + (-h) % 8, w + (-w) % 8
    cut_count = scene_cut_count(0.5, hp, wp)
    assert cut_count == hp * wp
    cuts_after = []
    for t, f in enumerate(frames):
        out = st.transform(f)
        cuts_after.append(st.cuts)
        if t == 0:
            continue
        # condition of the test: d is far from the threshold on both sides
        if t == 6:
            assert st.last_d > 1.5 * cut_count, (t, st.last_d, cut_count)
            if _f32_exact(f):
                assert _same(out, transform(f))
            else:  # gc, he do not depend on the clip points
                assert _same(out[1:], transform(f)[1:])
        else:
            assert st.last_d < 0.5 * cut_count, (t, st.last_d, cut_count)
    assert cuts_after == [0] * 6 + [1] * 6
    assert st.frames == 12


def test_cut_frame_output_is_per_frame_output():
    frames = two_scene_sequence(64, 64, per_scene=6, seed=CUT_SEED)
    assert _f32_exact(frames[6]), "test input precondition"
    st = TemporalStabilizer(0.3, 0.5)
    outs = [st.transform(f) for f in frames]
    assert st.cuts == 1
    assert _same(outs[6], transform(frames[6]))
    # the smoothing did something on the frames in between
    assert not _same(outs[3], transform(frames[3]))


def test_scene_cut_zero_and_one():
    """scene_cut=0 cuts on every frame that changes the histogram at all
    (per-frame behaviour); scene_cut=1 never cuts (d <= 2HW always)."""
    frames = two_scene_sequence(64, 64, per_scene=2, seed=CUT_SEED)
    every = TemporalStabilizer(0.3, 0.0)
    never = TemporalStabilizer(0.3, 1.0)
    for f in frames:
        every.transform(f)
        never.transform(f)
    assert every.cuts == 3 and never.cuts == 0


def test_blend_is_float32_and_unfused():
    """One blend step against the arithmetic spelled out per element."""
    rng = np.random.default_rng(0)
    st = TemporalState()
    g = np.full(256, 16, np.int64)
    p0 = rng.uniform(0, 255, (3, 2)).astype(np.float32)
    l0 = rng.integers(0, 256, (64, 256)).astype(np.uint8)
    temporal_blend(st, p0, l0, g, 0.3, 10)
    p1 = rng.uniform(0, 255, (3, 2)).astype(np.float32)
    l1 = rng.integers(0, 256, (64, 256)).astype(np.uint8)
    wb, used = temporal_blend(st, p1, l1, g, 0.3, 10)
    a = np.float32(0.3)
    for i in range(3):
        for j in range(2):
            diff = np.float32(p1[i, j] - p0[i, j])
            step = np.float32(a * diff)
            assert wb[i, j] == np.float32(p0[i, j] + step)
    s = l0.astype(np.float32)
    want = s + a * (l1.astype(np.float32) - s)
    assert want.dtype == np.float32
    assert np.array_equal(st.lut, want)
    assert np.array_equal(used, np.rint(want).astype(np.uint8))
    assert st.lhist.dtype == np.int32 and (st.frames, st.cuts) == (2, 0)


def _flicker(outs, mask, k):
    return float(np.mean([
        np.abs(outs[t][k][mask].astype(int)
               - outs[t - 1][k][mask].astype(int)).mean()
        for t in range(1, len(outs))]))


def test_flicker_is_reduced():
    frames, mask = blob_sequence(n=8)
    per_frame = [transform(f) for f in frames]
    st = TemporalStabilizer(0.2, 0.5)
    smooth = [st.transform(f) for f in frames]
    assert st.cuts == 0
    for k, name in ((0, "wb"), (2, "he")):
        before = _flicker(per_frame, mask, k)
        after = _flicker(smooth, mask, k)
        print(f"{name} flicker per-frame {before:.4f} smoothed {after:.4f}")
        assert before > 0, f"{name}: the inputs do not flicker per-frame"
        assert after < before, (name, before, after)


# ---------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------


def _cli():
    sys.path.insert(0, str(REPO))
    try:
        import inference
    finally:
        sys.path.pop(0)
    return inference


@pytest.mark.parametrize("bad", [
    ["--temporal-smooth", "0"], ["--temporal-smooth", "-0.2"],
    ["--temporal-smooth", "1.5"], ["--temporal-smooth", "nan"],
    ["--scene-cut", "-0.1"], ["--scene-cut", "1.01"],
    ["--temporal-smooth", "0.3", "--scene-cut", "nan"],
])
def test_cli_rejects_invalid_values(bad, capsys):
    with pytest.raises(SystemExit) as exc:
        _cli().parse_args(["--source", "x.mp4"] + bad)
    assert exc.value.code != 0
    err = capsys.readouterr().err
    assert bad[-2] in err and "must be in" in err


def test_cli_defaults_and_valid_values():
    cli = _cli()
    a = cli.parse_args(["--source", "x.mp4"])
    assert a.temporal_smooth is None and a.scene_cut == 0.5
    a = cli.parse_args(["--source", "x.mp4", "--temporal-smooth", "1",
                        "--scene-cut", "0"])
    assert a.temporal_smooth == 1.0 and a.scene_cut == 0.0
    with pytest.raises(ValueError):
        TemporalStabilizer(0.0)
    with pytest.raises(ValueError):
        TemporalStabilizer(0.5, scene_cut=1.5)


@pytest.fixture
def cpu_cli(tmp_path, monkeypatch):
    """inference.main in-process on the CPU path, cwd in tmp_path, with
    saved weights so that two runs enhance alike."""
    import torch

    from waternet_amd.models.waternet import WaterNet

    cli = _cli()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    weights = tmp_path / "w.pt"
    torch.save(WaterNet().state_dict(), weights)
    return cli, ["--weights", str(weights)]


def _fake_ffmpeg(tmp_path, monkeypatch, h, w):
    """Stub ffmpeg/ffprobe on PATH: a 'video' is its raw RGB frames."""
    fake = tmp_path / "bin"
    fake.mkdir()
    (fake / "ffprobe").write_text(
        "#!/bin/bash\n"
        f'echo \'{{"streams":[{{"width":{w},"height":{h},'
        '"r_frame_rate":"24/1"}]}\'\n')
    (fake / "ffmpeg").write_text(
        "#!/bin/bash\n"
        'prev=""; input=""\n'
        'for a in "$@"; do if [ "$prev" = "-i" ]; then input="$a"; fi; '
        'prev="$a"; done\n'
        'last="${@: -1}"\n'
        'if [ "$input" = "-" ]; then cat - > "$last"; else cat "$input"; fi\n')
    for f in ("ffprobe", "ffmpeg"):
        os.chmod(fake / f, stat.S_IRWXU)
    monkeypatch.setenv("PATH", f"{fake}:{os.environ['PATH']}")


def _levels_clip(h, w):
    """Four frames, two scenes on disjoint grey levels; the second frame of
    each scene is the first one shifted sideways: same global histograms
    (d = 0, same clip points, all integers), other tile LUTs."""
    rng = np.random.default_rng(9)
    frames = []
    for off in (10, 150):
        f = (rng.integers(0, 8, size=(h, w, 3)) * 8 + off).astype(np.uint8)
        frames += [f, np.roll(f, 5, axis=1)]
    assert all(_f32_exact(f) for f in frames), "test input precondition"
    return frames


def test_cli_video_smooths_and_prints_cuts(cpu_cli, tmp_path, monkeypatch,
                                           capsys):
    cli, weights = cpu_cli
    h, w = 16, 24
    _fake_ffmpeg(tmp_path, monkeypatch, h, w)
    (tmp_path / "a.mp4").write_bytes(np.stack(_levels_clip(h, w)).tobytes())

    def run(name, src, extra):
        cli.main(["--source", str(src), "--name", name] + weights + extra)
        out = capsys.readouterr().out
        got = {p.name: np.frombuffer(p.read_bytes(), np.uint8)
               for p in sorted((tmp_path / "output" / name).iterdir())}
        return out, got

    out, plain = run("plain", tmp_path / "a.mp4", [])
    assert "Wrote 4 frames" in out and "Scene cuts" not in out
    out, smooth = run("smooth", tmp_path / "a.mp4",
                      ["--temporal-smooth", "0.3"])
    assert "Wrote 4 frames" in out and "Scene cuts: 1" in out
    a, b = (x["a.mp4"].reshape(4, h, w, 3) for x in (plain, smooth))
    # frame 0 and the cut frame are the per-frame result, frames 1 and 3
    # are smoothed
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
    assert not np.array_equal(a[1], b[1])
    assert not np.array_equal(a[3], b[3])
    # alpha=1, never cutting: the per-frame result on every frame, and no
    # cut reported
    out, one = run("one", tmp_path / "a.mp4",
                   ["--temporal-smooth", "1", "--scene-cut", "1"])
    assert "Scene cuts: 0" in out
    assert np.array_equal(one["a.mp4"], plain["a.mp4"])


def test_cli_state_resets_per_video(cpu_cli, tmp_path, monkeypatch, capsys):
    """Two videos in one directory: the second starts from a fresh state,
    so two copies of one clip come out identical and each reports its own
    cut count."""
    cli, weights = cpu_cli
    h, w = 16, 24
    _fake_ffmpeg(tmp_path, monkeypatch, h, w)
    frames = _levels_clip(h, w)
    src = tmp_path / "clips"
    src.mkdir()
    for name in ("a.mp4", "b.mp4"):
        (src / name).write_bytes(np.stack(frames).tobytes())
    cli.main(["--source", str(src), "--name", "two", "--temporal-smooth",
              "0.3"] + weights)
    out = capsys.readouterr().out
    assert out.count("Scene cuts: 1") == 2
    outdir = tmp_path / "output" / "two"
    assert (outdir / "a.mp4").read_bytes() == (outdir / "b.mp4").read_bytes()


def test_cli_image_directory_ignores_the_flags(cpu_cli, tmp_path, capsys):
    from PIL import Image

    cli, weights = cpu_cli
    src = tmp_path / "imgs"
    src.mkdir()
    for name, f in zip(("a.png", "b.png"),
                       two_scene_sequence(24, 32, per_scene=1,
                                          seed=CUT_SEED)):
        Image.fromarray(f).save(src / name)
    cli.main(["--source", str(src), "--name", "off"] + weights)
    cli.main(["--source", str(src), "--name", "on", "--temporal-smooth",
              "0.2", "--scene-cut", "1"] + weights)
    assert "Scene cuts" not in capsys.readouterr().out
    for name in ("a.png", "b.png"):
        assert (tmp_path / "output" / "off" / name).read_bytes() == \
            (tmp_path / "output" / "on" / name).read_bytes()
