"""GPU tests for the no-reference quality telemetry on the frame engine:
InferenceEngine.frame_quality and inference.py --report-quality."""

import numpy as np
import pytest
import torch

from waternet_amd.utils import nr_metrics as nrm

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RTOL = ATOL = 1e-9  # derivation: tests/test_gpu_nr_metrics.py


def _model(seed):
    from waternet_amd.models.waternet import WaterNet

    torch.manual_seed(seed)
    return WaterNet().to(DEV)


def _dev(arr):
    return torch.from_numpy(np.ascontiguousarray(arr)).unsqueeze(0).to(DEV)


def test_frame_quality_is_nr_metrics_of_the_frame_and_leaves_it_alone():
    from waternet_amd.engine.inferencer import InferenceEngine

    rng = np.random.default_rng(23)
    frames = rng.integers(0, 256, size=(2, 64, 64, 3), dtype=np.uint8)
    eng = InferenceEngine(_model(23), 64, 64, device=DEV, use_graph=True)
    plain = InferenceEngine(_model(23), 64, 64, device=DEV, use_graph=True)
    with pytest.raises(RuntimeError, match="infer_frame"):
        eng.frame_quality()
    for frame in frames:  # first frame captures, second replays
        out = eng.infer_frame(frame)
        q = eng.frame_quality()
        assert q.shape == (2, 5) and q.dtype == torch.float64
        assert q.device.type == "cuda"
        assert torch.equal(q[0:1], nrm.nr_metrics(_dev(frame)))
        assert torch.equal(q[1:2], nrm.nr_metrics(_dev(out)))
        # an engine that never scores returns the same bytes
        assert np.array_equal(out, plain.infer_frame(frame))
    assert eng._graph is not None, "the graph path was not exercised"


def test_frame_quality_crops_the_padding():
    """A 33x45 frame runs on a 40x48 engine; frame_quality(33, 45) scores
    the real pixels only and matches NumPy."""
    from waternet_amd.engine.inferencer import InferenceEngine, pad8
    from waternet_amd.ops import ext

    rng = np.random.default_rng(29)
    rgb = rng.integers(0, 256, size=(33, 45, 3), dtype=np.uint8)
    padded, h, w = pad8(rgb)
    assert padded.shape == (40, 48, 3)
    eng = InferenceEngine(_model(29), 40, 48, device=DEV, use_graph=True)
    out = eng.infer_frame(padded)[:h, :w]
    got = eng.frame_quality(h, w).cpu().numpy()
    for row, img in zip(got, (rgb, out)):
        ref = [nrm.uicm(img), nrm.uism(img), nrm.uiconm(img), nrm.uiqm(img)]
        lab = ext().rgb2lab_u8(_dev(img))[0].cpu().numpy()
        print("got", row.tolist(), "ref", ref, nrm.uciqe_from_lab(lab))
        np.testing.assert_allclose(row[:4], ref, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(row[4], nrm.uciqe_from_lab(lab),
                                   rtol=RTOL, atol=ATOL)
    # the padded score is a different number: the crop is really applied
    assert not np.array_equal(got, eng.frame_quality().cpu().numpy())
    with pytest.raises(ValueError):
        eng.frame_quality(41, 48)


def test_inference_cli_report_quality_gpu(tmp_path, monkeypatch, capsys):
    """inference.py --report-quality on a two-PNG folder: the UIQM columns
    are the NumPy metrics of the source and of the saved (lossless) PNG."""
    from PIL import Image

    import inference as inf_cli
    from waternet_amd.models.waternet import WaterNet

    torch.manual_seed(31)
    ckpt = tmp_path / "w.pt"
    torch.save(WaterNet().state_dict(), ckpt)
    rng = np.random.default_rng(31)
    src = tmp_path / "imgs"
    src.mkdir()
    imgs = {"a.png": rng.integers(0, 256, size=(64, 64, 3), dtype=np.uint8),
            "b.png": rng.integers(0, 256, size=(33, 45, 3), dtype=np.uint8)}
    for name, im in imgs.items():
        Image.fromarray(im).save(src / name)

    monkeypatch.chdir(tmp_path)
    inf_cli.main(["--source", str(src), "--weights", str(ckpt),
                  "--name", "q", "--report-quality"])
    stdout = capsys.readouterr().out
    lines = (tmp_path / "output" / "q" / "quality.csv").read_text() \
        .splitlines()
    assert lines[0] == inf_cli.QUALITY_HEADER
    assert len(lines) == 3
    for line, name in zip(lines[1:], ("a.png", "b.png")):
        row = dict(zip(lines[0].split(","), line.split(",")))
        assert row["source"] == name and row["frames"] == "1"
        assert f"{name}: UIQM " in stdout
        with Image.open(tmp_path / "output" / "q" / name) as im:
            saved = np.asarray(im.convert("RGB"))
        assert saved.shape == imgs[name].shape
        for side, img in (("before", imgs[name]), ("after", saved)):
            for key, fn in (("uiqm", nrm.uiqm), ("uicm", nrm.uicm),
                            ("uism", nrm.uism), ("uiconm", nrm.uiconm)):
                assert row[f"{key}_{side}"] == "%.6f" % fn(img), (name, key)
