"""CPU tests for the remaining user-facing CLI/API surface: directory
inference with --show-split (reference inference.py:128-135, 202-233), the
hubconf pretrained offline error path (reference hubconf.py:78-83), and the
video-IO-without-ffmpeg error (reference uses cv2.VideoCapture,
inference.py:238-256)."""

import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent


def _no_gpu_env():
    """Child-process environment with every GPU hidden, so a test of the
    CPU-only behaviour checks the same thing on a GPU box."""
    import os

    return dict(os.environ, HIP_VISIBLE_DEVICES="-1",
                CUDA_VISIBLE_DEVICES="-1")


def test_inference_cli_dir_show_split(tmp_path):
    """A directory source enhances every image; --show-split writes the
    before/after composite (white divider at w//2)."""
    from PIL import Image

    rng = np.random.default_rng(0)
    srcdir = tmp_path / "imgs"
    srcdir.mkdir()
    for name in ("a.png", "b.jpg"):
        img = rng.integers(0, 256, size=(40, 56, 3), dtype=np.uint8)
        Image.fromarray(img).save(srcdir / name)
    (srcdir / "notes.txt").write_text("ignored: not an image suffix")

    out = subprocess.run(
        [sys.executable, "inference.py", "--source", str(srcdir),
         "--name", "pytest-split", "--show-split"],
        cwd=REPO, capture_output=True, text=True, timeout=600,
    )
    assert out.returncode == 0, out.stderr
    outdir = REPO / "output" / "pytest-split"
    for name in ("a.png", "b.jpg"):
        p = outdir / name
        assert p.exists(), f"missing {p}"
        with Image.open(p) as im:
            arr = np.asarray(im.convert("RGB"))
        assert arr.shape == (40, 56, 3)
        # the composite's vertical divider at w//2 is near-white (JPEG
        # compression smears it slightly on the .jpg output)
        assert arr[:, 56 // 2].mean() >= 200, "split divider missing"
    assert "Total images/videos: 2" in out.stdout


def test_hubconf_pretrained_offline_error(monkeypatch):
    """pretrained=True without network raises a clear, actionable error
    (mentioning checkpoint=/pretrained=False), not a bare URLError."""
    import torch

    sys.path.insert(0, str(REPO))
    try:
        import hubconf
    finally:
        sys.path.pop(0)

    def fail_download(*a, **k):
        raise OSError("simulated: no route to host")

    monkeypatch.setattr(torch.hub, "load_state_dict_from_url", fail_download)
    with pytest.raises(RuntimeError) as exc:
        hubconf.waternet(pretrained=True, device="cpu")
    msg = str(exc.value)
    assert "checkpoint=" in msg and "pretrained=False" in msg


def test_hubconf_pretrained_local_checkpoint(tmp_path):
    """checkpoint=<path> loads without network and returns the working
    (preprocess, postprocess, model) tuple."""
    import torch

    from waternet_amd.models.waternet import WaterNet

    sys.path.insert(0, str(REPO))
    try:
        import hubconf
    finally:
        sys.path.pop(0)

    ckpt = tmp_path / "w.pt"
    torch.save(WaterNet().state_dict(), ckpt)
    preprocess, postprocess, model = hubconf.waternet(
        pretrained=True, device="cpu", checkpoint=str(ckpt))
    rgb = np.random.default_rng(0).integers(
        0, 256, size=(32, 32, 3), dtype=np.uint8)
    tens = preprocess(rgb)
    out = model(*tens)
    arr = postprocess(out)
    # batched NHWC, as the reference's ten2arr (training_utils.py:31-43)
    assert arr.shape == (1, 32, 32, 3) and arr.dtype == np.uint8


def test_video_requires_ffmpeg_clear_error(monkeypatch, tmp_path):
    """Without the ffmpeg binary, video IO raises an actionable error
    instead of a FileNotFoundError deep in subprocess."""
    import shutil

    from waternet_amd.engine import video

    monkeypatch.setattr(shutil, "which", lambda name: None)
    with pytest.raises(RuntimeError, match="ffmpeg"):
        video.FFmpegReader(tmp_path / "clip.mp4")


def test_score_missing_weights_clear_error():
    out = subprocess.run(
        [sys.executable, "score.py", "--weights", "/nonexistent/w.pt",
         "--synthetic", "4", "--batch-size", "2",
         "--height", "32", "--width", "32"],
        cwd=REPO, capture_output=True, text=True, timeout=600,
    )
    assert out.returncode != 0
    assert "weights file not found" in out.stderr


def test_train_missing_dataset_clear_error(tmp_path):
    out = subprocess.run(
        [sys.executable, str(REPO / "train.py"), "--data-root",
         str(tmp_path / "absent"), "--epochs", "1"],
        cwd=tmp_path, capture_output=True, text=True, timeout=600,
    )
    assert out.returncode != 0
    assert "raw-890" in out.stderr  # names the expected layout


def test_train_resume_missing_savedir_clear_error(tmp_path):
    out = subprocess.run(
        [sys.executable, str(REPO / "train.py"), "--synthetic", "4",
         "--batch-size", "2", "--height", "32", "--width", "32",
         "--epochs", "1", "--resume", str(tmp_path / "absent")],
        cwd=tmp_path, capture_output=True, text=True, timeout=600,
    )
    assert out.returncode != 0
    assert "no last.pt" in out.stderr


def test_uieb_dataset_wrong_size_split_error(tmp_path):
    """A dataset dir with the wrong image count gets the explicit 800/90
    message, not torch's opaque random_split ValueError."""
    from PIL import Image

    (tmp_path / "raw-890").mkdir()
    (tmp_path / "reference-890").mkdir()
    img = np.zeros((40, 40, 3), dtype=np.uint8)
    for d in ("raw-890", "reference-890"):
        Image.fromarray(img).save(tmp_path / d / "0.png")
    out = subprocess.run(
        [sys.executable, str(REPO / "train.py"), "--data-root",
         str(tmp_path), "--epochs", "1"],
        cwd=tmp_path, capture_output=True, text=True, timeout=600,
    )
    assert out.returncode != 0
    assert "800/90" in out.stderr and "found 1" in out.stderr


def test_inference_failed_run_leaves_no_savedir(tmp_path):
    """Reference behavior (inference.py:198-200): the savedir is created at
    the first write, so a run that fails early leaves no empty output
    dir; successful numbered runs count up from 0."""
    from PIL import Image

    img = np.zeros((16, 16, 3), dtype=np.uint8)
    src = tmp_path / "x.png"
    Image.fromarray(img).save(src)

    # failing run: bad --weights aborts before any write
    out = subprocess.run(
        [sys.executable, str(REPO / "inference.py"), "--source", str(src),
         "--weights", str(tmp_path / "missing.pt")],
        cwd=tmp_path, capture_output=True, text=True, timeout=600,
    )
    assert out.returncode != 0
    assert not (tmp_path / "output").exists()

    # successful runs: output/0 then output/1
    for expect in ("0", "1"):
        out = subprocess.run(
            [sys.executable, str(REPO / "inference.py"),
             "--source", str(src)],
            cwd=tmp_path, capture_output=True, text=True, timeout=600,
        )
        assert out.returncode == 0, out.stderr
        assert (tmp_path / "output" / expect / "x.png").exists()


def test_example_notebook_executes():
    """examples/example-notebook.ipynb (the reference Colab-example analog)
    stays valid JSON and its code cells execute top to bottom on CPU."""
    import json

    nb = json.loads(
        (REPO / "examples" / "example-notebook.ipynb").read_text())
    assert nb["nbformat"] == 4
    ns = {}
    cwd = REPO / "examples"
    import os

    old = os.getcwd()
    os.chdir(cwd)
    try:
        for cell in nb["cells"]:
            if cell["cell_type"] != "code":
                continue
            exec(compile("".join(cell["source"]), "<cell>", "exec"), ns)
    finally:
        os.chdir(old)
    assert ns["out_im"].shape == (1, 480, 720, 3)


def test_video_pipeline_with_fake_ffmpeg(tmp_path):
    """End-to-end video inference (reference inference.py:238-323) with a
    stub ffmpeg/ffprobe on PATH: the reader parses probe JSON and streams
    raw RGB frames, every frame runs through the model, and the writer
    receives raw RGB back — closing the only otherwise-untestable-offline
    subsystem."""
    import os
    import stat

    h, w, frames = 6, 8, 2
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
        '# decode mode: -i <file> ... -   |   encode mode: -i - ... <file>\n'
        'if [ "$input" = "-" ]; then cat - > "$last"; else cat "$input"; fi\n')
    for f in ("ffprobe", "ffmpeg"):
        os.chmod(fake / f, stat.S_IRWXU)

    rng = np.random.default_rng(3)
    raw = rng.integers(0, 256, size=(frames, h, w, 3), dtype=np.uint8)
    clip = tmp_path / "clip.mp4"
    clip.write_bytes(raw.tobytes())

    env = dict(os.environ, PATH=f"{fake}:{os.environ['PATH']}")
    out = subprocess.run(
        [sys.executable, str(REPO / "inference.py"), "--source", str(clip)],
        cwd=tmp_path, capture_output=True, text=True, timeout=600, env=env,
    )
    assert out.returncode == 0, out.stderr
    assert "Wrote 2 frames" in out.stdout
    produced = (tmp_path / "output" / "0" / "clip.mp4").read_bytes()
    got = np.frombuffer(produced, dtype=np.uint8).reshape(frames, h, w, 3)
    # frames passed through the actual model: right shape, not a copy
    assert not np.array_equal(got, raw)


def test_quickstart_example_runs():
    """examples/quickstart.py (the README/Colab-analog workflow:
    train -> score -> enhance on synthetic data) completes on CPU."""
    out = subprocess.run(
        [sys.executable, str(REPO / "examples" / "quickstart.py")],
        capture_output=True, text=True, timeout=600, env=_no_gpu_env(),
    )
    assert out.returncode == 0, out.stderr
    assert "enhanced frame: (64, 64, 3) uint8" in out.stdout


def test_hub_demo_example_runs():
    """examples/hub_demo.py (the reference README torch.hub quickstart
    analog) completes on CPU."""
    out = subprocess.run(
        [sys.executable, str(REPO / "examples" / "hub_demo.py")],
        capture_output=True, text=True, timeout=600,
    )
    assert out.returncode == 0, out.stderr
    assert "-> out (112, 112, 3) uint8" in out.stdout


def test_reference_flag_sets_parse():
    """Every flag combination the reference CLIs accept must parse here
    (CLI contract): train.py:164-194, score.py:92-122 (incl. the vestigial
    --epochs), inference.py:57-80."""
    sys.path.insert(0, str(REPO))
    try:
        import inference as inf_cli
        import score as score_cli
        import train as train_cli
    finally:
        sys.path.pop(0)

    t = train_cli.parse_args(["--epochs", "400", "--batch-size", "16",
                              "--height", "112", "--width", "112",
                              "--weights", "w.pt", "--seed", "5"])
    assert t.epochs == 400 and t.seed == 5

    s = score_cli.parse_args(["--weights", "w.pt", "--epochs", "400",
                              "--batch-size", "16", "--height", "112",
                              "--width", "112", "--seed", "5"])
    assert s.weights == "w.pt"

    i = inf_cli.parse_args(["--source", "x.png", "--weights", "w.pt",
                            "--name", "run", "--show-split"])
    assert i.show_split and i.name == "run"


def test_engine_fast_on_cpu_clear_error():
    """--engine fast without a GPU exits with the requirement message
    instead of failing deep in the engine."""
    out = subprocess.run(
        [sys.executable, str(REPO / "train.py"), "--engine", "fast",
         "--synthetic", "4", "--epochs", "1",
         "--batch-size", "2", "--height", "32", "--width", "32"],
        capture_output=True, text=True, timeout=600, env=_no_gpu_env(),
    )
    assert out.returncode != 0
    assert "--engine fast requires a ROCm GPU" in out.stderr

    out = subprocess.run(
        [sys.executable, str(REPO / "score.py"), "--engine", "fast",
         "--weights", "w.pt", "--synthetic", "4",
         "--batch-size", "2", "--height", "32", "--width", "32"],
        capture_output=True, text=True, timeout=600, env=_no_gpu_env(),
    )
    assert out.returncode != 0
    assert "requires a ROCm GPU" in out.stderr
