"""Inference entry point — CLI-compatible with the reference inference.py
(/root/reference/inference.py): --source image/video/directory, --weights,
--name, --show-split. Images are enhanced one by one; videos frame by frame
(bs=1, fixed shapes — on GPU this path is hipGraph-captured via
waternet_amd.engine.inferencer).

Differences from the reference, forced by this environment:
  - PIL replaces OpenCV for image IO (no cv2 wheel offline); --show-split
    text is drawn with PIL instead of cv2.putText.
  - Video IO uses the ffmpeg binary when present; otherwise video sources
    raise a clear error (no cv2.VideoCapture available).
  - No weight auto-download (no network): --weights is optional but
    random-init weights produce garbage, so a warning is printed.
"""

import argparse
import sys
from pathlib import Path

import numpy as np
import torch

from waternet_amd.data.bridge import arr2ten, ten2arr
from waternet_amd.data.transforms import transform
from waternet_amd.models.waternet import WaterNet

# strict supersets of the reference's lists (inference.py:17-18: bmp/jpg/
# jpeg/png/gif and mp4/mpeg/avi) — PIL takes the first frame of a .gif
IM_SUFFIXES = [".bmp", ".jpg", ".jpeg", ".png", ".gif", ".tiff", ".webp"]
VID_SUFFIXES = [".mp4", ".mpeg", ".avi", ".mov", ".mkv", ".webm"]


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--source", type=str, required=True,
                        help="image / video / directory of images")
    parser.add_argument("--weights", type=str, default=None)
    parser.add_argument("--name", type=str, default=None,
                        help="output subdirectory name under ./output")
    parser.add_argument("--show-split", action="store_true",
                        help="write before/after composites")
    parser.add_argument("--report-quality", action="store_true",
                        help="print no-reference UIQM/UCIQE before and "
                             "after per source and append them to "
                             "<savedir>/quality.csv")
    parser.add_argument("--temporal-smooth", type=float, default=None,
                        metavar="A",
                        help="video sources only: smooth the white-balance "
                             "clip points and CLAHE tile LUTs over the "
                             "frames with weight A in (0,1] on the new "
                             "frame (1 = per-frame statistics, smaller = "
                             "steadier); default off. Images stay "
                             "independent.")
    parser.add_argument("--scene-cut", type=float, default=0.5, metavar="T",
                        help="with --temporal-smooth: restart the smoothing "
                             "when the luminance histogram changes by more "
                             "than the fraction T in [0,1] of its largest "
                             "possible change. The default 0.5 is untuned "
                             "on real footage.")
    args = parser.parse_args(argv)
    a = args.temporal_smooth
    if a is not None and not 0.0 < a <= 1.0:  # also false for nan
        parser.error(f"--temporal-smooth must be in (0,1], got {a}")
    if not 0.0 <= args.scene_cut <= 1.0:
        parser.error(f"--scene-cut must be in [0,1], got {args.scene_cut}")
    return args


def make_savedir(name):
    """Pick output/<name or next number>. The directory itself is created
    as late as possible — at the first write — so failed runs leave no
    empty savedirs (reference inference.py:198-200)."""
    outputdir = Path("output")
    if name is not None:
        return outputdir / name
    nums = [int(p.stem) for p in outputdir.glob("*")
            if p.is_dir() and p.stem.isdecimal()] if outputdir.is_dir() \
        else []
    return outputdir / str(max(nums) + 1 if nums else 0)


def load_model(weights, device):
    """--weights path, or the reference's auto-download scheme (reference
    inference.py:15-21,103-109): fetch the published hash-named checkpoint
    next to this script with torch.hub's check_hash; falls back to a
    random-init warning when offline."""
    model = WaterNet()
    if weights is not None:
        with open(weights, "rb") as f:
            model.load_state_dict(torch.load(f, map_location="cpu"))
    else:
        import hubconf

        wd = Path(__file__).resolve().parent
        local = wd / hubconf.WEIGHTS_FILE
        try:
            if local.exists():
                model.load_state_dict(torch.load(local, map_location="cpu"))
            else:
                sd = torch.hub.load_state_dict_from_url(
                    hubconf.WEIGHTS_URL, map_location="cpu",
                    model_dir=str(wd), file_name=hubconf.WEIGHTS_FILE,
                    check_hash=True,
                )
                model.load_state_dict(sd)
        except Exception as e:  # noqa: BLE001 — offline environment
            print(
                "WARNING: no --weights given and auto-download failed "
                f"({e!r}); using random-init weights.",
                file=sys.stderr,
            )
    model.to(device).eval()
    return model


_ENGINES = {}


def _gpu_engine(model, h, w, device, temporal=None):
    key = (id(model), h, w) if temporal is None else \
        (id(model), h, w, temporal.alpha, temporal.scene_cut)
    eng = _ENGINES.get(key)
    if eng is None:
        from waternet_amd.engine.inferencer import InferenceEngine

        kw = {} if temporal is None else dict(
            temporal_alpha=temporal.alpha, scene_cut=temporal.scene_cut)
        eng = InferenceEngine(model, h, w, device=device, **kw)
        _ENGINES[key] = eng
    return eng


class VideoTemporal:
    """--temporal-smooth state of ONE video: which path carries the
    smoothed statistics (the GPU engine's device state or the CPU
    TemporalStabilizer) and its scene-cut count. A new one per video is
    what resets the state: engines are cached across videos."""

    def __init__(self, alpha, scene_cut):
        self.alpha, self.scene_cut = alpha, scene_cut
        self._engine = None
        self._cpu = None

    def engine(self, model, h, w, device):
        eng = _gpu_engine(model, h, w, device, self)
        if eng is not self._engine:  # first frame of this video
            eng.reset_temporal()
            self._engine = eng
        return eng

    def cpu_transform(self, rgb):
        if self._cpu is None:
            from waternet_amd.data.temporal import TemporalStabilizer

            self._cpu = TemporalStabilizer(self.alpha, self.scene_cut)
        return self._cpu.transform(rgb)

    def cuts(self):
        if self._engine is not None:
            return self._engine.temporal_counters()["cuts"]
        return self._cpu.cuts if self._cpu is not None else 0


QUALITY_HEADER = ("source,frames,uiqm_before,uiqm_after,uciqe_before,"
                  "uciqe_after,uicm_before,uicm_after,uism_before,uism_after,"
                  "uiconm_before,uiconm_after")


class QualityReport:
    """--report-quality state of one source: the (2,5) before/after
    no-reference metrics summed over its frames. On the GPU path the sum
    stays on the device and is read once, in finish()."""

    def __init__(self):
        self.total = None
        self.frames = 0

    def add(self, pair):
        self.total = pair if self.total is None else self.total + pair
        self.frames += 1

    def add_cpu(self, before: np.ndarray, after: np.ndarray):
        from waternet_amd.utils.nr_metrics import nr_metrics

        self.add(np.concatenate([nr_metrics(before), nr_metrics(after)]))

    def finish(self, name: str, savedir: Path):
        if self.frames == 0:
            return
        total = self.total
        if isinstance(total, torch.Tensor):
            total = total.cpu().numpy()  # the one host read of this source
        m = total / self.frames
        # m rows: before, after; columns: uicm, uism, uiconm, uiqm, uciqe
        print(f"{name}: UIQM {m[0, 3]:.4f} -> {m[1, 3]:.4f}, "
              f"UCIQE {m[0, 4]:.4f} -> {m[1, 4]:.4f} "
              f"({self.frames} frame{'s' if self.frames != 1 else ''})")
        savedir.mkdir(parents=True, exist_ok=True)
        csv = savedir / "quality.csv"
        new = not csv.exists()
        with open(csv, "a") as f:
            if new:
                f.write(QUALITY_HEADER + "\n")
            vals = [m[r, c] for c in (3, 4, 0, 1, 2) for r in (0, 1)]
            f.write(",".join([name, str(self.frames)]
                             + ["%.6f" % v for v in vals]) + "\n")


@torch.no_grad()
def enhance_frame(model, rgb: np.ndarray, device,
                  quality=None, temporal=None) -> np.ndarray:
    """uint8 HWC RGB -> enhanced uint8 HWC RGB. On GPU the whole frame
    pipeline (preprocess + forward + postprocess) runs as a hipGraph-
    captured on-device pipeline; on CPU the reference-semantics numpy
    transforms + eager model run. A QualityReport, when given, is fed the
    frame's before/after no-reference metrics. A VideoTemporal, when given,
    makes the frame the next one of its video: the WB/CLAHE statistics are
    smoothed over the frames instead of taken from this frame alone."""
    if device.type == "cuda":
        from waternet_amd.ops import native_available

        if native_available():
            from waternet_amd.engine.inferencer import pad8

            padded, h, w = pad8(rgb)
            if temporal is None:
                eng = _gpu_engine(model, padded.shape[0], padded.shape[1],
                                  device)
            else:
                eng = temporal.engine(model, padded.shape[0],
                                      padded.shape[1], device)
            out = eng.infer_frame(padded)[:h, :w]
            if quality is not None:
                quality.add(eng.frame_quality(h, w))
            return out
    wb, gc, he = transform(rgb) if temporal is None \
        else temporal.cpu_transform(rgb)
    rgb_ten = arr2ten(rgb, add_batch_dim=True).to(device)
    wb_ten = arr2ten(wb, add_batch_dim=True).to(device)
    gc_ten = arr2ten(gc, add_batch_dim=True).to(device)
    he_ten = arr2ten(he, add_batch_dim=True).to(device)
    # he fills the `ce` slot — reference call order (inference.py:191)
    out = ten2arr(model(rgb_ten, wb_ten, he_ten, gc_ten))[0]
    if quality is not None:
        quality.add_cpu(rgb, out)
    return out


def compose_split(before: np.ndarray, after: np.ndarray) -> np.ndarray:
    """Left half original ('Before'), right half enhanced ('After'),
    replicating the reference's --show-split composite
    (inference.py:202-233)."""
    from PIL import Image, ImageDraw

    h, w = before.shape[:2]
    comp = np.concatenate([before[:, : w // 2], after[:, w // 2:]], axis=1)
    im = Image.fromarray(comp)
    draw = ImageDraw.Draw(im)
    draw.line([(w // 2, 0), (w // 2, h)], fill=(255, 255, 255), width=2)
    draw.text((10, 10), "Before", fill=(255, 255, 255))
    draw.text((w // 2 + 10, 10), "After", fill=(255, 255, 255))
    return np.asarray(im)


def run_image(model, path: Path, savedir: Path, device, show_split,
              report_quality=False):
    from PIL import Image

    quality = QualityReport() if report_quality else None
    with Image.open(path) as im:
        rgb = np.asarray(im.convert("RGB"))
    out = enhance_frame(model, rgb, device, quality)
    result = compose_split(rgb, out) if show_split else out
    savedir.mkdir(parents=True, exist_ok=True)  # late, ref inference.py:198
    Image.fromarray(result).save(savedir / path.name)
    if quality is not None:
        quality.finish(path.name, savedir)


def run_video(model, path: Path, savedir: Path, device, show_split,
              report_quality=False, temporal_smooth=None, scene_cut=0.5):
    from waternet_amd.engine.video import FFmpegReader, FFmpegWriter

    quality = QualityReport() if report_quality else None
    temporal = None if temporal_smooth is None \
        else VideoTemporal(temporal_smooth, scene_cut)
    reader = FFmpegReader(path)
    savedir.mkdir(parents=True, exist_ok=True)  # late, ref inference.py:198
    outpath = savedir / path.name
    writer = FFmpegWriter(outpath, reader.width, reader.height, reader.fps)
    n = 0
    for frame in reader:
        out = enhance_frame(model, frame, device, quality, temporal)
        writer.write(compose_split(frame, out) if show_split else out)
        n += 1
        if n % 50 == 0:
            print(f"{n} frames processed")
    writer.close()
    print(f"Wrote {n} frames to {outpath}")
    if temporal is not None:
        print(f"Scene cuts: {temporal.cuts()}")
    if quality is not None:
        quality.finish(path.name, savedir)


def main(argv=None):
    args = parse_args(argv)
    device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    print(f"Using device: {device}")

    source = Path(args.source)
    if not source.exists():
        raise SystemExit(f"{args.source} does not exist!")
    if source.is_dir():
        # both images and videos, as the reference (inference.py:128-135)
        sources = sorted(
            p for p in source.iterdir()
            if p.suffix.lower() in IM_SUFFIXES
            or p.suffix.lower() in VID_SUFFIXES
        )
    else:
        sources = [source]
    print(f"Total images/videos: {len(sources)}")

    model = load_model(args.weights, device)
    savedir = make_savedir(args.name)

    for p in sources:
        if p.suffix.lower() in VID_SUFFIXES:
            run_video(model, p, savedir, device, args.show_split,
                      args.report_quality, args.temporal_smooth,
                      args.scene_cut)
        elif p.suffix.lower() in IM_SUFFIXES:
            run_image(model, p, savedir, device, args.show_split,
                      args.report_quality)
        else:
            print(f"Skipping unrecognized suffix: {p}", file=sys.stderr)

    print(f"Results saved to {savedir}")


if __name__ == "__main__":
    main()
