"""Validation scoring entry point — CLI-compatible with the reference
score.py (/root/reference/score.py:84-177): rebuilds the seed-dependent
train/val split, loads --weights, runs eval over the val split, prints the
metrics dict.

--no-ref DIR scores a folder of images that have no reference instead: mean
no-reference UIQM and UCIQE (waternet_amd.utils.nr_metrics) over the images
in DIR. It needs no dataset, no reference images and no weights.
"""

import argparse
from pathlib import Path
from pprint import pprint

import numpy as np
import torch

from waternet_amd.data.dataset import SyntheticUIEBDataset, UIEBDataset
from waternet_amd.engine.trainer import eval_one_epoch
from waternet_amd.models.vgg import PerceptualModel
from waternet_amd.models.waternet import WaterNet


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    # required unless --no-ref is given (checked below)
    parser.add_argument("--weights", type=str, default=None)
    parser.add_argument("--no-ref", type=str, default=None, metavar="DIR",
                        help="mean no-reference UIQM/UCIQE over the images "
                             "in DIR; needs no dataset, references or "
                             "weights")
    # accepted-but-unused, as the reference (score.py:99-101: scoring takes
    # no epochs; the flag exists there and must keep parsing here)
    parser.add_argument("--epochs", type=int, default=400,
                        help="(unused; reference CLI compatibility)")
    parser.add_argument("--batch-size", type=int, default=16)
    parser.add_argument("--height", type=int, default=112)
    parser.add_argument("--width", type=int, default=112)
    parser.add_argument("--seed", type=int, default=None)
    parser.add_argument("--data-root", type=str, default="data")
    parser.add_argument("--synthetic", type=int, default=None)
    parser.add_argument("--engine", choices=["auto", "fast", "eager"],
                        default="auto",
                        help="fast = GPU preprocess + native eval (same "
                             "metrics; minutes -> seconds on real datasets)")
    parser.add_argument("--num-workers", type=int, default=0,
                        help="DataLoader workers for the val loader "
                             "(parallelizes the CPU preprocess on the "
                             "eager engine; reference default 0)")
    args = parser.parse_args(argv)
    if args.weights is None and args.no_ref is None:
        parser.error("the following arguments are required: --weights")
    return args


def score_no_ref(dirpath):
    """Mean UIQM / UCIQE and image count over the images in dirpath; on a
    GPU with the native extension the HIP kernels score them."""
    from PIL import Image

    from inference import IM_SUFFIXES
    from waternet_amd.ops import native_available
    from waternet_amd.utils.nr_metrics import KEYS, nr_metrics

    root = Path(dirpath)
    if not root.is_dir():
        raise SystemExit(f"--no-ref: {dirpath} is not a directory")
    paths = sorted(p for p in root.iterdir()
                   if p.suffix.lower() in IM_SUFFIXES)
    if not paths:
        raise SystemExit(f"--no-ref: no images found in {dirpath}")
    on_gpu = torch.cuda.is_available() and native_available()
    total = None
    for p in paths:
        with Image.open(p) as im:
            rgb = np.ascontiguousarray(im.convert("RGB"))
        if on_gpu:
            m = nr_metrics(torch.from_numpy(rgb).unsqueeze(0).cuda())
        else:
            m = nr_metrics(rgb)
        total = m if total is None else total + m
    if on_gpu:
        total = total.cpu().numpy()
    mean = total[0] / len(paths)
    metrics = {"uiqm": float(mean[KEYS.index("uiqm")]),
               "uciqe": float(mean[KEYS.index("uciqe")]),
               "images": len(paths)}
    pprint(metrics)
    return metrics


def main(argv=None):
    args = parse_args(argv)
    if args.no_ref is not None:
        return score_no_ref(args.no_ref)
    torch.manual_seed(0)
    if args.seed is not None:
        torch.manual_seed(args.seed)

    device = torch.device("cuda" if torch.cuda.is_available() else "cpu")

    use_fast = args.engine != "eager" and device.type == "cuda" \
        and args.height % 8 == 0 and args.width % 8 == 0
    if use_fast:
        from waternet_amd.ops import native_available

        use_fast = native_available()
    if args.engine == "fast" and not use_fast:
        raise SystemExit("--engine fast requires a ROCm GPU with the "
                         "native extension and H,W divisible by 8")

    if args.synthetic is not None:
        dataset = SyntheticUIEBDataset(
            n_images=args.synthetic, im_height=args.height,
            im_width=args.width, raw_mode=use_fast,
        )
        n_val = max(1, int(0.1 * len(dataset)))
        split = [len(dataset) - n_val, n_val]
    else:
        dataset = UIEBDataset(
            Path(args.data_root) / "raw-890",
            Path(args.data_root) / "reference-890",
            im_height=args.height,
            im_width=args.width,
            raw_mode=use_fast,
        )
        split = [800, 90]
    if len(dataset) != sum(split):
        raise SystemExit(
            f"the UIEB 800/90 split (reference train.py:233) needs exactly "
            f"{sum(split)} images; found {len(dataset)} under "
            f"{args.data_root}")
    _, val_dataset = torch.utils.data.random_split(dataset, split)
    val_loader = torch.utils.data.DataLoader(val_dataset,
                                             batch_size=args.batch_size,
                                             num_workers=args.num_workers)

    model = WaterNet()
    if not Path(args.weights).is_file():
        raise SystemExit(f"weights file not found: {args.weights}")
    with open(args.weights, "rb") as f:
        model.load_state_dict(torch.load(f, map_location="cpu"))
    model.to(device).eval()

    vgg_model = PerceptualModel().to(device).eval()

    if use_fast:
        # GPU preprocess + native NHWC eval (same metric definitions; the
        # same-checkpoint eager/fast scores cross-validated within noise)
        from waternet_amd.engine.fast import VAL_KEYS, eval_metrics_batch

        sums = torch.zeros(4, dtype=torch.float64, device=device)
        n_batches = 0
        for batch in val_loader:
            sums += eval_metrics_batch(
                model, vgg_model,
                batch["raw"].to(device, non_blocking=True),
                batch["ref"].to(device, non_blocking=True))
            n_batches += 1
        vals = (sums / max(n_batches, 1)).tolist()
        metrics = dict(zip(VAL_KEYS, vals))
    else:
        metrics = eval_one_epoch(model, val_loader, device, vgg_model)
    pprint(metrics)
    return metrics


if __name__ == "__main__":
    main()
