"""Benchmark entry point (driver contract).

Measures the flagship workload: WaterNet training, bs=16/GPU, 112x112, bf16
compute, on synthetic data with random-init weights — the BASELINE.json
metric ("train images/sec whole node at 112x112 bs=16/GPU"). Each timed step
performs the full reference per-minibatch work: preprocess
(white balance + gamma + CLAHE, GPU-native), forward, VGG-perceptual + MSE
loss, backward, Adam + StepLR, and the SSIM/PSNR minibatch metrics
(accumulated on-device; the reference's per-step .item() syncs are not
replicated inside the timed loop).

Usage: python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR]
For N>1 the driver launches this under torch.distributed.run with one rank
per GPU (RCCL); `value` is the whole-job aggregate images/sec.

A plain run does only what the headline figure needs: set up, warm up, time
the K steps, optionally write the outputs, print the result line. `--full`
is where any further measurement or check belongs (none exists today, so
it currently changes nothing).

`--dump-outputs DIR` writes what the last timed step left behind, as
DIR/<name>.npy. The inputs are seeded, and a dump run rewinds the trainer
to its initial state (with the clock stopped) just before the last timed
step, so that step sees the same state and batch every run and two builds
run with the same arguments can be compared array for array:
  train:      params, grads (the FusedAdam fp32 flat arenas after the
              step), metric_sums (float64, TRAIN_KEYS order, of that step)
  infer1080p: frame (the enhanced HWC frame the last call returned)
"""

import argparse
import json
import os
import time

import torch

BASELINE_IMG_PER_SEC = 12.8  # reference epoch-400 throughput


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--batch-size", type=int, default=16)
    p.add_argument("--height", type=int, default=112)
    p.add_argument("--width", type=int, default=112)
    p.add_argument("--no-graph", action="store_true",
                   help="disable hipGraph capture of the train step")
    p.add_argument("--mode", choices=["train", "infer1080p"], default="train",
                   help="train = flagship training step (driver metric); "
                        "infer1080p = BASELINE config 4, hipGraph-captured "
                        "bs=1 1080p per-frame video inference")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write the last step's "
                        "outputs to DIR/<name>.npy")
    p.add_argument("--full", action="store_true",
                   help="also run every extra measurement and check beyond "
                        "the headline figure (none today)")
    return p.parse_args()


def dump_outputs(out_dir, arrays):
    """Write {name: tensor | ndarray} as out_dir/<name>.npy, float32 or
    float64. Everything dumped here is far below the 64 MB budget (the
    largest is the 1080p frame, 25 MB as float32), so nothing is sampled."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        a = torch.as_tensor(a).detach().cpu()
        if a.dtype != torch.float64:
            a = a.float()
        a = a.numpy()
        np.save(os.path.join(out_dir, f"{name}.npy"), a)


_ARENAS = ("master", "grads", "exp_avg", "exp_avg_sq", "step_buf")


def snapshot_state(trainer):
    """Copy of everything a train step reads and advances: the FusedAdam
    arenas and step counters, the StepLR state and the metric sums."""
    o = trainer.opt
    return {
        "arenas": {k: getattr(o, k).clone() for k in _ARENAS},
        "metric": trainer.metric_sums.clone(),
        "host_step": o._step,
        "steps": trainer._steps,
        "lr": o.param_groups[0]["lr"],
        "sched": trainer.sched.state_dict(),
    }


def restore_state(trainer, snap):
    """Rewind the trainer to snapshot_state()'s point (the same buffers a
    graph capture rewinds, plus the scheduler). The captured graph and the
    data pool position are kept."""
    o = trainer.opt
    for k in _ARENAS:
        getattr(o, k).copy_(snap["arenas"][k])
    trainer.metric_sums.copy_(snap["metric"])
    o._step = snap["host_step"]
    trainer._steps = snap["steps"]
    trainer.sched.load_state_dict(snap["sched"])
    o.param_groups[0]["lr"] = snap["lr"]
    o._mark_model_dirty()  # packed-weight caches reflect restored masters


def infer1080p(args):
    """BASELINE config 4: 1080p (1920x1088, /32-padded as the reference
    requires multiples of 32 — training_utils.py:99-103) bs=1 per-frame
    pipeline, hipGraph-captured: H2D -> GPU preprocess -> forward -> fused
    u8 postprocess -> D2H."""
    import numpy as np

    from waternet_amd.engine.inferencer import InferenceEngine
    from waternet_amd.models.waternet import WaterNet

    h, w = 1088, 1920
    torch.manual_seed(0)
    model = WaterNet().to("cuda:0")
    eng = InferenceEngine(model, h, w, device="cuda:0",
                          use_graph=not args.no_graph)
    rng = np.random.default_rng(0)
    frames = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
              for _ in range(4)]
    for i in range(max(args.warmup, 2)):
        eng.infer_frame(frames[i % len(frames)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = None
    for i in range(args.steps):
        out = eng.infer_frame(frames[i % len(frames)])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if args.dump_outputs and out is not None:
        dump_outputs(args.dump_outputs, {"frame": out})
    print(json.dumps({
        "metric": "video inference frames/sec at 1080p bs=1 (hipGraph)",
        "value": args.steps / dt,
        "unit": "frames/sec",
        "n_gpus": 1,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1000.0,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "bf16",
        "data": "synthetic",
        "config": {"model": "waternet", "global_batch": 1,
                   "im_size": f"{h}x{w}", "parallelism": "single",
                   "graph": not args.no_graph},
    }))


def main():
    args = parse_args()
    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local_rank = int(os.environ.get("LOCAL_RANK", rank))

    if not torch.cuda.is_available():
        raise SystemExit("bench.py requires a ROCm GPU")

    if args.mode == "infer1080p":
        infer1080p(args)
        return

    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)

    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        torch.distributed.init_process_group("nccl", rank=rank,
                                             world_size=world)

    from waternet_amd.engine.fast import BenchTrainer

    torch.manual_seed(1234 + rank)
    trainer = BenchTrainer(
        batch_size=args.batch_size,
        height=args.height,
        width=args.width,
        device=device,
        world_size=world,
        seed=1234 + rank,
        # The step is GPU-bound (graph vs eager measured equal at bs=16
        # 112^2); keep the RCCL collective out of graph capture under DDP.
        use_graph=(not args.no_graph) and world == 1,
    )

    if world > 1:
        # all ranks start from rank0's params (one-time, untimed)
        torch.distributed.broadcast(trainer.opt.master, src=0)

    # The step's atomic fp32 accumulation order varies run to run at
    # rounding level, and Adam amplifies that over many steps. So a dump
    # run rewinds to this initial state (clock stopped) just before its
    # last timed step: that step then computes from the same state and
    # batch every run, and the dump differs by rounding only.
    init_state = snapshot_state(trainer) if args.dump_outputs else None

    for _ in range(max(args.warmup, 1)):
        trainer.step()

    if world > 1:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    paused = 0.0
    for i in range(args.steps):
        if init_state is not None and i == args.steps - 1:
            torch.cuda.synchronize()
            p0 = time.perf_counter()
            restore_state(trainer, init_state)
            torch.cuda.synchronize()
            paused = time.perf_counter() - p0
        trainer.step()
    torch.cuda.synchronize()
    if world > 1:
        torch.distributed.barrier()
    t1 = time.perf_counter()

    elapsed = t1 - t0 - paused
    if world > 1:
        t = torch.tensor([elapsed], device=device)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = t.item()

    total_images = world * args.batch_size * args.steps
    value = total_images / elapsed
    ms_per_step = elapsed / args.steps * 1000.0

    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {
            "params": trainer.opt.master,
            "grads": trainer.opt.grads,
            "metric_sums": trainer.metric_sums,
        })

    if rank == 0:
        result = {
            "metric": "train images/sec (whole node) at 112x112 bs=16/GPU",
            "value": value,
            "unit": "images/sec",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": value / BASELINE_IMG_PER_SEC,
            "dtype": "bf16",
            "data": "synthetic",
            "config": {
                "model": "waternet",
                "global_batch": world * args.batch_size,
                "im_size": f"{args.height}x{args.width}",
                "parallelism": f"dp{world}",
                "loss": "0.05*vgg19_perceptual + mse255",
                "preprocess": "gpu wb/gamma/clahe in-step",
            },
        }
        print(json.dumps(result))

    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
