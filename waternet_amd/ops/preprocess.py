"""GPU-native batch preprocess (white balance / gamma / CLAHE hist-eq).

gpu_transform_batch replaces the reference's per-image CPU transform loop
(data.py:81-90; the dataloader bottleneck per SURVEY §6) with 7 CDNA4
kernels over the whole uint8 batch on-device.

gpu_transform_stream is the video variant: the same 7 kernels with
k_temporal_blend between the statistics and the apply half, smoothing the
clip points and tile LUTs over the frames of N independent streams
(definition: waternet_amd/data/temporal.py).
"""

import torch

from waternet_amd.ops import ext


def gpu_transform_batch(raw_u8: torch.Tensor):
    """raw_u8: (N,H,W,3) uint8 CUDA -> (wb, gc, he) uint8 same shape.
    Requires H, W divisible by 8 (CLAHE tile grid); callers fall back to the
    CPU transforms otherwise."""
    assert raw_u8.is_cuda and raw_u8.dtype == torch.uint8
    wb, gc, he = ext().preprocess_all(raw_u8.contiguous())
    return wb, gc, he


def new_temporal_state(n: int, device) -> dict:
    """Zeroed state of n streams for gpu_transform_stream: has_state == 0,
    so each stream's next frame is its frame 0."""
    z = dict(device=device)
    return {
        "wb": torch.zeros(n, 3, 2, dtype=torch.float32, **z),
        "lut": torch.zeros(n, 64, 256, dtype=torch.float32, **z),
        "lhist": torch.zeros(n, 256, dtype=torch.int32, **z),
        # [has_state, frames, cuts] per stream
        "counters": torch.zeros(n, 3, dtype=torch.int32, **z),
        # the rounded LUTs the current frame is transformed with
        "lut_u8": torch.zeros(n, 64, 256, dtype=torch.uint8, **z),
    }


def gpu_transform_stream(raw_u8: torch.Tensor, state: dict, alpha: float,
                         cut_count: int):
    """One frame of each of N streams: raw_u8 (N,H,W,3) uint8 CUDA ->
    (wb, gc, he), `state` (new_temporal_state) updated in place. No host
    read: the whole step can be captured in a graph."""
    e = ext()
    raw = raw_u8.contiguous()
    wb_params, luts, lab, tile_hists = e.preprocess_stats(raw)
    e.temporal_blend(state["wb"], state["lut"], state["lhist"],
                     state["counters"], state["lut_u8"], wb_params, luts,
                     tile_hists, alpha, cut_count)
    wb, gc, he = e.preprocess_apply(raw, lab, state["wb"], state["lut_u8"])
    return wb, gc, he
