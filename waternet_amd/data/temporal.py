"""Temporally stable video enhancement: the NumPy definition.

A per-frame enhancer recomputes the white-balance clip points and the 64
CLAHE tile LUTs from each frame's own histograms, so a torch beam or a fish
crossing a tile moves them from one frame to the next and the output video
flickers. Here they are a small recurrent state per stream, smoothed
exponentially and re-initialised at a scene cut. This module is the
specification the HIP kernel k_temporal_blend (csrc/preprocess.hip) is tested
against, bit for bit, and the CPU path of `inference.py --temporal-smooth`.

State of one stream (TemporalState):
  wb     float32 (3,2)     smoothed lo/hi clip points
  lut    float32 (64,256)  smoothed CLAHE tile LUTs
  lhist  int32 (256)       the previous frame's global L histogram: the sum
                           of the 64 tile histograms before clipping
  has_state, frames, cuts  int counters

One step (temporal_blend), for a frame with per-frame clip points p (float32),
tile LUTs L (uint8) and global L histogram g:
  d   = sum_v |g[v] - lhist[v]|                  exact integer
  cut = has_state == 0 or d > cut_count          integers only
  cut:      wb <- p, lut <- float32(L), cuts += 1 (not for the first frame)
  no cut:   s <- s + a*(x - s) elementwise, float32 a = float32(alpha), every
            operation rounded to float32 on its own (no fused multiply-add)
  always:   lhist <- g, has_state <- 1, frames += 1
The frame is then transformed with the clip points wb and the LUTs
uint8(clip(rint(lut), 0, 255)), rint rounding half to even. Gamma correction
has no state.

cut_count = floor(scene_cut * 2 * H * W) is taken once on the host (d ranges
over [0, 2*H*W]: 2*H*W is two frames with disjoint histograms).

Consequences: the first frame and every cut frame are the per-frame
transform; a constant sequence is a fixed point; alpha = 1 is the per-frame
transform. The last one is exact for the LUTs (integers below 256), and for
clip points that float32 holds exactly, i.e. integer quantiles, which is
every quantile whose two neighbouring order statistics coincide. An
interpolated, fractional clip point may come back from s + 1*(x - s) one
float32 ulp away from x.
"""

from dataclasses import dataclass, field
from typing import Tuple

import numpy as np

from waternet_amd.data.transforms import (
    clahe_apply,
    clahe_luts,
    gamma_correction,
    lab2rgb_u8,
    rgb2lab_u8,
    white_balance_apply,
    white_balance_params,
)


def scene_cut_count(scene_cut: float, height: int, width: int) -> int:
    """The integer threshold on d for a frame of height x width pixels (the
    size the histograms count, padding included)."""
    if not 0.0 <= scene_cut <= 1.0:
        raise ValueError(f"scene_cut must be in [0,1], got {scene_cut}")
    return int(np.floor(scene_cut * 2 * height * width))


def check_alpha(alpha: float) -> float:
    if not 0.0 < alpha <= 1.0:
        raise ValueError(f"alpha must be in (0,1], got {alpha}")
    return float(alpha)


@dataclass
class TemporalState:
    wb: np.ndarray = field(
        default_factory=lambda: np.zeros((3, 2), np.float32))
    lut: np.ndarray = field(
        default_factory=lambda: np.zeros((64, 256), np.float32))
    lhist: np.ndarray = field(
        default_factory=lambda: np.zeros(256, np.int32))
    has_state: int = 0
    frames: int = 0
    cuts: int = 0

    def reset(self):
        self.has_state = self.frames = self.cuts = 0


def temporal_blend(state: TemporalState, p: np.ndarray, luts: np.ndarray,
                   g: np.ndarray, alpha: float,
                   cut_count: int) -> Tuple[np.ndarray, np.ndarray]:
    """One step of the definition above, `state` updated in place.
    p: (3,2) float32, luts: (64,256) uint8, g: (256,) integer.
    Returns the clip points (3,2) float32 and LUTs (64,256) uint8 to
    transform this frame with."""
    p = np.asarray(p)
    luts = np.asarray(luts)
    assert p.dtype == np.float32 and p.shape == (3, 2)
    assert luts.dtype == np.uint8 and luts.shape == (64, 256)
    g = np.asarray(g).astype(np.int64).reshape(256)
    a = np.float32(check_alpha(alpha))
    x_lut = luts.astype(np.float32)

    d = int(np.abs(g - state.lhist.astype(np.int64)).sum())
    cut = state.has_state == 0 or d > cut_count
    if cut:
        state.wb = p.copy()
        state.lut = x_lut
        state.cuts += int(state.has_state != 0)
    else:
        # float32 arrays and a float32 scalar: every op rounds to float32
        state.wb = state.wb + a * (p - state.wb)
        state.lut = state.lut + a * (x_lut - state.lut)
    state.lhist = g.astype(np.int32)
    state.has_state = 1
    state.frames += 1
    used = np.clip(np.rint(state.lut), 0, 255).astype(np.uint8)
    return state.wb.copy(), used


class TemporalStabilizer:
    """The CPU path: transform(rgb) -> (wb, gc, he) like
    data.transforms.transform, with the statistics smoothed over the frames
    of one stream. reset() starts a new stream."""

    def __init__(self, alpha: float, scene_cut: float = 0.5):
        self.alpha = check_alpha(alpha)
        scene_cut_count(scene_cut, 1, 1)  # range check
        self.scene_cut = float(scene_cut)
        self.state = TemporalState()
        self.last_d = None  # d of the last frame, for diagnostics and tests

    def reset(self):
        self.state.reset()
        self.last_d = None

    @property
    def frames(self) -> int:
        return self.state.frames

    @property
    def cuts(self) -> int:
        return self.state.cuts

    def transform(self, rgb: np.ndarray):
        p = white_balance_params(rgb).astype(np.float32)
        lab = rgb2lab_u8(rgb)
        luts, hists = clahe_luts(lab[:, :, 0], clip_limit=0.1,
                                 tile_grid=(8, 8), return_hists=True)
        g = hists.reshape(64, 256).sum(axis=0)
        # the histograms count the image padded to the 8x8 tile grid
        n_pix = int(g.sum())
        st = self.state
        self.last_d = int(np.abs(g - st.lhist.astype(np.int64)).sum()) \
            if st.has_state else None
        cut_count = int(np.floor(self.scene_cut * 2 * n_pix))
        wb_p, used = temporal_blend(st, p, luts.reshape(64, 256), g,
                                    self.alpha, cut_count)
        wb = white_balance_apply(rgb, wb_p)
        gc = gamma_correction(rgb)
        lab[:, :, 0] = clahe_apply(lab[:, :, 0], used.reshape(8, 8, 256),
                                   tile_grid=(8, 8))
        he = lab2rgb_u8(lab)
        return wb, gc, he
