"""hipGraph-captured per-frame inference engine (BASELINE config 4).

The reference's video loop (inference.py:261-323) runs CPU preprocess +
bs=1 forward + CPU postprocess per frame. This engine keeps the whole frame
pipeline on-GPU with fixed shapes and captures it in ONE hipGraph:

  raw u8 frame (static buffer) -> GPU preprocess (wb/gamma/clahe)
  -> fused input build -> WaterNet forward (MFMA kernels)
  -> fused postprocess (clip*255 -> u8)

Per frame at steady state: one H2D copy in, one graph replay, one D2H copy
out. Falls back to eager kernel launches if capture fails.
"""

import numpy as np
import torch

from waternet_amd.ops import ext
from waternet_amd.ops.preprocess import (gpu_transform_batch,
                                         gpu_transform_stream,
                                         new_temporal_state)


def pad8(rgb_u8: np.ndarray):
    """Reflect-pad an HWC frame to the next multiple of 8 per side (the
    GPU CLAHE tile-grid requirement). Returns (padded, orig_h, orig_w).

    Note: the padded rows/cols (<= 7 px, reflected) participate in the
    WB quantile and CLAHE tile statistics — a boundary-only deviation
    from the CPU transforms, accepted so ANY resolution runs the
    hipGraph GPU pipeline (crop back with [:h, :w] after)."""
    h, w = rgb_u8.shape[:2]
    ph, pw = (-h) % 8, (-w) % 8
    if ph == 0 and pw == 0:
        return rgb_u8, h, w
    return (np.pad(rgb_u8, ((0, ph), (0, pw), (0, 0)), mode="reflect"),
            h, w)


class InferenceEngine:
    def __init__(self, model, height, width, device="cuda:0",
                 use_graph=True, temporal_alpha=None, scene_cut=0.5):
        """temporal_alpha in (0,1] turns on temporally smoothed WB/CLAHE
        statistics (waternet_amd/data/temporal.py) for a video stream, with
        a state reset where the L histogram moves by more than scene_cut of
        its range; None is the per-frame pipeline."""
        self.model = model.eval()
        self.device = torch.device(device)
        self.h, self.w = height, width
        self.raw_static = torch.empty(1, height, width, 3,
                                      dtype=torch.uint8, device=self.device)
        self.out_static = None
        self._graph = None
        self._use_graph = use_graph and height % 8 == 0 and width % 8 == 0
        self._temporal = None
        if temporal_alpha is not None:
            from waternet_amd.data.temporal import (check_alpha,
                                                    scene_cut_count)

            # allocated here, outside capture: the state outlives replays
            self._temporal = new_temporal_state(1, self.device)
            self._alpha = check_alpha(temporal_alpha)
            self._cut_count = scene_cut_count(scene_cut, height, width)

    @torch.no_grad()
    def _body(self):
        from waternet_amd.engine.native import waternet_forward_from_inputs

        raw = self.raw_static
        if self._temporal is None:
            wb, gc, he = gpu_transform_batch(raw)
        else:
            wb, gc, he = gpu_transform_stream(raw, self._temporal,
                                              self._alpha, self._cut_count)
        e = ext()
        # he fills the ce slot (reference inference.py:191 -> net.py:99);
        # full-NHWC: fused uint8 cat-fold -> convs -> fused u8 postprocess,
        # no NCHW tensor anywhere in the frame pipeline.
        inputs = e.build_inputs_u8(raw, wb, he, gc)
        out_nhwc = waternet_forward_from_inputs(self.model, *inputs)
        self.out_static = e.out_to_u8(out_nhwc)

    def _capture(self):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                self._body()
        torch.cuda.current_stream().wait_stream(s)
        try:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._body()
            self._graph = g
        except Exception as e:  # noqa: BLE001
            import sys

            print(f"[inferencer] graph capture failed, eager: {e!r}",
                  file=sys.stderr)
            self._use_graph = False
        # warm-up and capture ran _body on whatever the buffer held: the
        # first real frame is frame 0
        self.reset_temporal()

    def reset_temporal(self):
        """Start a new stream: the next frame initialises the state. One
        memset of [has_state, frames, cuts], outside the graph."""
        if self._temporal is not None:
            self._temporal["counters"].zero_()

    def temporal_counters(self) -> dict:
        """{frames, cuts} of the current stream (one host read)."""
        if self._temporal is None:
            raise RuntimeError("temporal_counters() needs an engine built "
                               "with temporal_alpha")
        _, frames, cuts = self._temporal["counters"][0].tolist()
        return {"frames": frames, "cuts": cuts}

    @torch.no_grad()
    def infer_frame(self, rgb_u8: np.ndarray) -> np.ndarray:
        """uint8 HWC RGB frame -> enhanced uint8 HWC RGB."""
        assert rgb_u8.shape == (self.h, self.w, 3)
        # from_numpy on a read-only array (e.g. PIL-derived) warns once;
        # intentional zero-copy — the tensor is only ever READ by copy_
        self.raw_static.copy_(
            torch.from_numpy(np.ascontiguousarray(rgb_u8)).unsqueeze(0)
        )
        if self._use_graph and self._graph is None:
            self._capture()
        if self._graph is not None:
            self._graph.replay()
        else:
            self._body()
        return self.out_static[0].cpu().numpy()

    @torch.no_grad()
    def frame_quality(self, h=None, w=None) -> torch.Tensor:
        """No-reference quality of the last frame: a (2,5) float64 device
        tensor [uicm, uism, uiconm, uiqm, uciqe], row 0 the uploaded frame
        (before), row 1 the enhanced one (after), both cropped to [:h, :w]
        so a padded engine scores only real pixels. Runs eagerly after the
        replay; the captured graph does not contain it."""
        from waternet_amd.utils.nr_metrics import nr_metrics

        if self.out_static is None:
            raise RuntimeError("frame_quality() needs a frame: call "
                               "infer_frame() first")
        h = self.h if h is None else h
        w = self.w if w is None else w
        if not (0 < h <= self.h and 0 < w <= self.w):
            raise ValueError(f"crop {h}x{w} outside the {self.h}x{self.w} "
                             "engine")
        pair = torch.cat([self.raw_static[:, :h, :w],
                          self.out_static[:, :h, :w]])
        return nr_metrics(pair)
