"""Frame sequences shared by test_temporal_cpu.py and test_gpu_temporal.py.

All deterministic (seeded). Independent uniform-random frames are useless
here: their L histograms are all flat, so nothing ever cuts."""

import numpy as np


def gradient_base(h, w, offset, span=60):
    """A smooth diagonal gradient scene, HWC uint8, channel values within
    [offset, offset + span + 20]."""
    y = np.linspace(0.0, 1.0, h)[:, None]
    x = np.linspace(0.0, 1.0, w)[None, :]
    r = offset + span * (0.6 * x + 0.4 * y)
    g = offset + 10 + span * (0.5 * x + 0.5 * (1 - y))
    b = offset + 20 + span * (0.3 * (1 - x) + 0.7 * y)
    return np.stack([r, g, b], axis=-1)


def two_scene_sequence(h, w, per_scene=6, seed=0, offsets=(30, 150)):
    """Two scenes of `per_scene` frames each: a gradient base with its own
    brightness offset plus independent +-2 noise per frame. The one scene
    cut is at frame index `per_scene`."""
    rng = np.random.default_rng(seed)
    frames = []
    for off in offsets:
        base = gradient_base(h, w, off)
        for _ in range(per_scene):
            noise = rng.integers(-2, 3, size=base.shape)
            frames.append(np.clip(np.rint(base) + noise, 0, 255)
                          .astype(np.uint8))
    return frames


def blob_sequence(n=8, h=64, w=64):
    """A static gradient scene with a bright 8x8 blob (inside tile (2,3) of
    the 8x8 grid of 8x8-pixel tiles) on odd frames only. Returns the frames
    and the boolean mask of background pixels: everything outside the
    blob's tile. Those pixels are identical in every frame; per-frame
    statistics still move them, through the WB clip points (whole image)
    and through the blob tile's LUT (bilinear reach: the 8 neighbours)."""
    base = np.clip(np.rint(gradient_base(h, w, 40)), 0, 255).astype(np.uint8)
    th, tw = h // 8, w // 8
    ty, tx = 2, 3
    frames = []
    for t in range(n):
        f = base.copy()
        if t % 2 == 1:
            f[ty * th:ty * th + 8, tx * tw:tx * tw + 8] = 250
        frames.append(f)
    mask = np.ones((h, w), dtype=bool)
    mask[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw] = False
    return frames, mask
