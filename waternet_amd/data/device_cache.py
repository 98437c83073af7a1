"""Device-resident dataset cache for the fast engine.

The UIEB training set at the training resolution is tiny (800 pairs at
112x112 is 60 MB of uint8), yet the DataLoader path decodes, resizes and
uploads it again every epoch. This module decodes and resizes each pair
ONCE, keeps the uint8 HWC pairs on the GPU, and per step has one HIP kernel
(csrc/elementwise.hip k_gather_augment_u8) gather the minibatch and apply
the joint flip/rot90 augmentation straight into the engine's static input
buffers — no per-step host work beyond the launch, no H2D traffic.

Augmentation code (one int32 per batch slot), PairedAugment's semantics
(data/augment.py: hflip, then vflip, then np.rot90 by k):
  bit 0 hflip, bit 1 vflip, bits 2-3 k (counter-clockwise quarter turns,
  0 when the rotation did not fire).
Odd k transposes the image, so it needs H == W; on non-square images k is
replaced by k & 2 (sample_codes(square=False), and the kernel again when
allow_transpose is clear).

Everything above the kernel also runs on CPU tensors through a NumPy
composition of apply_code, so the sampling, ordering and epoch logic are
testable without a GPU. On a GPU the HIP op is mandatory.
"""

from timeit import default_timer as timer

import numpy as np
import torch

P_HFLIP = P_VFLIP = P_ROT90 = 0.5  # PairedAugment defaults


def identity_pair(image, mask):
    """No-op paired transform for UIEBDataset(transform=...): the cache
    stores un-augmented pairs (transform=None there means PairedAugment)."""
    return image, mask


def make_code(hflip, vflip, k):
    return int(bool(hflip)) | (int(bool(vflip)) << 1) | ((int(k) & 3) << 2)


def sample_codes(rng, n, square=True):
    """n augmentation codes drawn per sample in PairedAugment's order and
    with its probabilities: random() hflip, random() vflip, random()
    rotate, then integers(0, 4) only if rotate fired. Scalar draws on
    purpose — a vectorised draw consumes the generator's stream
    differently, and parity with PairedAugment(rng=...) is tested."""
    codes = np.zeros(n, dtype=np.int32)
    for i in range(n):
        h = rng.random() < P_HFLIP
        v = rng.random() < P_VFLIP
        k = 0
        if rng.random() < P_ROT90:
            k = int(rng.integers(0, 4))
        if not square:
            k &= 2
        codes[i] = make_code(h, v, k)
    return codes


def apply_code(img, code):
    """NumPy reference of one augmentation code on an (H, W, C) image."""
    code = int(code)
    if code & 1:
        img = img[:, ::-1]
    if code & 2:
        img = img[::-1]
    k = (code >> 2) & 3
    if k:
        img = np.rot90(img, k)
    return np.ascontiguousarray(img)


def check_indices(idx, n):
    """Host-side validation of cache indices (before any upload)."""
    idx = np.asarray(idx)
    if idx.size and (idx.min() < 0 or idx.max() >= n):
        bad = idx[(idx < 0) | (idx >= n)][0]
        raise IndexError(
            f"device cache index {int(bad)} out of range for {n} cached "
            "pairs")


def gather_augment(cache_raw, cache_ref, idx, codes, out_raw, out_ref,
                   allow_transpose=None):
    """out[b] = apply_code(cache[idx[b]], codes[b]) for raw and ref, in
    place. Device tensors go through the HIP op (one launch for both
    images of every pair); CPU tensors through NumPy. allow_transpose
    defaults to H == W; when clear, k acts as k & 2."""
    h, w = cache_raw.shape[1], cache_raw.shape[2]
    if allow_transpose is None:
        allow_transpose = h == w
    if cache_raw.is_cuda or out_raw.is_cuda:
        from waternet_amd.ops import ext

        ext().gather_augment_u8(cache_raw, cache_ref, idx, codes, out_raw,
                                out_ref, bool(allow_transpose))
        return
    if allow_transpose and h != w:
        raise ValueError("allow_transpose (odd rot90 k) needs H == W")
    idx_np = idx.numpy()
    check_indices(idx_np, cache_raw.shape[0])
    mask = 15 if allow_transpose else 11  # 11 clears k's low bit
    for cache, out in ((cache_raw, out_raw), (cache_ref, out_ref)):
        c, o = cache.numpy(), out.numpy()
        for b, (i, code) in enumerate(zip(idx_np, codes.numpy())):
            o[b] = apply_code(c[int(i)], int(code) & mask)


def build_cache(dataset, device, num_workers=0, batch_size=32):
    """Decode/resize every pair of a raw-mode dataset (or Subset) once and
    return (raw, ref) as two (N, H, W, 3) uint8 tensors on `device`."""
    t0 = timer()
    device = torch.device(device)
    n = len(dataset)
    if n == 0:
        raise ValueError("build_cache: empty dataset")
    first = dataset[0]["raw"]
    if first.dtype != torch.uint8 or first.dim() != 3 or first.shape[2] != 3:
        raise ValueError(
            "build_cache needs a raw-mode dataset yielding {raw, ref} uint8 "
            f"HWC tensors (got {first.dtype} {tuple(first.shape)})")
    h, w = int(first.shape[0]), int(first.shape[1])
    nbytes = 2 * n * h * w * 3
    if device.type == "cuda":
        free, _ = torch.cuda.mem_get_info(device)
        if nbytes > free // 2:
            raise RuntimeError(
                f"device cache of {n} pairs {h}x{w} needs "
                f"{nbytes / 1e6:.0f} MB, more than half of the "
                f"{free / 1e6:.0f} MB free on {device}; train without "
                "--device-cache or at a smaller resolution")
    raw = torch.empty((n, h, w, 3), dtype=torch.uint8, device=device)
    ref = torch.empty_like(raw)
    loader = torch.utils.data.DataLoader(
        dataset, batch_size=batch_size, shuffle=False,
        num_workers=num_workers)
    at = 0
    for batch in loader:
        b = batch["raw"].shape[0]
        if tuple(batch["raw"].shape[1:]) != (h, w, 3):
            raise ValueError("build_cache: images differ in size; pass "
                             "--height/--width so the dataset resizes them")
        raw[at:at + b].copy_(batch["raw"])
        ref[at:at + b].copy_(batch["ref"])
        at += b
    assert at == n, (at, n)
    if device.type == "cuda":
        torch.cuda.synchronize(device)
    print(f"[cache] {n} pairs {h}x{w}, {nbytes / 1e6:.1f} MB, "
          f"built in {timer() - t0:.2f} s")
    return raw, ref


class DeviceEpochSource:
    """Per-epoch (index, code) batches over a cache, as device views.

    epoch(e) builds the whole epoch's order and codes on the host,
    validates them, uploads each array in ONE copy and yields
    (idx_view, codes_view, n) per batch — no per-step host-to-device
    traffic and no sync. Deterministic given (seed, rank, e); it does not
    reproduce DataLoader(shuffle=True)'s order."""

    def __init__(self, cache_raw, cache_ref, batch_size, shuffle=False,
                 augment=False, seed=0, rank=0):
        if cache_raw.shape != cache_ref.shape:
            raise ValueError("cache_raw / cache_ref shapes differ")
        self.cache_raw, self.cache_ref = cache_raw, cache_ref
        self.n = int(cache_raw.shape[0])
        self.batch_size = int(batch_size)
        self.shuffle, self.augment = bool(shuffle), bool(augment)
        self.seed, self.rank = int(seed), int(rank)
        self.square = cache_raw.shape[1] == cache_raw.shape[2]
        self.device = cache_raw.device

    def __len__(self):
        return (self.n + self.batch_size - 1) // self.batch_size

    def host_epoch(self, e):
        """(order int32, codes int32) of epoch e, on the host."""
        key = [self.seed, self.rank, int(e)]
        if self.shuffle:
            g = torch.Generator()
            s = np.random.SeedSequence(key).generate_state(2)
            g.manual_seed((int(s[0]) << 31) ^ int(s[1]))
            order = torch.randperm(self.n, generator=g).numpy()
        else:
            order = np.arange(self.n)
        if self.augment:
            codes = sample_codes(np.random.default_rng(key), self.n,
                                 self.square)
        else:
            codes = np.zeros(self.n, dtype=np.int32)
        return order.astype(np.int32), codes

    def epoch(self, e, order=None):
        """Yield (idx_view, codes_view, n) per batch; the last may be
        short. `order` overrides the epoch's index order (validated like
        the generated one)."""
        gen_order, codes = self.host_epoch(e)
        if order is None:
            order = gen_order
        else:
            order = np.asarray(order)
            if order.shape != gen_order.shape:
                raise ValueError(f"order must hold {self.n} indices")
            check_indices(order, self.n)  # before the int32 cast can wrap
            order = order.astype(np.int32)
        check_indices(order, self.n)
        idx_d = torch.from_numpy(np.ascontiguousarray(order))
        codes_d = torch.from_numpy(np.ascontiguousarray(codes))
        if self.device.type == "cuda":
            idx_d = idx_d.pin_memory().to(self.device, non_blocking=True)
            codes_d = codes_d.pin_memory().to(self.device, non_blocking=True)
        return self._batches(idx_d, codes_d)

    def _batches(self, idx_d, codes_d):
        total = idx_d.shape[0]
        for at in range(0, total, self.batch_size):
            n = min(self.batch_size, total - at)
            yield idx_d[at:at + n], codes_d[at:at + n], n
