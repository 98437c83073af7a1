"""No-reference underwater image quality: UIQM (Panetta, Gao, Agaian 2016)
and UCIQE (Yang, Sowmya 2015), the two scores the UIEB paper reports on its
reference-less "challenging" set.

The NumPy float64 functions here are the definition; the HIP kernels in
csrc/nr_metrics.hip match them. Input is a uint8 HxWx3 RGB image with
H, W >= 8. Everything that can be an integer is exact int64 arithmetic.

  UICM    colourfulness: alpha-trimmed means (10% each side, T_L=(N+9)//10,
          T_R=N//10) and full variances of RG = R-G and YB = (R+G-2B)/2.
  UISM    sharpness: per channel, EME over top-left-anchored 8x8 blocks of
          the integer Sobel energy E2 = (gx^2+gy^2)*c^2 (replicate border);
          a block's term is 0.5*ln(max/min), or 0 when min == 0. The usual
          255/max edge normalisation cancels in max/min and is dropped.
  UIConM  contrast: per block over all three channels, t=M-m, s=M+m, term
          (t/s)*ln(t/s), or 0 when t == 0.
  UIQM    0.0282*UICM + 0.2953*UISM + 3.5753*UIConM
  UCIQE   on the project's 8-bit LAB (rgb2lab_u8): 0.4680*sigma_c +
          0.2745*con + 0.2576*mu_s, with chroma c = sqrt(a^2+b^2),
          con the 1%..99% spread of L and mu_s the mean of c/l.

Rows and columns beyond the last whole 8x8 block belong to no block; they
still count in UICM and UCIQE, and as Sobel neighbours.
"""

import numpy as np

from waternet_amd.data.transforms import rgb2lab_u8

KEYS = ("uicm", "uism", "uiconm", "uiqm", "uciqe")
BLOCK = 8


def _check(img: np.ndarray) -> np.ndarray:
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("expected a uint8 HxWx3 RGB image, got "
                         f"{img.dtype} {img.shape}")
    if img.shape[0] < BLOCK or img.shape[1] < BLOCK:
        raise ValueError("no-reference metrics need an image of at least "
                         f"8x8 pixels, got {img.shape[0]}x{img.shape[1]}")
    return img


def trimmed_mean(x: np.ndarray) -> float:
    """Mean of sorted(x)[T_L : N-T_R] with T_L=(N+9)//10, T_R=N//10 (the
    integer forms of ceil/floor(0.1*N), which floating point gets wrong
    for e.g. N=30)."""
    xs = np.sort(np.asarray(x).ravel())
    n = xs.size
    return float(np.mean(xs[(n + 9) // 10: n - n // 10]))


def uicm(img: np.ndarray) -> float:
    v = _check(img).astype(np.int64)
    r, g, b = v[..., 0], v[..., 1], v[..., 2]
    rg = r - g
    yb = (r + g - 2 * b) / 2.0
    mu_rg, mu_yb = trimmed_mean(rg), trimmed_mean(yb)
    var_rg = float(np.mean((rg - mu_rg) ** 2))
    var_yb = float(np.mean((yb - mu_yb) ** 2))
    return float(-0.0268 * np.sqrt(mu_rg * mu_rg + mu_yb * mu_yb)
                 + 0.1586 * np.sqrt(var_rg + var_yb))


def _blocks(plane: np.ndarray) -> np.ndarray:
    """(H,W,...) -> (k2,k1,64,...) over the whole top-left-anchored blocks."""
    k2, k1 = plane.shape[0] // BLOCK, plane.shape[1] // BLOCK
    rest = plane.shape[2:]
    p = plane[: k2 * BLOCK, : k1 * BLOCK].reshape(
        (k2, BLOCK, k1, BLOCK) + rest)
    p = np.moveaxis(p, 2, 1)  # (k2,k1,8,8,...)
    return p.reshape((k2, k1, BLOCK * BLOCK) + rest)


def sobel_energy(chan: np.ndarray) -> np.ndarray:
    """Integer E2 = (gx^2+gy^2)*c^2 of one uint8 channel, replicate border."""
    c = chan.astype(np.int64)
    p = np.pad(c, 1, mode="edge")
    gx = (p[:-2, 2:] + 2 * p[1:-1, 2:] + p[2:, 2:]) \
        - (p[:-2, :-2] + 2 * p[1:-1, :-2] + p[2:, :-2])
    gy = (p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) \
        - (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:])
    return (gx * gx + gy * gy) * (c * c)


def _eme(chan: np.ndarray) -> float:
    e2 = _blocks(sobel_energy(chan))
    mx = e2.max(axis=2).astype(np.float64)
    mn = e2.min(axis=2).astype(np.float64)
    ok = mn > 0
    ratio = np.divide(mx, mn, out=np.ones_like(mx), where=ok)
    terms = np.where(ok, 0.5 * np.log(ratio), 0.0)
    return float(2.0 / terms.size * terms.sum())


def uism(img: np.ndarray) -> float:
    img = _check(img)
    return float(0.299 * _eme(img[..., 0]) + 0.587 * _eme(img[..., 1])
                 + 0.114 * _eme(img[..., 2]))


def uiconm(img: np.ndarray) -> float:
    b = _blocks(_check(img).astype(np.int64))  # (k2,k1,64,3)
    mx = b.max(axis=(2, 3))
    mn = b.min(axis=(2, 3))
    t = (mx - mn).astype(np.float64)
    s = (mx + mn).astype(np.float64)
    ok = t > 0
    q = np.divide(t, s, out=np.ones_like(t), where=ok)
    terms = np.where(ok, q * np.log(q), 0.0)
    return float(-(1.0 / terms.size) * terms.sum())


def _uiqm(cm: float, sm: float, conm: float) -> float:
    return 0.0282 * cm + 0.2953 * sm + 3.5753 * conm


def uiqm(img: np.ndarray) -> float:
    return float(_uiqm(uicm(img), uism(img), uiconm(img)))


def uciqe_from_lab(lab_u8: np.ndarray) -> float:
    """UCIQE of an 8-bit LAB image (L*255/100, a+128, b+128).

    sigma_c^2 = mean(c^2) - mean(c)^2 is evaluated in the shifted form
    mean(d^2) - mean(d)^2 with d = c - c[first pixel]: algebraically the
    same, exactly zero for constant chroma and free of the cancellation
    that the raw form suffers when the chroma spread is small."""
    lab = _check(lab_u8).reshape(-1, 3).astype(np.int64)
    n = lab.shape[0]
    L8 = lab[:, 0]
    ia, ib = lab[:, 1] - 128, lab[:, 2] - 128
    c = np.sqrt((ia * ia + ib * ib).astype(np.float64)) / 255.0
    d = c - c[0]
    md = d.sum() / n
    sigma_c = np.sqrt(max(0.0, (d * d).sum() / n - md * md))
    ls = np.sort(L8)
    con = float(ls[min(n - 1, (99 * n) // 100)] - ls[n // 100]) / 255.0
    pos = L8 > 0
    sat = np.divide(c, L8 / 255.0, out=np.zeros_like(c), where=pos)
    mu_s = sat.sum() / n
    return float(0.4680 * sigma_c + 0.2745 * con + 0.2576 * mu_s)


def uciqe(img: np.ndarray) -> float:
    return uciqe_from_lab(rgb2lab_u8(_check(img)))


def _nr_metrics_cpu(img: np.ndarray) -> np.ndarray:
    cm, sm, conm = uicm(img), uism(img), uiconm(img)
    return np.array([cm, sm, conm, _uiqm(cm, sm, conm), uciqe(img)],
                    dtype=np.float64)


def nr_metrics(x):
    """(N,5) float64 [uicm, uism, uiconm, uiqm, uciqe] per image.

    A NumPy HWC / NHWC uint8 array is scored by the NumPy functions above
    and returns an ndarray; a CUDA (N,H,W,3) uint8 tensor is scored by the
    HIP kernels and returns a tensor on the same device."""
    if isinstance(x, np.ndarray):
        if x.ndim == 3:
            x = x[None]
        if x.ndim != 4:
            raise ValueError(f"expected HWC or NHWC uint8, got {x.shape}")
        return np.stack([_nr_metrics_cpu(im) for im in x]) if len(x) \
            else np.zeros((0, 5), dtype=np.float64)
    import torch

    if not (isinstance(x, torch.Tensor) and x.is_cuda):
        raise TypeError("nr_metrics takes a NumPy uint8 array (CPU path) or "
                        "a CUDA uint8 (N,H,W,3) tensor (HIP path)")
    from waternet_amd.ops import ext

    return ext().nr_metrics(x)
