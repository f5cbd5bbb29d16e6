"""The serving resize in exact (fp64) arithmetic: the oracle of
``ops.resize_u8_ragged`` (csrc/kernels/resize.hip) and of the native
``resize_u8_host``, before rounding to u8.

Geometry: short side -> S, long side floor(S * long / short), centre crop at
((RH - S) // 2, (RW - S) // 2); an S x S source is copied. Per axis
(n_in -> n_out, scale = n_in / n_out), output index i before the crop:

* plain: s = clamp(scale * (i + 0.5) - 0.5, 0, n_in - 1), taps floor(s) and
  min(floor(s) + 1, n_in - 1) with weights 1 - frac(s), frac(s);
* antialiased: sup = max(scale, 1), c = scale * (i + 0.5), taps j in
  [max(0, int(c - sup + 0.5)), min(n_in, int(c + sup + 0.5))) with weights
  max(0, 1 - |(j - c + 0.5) / sup|), normalised to sum 1 (PIL's and torch's
  ``antialias=True`` bilinear).
"""
from __future__ import annotations

import numpy as np


def resized_dims(h: int, w: int, size: int) -> tuple[int, int]:
    return (size, size * w // h) if h <= w else (size * h // w, size)


def axis_weights(n_in: int, n_out: int, first: int, count: int, antialias: bool) -> np.ndarray:
    """fp64 [count, n_in]: row k holds the weights of output index first + k."""
    W = np.zeros((count, n_in), dtype=np.float64)
    scale = n_in / n_out
    for k in range(count):
        i = first + k
        if antialias:
            sup = max(scale, 1.0)
            c = scale * (i + 0.5)
            lo, hi = max(0, int(c - sup + 0.5)), min(n_in, int(c + sup + 0.5))
            j = np.arange(lo, hi)
            wj = np.maximum(0.0, 1.0 - np.abs((j - c + 0.5) / sup))
            W[k, lo:hi] = wj / wj.sum()
        else:
            s = min(max(scale * (i + 0.5) - 0.5, 0.0), n_in - 1.0)
            i0 = int(s)
            i1 = min(i0 + 1, n_in - 1)
            W[k, i0] += 1.0 - (s - i0)
            W[k, i1] += s - i0
    return W


def _weights(h: int, w: int, size: int, antialias: bool) -> tuple[np.ndarray, np.ndarray]:
    rh, rw = resized_dims(h, w, size)
    return (axis_weights(h, rh, (rh - size) // 2, size, antialias),
            axis_weights(w, rw, (rw - size) // 2, size, antialias))


def resize_exact(img: np.ndarray, size: int, antialias: bool) -> np.ndarray:
    """u8 [H, W, 3] -> fp64 [size, size, 3], not rounded."""
    h, w, _ = img.shape
    x = img.astype(np.float64)
    if h == size and w == size:
        return x
    wy, wx = _weights(h, w, size, antialias)
    return np.einsum("yr,rxc,ox->yoc", wy, x, wx, optimize=True)


__all__ = ["resized_dims", "axis_weights", "resize_exact"]
