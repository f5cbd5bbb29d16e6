"""The bar of the resize tests (test_resize_aa_cpu.py, test_resize_aa_gpu.py):
a u8 result against the exact (fp64) values of dmlc.utils.resize_ref.

An fp32 rounding argument, not a measurement: fp32 error over <= ~50 separable
taps of values <= 255 is below 0.002, so with EPS = 0.01 every value whose
exact result is further than EPS from a half must equal rint(exact) and the
others may differ by 1; at most 8 % of an image's values may be that close to
a half (a condition on the inputs, which uniform noise meets)."""
import math

import numpy as np

from dmlc.utils.resize_ref import axis_weights, resized_dims

EPS = 0.01


def sixteenths(h, w, size, antialias):
    """True where every filter weight of this resize is a multiple of 1/16: the
    copy case, and the two-tap rule at even integer scales (2, 8, 10), whose
    sample fractions are all exactly one half. fp32 filtering of u8 data is
    then exact (a row sum has at most 12 significant bits, its product with a
    column weight 16, their sum fewer than 24), and a quarter of the exact
    values are ties whatever the pixels."""
    if h == size and w == size:
        return True
    rh, rw = resized_dims(h, w, size)
    axes = (axis_weights(h, rh, (rh - size) // 2, size, antialias),
            axis_weights(w, rw, (rw - size) // 2, size, antialias))
    return all(bool((a * 16 == np.rint(a * 16)).all()) for a in axes)


def compare_u8(got, exact, eps=EPS, ties_exact=False):
    """(share of values within eps of a half; number of values outside that
    set that are not rint(exact); largest |got - rint(exact)|). ties_exact
    (for a `sixteenths` resize, where fp32 is exact): a fraction of exactly one
    half is not excluded, it must be rint's ties-to-even like any other."""
    frac = exact - np.floor(exact)
    near = np.abs(frac - 0.5) <= eps
    if ties_exact:
        near &= frac != 0.5
    d = np.abs(got.astype(np.int64) - np.clip(np.rint(exact), 0, 255).astype(np.int64))
    return float(near.mean()), int((d[~near] != 0).sum()), int(d.max())


def assert_bar(got, exact, what, ties_exact=False):
    near, wrong, worst = compare_u8(got, exact, EPS, ties_exact)
    print(f"{what}: {near * 100:.2f} % within {EPS} of a half, {wrong} wrong elsewhere, largest difference {worst}")
    assert near <= 0.08, what
    assert wrong == 0 and worst <= 1, what


def two_tap_coordinate_eps(h, w):
    """What the fp32 sample coordinate of the two-tap rule can cost, in grey
    levels. Per axis of n source pixels: the scale is rounded once (relative
    2^-24, so up to n * 2^-24 at the far end), the product scale * (i + 0.5)
    once more (half an ulp of a coordinate below n); the - 0.5 and the
    fraction are exact. A fraction off by that much moves the value by up to
    255 times it, per axis; the interpolation's own three roundings add less
    than 1e-4. 0.086 for 1536 x 2048, 0.02 for 375 x 500."""
    def axis(n):
        return n * 2.0 ** -24 + 2.0 ** (math.floor(math.log2(max(n - 1, 1))) - 24)
    return 255 * (axis(h) + axis(w)) + 1e-4


def assert_envelope(got, exact, eps, what):
    """Every value is the rounding of something within eps of the exact one."""
    lo, hi = np.clip(np.rint(exact - eps), 0, 255), np.clip(np.rint(exact + eps), 0, 255)
    g = got.astype(np.float64)
    bad = int(((g < lo) | (g > hi)).sum())
    print(f"{what}: {bad} values outside rint(exact -+ {eps:.3f}), "
          f"{float((np.abs(exact - np.floor(exact) - 0.5) <= eps).mean()) * 100:.1f} % within that of a half")
    assert bad == 0, what
