"""Expected values of the 8-bit display transform (spt_display*, include/smallpt_mi355x.h), from the ORACLE's toInt (orc_to_int) and never
from the library under test:
    v = sum * weight[channel]      one float32 multiply (numpy float32)
    q = orc_to_int(v), NaN -> 0    per value, through the oracle's C function (no vectorised pow stands in for it)
plus the inputs the tests share: every float within +-64 ulps of every threshold, and the special values."""
import numpy as np

import oracle_binding

BAND = 64


def to_int(values):
    """uint8 array of values' shape: orc_to_int per float32 value, NaN -> 0."""
    v = np.ascontiguousarray(values, dtype=np.float32)
    f = oracle_binding.lib().orc_to_int
    out = np.fromiter((0 if x != x else f(x) for x in v.ravel().tolist()), dtype=np.int64, count=v.size)
    assert out.min(initial=0) >= 0 and out.max(initial=0) <= 255
    return out.astype(np.uint8).reshape(v.shape)


def prev_float(x):
    """The float32 just below each positive float32 of x."""
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) - np.uint32(1)).view(np.float32)


def threshold_bands(thresholds):
    """Every float32 within +-BAND ulps of each of the 255 thresholds: (255 * 129,) float32 (all positive normals, so ulps = bit steps)."""
    bits = np.ascontiguousarray(thresholds, dtype=np.float32).view(np.uint32).astype(np.int64)
    return (bits[:, None] + np.arange(-BAND, BAND + 1)[None, :]).astype(np.uint32).view(np.float32).ravel()


def specials():
    """+-0, denormals, negatives, 1, next-above-1, 7, +-inf -- no NaN (test it apart: its expected value is the contract's 0)."""
    one = np.float32(1.0)
    return np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, 1.1754942e-38, -1.0, -0.5, -3e38, 0.5, np.nextafter(one, np.float32(0)), 1.0,
                     np.nextafter(one, np.float32(2)), 7.0, 3e38, np.inf, -np.inf], dtype=np.float32)


def expected(rgb_sum, weight=(1.0, 1.0, 1.0), rgba=False, flip_y=False):
    """uint8 (h, w, 3|4) for an (h, w, 3) float32 sum image (row 0 = bottom): the model of spt_display."""
    s = np.ascontiguousarray(rgb_sum, dtype=np.float32)
    with np.errstate(all="ignore"):
        v = s * np.asarray(weight, dtype=np.float32)[None, None, :]          # float32 * float32 -> one float32 rounding
    assert v.dtype == np.float32
    q = to_int(v)
    if rgba:
        q = np.concatenate([q, np.full(q.shape[:2] + (1,), 255, dtype=np.uint8)], axis=2)
    return np.ascontiguousarray(q[::-1] if flip_y else q)
