"""Pillow's uint8 resampler (`Image.resize` of an 'L' or 'RGB' image with BILINEAR / BICUBIC / LANCZOS, no box, no
reducing_gap) restated in Python + numpy.  It is the yardstick of the library's se_resample_coeffs tables and of its
resize kernels (sketchedit_amd/csrc/se_resize.hip), and is itself checked byte for byte against the installed Pillow
(tests/test_resize_host.py).

Per axis the coefficients are computed in double precision, one IEEE operation at a time (plain Python floats: no
contraction, no reassociation), normalised by their sum and converted to fixed point with 22 fractional bits, rounding
away from zero.  A pass accumulates in integers from 1 << 21 and clips (acc >> 22) to [0, 255].  The horizontal pass runs
first and writes uint8; the vertical pass reads that.  An axis whose size does not change is skipped."""
import math

import numpy as np

LANCZOS, BILINEAR, BICUBIC = 1, 2, 3          # PIL.Image.Resampling values
PRECISION_BITS = 22


def _bilinear(x):
    if x < 0.0:
        x = -x
    if x < 1.0:
        return 1.0 - x
    return 0.0


def _bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    if -3.0 <= x < 3.0:
        return _sinc(x) * _sinc(x / 3)
    return 0.0


FILTERS = {BILINEAR: (_bilinear, 1.0), BICUBIC: (_bicubic, 2.0), LANCZOS: (_lanczos, 3.0)}


def coeffs(in_size, out_size, filt):
    """-> (bounds int32 (out, 2) = (first input index, tap count), k int32 (out, ksize) fixed-point weights, zero padded)"""
    f, fsupport = FILTERS[filt]
    scale = in_size / out_size
    filterscale = scale if scale > 1.0 else 1.0
    support = fsupport * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((out_size, 2), np.int32)
    k = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [f((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            k[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, k


def _pass(a, axis, bounds, k):
    """one pass over `axis` of an (H, W, C) uint8 array"""
    a = np.moveaxis(a.astype(np.int64), axis, 0)
    out = np.empty((len(bounds),) + a.shape[1:], np.int64)
    for o, (x0, n) in enumerate(bounds):
        w = k[o, :n].astype(np.int64).reshape((n,) + (1,) * (a.ndim - 1))
        out[o] = (1 << (PRECISION_BITS - 1)) + (a[x0:x0 + n] * w).sum(axis=0)
    assert np.abs(out).max(initial=0) < 2 ** 31          # Pillow accumulates in int32
    out = np.clip(out >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize(a, size, filt=BICUBIC):
    """Image.fromarray(a).resize(size, filt) for a (H, W) or (H, W, C) uint8 array; size = (width, height) as Pillow takes it"""
    a = np.asarray(a, np.uint8)
    flat = a.ndim == 2
    if flat:
        a = a[..., None]
    w_out, h_out = size
    h_in, w_in = a.shape[:2]
    out = a.copy()
    if w_out != w_in:
        out = _pass(out, 1, *coeffs(w_in, w_out, filt))
    if h_out != h_in:
        out = _pass(out, 0, *coeffs(h_in, h_out, filt))
    return out[..., 0] if flat else out
