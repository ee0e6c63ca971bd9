"""The rule of the stroke rasteriser restated in numpy int64: the yardstick of se_sketch_strokes_u8 and of
`serve.EditSession.edit_strokes`.  Quarter pixels: the centre of pixel (y, x) is P = (4 x + 2, 4 y + 2); a segment is
[ax, ay, bx, by, r].  With d = B - A, e = P - A, f = P - B, t = e.d, dd = d.d, cr = ex dy - ey dx the segment covers the pixel
iff, in this order:  t <= 0: e.e <= r r;  t >= dd: f.f <= r r;  otherwise cr cr <= r r dd."""
import numpy as np


def spec_cover(seg, ys, xs):
    """one segment over the pixels ys x xs (frame coordinates) -> bool (len(ys), len(xs))"""
    ax, ay, bx, by, r = (np.int64(v) for v in seg)
    px = (4 * np.asarray(xs, np.int64) + 2)[None, :]
    py = (4 * np.asarray(ys, np.int64) + 2)[:, None]
    dx, dy = bx - ax, by - ay
    ex, ey, fx, fy = px - ax, py - ay, px - bx, py - by
    t, dd, cr = ex * dx + ey * dy, dx * dx + dy * dy, ex * dy - ey * dx
    return np.where(t <= 0, ex * ex + ey * ey <= r * r, np.where(t >= dd, fx * fx + fy * fy <= r * r, cr * cr <= r * r * dd))


def spec_raster(segs, frame_hw, window=None):
    """the sketch of `window` = (y0, x0, h, w) (None: the whole frame) for the (N,5) segments: (h, w) uint8, 255 where any
    segment covers the pixel, else 0"""
    y0, x0, h, w = (0, 0, frame_hw[0], frame_hw[1]) if window is None else window
    assert 0 <= y0 and y0 + h <= frame_hw[0] and 0 <= x0 and x0 + w <= frame_hw[1]
    hit = np.zeros((h, w), bool)
    for seg in np.asarray(segs, np.int64).reshape(-1, 5):
        hit |= spec_cover(seg, np.arange(y0, y0 + h), np.arange(x0, x0 + w))
    return np.where(hit, np.uint8(255), np.uint8(0))
