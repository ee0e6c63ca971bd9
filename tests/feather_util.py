"""The rule of the feathered paste (include/sketchedit_feather.h) restated in numpy int64: the yardstick of
se_window_paste_feather_u8 and of EditSession.edit(feather=...).  Nothing here is shared with the library: the selection is
padded by the edge rule, the box count is a pair of cumulative sums, the blend is one integer expression."""
import numpy as np

MAX_RADIUS = 16


def selection(mask, lock, origin, frame_hw):
    """sel inside the window: mask (hs,ws) > 0 and the frame's lock plane (Hi,Wi), or None, == 0 under the window"""
    hs, ws = mask.shape
    y0, x0 = origin
    sel = np.asarray(mask) > 0
    if lock is not None:
        assert lock.shape == tuple(frame_hw)
        sel = sel & (np.asarray(lock)[y0:y0 + hs, x0:x0 + ws] == 0)
    return sel


def padded_selection(sel, origin, frame_hw, r):
    """sel extended by r on every side: a side of the window on the frame's own edge replicates the window's edge, any other side
    is 0; a corner is 0 if either of its axes says 0, else the window's corner pixel"""
    hs, ws = sel.shape
    (y0, x0), (Hi, Wi) = origin, frame_hw
    assert 0 <= y0 and y0 + hs <= Hi and 0 <= x0 and x0 + ws <= Wi
    ys, xs = np.arange(-r, hs + r), np.arange(-r, ws + r)
    y_ok = ~(((ys < 0) & (y0 != 0)) | ((ys >= hs) & (y0 + hs != Hi)))
    x_ok = ~(((xs < 0) & (x0 != 0)) | ((xs >= ws) & (x0 + ws != Wi)))
    rep = np.asarray(sel, np.int64)[np.clip(ys, 0, hs - 1)][:, np.clip(xs, 0, ws - 1)]
    return rep * (y_ok[:, None] & x_ok[None, :])


def box_count(pad, r):
    """pad (hs + 2r, ws + 2r) -> c (hs, ws): the sum over the (2r + 1)^2 box around each pixel of the window"""
    k = 2 * r + 1
    s = np.zeros((pad.shape[0] + 1, pad.shape[1] + 1), np.int64)
    s[1:, 1:] = pad.cumsum(0).cumsum(1)
    return s[k:, k:] - s[:-k, k:] - s[k:, :-k] + s[:-k, :-k]


def feather_paste(frame, origin, rgb, mask, r, lock=None):
    """-> the frame after the feathered paste of rgb (hs,ws,3) / mask (hs,ws) at origin = (y0, x0) with radius r (a new array;
    `frame` (Hi,Wi,3) uint8 is not changed).  lock: the frame's (Hi,Wi) plane, non-zero = locked, or None."""
    r = int(r)
    assert 0 <= r <= MAX_RADIUS and frame.dtype == np.uint8 and rgb.dtype == np.uint8 and mask.dtype == np.uint8
    hs, ws = mask.shape
    y0, x0 = origin
    assert rgb.shape == (hs, ws, 3) and frame.ndim == 3 and frame.shape[2] == 3
    sel = selection(mask, lock, origin, frame.shape[:2])
    n = (2 * r + 1) ** 2
    c = box_count(padded_selection(sel, origin, frame.shape[:2], r), r)
    assert c.shape == (hs, ws) and (c[sel] >= 1).all() and (c <= n).all()
    out = frame.copy()
    old = frame[y0:y0 + hs, x0:x0 + ws].astype(np.int64)
    new = (c[:, :, None] * rgb.astype(np.int64) + (n - c)[:, :, None] * old + (n - 1) // 2) // n
    assert new.max(initial=0) < 2 ** 31
    out[y0:y0 + hs, x0:x0 + ws] = np.where(sel[:, :, None], new, old).astype(np.uint8)
    return out
