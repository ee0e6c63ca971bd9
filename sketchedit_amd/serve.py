"""Serving helpers for the inference path: the per-request pre/post-processing of the reference's demo
(/root/reference/demo.py:39-73, `process_image`) and a small dynamic batcher for concurrent callers
(demo.py:120 runs Flask with threaded=True, i.e. concurrent forwards on one model object),
with one worker per GPU when several models are given.

No web framework here -- the Flask UI is out of scope; these are the pieces of it that touch the hot path.
"""
import math
import threading
import time
from fractions import Fraction

import numpy as np

from . import _lib
# the limits and codes of include/*.h, from their one Python mirror
from ._lib import (ADJUST_MAX_CLIP, ADJUST_MAX_COEF, ADJUST_MAX_OFFSET, BLEND_MAX_SIDE, CANVAS_CONSTANT, CANVAS_MAX_OFFSET, CANVAS_MAX_SIDE,   # noqa: F401
                   COMBINE_INVERT, FEATHER_MAX_RADIUS, FILTER_MAX_CELL, FILTER_MAX_RADIUS, FILTER_ONE, LASSO_MAX_EDGES, MODIFY_MAX_RADIUS,
                   MOVE_MAX_OFFSET, OUTLINE_MAX_CAP, SELECT_MAX_GROW, WARP_MAX_COEF, WARP_MAX_TRANSLATION)


def _to_tensors(img, mask):
    """demo.py:40-56: RGB, sizes floored to multiples of 8, image to [-1, 1], mask > 0."""
    import torch
    img = img.convert("RGB")
    w_raw, h_raw = img.size
    h_t, w_t = h_raw // 8 * 8, w_raw // 8 * 8
    if h_t < 16 or w_t < 16:
        raise ValueError("image too small: %dx%d" % (w_raw, h_raw))
    x = np.array(img.resize((w_t, h_t))).transpose((2, 0, 1))
    m = np.array(mask.resize((w_t, h_t)))
    if m.ndim == 3:
        m = m[..., 0]
    m = (torch.from_numpy(m.astype(np.float32)) > 0).float()
    x = (torch.from_numpy(x.astype(np.float32)) / 255 - 0.5) / 0.5
    return x[None], m[None, None], (w_raw, h_raw)


def _device_inputs(img, mask):
    """What the device path takes from a request (device_io=True): the image as an RGB uint8 array and the sketch as one
    uint8 plane -- mode 'L' as is, 'RGB' its channel 0 (Pillow resamples channels independently, so that is the plane
    `(mask.resize(...))[..., 0]` comes from).  None for any other sketch mode ('1', 'P', 'RGBA', ...: Pillow resamples
    those differently), which then takes the host preparation.  Sizes under the working minimum raise as _to_tensors does."""
    img = img.convert("RGB")
    w_raw, h_raw = img.size
    if h_raw // 8 * 8 < 16 or w_raw // 8 * 8 < 16:
        raise ValueError("image too small: %dx%d" % (w_raw, h_raw))
    if mask.mode == "L":
        m = np.asarray(mask)
    elif mask.mode == "RGB":
        m = np.ascontiguousarray(np.asarray(mask)[..., 0])
    else:
        return None
    return np.asarray(img), m


def _to_image(generated, size_raw):
    """demo.py:62-70: clamp, (x+1)/2*255, uint8, HWC, resize back to the request's size."""
    import torch
    from PIL import Image
    g = torch.clamp(generated, -1, 1)
    g = ((g + 1) / 2 * 255).cpu().numpy().astype(np.uint8)
    return Image.fromarray(g[0].transpose((1, 2, 0))).resize(size_raw)


def _accepts_low_latency(model):
    import inspect
    try:
        return "low_latency" in inspect.signature(getattr(model, "forward", model)).parameters
    except (TypeError, ValueError):
        return False


def process_image(model, img, mask, low_latency=None, device_io=False):
    """One request, as demo.py:39-73 handles it: PIL image + PIL sketch/mask in, PIL result out.  `low_latency` pins the
    library's execution mode (EditLine2Model.forward); None = by call size.

    device_io=True (an EditLine2Model): only the decoded uint8 arrays cross to the device; the resizes to and from the
    working size (Pillow-exact), the normalisation, the forward and the output quantisation run there as one library call
    (EditLine2Model.edit_u8) -- byte-identical to the host steps.  A sketch of another mode than 'L' / 'RGB' takes the host
    path."""
    import torch
    if device_io:
        arrays = _device_inputs(img, mask)
        if arrays is not None:
            from PIL import Image
            rgb = model.edit_u8(arrays[0], arrays[1], low_latency=low_latency)
            return Image.fromarray(rgb.cpu().numpy())
    x, m, size_raw = _to_tensors(img, mask)
    with torch.no_grad():
        if low_latency is None:
            generated, _ = model({"image": x, "mask": m}, mode="inference")
        else:
            generated, _ = model({"image": x, "mask": m}, mode="inference", low_latency=low_latency)
    return _to_image(generated, size_raw)


def sketch_bbox(sketch):
    """Tight box of `sketch > 0` of a 2-D uint8 array as (y0, x0, y1, x1), half open; None for an empty sketch."""
    rows = np.flatnonzero(np.any(sketch > 0, axis=1))
    if rows.size == 0:
        return None
    cols = np.flatnonzero(np.any(sketch[rows[0]:rows[-1] + 1] > 0, axis=0))
    return int(rows[0]), int(cols[0]), int(rows[-1]) + 1, int(cols[-1]) + 1


def choose_window(bbox, frame_hw, margin=0.5, bucket=64, min_side=256):
    """The window a sketch is edited through (pure host arithmetic).  `bbox` = (y0, x0, y1, x1), half open, the
    tight box of `sketch > 0` (sketch_bbox); `frame_hw` = (Hi, Wi).  Per axis the side is the box's extent plus
    ceil(margin * max(box height, box width)) on both ends, raised to `min_side` (and to the forward's minimum, 16), rounded
    UP to a multiple of `bucket` and capped at the frame's extent floored to a multiple of 8; the window is centred on the
    box and shifted to lie inside the frame.  -> (y0, x0, h, w), or None for an empty sketch (bbox None or empty).  A frame
    under the forward's minimum raises ValueError, as _to_tensors does.
    The defaults are a policy, not a measurement: context of half the edit's size around it, the reference's 256 x 256
    training size as the floor, and buckets so that windows of different requests share sizes and batch."""
    Hi, Wi = int(frame_hw[0]), int(frame_hw[1])
    if Hi // 8 * 8 < 16 or Wi // 8 * 8 < 16:
        raise ValueError("image too small: %dx%d" % (Wi, Hi))
    if bucket < 8 or bucket % 8:
        raise ValueError("bucket must be a positive multiple of 8: %r" % (bucket,))
    if margin < 0:
        raise ValueError("margin must not be negative: %r" % (margin,))
    if bbox is None:
        return None
    by0, bx0, by1, bx1 = (int(v) for v in bbox)
    by0, bx0, by1, bx1 = max(by0, 0), max(bx0, 0), min(by1, Hi), min(bx1, Wi)
    if by1 <= by0 or bx1 <= bx0:
        return None
    pad = int(np.ceil(margin * max(by1 - by0, bx1 - bx0)))

    def axis(lo, hi, extent):
        side = max(hi - lo + 2 * pad, int(min_side), 16)
        side = min(-(-side // bucket) * bucket, extent // 8 * 8)
        start = lo - (side - (hi - lo)) // 2              # centred (a box larger than the window: its centre part)
        return min(max(start, 0), extent - side), side

    y0, h = axis(by0, by1, Hi)
    x0, w = axis(bx0, bx1, Wi)
    return y0, x0, h, w


def choose_working_size(window_hw, max_side):
    """The working size (H, W) the forward of a window edit runs at (pure host arithmetic).  `window_hw` =
    (hs, ws), the window's extent in the frame, each >= 16.  If max(hs, ws) <= max_side the window is only floored to
    multiples of 8; otherwise both sides are scaled by max_side / max(hs, ws), floored to multiples of 8 and kept at
    least 16 -- the aspect ratio is preserved up to that flooring.  Never upscales.
    `max_side` is a policy, not a measurement: it bounds an edit's cost whatever the sketch's extent.  The reference demo
    resamples every request to at most 640 on a side (demo.py `max_size = 640`), which is the obvious value to offer;
    nothing here measures what it does to the result."""
    hs, ws = int(window_hw[0]), int(window_hw[1])
    max_side = int(max_side)
    if hs < 16 or ws < 16:
        raise ValueError("window too small: %dx%d" % (ws, hs))
    if max_side < 16:
        raise ValueError("max_side must be at least 16: %r" % (max_side,))
    long_side = max(hs, ws)
    if long_side <= max_side:
        return hs // 8 * 8, ws // 8 * 8
    return max(hs * max_side // long_side // 8 * 8, 16), max(ws * max_side // long_side // 8 * 8, 16)


def window_saved_bytes(hs, ws):
    """Bytes of one undo-journal slot of an hs x ws window: hs rows of 3 ws bytes rounded up to 16; 0 for a
    window under 16 x 16.  The library's se_window_saved_bytes in host arithmetic (the host tests compare the two)."""
    hs, ws = int(hs), int(ws)
    return 0 if hs < 16 or ws < 16 else hs * ((3 * ws + 15) // 16 * 16)


def _windows_intersect(a, b):
    return a[0] < b[0] + b[2] and b[0] < a[0] + a[2] and a[1] < b[1] + b[3] and b[1] < a[1] + a[3]


def merge_regions(boxes, frame_hw, margin=0.5, bucket=64, min_side=256):
    """The merge rule of a region edit (pure host arithmetic): every box (y0, x0, y1, x1) gets its
    choose_window; while any two windows intersect, the lowest-indexed intersecting pair -- with the components kept sorted by
    their boxes, so the result is a function of the SET of boxes, not of the order they came in -- becomes one component with
    the union box and a new window.  Each merge leaves one component fewer, so the loop ends.  -> [(box, window)], windows
    pairwise disjoint, sorted by window (y0, x0)."""
    comps = sorted({tuple(int(v) for v in b) for b in boxes})
    while True:
        wins = [choose_window(b, frame_hw, margin, bucket, min_side) for b in comps]
        pair = next(((i, j) for i in range(len(comps)) for j in range(i + 1, len(comps)) if _windows_intersect(wins[i], wins[j])), None)
        if pair is None:
            return sorted(zip(comps, wins), key=lambda r: r[1][:2])
        a, b = comps[pair[0]], comps[pair[1]]
        union = (min(a[0], b[0]), min(a[1], b[1]), max(a[2], b[2]), max(a[3], b[3]))
        comps = sorted(set(c for k, c in enumerate(comps) if k not in pair) | {union})


def split_regions(tiles, tile, frame_hw, margin=0.5, bucket=64, min_side=256):
    """The windows a sketch of several separate strokes is edited through (pure host arithmetic).  `tiles`: the
    (ceil(Hi / tile), ceil(Wi / tile), 5) grid of [count, y0, x0, y1, x1] records of the sketch (se_sketch_tiles_u8).  The
    8-connected components of the non-empty tiles are the strokes, each with the union of its tiles' tight boxes; they get
    windows by merge_regions.  -> [(box, window)] sorted by window (y0, x0), [] for an all-empty grid.  One component gives
    exactly choose_window(sketch_bbox(sketch)): a single-blob sketch gets the window `EditSession.edit` gives it.
    `tile` and the three policy arguments are a policy, not a measurement: choose_window's defaults, and a tile fine enough
    that strokes a window apart are never one component."""
    tiles = np.asarray(tiles)
    nty, ntx = -(-int(frame_hw[0]) // int(tile)), -(-int(frame_hw[1]) // int(tile))
    if tiles.shape != (nty, ntx, 5):
        raise ValueError("tiles is %r, a %dx%d frame at tile %d has (%d, %d, 5)" % (tiles.shape, frame_hw[1], frame_hw[0], tile, nty, ntx))
    full = tiles[..., 0] > 0
    label = np.full((nty, ntx), -1, np.int64)
    boxes = []
    for ty, tx in zip(*np.nonzero(full)):                 # raster order: a component is numbered by its first tile
        if label[ty, tx] >= 0:
            continue
        label[ty, tx] = len(boxes)
        stack, members = [(ty, tx)], []
        while stack:
            y, x = stack.pop()
            members.append(tiles[y, x, 1:])
            for v in range(max(y - 1, 0), min(y + 2, nty)):
                for u in range(max(x - 1, 0), min(x + 2, ntx)):
                    if full[v, u] and label[v, u] < 0:
                        label[v, u] = len(boxes)
                        stack.append((v, u))
        m = np.stack(members)
        boxes.append((int(m[:, 0].min()), int(m[:, 1].min()), int(m[:, 2].max()), int(m[:, 3].max())))
    return merge_regions(boxes, frame_hw, margin, bucket, min_side)


STROKE_Q = 4                # quarter pixels: the unit of a segment's coordinates and radius
STROKE_R_MIN, STROKE_R_MAX = 3, 512
STROKE_MAX_EXTENT = 8192


def stroke_segments(strokes, frame_hw):
    """Strokes as a drawing front end has them -> the segments the rasteriser takes (pure host arithmetic).
    `strokes`: [(points, width_px)], points = [(x, y)] floats in pixels of the frame (pixel (y, x) covers [x, x + 1) x [y, y + 1):
    its centre is (x + 0.5, y + 0.5)), width_px the brush's diameter.  Coordinates are rounded to quarter pixels (half up) and
    clamped to the frame's rectangle [0, 4 Wi] x [0, 4 Hi]; r = round(2 width_px), the radius in quarter pixels, must lie in
    [3, 512] -- a brush of 1.5 to 256 pixels.  n points give n - 1 segments, one point a dot (a segment of length zero).
    -> (segs, ranges): an (N,5) int32 array of [ax, ay, bx, by, r] and each stroke's (first, count).  ValueError for no
    strokes, a stroke without points, a value that is not finite, a width outside the range, a frame over 8192 on a side."""
    Hi, Wi = int(frame_hw[0]), int(frame_hw[1])
    if not (1 <= Hi <= STROKE_MAX_EXTENT and 1 <= Wi <= STROKE_MAX_EXTENT):
        raise ValueError("strokes are rasterised on frames of at most %d pixels on a side (got %dx%d)" % (STROKE_MAX_EXTENT, Wi, Hi))
    strokes = list(strokes)
    if not strokes:
        raise ValueError("no strokes: nothing to edit")
    segs, ranges = [], []
    for k, (points, width) in enumerate(strokes):
        pts = np.asarray(points, np.float64)
        if pts.ndim != 2 or pts.shape[1] != 2 or pts.shape[0] < 1:
            raise ValueError("stroke %d: points are a non-empty list of (x, y)" % k)
        if not (np.isfinite(pts).all() and np.isfinite(width)):
            raise ValueError("stroke %d: coordinates and width must be finite" % k)
        r = int(np.floor(2.0 * float(width) + 0.5))
        if not STROKE_R_MIN <= r <= STROKE_R_MAX:
            raise ValueError("stroke %d: width %r gives a radius of %d quarter pixels, outside [%d, %d]" % (k, width, r, STROKE_R_MIN, STROKE_R_MAX))
        q = np.floor(STROKE_Q * pts + 0.5)
        qx = np.clip(q[:, 0], 0, STROKE_Q * Wi).astype(np.int64)
        qy = np.clip(q[:, 1], 0, STROKE_Q * Hi).astype(np.int64)
        ends = [(0, 0)] if len(pts) == 1 else [(i, i + 1) for i in range(len(pts) - 1)]
        ranges.append((len(segs), len(ends)))
        segs.extend([qx[i], qy[i], qx[j], qy[j], r] for i, j in ends)
    return np.asarray(segs, np.int32).reshape(-1, 5), ranges


def stroke_box(segs, frame_hw):
    """The box of a stroke's segments (pure host arithmetic): (y0, x0, y1, x1), half open, in pixels -- per axis
    [ceil((min - r - 2) / 4), floor((max + r - 2) / 4) + 1) over the segments' end points, clipped to the frame.  A pixel a
    segment covers has its centre 4 x + 2 within r of the segment, so the box holds every covered pixel; with r >= 3 and the
    end points inside the frame's rectangle it is never empty (a centre lies within 2 of every point of [0, 4 W])."""
    s = np.asarray(segs, np.int64).reshape(-1, 5)
    if s.shape[0] < 1:
        raise ValueError("a stroke has at least one segment")
    Hi, Wi = int(frame_hw[0]), int(frame_hw[1])
    r = s[:, 4]
    lo = lambda a, b: int(-((-(np.minimum(a, b) - r - 2).min()) // STROKE_Q))
    hi = lambda a, b: int((np.maximum(a, b) + r - 2).max() // STROKE_Q) + 1
    return (max(lo(s[:, 1], s[:, 3]), 0), max(lo(s[:, 0], s[:, 2]), 0), min(hi(s[:, 1], s[:, 3]), Hi), min(hi(s[:, 0], s[:, 2]), Wi))


COMBINE_OPS = {"add": _lib.COMBINE_ADD, "subtract": _lib.COMBINE_SUBTRACT, "intersect": _lib.COMBINE_INTERSECT, "xor": _lib.COMBINE_XOR}
MODIFY_OPS = {"expand": _lib.MODIFY_EXPAND, "contract": _lib.MODIFY_CONTRACT, "smooth": _lib.MODIFY_SMOOTH}
MODIFY_KINDS = ("expand", "contract", "border", "smooth")
MODIFY_SIDES = ("inside", "outside", "both")


def lasso_edges(rings, frame_hw):
    """Outlines as a drawing front end has them -> the edges the lasso's rasteriser takes (pure host arithmetic).
    `rings`: a list of point lists [(x, y)], floats in pixels of the frame as stroke_segments takes them, at least 3 points
    each; every ring is closed here (its last point is joined to its first).  Coordinates are rounded to quarter pixels (half up)
    and clamped to the frame's rectangle [0, 4 Wi] x [0, 4 Hi]: a vertex outside the frame moves to its border.  The interior
    is even-odd over all rings together: a ring inside a ring is a hole.
    -> an (N,4) int32 array of [ax, ay, bx, by], one edge per point (horizontal and zero-length edges are kept: they never
    count).  ValueError for no rings, a ring under 3 points, a value that is not finite, more than 65 536 edges, a frame over
    8192 on a side."""
    Hi, Wi = int(frame_hw[0]), int(frame_hw[1])
    if not (1 <= Hi <= STROKE_MAX_EXTENT and 1 <= Wi <= STROKE_MAX_EXTENT):
        raise ValueError("a lasso is rasterised on frames of at most %d pixels on a side (got %dx%d)" % (STROKE_MAX_EXTENT, Wi, Hi))
    rings = list(rings)
    if not rings:
        raise ValueError("no rings: nothing to select")
    edges = []
    for k, points in enumerate(rings):
        try:
            pts = np.asarray(points, np.float64)
        except (TypeError, ValueError):
            raise ValueError("ring %d: points are a list of (x, y)" % k)
        if pts.ndim != 2 or pts.shape[1] != 2 or pts.shape[0] < 3:
            raise ValueError("ring %d: an outline is a list of at least 3 points (x, y)" % k)
        if not np.isfinite(pts).all():
            raise ValueError("ring %d: coordinates must be finite" % k)
        q = np.floor(STROKE_Q * pts + 0.5)
        qx = np.clip(q[:, 0], 0, STROKE_Q * Wi).astype(np.int64)
        qy = np.clip(q[:, 1], 0, STROKE_Q * Hi).astype(np.int64)
        edges.append(np.stack([qx, qy, np.roll(qx, -1), np.roll(qy, -1)], axis=1))
        if sum(e.shape[0] for e in edges) > LASSO_MAX_EDGES:
            raise ValueError("a lasso has at most %d edges" % LASSO_MAX_EDGES)
    return np.concatenate(edges).astype(np.int32).reshape(-1, 4)


def lasso_box(edges, frame_hw):
    """A box that holds every pixel a lasso selects (pure host arithmetic): (y0, x0, y1, x1), half open -- rows
    [ceil((min_y - 2) / 4), floor((max_y - 3) / 4) + 1), columns [floor((min_x - 2) / 4) + 1, floor((max_x - 2) / 4) + 1) over the
    edges' end points, clipped to the frame -- or None when that is empty (no centre can be selected).  A selected centre has
    min_y <= py < max_y (an edge spans its scanline) and min_x < px <= max_x (a crossing lies strictly left of it, and for
    closed rings one lies at or right of it).  A bound, not the tight box."""
    e = np.asarray(edges, np.int64).reshape(-1, 4)
    if e.shape[0] < 1:
        return None
    Hi, Wi = int(frame_hw[0]), int(frame_hw[1])
    xs, ys = e[:, [0, 2]], e[:, [1, 3]]
    y0, y1 = max(int(-((-(ys.min() - 2)) // STROKE_Q)), 0), min(int((ys.max() - 3) // STROKE_Q) + 1, Hi)
    x0, x1 = max(int((xs.min() - 2) // STROKE_Q) + 1, 0), min(int((xs.max() - 2) // STROKE_Q) + 1, Wi)
    return (y0, x0, y1, x1) if y0 < y1 and x0 < x1 else None


def outline_rings(records):
    """The boundary records of a selection (se_outline_u8 / Selection.edges: (N,4) [ax, ay, bx, by] in quarter pixels, axis
    parallel, clockwise with the interior on the right) -> its outline as closed rings (pure host arithmetic, time linear in N;
    DESIGN.md 6q).  Each record's end is linked to the record that starts there; where two start at a vertex -- two selected
    pixels touching diagonally -- the RIGHT turn is taken, so the selected set is traced 4-connected (as select_similar connects
    it) and the background 8-connected.  Collinear neighbours are merged, which removes the splits at tile boundaries.
    -> [[(x, y), ...], ...]: integer corner points in frame pixels, the format select_lasso takes.  A ring starts at its
    smallest vertex in (y, x) order (no two rings share it) and the rings are sorted by it; outer rings run clockwise on the
    screen (positive shoelace area with y down), holes counter-clockwise, and the signed areas sum to the selection's count.
    ValueError for records that are not the whole outline of a pixel set (a capped download, say)."""
    e = np.asarray(records, np.int64).reshape(-1, 4)
    n = e.shape[0]
    if n == 0:
        return []
    dx, dy = np.sign(e[:, 2] - e[:, 0]), np.sign(e[:, 3] - e[:, 1])
    if ((dx != 0) == (dy != 0)).any() or (e % STROKE_Q != 0).any():
        raise ValueError("outline records are axis-parallel edges of non-zero length between pixel corners")
    dirs = list(zip(dx.tolist(), dy.tolist()))
    rows = e.tolist()
    starts = {}
    for i, r in enumerate(rows):
        starts.setdefault((r[0], r[1]), []).append(i)
    succ = [0] * n
    for i, r in enumerate(rows):
        c = starts.get((r[2], r[3]), ())
        if len(c) == 1:
            succ[i] = c[0]
        else:
            right = (-dirs[i][1], dirs[i][0])
            c = [j for j in c if dirs[j] == right]
            if len(c) != 1:
                raise ValueError("the records are not the closed outline of a pixel set (a record's end starts no other)")
            succ[i] = c[0]
    seen, rings = [False] * n, []
    for first in range(n):
        if seen[first]:
            continue
        pts, i, prev = [], first, None
        while not seen[i]:
            seen[i] = True
            pts.append((i, prev))
            prev, i = i, succ[i]
        if i != first:
            raise ValueError("the records are not the closed outline of a pixel set (two records share a successor)")
        ring = [(rows[j][0] // STROKE_Q, rows[j][1] // STROKE_Q) for j, pj in pts if dirs[j] != dirs[prev if pj is None else pj]]
        k = min(range(len(ring)), key=lambda t: (ring[t][1], ring[t][0]))
        rings.append(ring[k:] + ring[:k])
    rings.sort(key=lambda r: (r[0][1], r[0][0]))
    return rings


def rings_svg_path(rings):
    """Rings as outline_rings returns them -> the `d` attribute of ONE SVG path: "M x0 y0 L x1 y1 ... Z" per ring (an "L" in
    front of every further point), the rings joined by single spaces; "" for no rings.  Holes wind the other way, so the
    path fills as the selection under either fill rule."""
    return " ".join("M %d %d " % tuple(r[0]) + "".join("L %d %d " % tuple(q) for q in r[1:]) + "Z" for r in rings)


MOVE_FLIPS = {None: 0, "h": _lib.MOVE_FLIP_X, "v": _lib.MOVE_FLIP_Y, "hv": _lib.MOVE_FLIP_X | _lib.MOVE_FLIP_Y}
MOVE_MIN_SIDE = 16           # the smallest side of a journal slot's rectangle
MOVE_BLENDS = (None, "seamless")                    # move_selection's `blend`


def move_rect(box, offset, frame_hw):
    """The rectangle of the frame a moved selection lands in (pure host arithmetic): `box` = (y0, x0, y1, x1), half
    open, shifted by `offset` = (dy, dx) and clipped to the frame of `frame_hw` = (Hi, Wi), both >= 16.  A side under 16 -- what a
    journal slot takes at least -- is then widened to 16 inside the frame: by half the missing pixels at its low end (rounded
    down), the rest at its high end, and where that would leave the frame the rectangle is shifted back into it, towards the
    interior.  It always holds the clipped box.  A mirrored move lands in the same rectangle: the flips mirror about the box.
    -> (y0, x0, h, w), or None when nothing of the box lands in the frame.  offset (0, 0) gives the rectangle a move LIFTS."""
    by0, bx0, by1, bx1 = (int(v) for v in box)
    dy, dx = int(offset[0]), int(offset[1])

    def axis(lo, hi, extent):
        lo, hi = max(lo, 0), min(hi, extent)
        if hi <= lo:
            return None
        if hi - lo < MOVE_MIN_SIDE:
            lo = min(max(lo - (MOVE_MIN_SIDE - (hi - lo)) // 2, 0), extent - MOVE_MIN_SIDE)
            hi = lo + MOVE_MIN_SIDE
        return lo, hi - lo

    ya, xa = axis(by0 + dy, by1 + dy, int(frame_hw[0])), axis(bx0 + dx, bx1 + dx, int(frame_hw[1]))
    return None if ya is None or xa is None else (ya[0], xa[0], ya[1], xa[1])


# (FILTER_ONE is the sum of a filter's taps, t[0] + 2 (t[1] + .. + t[R]))
FILTER_MAX_AMOUNT = 4.0              # SE_FILTER_MAX_AMOUNT / 256: the strongest unsharp mask, a factor here (_lib's is in 1/256 units)
FILTER_KINDS = ("blur", "box", "sharpen", "pixelate")


def _filter_int(v, lo, hi, what):
    if not isinstance(v, (int, np.integer)) or isinstance(v, (bool, np.bool_)) or not lo <= v <= hi:
        raise ValueError("%s is an int %d .. %d (got %r)" % (what, lo, hi, v))
    return int(v)


def filter_taps(kind, radius, sigma=None):
    """The taps [t0 .. tR] of a separable filter of `radius` R = 1 .. 32 (pure host arithmetic): ints >= 0 with
    t0 + 2 (t1 + .. + tR) == 4096, t0 > 0 and t1 >= t2 >= .. >= tR.  `kind` "gauss": w_k = exp(-k^2 / (2 sigma^2)) with `sigma` =
    max(R / 3, 0.5) unless given (0 < sigma <= R), t_k = floor(4096 w_k / sum of w + 0.5) for k >= 1 and t0 the rest -- for a wide
    sigma t0 may be a unit below t1.  `kind` "box": t_k = 4096 // (2R + 1) for k >= 1 and t0 the rest; it takes no sigma.
    ValueError for a bad argument."""
    if not isinstance(kind, str) or kind not in ("gauss", "box"):
        raise ValueError("kind is 'gauss' or 'box' (got %r)" % (kind,))
    R = _filter_int(radius, 1, FILTER_MAX_RADIUS, "radius")
    if kind == "box":
        if sigma is not None:
            raise ValueError("a box filter takes no sigma (got %r)" % (sigma,))
        t = [FILTER_ONE // (2 * R + 1)] * R
    else:
        if sigma is None:
            sigma = max(R / 3.0, 0.5)
        if isinstance(sigma, (bool, np.bool_)) or not isinstance(sigma, (int, float, np.integer, np.floating)) or not 0 < sigma <= R:
            raise ValueError("sigma is a number in (0, radius] (got %r)" % (sigma,))
        w = [math.exp(-k * k / (2.0 * float(sigma) ** 2)) for k in range(R + 1)]
        total = w[0] + 2.0 * sum(w[1:])
        t = [int(math.floor(FILTER_ONE * w[k] / total + 0.5)) for k in range(1, R + 1)]
    return [FILTER_ONE - 2 * sum(t)] + t


def filter_rect(box, radius, frame_hw):
    """The rectangle a filter LIFTS (pure host arithmetic): `box` = (y0, x0, y1, x1), half open, grown by `radius` on
    every side and clipped to the frame of `frame_hw`, sides under 16 widened exactly as move_rect widens them.  It holds every
    pixel a tap of that radius reads and every pixel the filter writes.  -> (y0, x0, h, w)."""
    by0, bx0, by1, bx1 = (int(v) for v in box)
    r = int(radius)
    return move_rect((by0 - r, bx0 - r, by1 + r, bx1 + r), (0, 0), frame_hw)


ADJUST_ONE = 4096                    # 1.0 in the Q12 of an adjustment's matrix
ADJUST_GREY = (1225, 2404, 467)      # the luma weights in Q12: a row of the matrix of saturation 0
ADJUST_AUTO = {"levels": _lib.ADJUST_STRETCH, "equalize": _lib.ADJUST_EQUALIZE, "match": _lib.ADJUST_MATCH}
ADJUST_WHICH = {"channels": _lib.ADJUST_PER_CHANNEL, "luma": _lib.ADJUST_LUMA}


def _adjust_number(v, lo, hi, what):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not lo <= v <= hi:
        raise ValueError("%s is a number %g .. %g (got %r)" % (what, lo, hi, v))
    return float(v)


def adjust_lut(brightness=0, contrast=0, gamma=1.0, levels=None, curve=None, invert=False, posterize=None):
    """A table for EditSession.adjust_selection (pure host arithmetic) -> a (3, 256) uint8 array, the same row for the
    three channels.  Every value v = 0 .. 255 goes through the steps below IN THIS ORDER, as a float clamped to 0 .. 255 after each
    step, and is rounded once at the end, floor(x + 0.5):
      1. `levels` = (black, white) or (black, white, out_black, out_white), ints 0 .. 255 with black < white:
         x = out_black + (out_white - out_black) clamp((x - black) / (white - black), 0, 1);
      2. `gamma` 0.1 .. 10: x = 255 (x / 255) ^ (1 / gamma) -- above 1 lifts the mid-tones;
      3. `contrast` -100 .. 100 about the pivot 128 and `brightness` -255 .. 255: x = (x - 128) (100 + contrast) / 100 + 128 + brightness;
      4. `curve` = [(x0, y0), (x1, y1), ...], ints 0 .. 255, at least two points, x strictly increasing: linear between the points,
         flat outside them;
      5. `posterize` = n in 2 .. 256 levels: x = floor(x n / 256) 255 / (n - 1);
      6. `invert`: x = 255 - x.
    ValueError for a bad argument."""
    b = _adjust_number(brightness, -255, 255, "brightness")
    c = _adjust_number(contrast, -100, 100, "contrast")
    g = _adjust_number(gamma, 0.1, 10, "gamma")
    if levels is not None:
        try:
            levels = tuple(levels)
        except TypeError:
            raise ValueError("levels is (black, white) or (black, white, out_black, out_white) (got %r)" % (levels,))
        if len(levels) not in (2, 4):
            raise ValueError("levels is (black, white) or (black, white, out_black, out_white) (got %r)" % (levels,))
        levels = tuple(_filter_int(v, 0, 255, "a level") for v in levels)
        if not levels[0] < levels[1]:
            raise ValueError("levels: black < white (got %r)" % (levels,))
    if curve is not None:
        try:
            curve = [(_filter_int(px, 0, 255, "a curve point's x"), _filter_int(py, 0, 255, "a curve point's y")) for px, py in curve]
        except TypeError:
            raise ValueError("curve is a list of (x, y) points (got %r)" % (curve,))
        if len(curve) < 2 or any(a[0] >= b_[0] for a, b_ in zip(curve, curve[1:])):
            raise ValueError("curve: at least two points, x strictly increasing (got %r)" % (curve,))
    if not isinstance(invert, (bool, np.bool_)):
        raise ValueError("invert is a bool (got %r)" % (invert,))
    if posterize is not None:
        posterize = _filter_int(posterize, 2, 256, "posterize")
    clamp = lambda x: min(max(x, 0.0), 255.0)       # noqa: E731
    row = []
    for v in range(256):
        x = float(v)
        if levels is not None:
            t = min(max((x - levels[0]) / float(levels[1] - levels[0]), 0.0), 1.0)
            x = clamp(t * 255.0) if len(levels) == 2 else clamp(levels[2] + (levels[3] - levels[2]) * t)
        if g != 1.0:
            x = clamp(255.0 * (x / 255.0) ** (1.0 / g))
        x = clamp((x - 128.0) * (100.0 + c) / 100.0 + 128.0 + b)
        if curve is not None:
            if x <= curve[0][0]:
                x = float(curve[0][1])
            elif x >= curve[-1][0]:
                x = float(curve[-1][1])
            else:
                k = max(i for i in range(len(curve) - 1) if curve[i][0] <= x)
                (xa, ya), (xb, yb) = curve[k], curve[k + 1]
                x = ya + (yb - ya) * (x - xa) / float(xb - xa)
        if posterize is not None:
            x = clamp(math.floor(x * posterize / 256.0) * 255.0 / (posterize - 1))
        if invert:
            x = 255.0 - x
        row.append(int(math.floor(x + 0.5)))
    return np.tile(np.asarray(row, np.uint8), (3, 1))


def adjust_matrix(saturation=1.0, hue=0.0, mix=None):
    """The 12 ints of an adjustment's matrix (pure host arithmetic): m[c][j] in Q12 row by row, then o[c].
    `hue` (degrees, -360 .. 360) turns the colour about the grey axis, then `saturation` (0 .. 4) scales its distance from the luma
    (77, 150, 29) / 256 -- in Q12 (1225, 2404, 467): saturation 0 gives three such rows, the grey matrix; 1 and hue 0 the identity.
    Every row sums to exactly 4096 -- a grey pixel stays what it is: the off-diagonal entries are rounded, the diagonal takes the
    rest; o = 0.  `mix` gives the matrix itself and excludes the other two: three rows of three floats (1.0 = 4096, |v| <= 8) or of
    four, the fourth an offset in pixel values (|v| <= 256).  ValueError for a bad argument."""
    s = _adjust_number(saturation, 0, 4, "saturation")
    h = _adjust_number(hue, -360, 360, "hue")
    if mix is not None:
        if s != 1.0 or h != 0.0:
            raise ValueError("mix gives the matrix itself: it excludes saturation and hue")
        try:
            rows = [[v for v in r] for r in mix]
        except TypeError:
            raise ValueError("mix is three rows of three or four numbers (got %r)" % (mix,))
        if len(rows) != 3 or len(rows[0]) not in (3, 4) or any(len(r) != len(rows[0]) for r in rows):
            raise ValueError("mix is three rows of three or four numbers (got %r)" % (mix,))
        m = [int(round(ADJUST_ONE * _adjust_number(r[j], -8, 8, "a mix coefficient"))) for r in rows for j in range(3)]
        o = [int(round(ADJUST_ONE * _adjust_number(r[3], -256, 256, "a mix offset"))) if len(r) == 4 else 0 for r in rows]
        return m + o
    w = [v / float(ADJUST_ONE) for v in ADJUST_GREY]
    cs, sn = math.cos(math.radians(h)), math.sin(math.radians(h))
    k = sn / math.sqrt(3.0)
    rot = [[cs + (1 - cs) / 3.0, (1 - cs) / 3.0 - k, (1 - cs) / 3.0 + k],
           [(1 - cs) / 3.0 + k, cs + (1 - cs) / 3.0, (1 - cs) / 3.0 - k],
           [(1 - cs) / 3.0 - k, (1 - cs) / 3.0 + k, cs + (1 - cs) / 3.0]]
    sat = [[(1 - s) * w[j] + (s if i == j else 0.0) for j in range(3)] for i in range(3)]
    a = [[sum(sat[i][t] * rot[t][j] for t in range(3)) for j in range(3)] for i in range(3)]
    m = [[int(round(ADJUST_ONE * a[i][j])) for j in range(3)] for i in range(3)]
    for i in range(3):
        m[i][i] = ADJUST_ONE - sum(m[i][j] for j in range(3) if j != i)
    return [m[i][j] for i in range(3) for j in range(3)] + [0, 0, 0]


def _check_adjust_matrix(matrix):
    try:
        vals = list(matrix)
    except TypeError:
        vals = []
    if len(vals) != 12 or any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) for v in vals):
        raise ValueError("matrix is 12 ints, what adjust_matrix returns (got %r)" % (matrix,))
    vals = [int(v) for v in vals]
    if any(abs(v) > ADJUST_MAX_COEF for v in vals[:9]) or any(abs(v) > ADJUST_MAX_OFFSET for v in vals[9:]):
        raise ValueError("matrix: a coefficient is at most %d and an offset at most %d in magnitude (got %r)" % (ADJUST_MAX_COEF, ADJUST_MAX_OFFSET, vals))
    return vals


def _check_adjust_lut(lut):
    a = np.asarray(lut)
    if a.dtype.kind not in "iu" or a.shape not in ((256,), (3, 256)) or a.min() < 0 or a.max() > 255:
        raise ValueError("lut is a (3, 256) or (256,) array of ints 0 .. 255, what adjust_lut returns")
    return np.ascontiguousarray(np.broadcast_to(a.astype(np.uint8), (3, 256)))


WARP_ONE = 1 << 16                   # 1.0 in the Q16 of a warp's inverse map
WARP_MIN_SCALE, WARP_MAX_SCALE = 0.125, 8.0


def _warp_number(v, what):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
        raise ValueError("%s is a finite number (got %r)" % (what, v))
    return float(v)


def warp_matrix(box, scale=1.0, angle=0.0, offset=(0, 0), flip=None):
    """The inverse map of a scale, a turn, a mirror and an offset of a selection's box, as six ints in Q16 (pure host arithmetic,
    exact and the same on every machine): (ayy, ayx, ay0, axy, axx, ax0) take a destination pixel (y, x) to its
    source position sy = ayy y + ayx x + ay0, sx = axy y + axx x + ax0, where k << 16 is the centre of source row or column k.
    The forward map turns the object by `angle` degrees, counter-clockwise on the screen, about the centre c of `box` =
    (y0, x0, y1, x1), half open; scales it by `scale`, a number or a (sy, sx) pair, each in 1/8 .. 8, along the object's own axes;
    mirrors it by `flip` (None, "h", "v" or "hv", about the box as move_selection mirrors) and puts the centre at c + `offset` =
    (dy, dx), ints or floats that are quantised to half pixels -- a quarter turn of a box whose sides differ in parity leaves
    the object half a pixel off the grid, and a front end cancels that with an offset of one half.  The inverse's linear part is
    Fl diag(1 / sy, 1 / sx) R^T, each entry round(float64 * 65536) with the cosine and sine of a multiple of 90 degrees taken as
    exactly 0 and +-1; the translation is made from doubled coordinates in integers.  Below a scale of 1/2 the bilinear taps
    undersample: there is no prefilter and no claim of quality, as with max_side.  ValueError for a bad argument."""
    try:
        by0, bx0, by1, bx1 = (int(v) for v in box)
    except (TypeError, ValueError):
        raise ValueError("box is (y0, x0, y1, x1) (got %r)" % (box,))
    if by1 <= by0 or bx1 <= bx0:
        raise ValueError("box (y0, x0, y1, x1) is half open and not empty (got %r)" % (box,))
    if isinstance(scale, (tuple, list)):
        if len(scale) != 2:
            raise ValueError("scale is a number or a (sy, sx) pair (got %r)" % (scale,))
        scy, scx = _warp_number(scale[0], "scale"), _warp_number(scale[1], "scale")
    else:
        scy = scx = _warp_number(scale, "scale")
    if not (WARP_MIN_SCALE <= scy <= WARP_MAX_SCALE and WARP_MIN_SCALE <= scx <= WARP_MAX_SCALE):
        raise ValueError("scale lies in 1/8 .. 8 (got %r)" % (scale,))
    angle = _warp_number(angle, "angle")
    try:
        dy, dx = offset
    except (TypeError, ValueError):
        raise ValueError("offset is (dy, dx), two numbers (got %r)" % (offset,))
    dy, dx = _warp_number(dy, "offset"), _warp_number(dx, "offset")
    if abs(dy) > MOVE_MAX_OFFSET or abs(dx) > MOVE_MAX_OFFSET:
        raise ValueError("offset is (dy, dx), at most %d in magnitude (got %r)" % (MOVE_MAX_OFFSET, offset))
    if not (flip is None or isinstance(flip, str)) or flip not in MOVE_FLIPS:
        raise ValueError("flip is None, 'h', 'v' or 'hv' (got %r)" % (flip,))
    quarter = angle % 360.0
    if quarter % 90.0 == 0.0:
        cos, sin = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[int(quarter // 90.0)]
    else:
        cos, sin = math.cos(math.radians(angle)), math.sin(math.radians(angle))
    fy, fx = (-1.0 if MOVE_FLIPS[flip] & 2 else 1.0), (-1.0 if MOVE_FLIPS[flip] & 1 else 1.0)
    ayy, ayx = round(fy * (1.0 / scy) * cos * WARP_ONE), round(fy * (1.0 / scy) * sin * WARP_ONE)
    axy, axx = round(fx * (1.0 / scx) * -sin * WARP_ONE), round(fx * (1.0 / scx) * cos * WARP_ONE)
    cy2, cx2 = by0 + by1 - 1, bx0 + bx1 - 1                            # the centre, doubled
    dy2, dx2 = cy2 + round(2 * dy), cx2 + round(2 * dx)                # where it lands, doubled
    return (ayy, ayx, (cy2 * WARP_ONE - (ayy * dy2 + ayx * dx2)) >> 1, axy, axx, (cx2 * WARP_ONE - (axy * dy2 + axx * dx2)) >> 1)


def _check_warp_map(m):
    """six ints within the limits of include/sketchedit_warp.h -> a tuple of Python ints"""
    try:
        vals = tuple(m)
    except TypeError:
        raise TypeError("matrix is six ints (ayy, ayx, ay0, axy, axx, ax0) in Q16 (got %r)" % (m,))
    if len(vals) != 6 or not all(isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) for v in vals):
        raise ValueError("matrix is six ints (ayy, ayx, ay0, axy, axx, ax0) in Q16 (got %r)" % (m,))
    vals = tuple(int(v) for v in vals)
    if any(abs(vals[i]) > WARP_MAX_COEF for i in (0, 1, 3, 4)) or any(abs(vals[i]) > WARP_MAX_TRANSLATION for i in (2, 5)):
        raise ValueError("matrix: a coefficient is at most 2^20 and a translation at most 2^40 in magnitude (got %r)" % (vals,))
    return vals


def warp_rect(box, m, frame_hw):
    """The rectangle of the frame a warped selection lands in (pure host arithmetic in exact integers and fractions; DESIGN.md
    6s): no pixel outside it has a tap with weight inside `box` = (y0, x0, y1, x1) under the inverse map `m` (six Q16 ints).  A
    pixel has one only where its source position lies in [y0 - 1, y1] x [x0 - 1, x1]; the forward image of that rectangle's four
    corners under the inverse of `m` bounds those pixels: floor of the minimum to ceil of the maximum, plus one.  Clipped to the
    frame of `frame_hw` = (Hi, Wi), and a side under 16 widened to 16 inside the frame exactly as move_rect widens it.
    -> (y0, x0, h, w), or None when nothing lands in the frame.  ValueError for a singular `m`."""
    by0, bx0, by1, bx1 = (int(v) for v in box)
    ayy, ayx, ay0, axy, axx, ax0 = (int(v) for v in m)
    det = ayy * axx - ayx * axy
    if det == 0:
        raise ValueError("the map %r is singular" % (tuple(m),))
    ys, xs = [], []
    for qy in (by0 - 1, by1):
        for qx in (bx0 - 1, bx1):
            u, v = qy * WARP_ONE - ay0, qx * WARP_ONE - ax0
            ys.append(Fraction(axx * u - ayx * v, det))
            xs.append(Fraction(ayy * v - axy * u, det))

    def axis(vals, extent):
        lo, hi = max(math.floor(min(vals)), 0), min(math.ceil(max(vals)) + 1, extent)
        if hi <= lo:
            return None
        if hi - lo < MOVE_MIN_SIDE:
            lo = min(max(lo - (MOVE_MIN_SIDE - (hi - lo)) // 2, 0), extent - MOVE_MIN_SIDE)
            hi = lo + MOVE_MIN_SIDE
        return lo, hi - lo

    ya, xa = axis(ys, int(frame_hw[0])), axis(xs, int(frame_hw[1]))
    return None if ya is None or xa is None else (ya[0], xa[0], ya[1], xa[1])


# ---- the canvas of a session (include/sketchedit_canvas.h) -----------------------------------------------------------
_MX, _MY, _T = _lib.CANVAS_MIRROR_X, _lib.CANVAS_MIRROR_Y, _lib.CANVAS_TRANSPOSE
CANVAS_ORIENTS = {None: 0, "h": _MX, "v": _MY, "180": _MX | _MY, "transpose": _T, "ccw": _T | _MX, "cw": _T | _MY, "transverse": _T | _MX | _MY}
CANVAS_PADS = {"edge": _lib.CANVAS_EDGE, "reflect": _lib.CANVAS_REFLECT}
CANVAS_FILLS = (None, "network")                 # extend_canvas' `fill`


def _canvas_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def canvas_orient(name):
    """An orientation's name -> its value 0 .. 7 (bit 0 mirrors x, bit 1 mirrors y, bit 2 transposes after the mirrors): None, "h"
    (flip horizontal), "v" (flip vertical), "180", "transpose", "ccw" and "cw" (quarter turns), "transverse".  ValueError for
    anything else."""
    if not (name is None or isinstance(name, str)) or name not in CANVAS_ORIENTS:
        raise ValueError("orient is one of %s (got %r)" % (", ".join(repr(k) for k in CANVAS_ORIENTS), name))
    return CANVAS_ORIENTS[name]


def canvas_pad(pad):
    """`pad` -> (mode, colour): "edge", "reflect", or an (r, g, b) triple of ints 0 .. 255 -- the constant's colour as the library
    takes it, r in the low byte.  ValueError for anything else."""
    if isinstance(pad, str) and pad in CANVAS_PADS:
        return CANVAS_PADS[pad], 0
    try:
        r, g, b = pad
    except (TypeError, ValueError):
        raise ValueError("pad is 'edge', 'reflect' or an (r, g, b) triple (got %r)" % (pad,))
    if not all(_canvas_int(v) and 0 <= v <= 255 for v in (r, g, b)):
        raise ValueError("pad is 'edge', 'reflect' or an (r, g, b) triple of ints 0 .. 255 (got %r)" % (pad,))
    return CANVAS_CONSTANT, int(r) | int(g) << 8 | int(b) << 16


def canvas_size(frame_hw, orient, rect):
    """The geometry of a canvas step, pure host arithmetic: a frame of `frame_hw` oriented by `orient` (a name canvas_orient
    takes) and cut or extended to `rect` = (y0, x0, h, w) in ORIENTED coordinates -- either origin may be negative and the
    rectangle may reach past the oriented frame; None: the whole oriented frame.  -> ((Hn, Wn), (oy, ox)): the new frame's
    size and the rectangle's origin.  ValueError for a rect that is not four ints, a side outside 1 .. 32768, 3 Hn Wn >= 2^31,
    an origin above 2^20 in magnitude, and a new frame below a session's minimum (H // 8 * 8 >= 16, likewise W)."""
    o = canvas_orient(orient)
    Ho, Wo = (frame_hw[1], frame_hw[0]) if o & 4 else (frame_hw[0], frame_hw[1])
    if rect is None:
        rect = (0, 0, Ho, Wo)
    try:
        y0, x0, h, w = rect
    except (TypeError, ValueError):
        raise ValueError("rect is (y0, x0, h, w), four ints in oriented coordinates (got %r)" % (rect,))
    if not all(_canvas_int(v) for v in (y0, x0, h, w)):
        raise ValueError("rect is (y0, x0, h, w), four ints in oriented coordinates (got %r)" % (rect,))
    y0, x0, h, w = int(y0), int(x0), int(h), int(w)
    if not (1 <= h <= CANVAS_MAX_SIDE and 1 <= w <= CANVAS_MAX_SIDE) or 3 * h * w >= 1 << 31:
        raise ValueError("rect %r: sides are 1 .. %d and 3 h w < 2^31" % ((y0, x0, h, w), CANVAS_MAX_SIDE))
    if abs(y0) > CANVAS_MAX_OFFSET or abs(x0) > CANVAS_MAX_OFFSET:
        raise ValueError("rect %r: an origin is at most %d in magnitude" % ((y0, x0, h, w), CANVAS_MAX_OFFSET))
    if h // 8 * 8 < 16 or w // 8 * 8 < 16:
        raise ValueError("rect %r: the new frame would be too small for a session: %dx%d" % ((y0, x0, h, w), w, h))
    return (h, w), (y0, x0)


def canvas_new_box(oriented_hw, new_hw, origin):
    """The tight box (y0, x0, y1, x1), half open, in the NEW frame's coordinates, of the area a canvas step adds -- the pixels of
    the rectangle that lie outside the oriented frame -- in closed form; None when the rectangle adds none (a crop)."""
    (Ho, Wo), (Hn, Wn), (oy, ox) = oriented_hw, new_hw, origin
    iy0, iy1, ix0, ix1 = max(-oy, 0), min(Ho - oy, Hn), max(-ox, 0), min(Wo - ox, Wn)      # the old pixels' rectangle
    if iy0 >= iy1 or ix0 >= ix1:
        return (0, 0, Hn, Wn)
    rows_full, cols_full = iy0 == 0 and iy1 == Hn, ix0 == 0 and ix1 == Wn
    if rows_full and cols_full:
        return None

    def axis(lo, hi, n, other_full):
        if not other_full or (lo > 0 and hi < n):
            return 0, n
        return (0, lo) if lo > 0 else (hi, n)
    (y0, y1), (x0, x1) = axis(iy0, iy1, Hn, cols_full), axis(ix0, ix1, Wn, rows_full)
    return (y0, x0, y1, x1)


def png_from_zlib(stream, h, w):
    """The PNG file around a zlib stream of filtered 8-bit RGB rows: signature, IHDR, ONE IDAT holding
    `stream` as it is, IEND -- the chunk framing and its CRCs are the host's part of a patch that was encoded on the device."""
    import struct
    from .png_worker import _SIG, _chunk
    return _SIG + _chunk(b"IHDR", struct.pack(">IIBBBBB", int(w), int(h), 8, 2, 0, 0, 0)) + _chunk(b"IDAT", bytes(stream)) + _chunk(b"IEND", b"")


PNG_SIDE_MIN, PNG_SIDE_MAX = 16, 8192       # the sides of a rectangle the device encoder takes (include/sketchedit_png.h)


# ---- the file around a device-encoded JPEG segment (include/sketchedit_jpg.h) ---------------------------------------
# Annex K's quantisation tables in zigzag order, and its Huffman tables as a DHT segment carries them (counts per length, symbols)
JPG_BASE_LUMA = (16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40, 26, 24, 22, 22, 24, 49, 35, 37, 29, 40, 58, 51, 61, 60,
                 57, 51, 56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56, 80, 109, 81, 87, 95, 98, 103, 104, 103, 62, 77, 113, 121, 112,
                 100, 120, 92, 101, 103, 99)
JPG_BASE_CHROMA = (17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66, 99) + (99,) * 49
JPG_DHT = (
    (0x00, (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12))),
    (0x10, (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125),
     (1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36, 51,
      98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85,
      86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137,
      138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185,
      186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232,
      233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250)),
    (0x01, (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12))),
    (0x11, (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119),
     (0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240, 21, 98,
      114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83,
      84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135,
      136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183,
      184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231,
      232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250)),
)
JPG_QUALITY = 90                             # encode="jpg"


def jpg_quant_table(base, quality):
    """Annex K's table `base` under libjpeg's quality scaling, in zigzag order (rule 4 of include/sketchedit_jpg.h)"""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError("quality is 1 .. 100 (got %r)" % (quality,))
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return [min(max((b * scale + 50) // 100, 1), 255) for b in base]


JPG_SUBSAMPLINGS = ("444", "420")
JPG_TABLE_BYTES = 272                        # one table of a device record: 16 counts of codes per length, 256 symbols (zero-padded)


def _check_subsampling(subsampling):
    if not (isinstance(subsampling, str) and subsampling in JPG_SUBSAMPLINGS):
        raise ValueError("subsampling is '444' or '420' (got %r)" % (subsampling,))
    return subsampling


def jpg_dht_from_record(tables):
    """A device table record (include/sketchedit_jpg2.h rule 5e: 4 x 272 bytes, DC lum, AC lum, DC chr, AC chr) -> the four
    (class/id, counts, symbols) of its DHT segments, with the true symbol counts, not the padding"""
    tables = bytes(tables)
    if len(tables) != 4 * JPG_TABLE_BYTES:
        raise ValueError("a table record is %d bytes (got %d)" % (4 * JPG_TABLE_BYTES, len(tables)))
    out = []
    for k, tc_th in enumerate((0x00, 0x10, 0x01, 0x11)):
        part = tables[k * JPG_TABLE_BYTES:(k + 1) * JPG_TABLE_BYTES]
        n = sum(part[:16])
        if not 1 <= n <= 256:
            raise ValueError("table %d of the record has %d symbols" % (k, n))
        out.append((tc_th, tuple(part[:16]), tuple(part[16:16 + n])))
    return out


def jpg_from_scan(scan, h, w, quality, subsampling="444", tables=None):
    """The baseline JPEG file around an entropy-coded segment of an h x w rectangle at `quality`: SOI, a JFIF
    APP0, two DQT, SOF0 (three components; Y's sampling factors 0x22 for subsampling="420"), four DHT (Annex K's, or those of
    `tables`, the device's record of an image coded with its own tables), DRI (one restart interval per row of MCUs), SOS, `scan`
    as it is, EOI -- the headers are the host's part of a patch that was encoded on the device."""
    h, w = int(h), int(w)
    mcu = 16 if _check_subsampling(subsampling) == "420" else 8
    dht = JPG_DHT if tables is None else jpg_dht_from_record(tables)

    def seg(marker, payload):
        return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)
    out = [b"\xff\xd8", seg(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0"),
           seg(0xDB, [0] + jpg_quant_table(JPG_BASE_LUMA, quality)), seg(0xDB, [1] + jpg_quant_table(JPG_BASE_CHROMA, quality)),
           seg(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([3, 1, 0x22 if mcu == 16 else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))]
    out += [seg(0xC4, (tc_th,) + counts + symbols) for tc_th, counts, symbols in dht]
    out += [seg(0xDD, (-(-w // mcu)).to_bytes(2, "big")), seg(0xDA, [3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]), bytes(scan), b"\xff\xd9"]
    return b"".join(out)


def _check_encode(encode):
    """-> None, "png", ("jpg", quality) or ("jpg", quality, subsampling, optimize)"""
    if encode is None or (isinstance(encode, str) and encode == "png"):
        return encode
    if isinstance(encode, str) and encode == "jpg":
        return ("jpg", JPG_QUALITY)
    if (isinstance(encode, tuple) and 2 <= len(encode) <= 4 and isinstance(encode[0], str) and encode[0] == "jpg" and isinstance(encode[1], int)
            and not isinstance(encode[1], bool) and 1 <= encode[1] <= 100
            and (len(encode) < 3 or (isinstance(encode[2], str) and encode[2] in JPG_SUBSAMPLINGS))
            and (len(encode) < 4 or isinstance(encode[3], bool))):
        sub, opt = encode[2] if len(encode) > 2 else "444", encode[3] if len(encode) > 3 else False
        if sub == "444" and not opt:             # the defaults spelled out: the call the backends have always received
            return ("jpg", int(encode[1]))
        return ("jpg", int(encode[1]), sub, opt)
    raise ValueError("encode is None (raw (h,w,3) arrays), 'png', 'jpg' (quality %d), ('jpg', quality 1 .. 100), ('jpg', quality, '444' | '420') "
                     "or ('jpg', quality, '444' | '420', a bool: per-image Huffman tables) (got %r)" % (JPG_QUALITY, encode))




def _check_feather(feather):
    """-> None (the hard paste: None or 0) or the radius 1 .. 16 of the feathered paste"""
    if feather is None:
        return None
    if not isinstance(feather, int) or isinstance(feather, bool) or not 0 <= feather <= FEATHER_MAX_RADIUS:
        raise ValueError("feather is None or an int 0 .. %d, the radius of the paste's soft edge in frame pixels (got %r)"
                         % (FEATHER_MAX_RADIUS, feather))
    return int(feather) or None


def _check_hole_grow(hole_grow):
    if not isinstance(hole_grow, (int, np.integer)) or isinstance(hole_grow, (bool, np.bool_)) or not 0 <= hole_grow <= SELECT_MAX_GROW:
        raise ValueError("hole_grow is an int 0 .. %d, in frame pixels (got %r)" % (SELECT_MAX_GROW, hole_grow))
    return int(hole_grow)


def _encoded(be, encode, frames, windows):
    """the windows of `frames` as files, by a checked `encode` that is not None: one backend call"""
    if encode == "png":
        return be.crop_png(frames, windows)
    if len(encode) == 2:                         # (the call the backends have always received)
        return be.crop_jpg(frames, windows, encode[1])
    return be.crop_jpg(frames, windows, encode[1], subsampling=encode[2], optimize=encode[3])


def _by_size(windows):
    """{(h, w): [indices into `windows`]}, sizes in the order they first appear"""
    out = {}
    for i, w in enumerate(windows):
        out.setdefault((w[2], w[3]), []).append(i)
    return out


class _Regions(tuple):
    """the windows of a region edit's journal entry (its slots are a list in the same order)"""


class _Sequence(tuple):
    """the rectangles of a move's journal entry, in the order its steps wrote them: they may overlap, so undo
    exchanges them in reverse order and redo in this one (its slots are a list in the same order)"""


class _Canvas(tuple):
    """the (H, W) of the state a canvas step's journal entry HOLDS: its slot is [frame, frame_hw, lock plane] whole --
    the other state of the session -- and undo / redo exchange the session's three fields with it: no kernel, no download"""


def _run_windows(be, frames, origins, crops, window_hw, work, locks, commit, low_latency):
    """The one choice of the backend entry a window edit takes: `locks` = a plane or None per request
    (None: no request of the call has one) -> run_locked; else `work` = the working size (None: no max_side; it is not
    compared with the window) -> run_scaled; else run.  -> what the entry returns."""
    if locks is not None:
        return be.run_locked(frames, origins, crops, locks, window_hw, work, commit, low_latency)
    if work is not None:
        return be.run_scaled(frames, origins, crops, window_hw, work, commit, low_latency)
    return be.run(frames, origins, crops, window_hw[0], window_hw[1], commit, low_latency)


def _paste_windows(be, frames, origins, window_hw, work, locks, rgb, m8):
    """the paste that belongs to an uncommitted `_run_windows` of the same `work` and `locks`"""
    if locks is not None:
        be.paste_locked(frames, origins, locks, window_hw, rgb, m8)
    elif work is not None:
        be.paste_scaled(frames, origins, window_hw, rgb, m8)
    else:
        be.paste(frames, origins, rgb, m8)


def _check_blend(blend, feather, be):
    """-> whether a fill is pasted seamlessly; its refusals, all in front of the first backend call"""
    if not (blend is None or isinstance(blend, str)) or blend not in MOVE_BLENDS:
        raise ValueError("blend is None or 'seamless' (got %r)" % (blend,))
    if blend is None:
        return False
    if feather is not None:
        raise ValueError("blend=%r and feather=%r are two edge rules for one paste: give one" % (blend, feather))
    if not all(callable(getattr(be, name, None)) for name in ("move_blend", "fill_lift")):
        raise NotImplementedError("this backend has no move_blend / fill_lift: blend=%r needs the seamless drop (DESIGN.md 6x, 6z)" % (blend,))
    return True


def _blend_box(box, win):
    """the box a seamless fill hands to the membrane: `box` (y0, x0, y1, x1) cut to the window -> it, or () where they do not
    meet (nothing is a target: no launch); ValueError for a side above BLEND_MAX_SIDE"""
    y0, x0, h, w = win
    b = (max(box[0], y0), max(box[1], x0), min(box[2], y0 + h), min(box[3], x0 + w))
    if b[0] >= b[2] or b[1] >= b[3]:
        return ()
    if max(b[2] - b[0], b[3] - b[1]) > BLEND_MAX_SIDE:
        raise ValueError("blend='seamless' takes a region whose box inside the window has sides of at most %d (got %r)" % (BLEND_MAX_SIDE, b))
    return b


def _edit_info(info, locked, work, undoable, feather=None):
    """an edit's `info` with what only some sessions report: locked (a lock plane), work (max_side), undoable (history),
    feather (a feathered paste)"""
    if feather is not None:
        info["feather"] = feather
    if locked:
        info["locked"] = True
    if work is not None:
        info["work"] = work
    if undoable is not None:
        info["undoable"] = undoable
    return info


SELECT_PASSES = 8            # flood passes per library call, and per download of their `changed` words


def tiles_box(tiles):
    """The tile records of a plane (se_sketch_tiles_u8: [count, y0, x0, y1, x1] per tile) -> (box, count): the tight box
    (y0, x0, y1, x1), half open, of its pixels > 0 and their number; (None, 0) for an empty plane.  Pure host arithmetic."""
    t = np.asarray(tiles).reshape(-1, 5)
    t = t[t[:, 0] > 0]
    if t.shape[0] == 0:
        return None, 0
    return (int(t[:, 1].min()), int(t[:, 2].min()), int(t[:, 3].max()), int(t[:, 4].max())), int(t[:, 0].sum())


class Selection:
    """A selection of an editing session: a frame-sized mask that lives on the device.  `.plane`: the (Hi,Wi)
    uint8 fill plane there, 255 = selected; `.box` = (y0, x0, y1, x1), half open, its tight box; `.count` its pixels;
    `.frame_hw` the size of the frame it was made on.  A selection is a mask, not a view of the frame: it stays what it is
    when the frame changes.  An EMPTY selection (what a subtraction can leave) has `.box` None and `.count` 0; its plane is
    all zeros."""

    def __init__(self, backend, plane, box, count, frame_hw):
        self._backend = backend
        self.plane, self.box, self.count, self.frame_hw = plane, None if box is None else tuple(int(v) for v in box), int(count), tuple(frame_hw)

    def mask(self):
        """the box's crop of the plane as a (y1 - y0, x1 - x0) uint8 array of 0 / 255 on the host (a download of the box only):
        what a front end outlines; a (0, 0) array, and no download, for an empty selection"""
        if self.box is None:
            return np.zeros((0, 0), np.uint8)
        y0, x0, y1, x1 = self.box
        return self._backend.crop(self.plane, y0, x0, y1 - y0, x1 - x0)

    def edges(self, first_cap=4096):
        """The boundary of the selection as raw records on the host: an (N,4) int32 array of [ax, ay, bx, by] in
        quarter pixels, one per boundary run of a 64 x 64 tile, in se_outline_u8's order -- a valid argument for the lasso's
        rasteriser, which re-makes the plane from them bit for bit.  Extracted on the device: 16 bytes per run come down, not
        the plane.  An empty selection gives a (0,4) array and no backend call; otherwise ONE backend call with room for
        `first_cap` records and, only if there are more, exactly one more with room for all.  NotImplementedError from a backend
        that cannot extract outlines."""
        if not isinstance(first_cap, (int, np.integer)) or isinstance(first_cap, (bool, np.bool_)) or not 0 <= first_cap <= OUTLINE_MAX_CAP:
            raise ValueError("first_cap is an int 0 .. %d (got %r)" % (OUTLINE_MAX_CAP, first_cap))
        if self.box is None:
            return np.zeros((0, 4), np.int32)
        return _outline_records(self._backend, self.plane, int(first_cap))

    def rings(self, first_cap=4096):
        """The outline of the selection as closed rings: outline_rings of `edges(first_cap)` -- integer corner
        points in frame pixels, outer rings clockwise on the screen and holes counter-clockwise, each from its smallest vertex
        in (y, x) order, sorted by it.  What a front end draws (rings_svg_path), the serialised form of a selection, and an exact
        round trip: select_lasso(selection.rings()) on a frame of this size re-makes the plane, box and count (while the rings
        have at most 65 536 edges, the lasso's limit).  [] for an empty selection, with no backend call."""
        return outline_rings(self.edges(first_cap))




def _outline_records(be, plane, first_cap):
    """all boundary records of a plane on the device: one `outline` call of the backend, and exactly one more when the first
    capacity was too small"""
    if not hasattr(be, "outline"):
        raise NotImplementedError("this session's backend (%s) cannot extract outlines: it has no `outline`" % type(be).__name__)
    total, rec = be.outline(plane, first_cap)
    if total > OUTLINE_MAX_CAP:
        raise ValueError("the outline has %d runs, more than one call returns (%d)" % (total, OUTLINE_MAX_CAP))
    if total > first_cap:
        total, rec = be.outline(plane, total)
    rec = np.asarray(rec, np.int32).reshape(-1, 4)
    if rec.shape[0] != total:
        raise RuntimeError("outline: %d records came back, %d were counted" % (rec.shape[0], total))
    return rec


class _ModelBackend:
    """The device side of an editing session: an EditLine2Model's engine and torch for the copies.  (A seam: the host
    logic of EditSession and of the window batcher is tested against a scripted stand-in.)"""

    def __init__(self, model):
        if not (hasattr(model, "engine") and hasattr(model, "edit_window_u8")):
            raise ValueError("an editing session needs an EditLine2Model (its library engine runs the window steps)")
        self.model = model

    def _device(self):
        import torch
        return torch.device("cuda", self.model.engine().device)

    def upload(self, a):
        return _lib.upload_u8(a, self._device())

    def run(self, frames, origins, sketches, h, w, commit, low_latency):
        """-> (rgb, mask_u8, counts): the device results and the border counts on the host (a synchronisation)"""
        rgb, m8, hits = self.model.edit_window_u8(frames, origins, sketches, h, w, commit=commit, low_latency=low_latency)
        return rgb, m8, hits.cpu().tolist()

    def paste(self, frames, origins, rgb, m8):
        self.model.engine().window_paste_u8(frames, origins, rgb, m8)

    def run_scaled(self, frames, origins, sketches, window_hw, work_hw, commit, low_latency):
        """`run` with the forward at the working size `work_hw`: rgb and mask_u8 come back at that size"""
        rgb, m8, hits = self.model.edit_window_u8(frames, origins, sketches, window_hw[0], window_hw[1], commit=commit,
                                                  low_latency=low_latency, work_hw=work_hw)
        return rgb, m8, hits.cpu().tolist()

    def paste_scaled(self, frames, origins, window_hw, rgb, m8):
        self.model.engine().window_paste_resize_u8(frames, origins, window_hw, rgb, m8)

    def run_locked(self, frames, origins, sketches, locks, window_hw, work_hw, commit, low_latency):
        """`run` (work_hw None) or `run_scaled` for a group in which at least one request's frame has a lock plane (DESIGN.md
        6g): locks[i] = that plane on the device, or None"""
        rgb, m8, hits = self.model.edit_window_u8(frames, origins, sketches, window_hw[0], window_hw[1], commit=commit,
                                                  low_latency=low_latency, work_hw=work_hw, locks=locks)
        return rgb, m8, hits.cpu().tolist()

    def paste_locked(self, frames, origins, locks, window_hw, rgb, m8):
        self.model.engine().window_paste_locked_u8(frames, origins, locks, window_hw, rgb, m8)

    def paste_feather(self, frames, origins, locks, window_hw, radius, rgb, m8):
        """the feathered paste of an uncommitted run's results: rgb and m8 as `run` / `run_scaled` /
        `run_locked` returned them (resized to the window here when they are at a working size), locks a plane or None per
        request, or None"""
        self.model.window_paste_feather_u8(frames, origins, locks, window_hw, radius, rgb, m8)

    def run_fill(self, frames, origins, sketches, holes, locks, window_hw, work_hw, low_latency, raw=False):
        """the fill of a group: holes[i] = the frame's fill plane on the device, sketches[i] the window's sketch
        or None, locks a plane or None per request, or None; never commits and downloads nothing.  -> (rgb, mask_u8), at the
        working size `work_hw` if that is not None.  raw: rgb is the generator's own prediction at every pixel,
        not the composite -- the lift of a seamless paste"""
        return self.model.fill_window_u8(frames, origins, sketches, holes, window_hw[0], window_hw[1], low_latency=low_latency,
                                         work_hw=work_hw, locks=locks, raw=raw)

    def fill_lift(self, rgb, window_hw):
        """the raw patch of ONE fill, run_fill(raw=True)'s (1,H,W,3), as the lift move_blend takes for the window:
        resized to the window's (h, w) with Pillow's BICUBIC when it is at a working size (Engine.resize_u8), its rows at a
        journal slot's pitch -- as it is where 3 w is a multiple of 16, else through the journal's save of the patch itself"""
        h, w = (int(v) for v in window_hw)
        eng = self.model.engine()
        if tuple(rgb.shape[1:3]) != (h, w):
            rgb = eng.resize_u8(rgb, (h, w))
        return rgb[0].view(h, 3 * w) if (3 * w) % 16 == 0 else eng.window_save_u8([rgb[0]], [(0, 0)], (h, w))[0]

    def fill_keep(self, frames, origins, holes, locks, window_hw):
        """the keep planes of a fill's paste: what paste_locked / paste_feather take in place of the locks"""
        return self.model.fill_keep_u8(frames, origins, holes, locks, window_hw)

    def select_similar(self, frame, seed, tolerance, contiguous, grow):
        """the selection by colour of a resident frame, made on the device: the state plane, if `contiguous`
        flood calls of SELECT_PASSES passes each until one reports a pass that stored nothing -- each call's `changed` words
        are ONE download, the only ones in front of the tile records -- then the grow and the records of its plane.
        -> (plane, box, count): the frame-sized fill plane on the device, its tight box (y0, x0, y1, x1) and its pixels"""
        Hi, Wi = int(frame.shape[0]), int(frame.shape[1])
        state = self.model.select_similar_u8(frame, seed, tolerance, contiguous)
        if contiguous:
            passes = 0
            while 0 not in self.model.select_flood_u8(state, passes=SELECT_PASSES).cpu().tolist():
                passes += SELECT_PASSES
                if passes > Hi * Wi:             # every productive pass reaches a pixel at least
                    raise RuntimeError("select_similar: %d passes over a %dx%d frame without a fixed point" % (passes, Wi, Hi))
        plane = self.model.select_grow_u8(state, grow)
        box, count = tiles_box(self.tiles(plane, 32))
        return plane, box, count

    def select_lasso(self, edges, frame_hw, grow):
        """the lasso selection of `edges`, the (N,4) int32 edges on the device: the even-odd fill, the grow when
        `grow` > 0 (a lasso's plane is a state plane of 6o as it is), the tile records of the result -- the one download.
        -> (plane, box, count) as select_similar returns them; box None and count 0 when no pixel centre is covered"""
        plane = self.model.lasso_fill_u8(edges, int(frame_hw[0]), int(frame_hw[1]))
        if grow > 0:
            plane = self.model.select_grow_u8(plane, grow)
        box, count = tiles_box(self.tiles(plane, 32))
        return plane, box, count

    def combine(self, a, b, op):
        """two selection planes (b None for the inversion) -> (plane, box, count) of a NEW plane, a op b; op is
        SE_COMBINE_*'s value"""
        plane = self.model.plane_combine_u8(a, b, op)
        box, count = tiles_box(self.tiles(plane, 32))
        return plane, box, count

    def modify(self, plane, op, radius, tiles=True):
        """a selection plane expanded, contracted or smoothed by the disc of `radius` -> (plane, box, count) of a NEW
        plane: one launch, then the tile records of the result -- the one download; op is SE_MODIFY_*'s value.  tiles=False: an
        intermediate of a border, nothing comes down and box and count are None"""
        out = self.model.plane_modify_u8(plane, op, radius)
        if not tiles:
            return out, None, None
        box, count = tiles_box(self.tiles(out, 32))
        return out, box, count

    def outline(self, plane, cap):
        """the boundary records of a plane on the device: three launches and ONE download, of 8 + 16 cap bytes
        -> (total, records (min(total, cap), 4) int32 on the host)"""
        words = self.model.outline_u8(plane, int(cap)).cpu().numpy()
        total, written = int(words[0]), int(words[1])
        return total, words[2:2 + 4 * written].reshape(-1, 4)

    def copy(self, plane):
        """a copy of a plane that is on the device, made there"""
        return plane.clone()

    def grow(self, plane, grow):
        """a NEW plane: the pixels within `grow` (1 .. 16) pixels of a selected one (DESIGN.md 6o's grow; a selection's 0 / 255
        plane is a state plane as it is)"""
        return self.model.select_grow_u8(plane, grow)

    def move_drop(self, frame, lift, lift_rect, plane, lock, box, offset, flip, radius):
        """the drop of a move, ONE launch in place on the frame: the pixels of `box` that `plane` selects, as the
        slot `lift` of `lift_rect` holds them, land `offset` away under `flip` (SE_MOVE_FLIP_*) where `lock` (or None) is 0, with a
        soft edge of `radius`"""
        self.model.move_drop_u8(frame, lift, lift_rect, plane, lock, box, offset, flip=flip, radius=radius)

    def move_blend(self, frame, lift, lift_rect, plane, lock, box, offset, flip):
        """the seamless drop of a move, in place on the frame: move_drop's arguments without the radius; the lifted
        pixels plus a membrane that equals frame - lift on the object's rim.  `lift_rect` holds the box grown by one pixel.  A
        fixed schedule of launches that depends on the box's size alone"""
        self.model.move_blend_u8(frame, lift, lift_rect, plane, lock, box, offset, flip=flip)

    def shift(self, plane, box, offset, flip):
        """a selection's plane moved as move_drop moves its pixels -> (plane, box, count) of a NEW plane: one
        launch, then the tile records of the result -- the one download"""
        out = self.model.plane_shift_u8(plane, box, offset, flip=flip)
        b, count = tiles_box(self.tiles(out, 32))
        return out, b, count

    def canvas(self, src, src_hw, out_hw, origin, orient, pad, rgb, tiles=False):
        """a NEW frame or plane, ONE launch: the rectangle `out_hw` at `origin` of `src` -- a frame, a plane, or None:
        a plane of zeros of `src_hw` that is never read -- oriented by `orient` (0 .. 7) and padded by `pad` (SE_CANVAS_*) with
        the colour `rgb`.  tiles=True (a carried selection): -> (plane, box, count), the tile records of the result being the one
        download"""
        out = self.model.canvas_u8(src, out_hw, origin=origin, orient=orient, pad=pad, pad_rgb=rgb, src_hw=src_hw)
        if not tiles:
            return out
        b, count = tiles_box(self.tiles(out, 32))
        return out, b, count

    def warp_drop(self, frame, lift, lift_rect, plane, lock, box, rect, m):
        """the drop of a transform, ONE launch in place on the frame: the pixels of `box` that `plane` selects, as
        the slot `lift` of `lift_rect` holds them, gathered through the inverse map `m` into `rect` where `lock` (or None) is 0"""
        self.model.warp_drop_u8(frame, lift, lift_rect, plane, lock, box, rect, m)

    def warp(self, plane, box, m):
        """a selection's plane warped as warp_drop warps its pixels -> (plane, box, count) of a NEW plane: one
        launch, then the tile records of the result -- the one download"""
        out = self.model.plane_warp_u8(plane, box, m)
        b, count = tiles_box(self.tiles(out, 32))
        return out, b, count

    def filter_blur(self, frame, lift, lift_rect, plane, lock, box, taps, amount, feather):
        """the blur or unsharp mask of a selection, ONE launch in place on the frame: the pixels of `box` that `plane`
        selects and `lock` (or None) leaves become the filter `taps` of the frame as the slot `lift` of `lift_rect` holds it, mixed
        by `amount` (Q8), with a soft edge of `feather`"""
        self.model.filter_blur_u8(frame, lift, lift_rect, plane, lock, box, taps, amount=amount, feather=feather)

    def filter_mosaic(self, frame, lift, lift_rect, plane, lock, box, cell, amount, feather):
        """the mosaic of a selection, ONE launch in place on the frame: as filter_blur with the mean of the pixel's
        `cell` x `cell` block of the lift"""
        self.model.filter_mosaic_u8(frame, lift, lift_rect, plane, lock, box, cell, amount=amount, feather=feather)

    def adjust(self, frame, lift, lift_rect, plane, lock, box, lut, matrix, amount, feather):
        """the tone and colour of a selection, ONE launch in place on the frame: the pixels of `box` that `plane`
        selects and `lock` (or None) leaves become the table `lut` (768 bytes on the device, or None), then the `matrix` (12 ints,
        or None), of the frame as the slot `lift` of `lift_rect` holds it, mixed by `amount` (Q8), with a soft edge of `feather`"""
        self.model.adjust_u8(frame, lift, lift_rect, plane, lock, box, lut=lut, matrix=matrix, amount=amount, feather=feather)

    def hist(self, frame, plane, box):
        """the histogram of the pixels of `box` that `plane` selects (None: all of them) -> a (4, 256) record that STAYS on the
        device: two launches, no download"""
        return self.model.adjust_hist_u8(frame, plane, box)

    def hist_lut(self, src, ref, mode, which, clip):
        """one or two hist records -> the table `adjust` takes, made and left on the device: one launch, no download"""
        return self.model.adjust_lut_u8(src, ref, mode, which, clip=clip)

    def save(self, frames, origins, window_hw):
        """the windows' rectangles -> one new journal slot each, on the stream the edit follows on"""
        return self.model.window_save_u8(frames, origins, window_hw)

    def swap(self, frames, origins, window_hw, slots):
        """rectangles <-> slots: undo, and redo"""
        self.model.window_swap_u8(frames, origins, window_hw, slots)

    def strokes(self, segs, frame_hw, windows):
        """the (h, w) sketches of `windows` (all of one size) of a frame of `frame_hw`, rasterised there from `segs` -- the
        (N,5) int32 segments, on the device -- in ONE call; -> one contiguous plane per window"""
        out = self.model.sketch_strokes_u8(segs, [frame_hw] * len(windows), [w[:2] for w in windows], windows[0][2:])
        return [out[i] for i in range(len(windows))]

    def tiles(self, sketch, tile):
        """the tile records of a full-size sketch that is on the device, on the host (a synchronisation)"""
        return self.model.sketch_tiles_u8(sketch, tile).cpu().numpy()

    def window_of(self, plane, y0, x0, h, w):
        """a window of a plane that is on the device, as a contiguous plane there"""
        return plane[y0:y0 + h, x0:x0 + w].contiguous()

    def select(self, t, idx):
        """rows `idx` of a batch result as a contiguous batch"""
        return t if list(idx) == list(range(t.shape[0])) else t[list(idx)].contiguous()

    def crop(self, frame, y0, x0, h, w):
        return frame[y0:y0 + h, x0:x0 + w].contiguous().cpu().numpy()

    def crop_png(self, frames, windows):
        """the windows (y0, x0, h, w) of `frames` as PNG files, encoded on the device: one encoder call per
        window size; the streams' sizes come down first (the synchronisation), then exactly that many bytes of each"""
        out = [None] * len(windows)
        for (h, w), idx in _by_size(windows).items():
            buf, sizes = self.model.png_encode_u8([frames[i] for i in idx], [windows[i][:2] for i in idx], (h, w))
            for k, (i, n) in enumerate(zip(idx, sizes.cpu().tolist())):
                out[i] = png_from_zlib(buf[k, :n].cpu().numpy().tobytes(), h, w)
        return out

    def crop_jpg(self, frames, windows, quality, subsampling="444", optimize=False):
        """the windows (y0, x0, h, w) of `frames` as baseline JPEG files at `quality`, encoded on the device: one
        encoder call per window size; the segments' sizes come down first (the synchronisation), then exactly that many bytes.
        subsampling="420" and/or optimize=True (four Huffman tables per image, which come down with the sizes) are the
        forms of DESIGN.md 6l."""
        out = [None] * len(windows)
        _check_subsampling(subsampling)
        for (h, w), idx in _by_size(windows).items():
            buf, sizes, tables = self.model.jpg2_encode_u8([frames[i] for i in idx], [windows[i][:2] for i in idx], (h, w), quality,
                                                           subsampling=subsampling, optimize=optimize)
            sizes = sizes.cpu().tolist()
            tables = tables.cpu().numpy() if tables is not None else None
            for k, (i, n) in enumerate(zip(idx, sizes)):
                out[i] = jpg_from_scan(buf[k, :n].cpu().numpy().tobytes(), h, w, quality, subsampling,
                                       tables[k].tobytes() if tables is not None else None)
        return out

    def download(self, frame):
        return frame.cpu().numpy()


def _sketch_array(sketch):
    """A request's sketch as a 2-D uint8 array: a PIL 'L' image or an array."""
    if hasattr(sketch, "mode"):
        if sketch.mode != "L":
            raise ValueError("a window edit takes an 'L' sketch (got mode %r)" % sketch.mode)
        sketch = np.asarray(sketch)
    sketch = np.asarray(sketch)
    if sketch.ndim != 2 or sketch.dtype != np.uint8:
        raise ValueError("a window edit takes a 2-D uint8 sketch")
    return sketch


class EditSession:
    """A frame that stays on the device and is edited in place through windows (INTEGRATION.md "Editing
    sessions").  `image`: a PIL image or an (H,W,3) uint8 array; uploaded once.  Every `edit` runs the forward on a window
    around the sketch only -- its result is DEFINED as the model's inference on that crop, pasted where the uint8 mask is
    > 0 -- so its time follows the edit, not the frame; pixels the edit does not select keep their bytes, and only the
    window's sketch and the window's result cross the bus.  The frame on the device is the session's state: the next edit
    sees this one's result.  Edits of one session are serialised; do not mix `edit` with a BatchingServer(window=True)
    that was handed the same session.
    `history` (0: no journal, the session as above): the number of edits `undo` can take back.  Before a
    committed paste the window's rectangle of the frame is copied into a journal slot on the device; `undo` exchanges
    rectangle and slot, `redo` exchanges them again -- the whole frame is byte-identical to what it was.  `history_bytes`
    caps the bytes of all slots (window_saved_bytes each, undo and redo together); over either cap the OLDEST undo entry is
    dropped; an edit whose own slot exceeds `history_bytes` is committed without a journal entry and clears the history
    (info["undoable"] = False).  A new edit drops the redo entries.
    `set_lock` gives the frame a lock plane: pixels no later edit may change.  The lock enters the forward
    where the mask is made -- a locked pixel is known context for the generator, not a hole it fills -- and the paste; it
    is the session's state like the frame, but not an edit: `undo` does not touch it -- but for a canvas step,
    whose undo brings back the frame's old size and, with it, the lock plane of that size.
    `canvas` and its wrappers crop_canvas, extend_canvas and orient_canvas replace the frame by a rectangle of
    itself, oriented, cut or extended, made on the device; frame_hw then changes."""

    def __init__(self, model, image, backend=None, history=0, history_bytes=None):
        if hasattr(image, "convert"):
            image = np.asarray(image.convert("RGB"))
        image = np.asarray(image)
        if image.ndim != 3 or image.shape[2] != 3 or image.dtype != np.uint8:
            raise ValueError("a session's frame is an (H,W,3) uint8 RGB image")
        Hi, Wi = image.shape[:2]
        if Hi // 8 * 8 < 16 or Wi // 8 * 8 < 16:
            raise ValueError("image too small: %dx%d" % (Wi, Hi))
        self.model = model
        self.backend = backend if backend is not None else _ModelBackend(model)
        self.frame_hw = (Hi, Wi)
        self._frame = self.backend.upload(image)
        self._lock = threading.Lock()
        if int(history) < 0 or (history_bytes is not None and int(history_bytes) < 0):
            raise ValueError("history and history_bytes must not be negative")
        self.history = int(history)
        self.history_bytes = None if history_bytes is None else int(history_bytes)
        self._undo, self._redo = [], []          # entries (window, slot, bytes); the next to undo / redo is the last
        self._lock_plane = None                  # the (Hi,Wi) uint8 lock plane on the device (0 / 255), or None

    # ---- locked regions -----------------------------------------------------------------------------------------
    def set_lock(self, mask):
        """`mask`: (Hi,Wi), a uint8 or bool array or a PIL 'L' image, non-zero = locked; uploaded once (as 0 / 255) and kept
        on the device until the next set_lock.  None frees it.  Every later edit leaves the locked pixels' bytes as they
        are.  Not an edit: nothing is journalled, and `undo` does not bring an earlier lock back -- with ONE exception: a canvas
        step changes the frame's geometry, so its undo and redo restore the lock plane that belonged to the
        geometry they return to, whatever set_lock did in between.
        A Selection of this frame's size locks its pixels: the lock plane is a COPY of its plane made on the
        device -- nothing is uploaded, and what is combined from the selection later cannot reach the lock; an empty selection
        is None."""
        if isinstance(mask, Selection):
            self._check_selection(mask, "set_lock")
            with self._lock:
                self._lock_plane = None if mask.box is None else self.backend.copy(mask.plane)
            return
        if mask is not None:
            if hasattr(mask, "mode"):
                if mask.mode != "L":
                    raise ValueError("a lock is an 'L' image (got mode %r)" % mask.mode)
                mask = np.asarray(mask)
            mask = np.asarray(mask)
            if mask.dtype != np.uint8 and mask.dtype != np.bool_:
                raise TypeError("a lock is a uint8 or bool array (got %s)" % mask.dtype)
            if mask.shape != self.frame_hw:
                raise ValueError("a lock is the frame's (%d,%d) plane (got %r)" % (self.frame_hw + (mask.shape,)))
            mask = np.where(mask != 0, np.uint8(255), np.uint8(0))
        with self._lock:
            self._lock_plane = None if mask is None else self.backend.upload(mask)

    def lock(self):
        """The lock plane as an (Hi,Wi) uint8 array of 0 / 255 (a download), or None."""
        with self._lock:
            return None if self._lock_plane is None else self.backend.download(self._lock_plane)

    @property
    def locked(self):
        return self._lock_plane is not None

    def lock_rings(self, first_cap=4096):
        """The outline of the lock plane as rings (Selection.rings describes them), extracted on the device; []
        without a lock.  NotImplementedError from a backend that cannot extract outlines."""
        with self._lock:
            if self._lock_plane is None:
                return []
            return outline_rings(_outline_records(self.backend, self._lock_plane, int(first_cap)))

    # ---- the undo journal; the helpers below run with the session's lock held ---------------------------------
    def _journals(self, h, w):
        """whether a committed edit of an h x w window gets a journal entry"""
        return self.history > 0 and (self.history_bytes is None or window_saved_bytes(h, w) <= self.history_bytes)

    def _bytes_used(self):
        return sum(e[2] for e in self._undo) + sum(e[2] for e in self._redo)

    def _record(self, window, slot):
        """A paste into `window` was committed; `slot` holds the rectangle's bytes from before it (None: the edit was not
        journalled).  -> undoable"""
        self._redo.clear()
        if slot is None:
            self._undo.clear()                   # an older entry could no longer restore a state the frame was in
            return False
        self._push((tuple(window), slot, window_saved_bytes(window[2], window[3])))
        return True

    def _push(self, entry):
        self._undo.append(entry)
        while len(self._undo) > self.history or (self.history_bytes is not None and self._bytes_used() > self.history_bytes):
            self._undo.pop(0)

    def _record_regions(self, windows, slots):
        """`_record` for a region edit: ONE entry with all its windows and their slots (None: not journalled)"""
        self._redo.clear()
        if slots is None:
            self._undo.clear()
            return False
        self._push((_Regions(windows), list(slots), sum(window_saved_bytes(w[2], w[3]) for w in windows)))
        return True

    def _exchange_regions(self, src, dst):
        """the region entry `src` ends in <-> the frame, one swap call per window size (the journal's calls take rectangles of
        one size); -> what undo / redo return for it: lists in edit_regions' shape"""
        wins, slots, _ = src[-1]
        for hw, idx in _by_size(wins).items():
            self.backend.swap([self._frame] * len(idx), [wins[i][:2] for i in idx], hw, [slots[i] for i in idx])
        dst.append(src.pop())
        info = dict(windows=list(wins), undo_depth=len(self._undo), redo_depth=len(self._redo))
        return [self.backend.crop(self._frame, *w) for w in wins], [(w[1], w[0]) for w in wins], info

    def _record_sequence(self, windows, slots):
        """`_record` for a move: ONE entry with its rectangles in the order they were written and their slots (None: not
        journalled)"""
        self._redo.clear()
        if slots is None:
            self._undo.clear()
            return False
        self._push((_Sequence(windows), list(slots), sum(window_saved_bytes(w[2], w[3]) for w in windows)))
        return True

    def _exchange_sequence(self, src, dst, reverse):
        """the move's entry `src` ends in <-> the frame: one swap call per rectangle -- they may overlap -- in the
        order they were written (redo) or the REVERSE of it (undo: a later slot holds what the earlier steps left); -> what
        undo / redo return for it, in the region entries' shape"""
        wins, slots, _ = src[-1]
        order = range(len(wins) - 1, -1, -1) if reverse else range(len(wins))
        for i in order:
            self.backend.swap([self._frame], [wins[i][:2]], wins[i][2:], [slots[i]])
        dst.append(src.pop())
        info = dict(windows=list(wins), undo_depth=len(self._undo), redo_depth=len(self._redo))
        return [self.backend.crop(self._frame, *w) for w in wins], [(w[1], w[0]) for w in wins], info

    @staticmethod
    def _canvas_bytes(frame_hw, lock_plane):
        """the bytes a canvas entry holds: the frame's 3 H W and a lock plane's H W"""
        return (3 if lock_plane is None else 4) * frame_hw[0] * frame_hw[1]

    def _record_canvas(self, held):
        """`_record` for a canvas step: `held` = [frame, frame_hw, lock plane] of the state the step replaced.  An
        entry that does not fit `history_bytes` is not made, and then every older entry goes too: they name the old geometry"""
        self._redo.clear()
        nbytes = self._canvas_bytes(held[1], held[2])
        if self.history <= 0 or (self.history_bytes is not None and nbytes > self.history_bytes):
            self._undo.clear()
            return False
        self._push((_Canvas(held[1]), list(held), nbytes))
        return True

    def _exchange_canvas(self, src, dst):
        """the canvas entry `src` ends in <-> the session's frame, size and lock plane: a pointer exchange, no backend call; the
        entry moves to `dst` holding the state that was current; -> what undo / redo return for it"""
        _, slot, _ = src.pop()
        held = [self._frame, self.frame_hw, self._lock_plane]
        self._frame, self.frame_hw, self._lock_plane = slot
        dst.append((_Canvas(held[1]), held, self._canvas_bytes(held[1], held[2])))
        return None, (0, 0), dict(canvas=self.frame_hw, undo_depth=len(self._undo), redo_depth=len(self._redo))

    def _exchanged(self, src, dst):
        """the entry `src` ends in was exchanged with the frame: it moves to `dst`; -> what undo / redo return"""
        dst.append(src.pop())
        y0, x0, h, w = dst[-1][0]
        info = dict(window=dst[-1][0], undo_depth=len(self._undo), redo_depth=len(self._redo))
        return self.backend.crop(self._frame, y0, x0, h, w), (x0, y0), info

    def _exchange(self, src, dst, what):
        with self._lock:
            if not src:
                raise IndexError("nothing to " + what)
            if isinstance(src[-1][0], _Canvas):
                return self._exchange_canvas(src, dst)
            if isinstance(src[-1][0], _Sequence):
                return self._exchange_sequence(src, dst, src is self._undo)
            if isinstance(src[-1][0], _Regions):
                return self._exchange_regions(src, dst)
            (y0, x0, h, w), slot, _ = src[-1]
            self.backend.swap([self._frame], [(y0, x0)], (h, w), [slot])
            return self._exchanged(src, dst)

    def undo(self):
        """Takes the last edit back: the frame is byte-identical to what it was before it.  -> (patch, (x0, y0), info) in
        `edit`'s shape: the window after the exchange (the only download), info = dict(window, undo_depth, redo_depth).
        A region edit (edit_regions) is one step: all its windows are exchanged and the three are lists in ITS shape, with
        info = dict(windows, undo_depth, redo_depth).  A move (move_selection) is one step too and returns in that shape; its
        rectangles may overlap, so they are exchanged in the reverse of the order they were written, and by `redo` in that
        order.  A canvas step is one step: the frame, its size and the lock plane of that size come
        back by a pointer exchange, nothing is downloaded, and it returns (None, (0, 0), dict(canvas=(H, W), undo_depth,
        redo_depth)).  IndexError when there is nothing to undo."""
        return self._exchange(self._undo, self._redo, "undo")

    def redo(self):
        """Puts the last undone edit back, byte for byte.  Returns as `undo`; IndexError when there is nothing to redo."""
        return self._exchange(self._redo, self._undo, "redo")

    @property
    def can_undo(self):
        return bool(self._undo)

    @property
    def can_redo(self):
        return bool(self._redo)

    @property
    def history_bytes_used(self):
        """bytes of the journal slots held, undo and redo together"""
        with self._lock:
            return self._bytes_used()

    def _full_size(self, sketch):
        sk = _sketch_array(sketch)
        if sk.shape != self.frame_hw:
            raise ValueError("sketch is %dx%d, the frame %dx%d: a sketch of another size takes the whole-frame path "
                             "(serve.process_image)" % (sk.shape[1], sk.shape[0], self.frame_hw[1], self.frame_hw[0]))
        return sk

    def _request(self, sketch):
        """-> (sketch array, bbox) of a full-size sketch; refusals of the window path"""
        sk = self._full_size(sketch)
        bbox = sketch_bbox(sk)
        if bbox is None:
            raise ValueError("empty sketch: nothing to edit")
        return sk, bbox

    def _check_window(self, window, scaled=False):
        """`scaled`: the forward runs at a working size, so the window's own sides need not be multiples of 8"""
        y0, x0, h, w = (int(v) for v in window)
        Hi, Wi = self.frame_hw
        if h < 16 or w < 16 or (not scaled and (h % 8 or w % 8)) or y0 < 0 or x0 < 0 or y0 + h > Hi or x0 + w > Wi:
            raise ValueError("window %r: sides are multiples of 8, >= 16, and the window lies inside the %dx%d frame" % (window, Wi, Hi))
        return y0, x0, h, w

    def _grown(self, bbox, window, margin):
        """The next larger automatic window: the margin doubles until the window changes.  -> (window, margin), or None when
        the window already is the floored frame (it cannot grow)."""
        Hi, Wi = self.frame_hw
        if (window[2], window[3]) == (Hi // 8 * 8, Wi // 8 * 8):
            return None
        while True:
            margin *= 2
            nxt = choose_window(bbox, self.frame_hw, margin=margin)
            if nxt != window:
                return nxt, margin

    def edit(self, sketch, window=None, max_grow=2, low_latency=None, max_side=None, encode=None, feather=None):
        """One edit.  `sketch`: the FULL-SIZE sketch (PIL 'L' / 2-D uint8 array, the frame's size).  The window is
        choose_window of the sketch's box, or `window` = (y0, x0, h, w) as given (then it never grows).  The forward runs on
        the window without committing; if its mask reaches an edge of the window (border counts, a side on the frame's own
        edge counts 0) and the window can still grow, the margin doubles and the edit is rerun on the larger window, at most
        `max_grow` times; then the result is pasted.  -> (patch, (x0, y0), info): `patch` (h,w,3) uint8 = the frame's window
        after the paste (the only download), its position, and info = dict(window=(y0, x0, h, w), counts=[top, bottom, left,
        right], reruns=n, margin=m).
        `max_side` (None: everything above, at the frame's own resolution): the forward runs at
        choose_working_size(window, max_side) -- the window is resampled into it, the result and its mask are resampled
        back and pasted where the resampled mask is > 0 -- so an edit's cost is bounded by `max_side` whatever the
        sketch's extent.  The window is chosen and grown in frame space as before and the working size follows it; the
        counts are those of the working-size mask; a given `window` then needs no multiple-of-8 sides; info gains
        work=(H, W).  Still only the window's sketch goes up and only the window comes down.
        With history on, the window that is finally committed is journalled (one save in front of its paste) and info
        gains undoable.  With a lock plane (set_lock) info gains locked = True (a session without one reports what it
        always did: read it as info.get("locked", False)) -- every run of the edit, committed or not, at either scale, used
        the plane, and the grow loop saw a mask that is 0 on locked pixels.
        `encode` (None: everything above): "png" returns `patch` as the bytes of a PNG file of the same window,
        encoded on the device -- what comes down is the compressed stream, not the pixels; the frame, the journal and info
        are what they are without it.  "jpg" (quality 90) or ("jpg", Q), Q = 1 .. 100, returns it as a baseline JPEG file
        instead: a lossy preview several times smaller; the frame itself stays byte-exact.  ("jpg", Q, "420")
        stores chroma at half resolution and ("jpg", Q, "444" | "420", True) codes with four Huffman tables made for the patch
        (DESIGN.md 6l): smaller files for the same decoder.
        `feather` (None or 0: everything above): the radius r = 1 .. 16, in frame pixels, of a soft edge.  No
        run commits; the final window's result -- resized to the window when `max_side` is set -- enters the frame through
        the feathered paste: a selected pixel (mask > 0, not locked) takes c / n of the result and (n - c) / n of the frame,
        c = the selected pixels in the (2r + 1)^2 box around it, so exactly the pixels the hard paste writes change, the
        interior of the mask takes the result itself and its rim fades into the frame.  A policy without a quality claim,
        like `max_side`; info gains feather=r."""
        encode = _check_encode(encode)
        feather = _check_feather(feather)
        sk, bbox = self._request(sketch)
        margin = 0.5
        fixed = window is not None
        scaled = max_side is not None
        win = self._check_window(window, scaled) if fixed else choose_window(bbox, self.frame_hw, margin=margin)
        reruns = 0
        be = self.backend
        with self._lock:
            planes = None if self._lock_plane is None else [self._lock_plane]
            while True:
                y0, x0, h, w = win
                nxt = None if fixed or reruns >= max_grow else self._grown(bbox, win, margin)
                # a run whose counts cannot change anything commits at once: no round trip between forward and paste
                # (a feathered paste is a call of its own: no run commits)
                last = nxt is None
                commit = last and feather is None
                crop = be.upload(sk[y0:y0 + h, x0:x0 + w])
                slot = be.save([self._frame], [(y0, x0)], (h, w))[0] if commit and self._journals(h, w) else None
                work = choose_working_size((h, w), max_side) if scaled else None
                rgb, m8, counts = _run_windows(be, [self._frame], [(y0, x0)], [crop], (h, w), work, planes, commit, low_latency)
                if last or not any(counts[0]):
                    break
                win, margin = nxt
                reruns += 1
            if not commit and self._journals(h, w):
                slot = be.save([self._frame], [(y0, x0)], (h, w))[0]
            if feather is not None:
                be.paste_feather([self._frame], [(y0, x0)], planes, (h, w), feather, rgb, m8)
            elif not commit:
                _paste_windows(be, [self._frame], [(y0, x0)], (h, w), work, planes, rgb, m8)
            undoable = self._record(win, slot) if self.history > 0 else None
            patch = be.crop(self._frame, y0, x0, h, w) if encode is None else _encoded(be, encode, [self._frame], [(y0, x0, h, w)])[0]
        info = dict(window=win, counts=list(counts[0]), reruns=reruns, margin=margin)
        return patch, (x0, y0), _edit_info(info, planes is not None, work, undoable, feather)

    def edit_regions(self, sketch, low_latency=None, max_side=None, tile=32, margin=0.5, bucket=64, min_side=256, encode=None,
                     feather=None):
        """One edit of SEPARATE strokes through separate windows, so that two small strokes in opposite
        corners cost two small windows, not the frame.  `sketch` as in `edit`.  The full sketch goes up once; the library's
        tile pass (se_sketch_tiles_u8; `tile` in 16 / 32 / 64) finds where it is drawn and its grid comes down -- the one
        synchronisation before the forwards; split_regions(grid, tile, frame, margin, bucket, min_side) gives pairwise
        disjoint windows w_k.  The frame after the call is DEFINED as the frame after
            edit(sketch, window=w_k, max_grow=0, low_latency=..., max_side=...)   for every k, in any order,
        byte for byte, all in one pinned execution mode: each region's sketch is the full sketch cropped to its window (on
        the device), a neighbouring stroke's pixels inside it included.  The windows are grouped by size and each group is
        ONE committing call with B = the group's size on this frame (the locked entry with the session's plane for every
        request if there is one, else the scaled entry if `max_side` is set).  No window grows; the border counts are
        reported so that a caller can edit again.  One sketch blob gives the window `edit` starts from.
        -> (patches, origins, info): the windows after the paste (the downloads), their (x0, y0), and info = dict(windows,
        boxes, counts=[[top, bottom, left, right], ...], groups=the number of forwards), plus locked / work (one working
        size per window) / undoable where `edit` reports them.  An empty sketch or one of another size raises ValueError.
        With history on the call is ONE undo step: every window's rectangle is saved in front of its group's commit and the
        entry holds all slots; if they exceed `history_bytes` together the edit commits unjournalled and clears the history.
        `encode` as in `edit`: "png", "jpg" or ("jpg", Q) returns the patches as files, encoded on the device (one backend call
        for all).  `feather` as in `edit`: every group runs uncommitted and is pasted with ONE feathered paste,
        behind the group's saves; the definition above holds with feather=... in each edit."""
        encode = _check_encode(encode)
        feather = _check_feather(feather)
        sk = self._full_size(sketch)
        be = self.backend
        with self._lock:
            plane = be.upload(sk)
            regions = split_regions(be.tiles(plane, tile), tile, self.frame_hw, margin, bucket, min_side)
            if not regions:
                raise ValueError("empty sketch: nothing to edit")
            return self._edit_windows(regions, lambda wins: [be.window_of(plane, *w) for w in wins], low_latency, max_side, encode,
                                      feather)

    def _edit_windows(self, regions, crops_of, low_latency, max_side, encode=None, feather=None):
        """The committing part of edit_regions and edit_strokes, with the session's lock held: `regions` = [(box, window)],
        windows pairwise disjoint; crops_of(windows of one size) -> their sketches on the device.  Groups the windows by size;
        per group the crops, the journal's saves and ONE committing call -- with `feather` the uncommitted call, the saves
        and ONE feathered paste.  -> what the two return."""
        be = self.backend
        scaled = max_side is not None
        lk = self._lock_plane
        wins = [w for _, w in regions]
        journal = self.history > 0 and (self.history_bytes is None or
                                        sum(window_saved_bytes(w[2], w[3]) for w in wins) <= self.history_bytes)
        counts, slots, works = [None] * len(wins), [None] * len(wins), [None] * len(wins)
        groups = _by_size(wins)
        try:
            for (h, w), idx in groups.items():
                frames, origins = [self._frame] * len(idx), [wins[i][:2] for i in idx]
                crops = crops_of([wins[i] for i in idx])
                work = choose_working_size((h, w), max_side) if scaled else None
                planes = None if lk is None else [lk] * len(idx)
                if feather is not None:
                    rgb, m8, hits = _run_windows(be, frames, origins, crops, (h, w), work, planes, False, low_latency)
                if journal:
                    for i, slot in zip(idx, be.save(frames, origins, (h, w))):
                        slots[i] = slot
                if feather is not None:
                    be.paste_feather(frames, origins, planes, (h, w), feather, rgb, m8)
                else:
                    _, _, hits = _run_windows(be, frames, origins, crops, (h, w), work, planes, True, low_latency)
                for i, c in zip(idx, hits):
                    counts[i], works[i] = list(c), work
        except Exception:
            if any(c is not None for c in counts):    # some groups are in the frame: no entry restores a state it was in
                self._undo.clear()
                self._redo.clear()
            raise
        undoable = self._record_regions(wins, slots if journal else None) if self.history > 0 else None
        patches = [be.crop(self._frame, *w) for w in wins] if encode is None else _encoded(be, encode, [self._frame] * len(wins), wins)
        info = dict(windows=wins, boxes=[b for b, _ in regions], counts=counts, groups=len(groups))
        return patches, [(w[1], w[0]) for w in wins], _edit_info(info, lk is not None, works if scaled else None, undoable, feather)

    def edit_strokes(self, strokes, low_latency=None, max_side=None, margin=0.5, bucket=64, min_side=256, encode=None, feather=None):
        """One edit of strokes given as POLYLINES: `strokes` = [(points, width_px)] as stroke_segments takes
        them.  No full-size sketch exists anywhere: the host knows each stroke's box in closed form (stroke_box), merge_regions
        turns the boxes into pairwise disjoint windows exactly as edit_regions' are made, and the windows' sketches are
        rasterised on the device from the segments (se_sketch_strokes_u8, one call per window size) -- the segments are the
        only upload and the border counts the only download in front of the forwards.  A window's sketch holds every segment
        of the call that reaches into it, a neighbouring stroke's too.  The frame after the call is DEFINED as the frame after
            edit(S, window=w_k, max_grow=0, low_latency=..., max_side=...)   for every k, in any order,
        byte for byte in one pinned execution mode, S being the full-size 0 / 255 sketch the integer rule of 6i gives for
        the segments.  Everything else -- groups, lock, working size, history (ONE undo step), the return value -- is
        edit_regions', `encode` and `feather` too.  ValueError for no strokes or one stroke_segments refuses."""
        encode = _check_encode(encode)
        feather = _check_feather(feather)
        segs, ranges = stroke_segments(strokes, self.frame_hw)
        regions = merge_regions([stroke_box(segs[f:f + n], self.frame_hw) for f, n in ranges], self.frame_hw, margin, bucket, min_side)
        be = self.backend
        with self._lock:
            dsegs = be.upload(segs)
            return self._edit_windows(regions, lambda wins: be.strokes(dsegs, self.frame_hw, wins), low_latency, max_side, encode,
                                      feather)

    # ---- fills -----------------------------------------------------------------------------------------------
    def _fill_plane(self, mask):
        """a fill's `mask` -> the (Hi,Wi) uint8 array of 0 / 255 that is uploaded; the refusals of set_lock (an empty one is
        refused by `fill`, which scans it for its box anyway)"""
        if hasattr(mask, "mode"):
            if mask.mode != "L":
                raise ValueError("a fill mask is an 'L' image (got mode %r)" % mask.mode)
            mask = np.asarray(mask)
        mask = np.asarray(mask)
        if mask.dtype != np.uint8 and mask.dtype != np.bool_:
            raise TypeError("a fill mask is a uint8 or bool array (got %s)" % mask.dtype)
        if mask.shape != self.frame_hw:
            raise ValueError("a fill mask is the frame's (%d,%d) plane (got %r)" % (self.frame_hw + (mask.shape,)))
        return np.where(mask != 0, np.uint8(255), np.uint8(0))

    def _fill_window(self, box, window, margin, max_side):
        """the window of a fill: `window` as given (checked), or choose_window of `box`, the box of painted region and sketch"""
        if window is not None:
            return self._check_window(window, max_side is not None)
        return choose_window(box, self.frame_hw, margin=margin)

    def _fill_steps(self, fill_plane, crop, win, low_latency, max_side, feather, journal, blend=None):
        """The steps of a fill that change the frame, with the session's lock held: keep plane, the forward, the journal's save
        when `journal`, ONE paste; no download in between.  The caller owns the journal entry.
        `blend`: None, or _blend_box's result -- then the forward hands out the generator's own prediction, its
        lift is made, and behind the same save the membrane's drop at offset 0 replaces keep plane and paste.
        -> (slot or None, work, planes)"""
        be = self.backend
        y0, x0, h, w = win
        frames, origins = [self._frame], [(y0, x0)]
        planes = None if self._lock_plane is None else [self._lock_plane]
        work = choose_working_size((h, w), max_side) if max_side is not None else None
        if blend is not None:
            rgb, _ = be.run_fill(frames, origins, [crop], [fill_plane], planes, (h, w), work, low_latency, raw=True)
            lift = be.fill_lift(rgb, (h, w))
            slot = be.save(frames, origins, (h, w))[0] if journal else None
            if blend:
                be.move_blend(self._frame, lift, win, fill_plane, self._lock_plane, blend, (0, 0), MOVE_FLIPS[None])
            return slot, work, planes
        keep = be.fill_keep(frames, origins, [fill_plane], planes, (h, w))
        rgb, m8 = be.run_fill(frames, origins, [crop], [fill_plane], planes, (h, w), work, low_latency)
        slot = be.save(frames, origins, (h, w))[0] if journal else None
        if feather is not None:
            be.paste_feather(frames, origins, keep, (h, w), feather, rgb, m8)
        else:
            be.paste_locked(frames, origins, keep, (h, w), rgb, m8)
        return slot, work, planes

    def _fill(self, fill_plane, crop, win, low_latency, max_side, encode, feather, blend=None):
        """The device part of fill and fill_strokes, with the session's lock held: `fill_plane` the frame-sized plane and `crop`
        the window's sketch (or None), both on the device.  Keep plane, the forward, the journal's save, ONE paste, the
        patch: no download in between.  `blend`: None, or _blend_box of the region's box for a seamless paste (_fill_steps)."""
        be = self.backend
        y0, x0, h, w = win
        frames = [self._frame]
        if blend is None:
            slot, work, planes = self._fill_steps(fill_plane, crop, win, low_latency, max_side, feather, self._journals(h, w))
        else:
            slot, work, planes = self._fill_steps(fill_plane, crop, win, low_latency, max_side, feather, self._journals(h, w), blend)
        undoable = self._record(win, slot) if self.history > 0 else None
        patch = be.crop(self._frame, y0, x0, h, w) if encode is None else _encoded(be, encode, frames, [win])[0]
        info = _edit_info(dict(window=win, fill=True), planes is not None, work, undoable, feather)
        if blend is not None:
            info["blend"] = "seamless"
        return patch, (x0, y0), info

    def fill(self, mask, sketch=None, window=None, margin=0.5, low_latency=None, max_side=None, encode=None, feather=None, blend=None):
        """One fill: "paint over this, fill it in".  `mask`: (Hi,Wi), a uint8 or bool array or a PIL 'L' image,
        non-zero = fill; uploaded once per call as 0 / 255.  `sketch`: an optional FULL-SIZE sketch that guides the fill, used
        as given (not masked by the hole).  netG alone runs, on the hole mask & ~lock: there is no mask predictor, no
        threshold and no grow loop.  The window is choose_window of the box of mask and sketch together at `margin`, or
        `window` = (y0, x0, h, w) as given.  The result enters the frame where the mask is painted and the lock plane
        (set_lock) is 0, both tested in frame space: at any scale only painted, unlocked pixels can change.
        `max_side`, `encode` and `feather` as in `edit`; with history on the call is ONE undo step.
        -> (patch, (x0, y0), info) in `edit`'s shape, info = dict(window, fill=True) plus work / undoable / locked / feather
        where `edit` reports them.  ValueError for an all-zero mask, a mask or sketch of another size, a bad window.
        `blend` = "seamless" (None: everything above): the fill keeps its detail and takes the local colour of the
        frame at its rim.  The forward hands out P, the generator's OWN prediction over the whole window (at a working size:
        its BICUBIC resize to the window), and the new frame is the membrane's drop of include/sketchedit_blend.h with the lift
        P held by the window, offset 0, no flip, the plane `mask`, the lock plane and the box of `mask` cut to the window:
        F' = P + m on the targets, m smooth and equal to F - P on their rim.  The targets are mask != 0 and lock == 0 inside
        the window, tested in frame space -- unscaled exactly the hard paste's; with `max_side` the hard paste's extra clause
        "the upsampled hole mask > 0" is NOT applied.  The rim is the frame's pixels next to a target that the window holds (a
        locked neighbour included); the window's and the frame's edges are left out of the sums.  Same save, same undo step,
        info gains blend="seamless".  ValueError, before the first backend call: a blend that is neither, blend with feather,
        a box inside the window with a side above 2048; NotImplementedError: a backend without move_blend / fill_lift."""
        encode = _check_encode(encode)
        feather = _check_feather(feather)
        seamless = _check_blend(blend, feather, self.backend)
        plane = self._fill_plane(mask)
        sk = None if sketch is None else self._full_size(sketch)
        box = sketch_bbox(plane)
        if box is None:
            raise ValueError("empty mask: nothing to fill")
        by0, bx0, by1, bx1 = box
        sb = None if sk is None else sketch_bbox(sk)
        if sb is not None:
            by0, bx0, by1, bx1 = min(by0, sb[0]), min(bx0, sb[1]), max(by1, sb[2]), max(bx1, sb[3])
        win = self._fill_window((by0, bx0, by1, bx1), window, margin, max_side)
        y0, x0, h, w = win
        cut = _blend_box(box, win) if seamless else None
        be = self.backend
        with self._lock:
            return self._fill(be.upload(plane), None if sk is None else be.upload(sk[y0:y0 + h, x0:x0 + w]), win, low_latency, max_side,
                              encode, feather, cut)

    def fill_strokes(self, strokes, sketch_strokes=None, window=None, margin=0.5, low_latency=None, max_side=None, encode=None,
                     feather=None, blend=None):
        """`fill` with the painted region given as POLYLINES with a brush width: `strokes` (and the optional
        `sketch_strokes` that guide the fill) = [(points, width_px)] as stroke_segments takes them.  Each set is rasterised on
        the device into a frame-sized plane (se_sketch_strokes_u8 with the whole frame as its one window) -- nothing but the
        segments is uploaded -- and the call proceeds as `fill` of those planes; the box is stroke_box of all segments.
        ValueError for no strokes or one stroke_segments refuses.  `blend` as in `fill`, its box stroke_box of
        `strokes` (the plane is made on the device: the box is the segments' bound, not a scan of the plane)."""
        encode = _check_encode(encode)
        feather = _check_feather(feather)
        seamless = _check_blend(blend, feather, self.backend)
        Hi, Wi = self.frame_hw
        segs, _ = stroke_segments(strokes, self.frame_hw)
        sk_segs = None if sketch_strokes is None else stroke_segments(sketch_strokes, self.frame_hw)[0]
        win = self._fill_window(stroke_box(segs if sk_segs is None else np.concatenate([segs, sk_segs]), self.frame_hw), window, margin,
                                max_side)
        cut = _blend_box(stroke_box(segs, self.frame_hw), win) if seamless else None
        be = self.backend
        with self._lock:
            plane = be.strokes(be.upload(segs), self.frame_hw, [(0, 0, Hi, Wi)])[0]
            sk = None if sk_segs is None else be.strokes(be.upload(sk_segs), self.frame_hw, [(0, 0, Hi, Wi)])[0]
            return self._fill(plane, None if sk is None else be.window_of(sk, *win), win, low_latency, max_side, encode, feather, cut)

    # ---- selection by colour ------------------------------------------------------------------------------------
    def _check_select(self, seed, tolerance, grow):
        """-> (seed, tolerance, grow) as ints; the refusals of a selection, all in front of the first backend call"""
        def integer(v):
            return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))
        try:
            sy, sx = seed
        except (TypeError, ValueError):
            raise ValueError("seed is (y, x), a pixel of the frame (got %r)" % (seed,))
        Hi, Wi = self.frame_hw
        if not (integer(sy) and integer(sx)) or not (0 <= sy < Hi and 0 <= sx < Wi):
            raise ValueError("seed is (y, x), two ints inside the %dx%d frame (got %r)" % (Wi, Hi, seed))
        if not integer(tolerance) or not 0 <= tolerance <= 255:
            raise ValueError("tolerance is an int 0 .. 255, the largest difference in any channel (got %r)" % (tolerance,))
        return (int(sy), int(sx)), int(tolerance), self._check_grow(grow)

    def _check_fill_args(self, box, sketch, window, margin, max_side):
        """what a fill of a selection refuses before its first backend call: a sketch of another size, a bad window or margin
        (tried on `box`), a bad max_side.  -> the sketch as an array, or None"""
        sk = None if sketch is None else self._full_size(sketch)
        self._fill_window(box, window, margin, max_side)
        if max_side is not None:
            choose_working_size((16, 16), max_side)
        return sk

    def _select(self, seed, tolerance, contiguous, grow):
        """with the session's lock held: ONE backend call"""
        plane, box, count = self.backend.select_similar(self._frame, seed, tolerance, bool(contiguous), grow)
        return Selection(self.backend, plane, box, count, self.frame_hw)

    def _fill_selected(self, selection, sk, window, margin, low_latency, max_side, encode, feather, seamless=False):
        """with the session's lock held: `_fill` of the selection's plane through the window of its box united with the
        sketch's; `seamless`: pasted through the membrane with the selection's box cut to the window"""
        by0, bx0, by1, bx1 = selection.box
        sb = None if sk is None else sketch_bbox(sk)
        if sb is not None:
            by0, bx0, by1, bx1 = min(by0, sb[0]), min(bx0, sb[1]), max(by1, sb[2]), max(bx1, sb[3])
        win = self._fill_window((by0, bx0, by1, bx1), window, margin, max_side)
        y0, x0, h, w = win
        cut = _blend_box(selection.box, win) if seamless else None
        crop = None if sk is None else self.backend.upload(sk[y0:y0 + h, x0:x0 + w])
        patch, pos, info = self._fill(selection.plane, crop, win, low_latency, max_side, encode, feather, cut)
        info["selected"] = selection.count
        return patch, pos, info

    def select_similar(self, seed, tolerance=16, contiguous=True, grow=0):
        """"Click on it" (DESIGN.md 6o): the pixels whose colour is within `tolerance` (0 .. 255) of the pixel at `seed` =
        (y, x) in every channel -- with `contiguous` only those 4-connected to the seed through such pixels (diagonals do not
        connect) -- and every pixel within `grow` (0 .. 16) pixels of one, to cover an object's soft edge.  Made on the
        device from the resident frame: nothing frame-sized moves; what comes down are the flood's pass flags and the tile
        records the box is made of.  The lock plane plays no part: a fill of the selection respects it as every fill does.
        -> Selection (.box, .count, .plane, .mask()).  Not an edit: nothing is journalled.  ValueError for a seed outside the
        frame or not two ints, a tolerance or grow outside its range."""
        seed, tolerance, grow = self._check_select(seed, tolerance, grow)
        with self._lock:
            return self._select(seed, tolerance, contiguous, grow)

    def fill_selection(self, selection, sketch=None, window=None, margin=0.5, low_latency=None, max_side=None, encode=None, feather=None,
                       blend=None):
        """`fill` of a Selection: its plane is on the device already, so only the optional sketch's window goes
        up.  The window is choose_window of the selection's box united with the sketch's at `margin`, or `window` as given;
        everything else -- netG alone on selection & ~lock, the paste in frame space, `max_side`, `encode`, `feather`, ONE undo
        step -- is `fill`'s.  -> what `fill` returns, with info["fill"] = True and info["selected"] = the selection's pixels.
        ValueError for a selection made on a frame of another size and for what `fill` refuses.  `blend` as in `fill`
        (DESIGN.md 6z), its box the selection's."""
        encode = _check_encode(encode)
        feather = _check_feather(feather)
        seamless = _check_blend(blend, feather, self.backend)
        self._check_selection(selection, "fill_selection")
        if selection.box is None:
            raise ValueError("empty selection: nothing to fill")
        sk = self._check_fill_args(selection.box, sketch, window, margin, max_side)
        with self._lock:
            return self._fill_selected(selection, sk, window, margin, low_latency, max_side, encode, feather, seamless)

    def fill_similar(self, seed, tolerance=16, contiguous=True, grow=2, sketch=None, window=None, margin=0.5, low_latency=None,
                     max_side=None, encode=None, feather=None, blend=None):
        """select_similar(seed, tolerance, contiguous, grow) and fill_selection of the result under ONE hold of the session's
        lock: "click on it, fill it in".  Nothing frame-sized crosses the bus in either direction.
        -> what fill_selection returns; ONE undo step.  Every ValueError comes before the first backend call -- but, with
        `blend` (as in `fill`), that of a box side above 2048: the box exists only once the selection is made, and
        the refusal comes behind it and in front of every call that changes the frame."""
        encode = _check_encode(encode)
        feather = _check_feather(feather)
        seamless = _check_blend(blend, feather, self.backend)
        seed, tolerance, grow = self._check_select(seed, tolerance, grow)
        sk = self._check_fill_args((seed[0], seed[1], seed[0] + 1, seed[1] + 1), sketch, window, margin, max_side)
        with self._lock:
            return self._fill_selected(self._select(seed, tolerance, contiguous, grow), sk, window, margin, low_latency, max_side,
                                       encode, feather, seamless)

    # ---- lasso selections and the algebra of selections -----------------------------------------------------------
    def _check_selection(self, selection, what):
        """a Selection made on a frame of this size, or TypeError / ValueError; no backend call"""
        if not isinstance(selection, Selection):
            raise TypeError("%s takes a Selection, what select_similar / select_lasso / combine returned (got %s)"
                            % (what, type(selection).__name__))
        if tuple(selection.frame_hw) != self.frame_hw:
            raise ValueError("the selection was made on a %dx%d frame, this one is %dx%d"
                             % (selection.frame_hw[1], selection.frame_hw[0], self.frame_hw[1], self.frame_hw[0]))

    @staticmethod
    def _check_grow(grow):
        if not isinstance(grow, (int, np.integer)) or isinstance(grow, (bool, np.bool_)) or not 0 <= grow <= SELECT_MAX_GROW:
            raise ValueError("grow is an int 0 .. %d, in frame pixels (got %r)" % (SELECT_MAX_GROW, grow))
        return int(grow)

    def _select_lasso(self, edges, grow):
        """with the session's lock held: the edges go up, ONE backend call makes the selection"""
        be = self.backend
        plane, box, count = be.select_lasso(be.upload(edges), self.frame_hw, grow)
        return Selection(be, plane, box, count, self.frame_hw)

    def select_lasso(self, rings, grow=0):
        """"Draw an outline around it" (DESIGN.md 6p): the pixels whose centres lie inside the closed outlines `rings` = [[(x, y),
        ...], ...] (floats in frame pixels, at least 3 points each, as lasso_edges takes them) by the even-odd rule -- a ring
        inside a ring is a hole, and so is the middle of a self-crossing outline -- and every pixel within `grow` (0 .. 16)
        pixels of one.  Rasterised on the device: only the edges go up, and the tile records of the result come down.
        -> Selection; EMPTY (.box None, .count 0) when the outline covers no pixel centre.  Not an edit: nothing is journalled;
        the frame and the lock play no part.  ValueError for what lasso_edges refuses and a grow outside its range.
        `selection.rings()` is a valid argument: integer points are exact under floor(4 v + 0.5) and no pixel
        centre lies on an edge between pixel corners, so the plane, box and count of that selection come back bit for bit --
        within the limit of 65 536 edges, which stays as it is (one edge per ring point)."""
        edges = lasso_edges(rings, self.frame_hw)
        grow = self._check_grow(grow)
        with self._lock:
            return self._select_lasso(edges, grow)

    def combine(self, a, b, op):
        """Two selections of this frame -> a NEW one, made on the device: `op` "add" (a or b), "subtract" (a and
        not b), "intersect" (a and b) or "xor".  a and b stay what they were; the result may be empty.  TypeError for an
        operand that is not a Selection, ValueError for one made on a frame of another size and for an unknown op, all before
        the one backend call."""
        self._check_selection(a, "combine")
        self._check_selection(b, "combine")
        if not isinstance(op, str) or op not in COMBINE_OPS:
            raise ValueError("op is one of %s (got %r)" % (", ".join(repr(k) for k in COMBINE_OPS), op))
        with self._lock:
            plane, box, count = self.backend.combine(a.plane, b.plane, COMBINE_OPS[op])
        return Selection(self.backend, plane, box, count, self.frame_hw)

    def invert(self, a):
        """Everything but `a`: a NEW selection, made on the device; `a` stays what it was."""
        self._check_selection(a, "invert")
        with self._lock:
            plane, box, count = self.backend.combine(a.plane, None, COMBINE_INVERT)
        return Selection(self.backend, plane, box, count, self.frame_hw)

    # ---- modify a selection's shape -----------------------------------------------------------------------------------
    def modify_selection(self, selection, kind, radius, side="both"):
        """"Select > Modify" (DESIGN.md 6w): a selection of this frame -> a NEW one whose shape is changed by a round brush of
        `radius` (an int 1 .. 32, in frame pixels), made on the device.  `kind`:
          "expand"    every pixel within `radius` (Euclidean) of a selected one;
          "contract"  the selected pixels with no unselected pixel of the frame within `radius`: a selection that touches the
                      frame's edge does not shrink away from it;
          "border"    a rim of the selection: `side` "inside" (the selection minus its contraction), "outside" (its expansion
                      minus the selection) or "both" (the expansion minus the contraction);
          "smooth"    the majority vote in the disc: specks and pinholes smaller than half a disc go, corners are rounded.
        `side` belongs to "border" alone.  One hold of the session's lock; one backend call, or for a border one or two
        modifications and one subtraction, of which only the last one's tile records come down.  The operand stays what it was;
        the result may be empty.  Not an edit: nothing is journalled; the frame and the lock play no part.
        An empty operand gives the empty selection with no backend call (the result shares the operand's all-zero plane).
        TypeError for an operand that is not a Selection; ValueError for one made on a frame of another size, an unknown kind
        or side, a side with another kind than "border", a radius that is not an int 1 .. 32; NotImplementedError from a backend
        that cannot modify selections -- all before the first backend call."""
        self._check_selection(selection, "modify_selection")
        if not isinstance(kind, str) or kind not in MODIFY_KINDS:
            raise ValueError("kind is one of %s (got %r)" % (", ".join(repr(k) for k in MODIFY_KINDS), kind))
        if not isinstance(side, str) or side not in MODIFY_SIDES:
            raise ValueError("side is one of %s (got %r)" % (", ".join(repr(k) for k in MODIFY_SIDES), side))
        if kind != "border" and side != "both":
            raise ValueError("side belongs to kind 'border' alone (got side=%r with kind=%r)" % (side, kind))
        if not isinstance(radius, (int, np.integer)) or isinstance(radius, (bool, np.bool_)) or not 1 <= radius <= MODIFY_MAX_RADIUS:
            raise ValueError("radius is an int 1 .. %d, in frame pixels (got %r)" % (MODIFY_MAX_RADIUS, radius))
        radius = int(radius)
        be = self.backend
        if not hasattr(be, "modify"):
            raise NotImplementedError("this session's backend (%s) cannot modify selections: it has no `modify`" % type(be).__name__)
        if selection.box is None:
            return Selection(be, selection.plane, None, 0, self.frame_hw)
        with self._lock:
            if kind != "border":
                plane, box, count = be.modify(selection.plane, MODIFY_OPS[kind], radius)
            else:
                outer = selection.plane if side == "inside" else be.modify(selection.plane, MODIFY_OPS["expand"], radius, tiles=False)[0]
                inner = selection.plane if side == "outside" else be.modify(selection.plane, MODIFY_OPS["contract"], radius, tiles=False)[0]
                plane, box, count = be.combine(outer, inner, COMBINE_OPS["subtract"])
        return Selection(be, plane, box, count, self.frame_hw)

    def fill_lasso(self, rings, grow=2, sketch=None, window=None, margin=0.5, low_latency=None, max_side=None, encode=None,
                   feather=None, blend=None):
        """select_lasso(rings, grow) and fill_selection of the result under ONE hold of the session's lock: "draw
        around it, fill it in".  Only the edges go up; nothing frame-sized crosses the bus in either direction.
        -> what fill_selection returns; ONE undo step.  Every ValueError comes before the first backend call (the window
        arguments are tried on lasso_box of the edges) but one: "the lasso covers no pixel centre" may be known only after
        the selection was made -- a sliver between two columns of centres has a box and no pixel; nothing was changed then.
        `blend` as in `fill`, its box the selection's; as in fill_similar the refusal of a box side above 2048
        comes behind the selection and in front of every call that changes the frame."""
        encode = _check_encode(encode)
        feather = _check_feather(feather)
        seamless = _check_blend(blend, feather, self.backend)
        edges = lasso_edges(rings, self.frame_hw)
        grow = self._check_grow(grow)
        box = lasso_box(edges, self.frame_hw)
        if box is None:
            raise ValueError("the lasso covers no pixel centre")
        sk = self._check_fill_args(box, sketch, window, margin, max_side)
        with self._lock:
            selection = self._select_lasso(edges, grow)
            if selection.box is None:
                raise ValueError("the lasso covers no pixel centre")
            return self._fill_selected(selection, sk, window, margin, low_latency, max_side, encode, feather, seamless)

    # ---- what the operators on a lifted selection share (DESIGN.md 6r .. 6u) -----------------------------------------------------------
    def _lift_fill_drop(self, selection, dst, window, margin, low_latency, max_side, encode, feather, keep_source, hole_grow, drop, remap,
                        info, drop_feathers, lift_grow=0):
        """move_selection and transform_selection once their own arguments are checked: the lift, the fill of the hole -- the
        selection grown by `hole_grow` -- unless `keep_source`, `drop(lift, lift_rect)` into the rectangle `dst`, and `remap()` ->
        (plane, box, count) of the new Selection; ONE ordered undo step.  `info`: the caller's own keys.  `drop_feathers`: the
        drop takes `feather` itself, so info reports it even where no fill ran.  `lift_grow`: the lift holds the box grown by
        that many pixels and clipped to the frame (the seamless drop reads the object's rim)."""
        Hi, Wi = self.frame_hw
        box = selection.box
        grown = (max(box[0] - hole_grow, 0), max(box[1] - hole_grow, 0), min(box[2] + hole_grow, Hi), min(box[3] + hole_grow, Wi))
        self._check_fill_args(grown, None, window, margin, max_side)
        win = None if keep_source else self._fill_window(grown, window, margin, max_side)
        wins = ([] if win is None else [win]) + [dst]
        journal = self.history > 0 and (self.history_bytes is None or
                                        sum(window_saved_bytes(w[2], w[3]) for w in wins) <= self.history_bytes)
        be = self.backend
        with self._lock:
            frames = [self._frame]
            lift_box = (max(box[0] - lift_grow, 0), max(box[1] - lift_grow, 0), min(box[2] + lift_grow, Hi), min(box[3] + lift_grow, Wi))
            lift_rect = move_rect(lift_box, (0, 0), self.frame_hw)
            lift = be.save(frames, [lift_rect[:2]], lift_rect[2:])[0]
            slots, work, pasted = [], None, False
            try:
                if win is not None:
                    hole = selection.plane if hole_grow == 0 else be.grow(selection.plane, hole_grow)
                    slot, work, _ = self._fill_steps(hole, None, win, low_latency, max_side, feather, journal)
                    slots.append(slot)
                    pasted = True
                if journal:
                    slots.append(be.save(frames, [dst[:2]], dst[2:])[0])
                drop(lift, lift_rect)
                pasted = True
                plane, nbox, count = remap()
            except Exception:
                if pasted:                       # the fill or the drop is in the frame: no entry restores a state it was in
                    self._undo.clear()
                    self._redo.clear()
                raise
            # the new selection exists before the step is recorded: a caller who gets an entry gets the selection too
            undoable = self._record_sequence(wins, slots if journal else None) if self.history > 0 else None
            made = Selection(be, plane, nbox, count, self.frame_hw)
            patches = [be.crop(self._frame, *w) for w in wins] if encode is None else _encoded(be, encode, frames * len(wins), wins)
            locked = self._lock_plane is not None
        info = dict(windows=wins, **info, selected=selection.count, selection=made)
        return patches, [(w[1], w[0]) for w in wins], _edit_info(info, locked, work, undoable, feather if drop_feathers or win is not None else None)

    def _lift_apply(self, selection, lift_rect, wins, apply, encode, info, feather, prepare=None):
        """filter_selection and adjust_selection once their arguments are checked: the lift of `lift_rect`, `apply(lift, *extra)` --
        ONE launch into the frame -- and the lift as the journal entry's slot.  `extra` = `prepare()`, backend calls that write
        nothing into the frame: they run after the lift and in front of the `try`, so a failure there leaves the history alone.
        `info`: the caller's own keys."""
        journal = self._journals(lift_rect[2], lift_rect[3])
        be = self.backend
        with self._lock:
            frames = [self._frame]
            lift = be.save(frames, [lift_rect[:2]], lift_rect[2:])[0]
            extra = prepare() if prepare is not None else ()
            try:
                apply(lift, *extra)
                undoable = self._record(lift_rect, lift if journal else None) if self.history > 0 else None
                patches = [be.crop(self._frame, *w) for w in wins] if encode is None else _encoded(be, encode, frames, wins)
            except Exception:                    # the launch may be in the frame: no entry restores a state it was in
                self._undo.clear()
                self._redo.clear()
                raise
            locked = self._lock_plane is not None
        info = dict(windows=wins, **info, selected=selection.count)
        return patches, [(w[1], w[0]) for w in wins], _edit_info(info, locked, None, undoable, feather)

    # ---- move or clone a selection ------------------------------------------------------------------------------------
    def move_selection(self, selection, offset, flip=None, keep_source=False, hole_grow=2, window=None, margin=0.5, low_latency=None,
                       max_side=None, encode=None, feather=None, blend=None):
        """"Drag this over there and mend the place it came from" (DESIGN.md 6r): the selected pixels land `offset` = (dy, dx) away
        -- two ints, each at most 16 384 in magnitude -- mirrored about the selection's box by `flip` (None, "h", "v" or "hv"),
        and the place they came from is filled.  Everything happens on the device under ONE hold of the session's lock:
          1. the LIFT: the rectangle move_rect(box, (0, 0)) of the frame is saved into a scratch slot (not a journal entry), so the
             object's pixels are the ORIGINAL ones whatever the next step does, and source and destination may overlap freely;
          2. unless `keep_source`, the HOLE -- the selection grown by `hole_grow` (0 .. 16) pixels, to cover the object's soft edge
             -- is filled exactly as fill_selection fills a selection: netG alone through choose_window of the grown box at
             `margin`, or `window` as given, with `max_side`, the lock plane and `feather` as there;
          3. the DROP: the lifted pixels are written at the destination, always at frame scale and always exact, whatever
             `max_side` is: a plain copy, or with `feather` = r the blend of the feathered paste, c / n of the object and
             (n - c) / n of the frame, c counted on the moved selection alone (an object pushed partly over the frame's edge
             does not fade towards the edge);
          4. the moved SELECTION is made: the selection's plane shifted the same way, with its box and count -- the call's one
             extra download.  What leaves the frame is dropped; the selection that was passed in stays what it was.
        Locked source pixels are not filled; they are still copied.  Locked destination pixels never change.
        -> (patches, positions, info) in edit_regions' shape over [fill window, destination rectangle] (the destination
        rectangle, move_rect(box, offset), alone with `keep_source`); `encode` applies to each patch.  info = dict(windows,
        move=True, offset, flip, selected, selection=the moved Selection) plus work / undoable / locked / feather where `fill`
        reports them.  With history on the call is ONE undo step: each rectangle is saved in front of its own step and the entry
        holds both slots, exchanged in reverse order by `undo` and in forward order by `redo`, since the two may overlap; if
        the slots exceed `history_bytes` together the move commits unjournalled and clears the history.  A backend call that
        fails once the frame was written clears the history too: no entry could restore a state the frame was in.
        clone_selection(...) is move_selection(..., keep_source=True).
        `blend` = "seamless"  makes step 3 a gradient-domain drop: the object keeps its own detail and takes the local
        colour of the place it lands in -- the lifted pixels plus a smooth membrane that equals frame - lift on the object's
        rim, made by a fixed schedule of integer steps (include/sketchedit_blend.h): the same bytes on every machine, and no claim
        of closeness to the harmonic solution beyond DESIGN.md's measured figures.  The lift is then of the box grown by one
        pixel (the rim's sources; only the frame's edge leaves a side of the object without a rim), `feather` goes to the fill of
        the hole only, info["blend"] = "seamless"; the journal, the lock, `keep_source` and the moved selection are as above.
        A side of the selection's box is at most 2048 pixels.
        TypeError / ValueError, all before the first backend call: a selection that is none, of another frame size or empty, an
        offset that is not two ints or is above the limit, one that moves the whole selection out of the frame, a bad flip,
        hole_grow, window, max_side, encode, feather or blend, a box too large for the blend.  NotImplementedError, before it
        too: `blend` on a backend without move_blend."""
        encode = _check_encode(encode)
        feather = _check_feather(feather)
        self._check_selection(selection, "move_selection")
        if selection.box is None:
            raise ValueError("empty selection: nothing to move")
        try:
            dy, dx = offset
        except (TypeError, ValueError):
            raise ValueError("offset is (dy, dx), two ints (got %r)" % (offset,))
        if not all(isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) and abs(int(v)) <= MOVE_MAX_OFFSET for v in (dy, dx)):
            raise ValueError("offset is (dy, dx), two ints of at most %d in magnitude (got %r)" % (MOVE_MAX_OFFSET, offset))
        offset = (int(dy), int(dx))
        if not (flip is None or isinstance(flip, str)) or flip not in MOVE_FLIPS:
            raise ValueError("flip is None, 'h', 'v' or 'hv' (got %r)" % (flip,))
        hole_grow = _check_hole_grow(hole_grow)
        if not (blend is None or isinstance(blend, str)) or blend not in MOVE_BLENDS:
            raise ValueError("blend is None or 'seamless' (got %r)" % (blend,))
        box, flips = selection.box, MOVE_FLIPS[flip]
        dst = move_rect(box, offset, self.frame_hw)
        if dst is None:
            raise ValueError("offset %r moves the whole selection out of the frame" % (offset,))
        be = self.backend
        if blend is not None:
            if max(box[2] - box[0], box[3] - box[1]) > BLEND_MAX_SIDE:
                raise ValueError("blend=%r takes a selection whose box has sides of at most %d (got %r)" % (blend, BLEND_MAX_SIDE, box))
            if not callable(getattr(be, "move_blend", None)):
                raise NotImplementedError("this backend has no move_blend: blend=%r needs the seamless drop (DESIGN.md 6x)" % (blend,))
            return self._lift_fill_drop(
                selection, dst, window, margin, low_latency, max_side, encode, feather, keep_source, hole_grow,
                lambda lift, lift_rect: be.move_blend(self._frame, lift, lift_rect, selection.plane, self._lock_plane, box, offset, flips),
                lambda: be.shift(selection.plane, box, offset, flips), dict(move=True, offset=offset, flip=flip, blend=blend), False, lift_grow=1)
        return self._lift_fill_drop(
            selection, dst, window, margin, low_latency, max_side, encode, feather, keep_source, hole_grow,
            lambda lift, lift_rect: be.move_drop(self._frame, lift, lift_rect, selection.plane, self._lock_plane, box, offset, flips, feather or 0),
            lambda: be.shift(selection.plane, box, offset, flips), dict(move=True, offset=offset, flip=flip), True)

    def clone_selection(self, selection, offset, **kw):
        """move_selection(selection, offset, keep_source=True, ...): a copy of the selected pixels lands `offset`
        away and the source stays what it is -- no forward runs; ONE undo step over the destination rectangle."""
        kw["keep_source"] = True
        return self.move_selection(selection, offset, **kw)

    # ---- scale and rotate a selection -----------------------------------------------------------------------------------
    def transform_selection(self, selection, scale=1.0, angle=0.0, offset=(0, 0), flip=None, matrix=None, keep_source=False, hole_grow=2,
                            window=None, margin=0.5, low_latency=None, max_side=None, encode=None, feather=None):
        """"Make this bigger, turn it, and mend the place it came from" (DESIGN.md 6s): move_selection with a drop that resamples.
        The selected pixels are turned by `angle` degrees (counter-clockwise on the screen) about the centre of the selection's
        box, scaled by `scale` (a number or a (sy, sx) pair, each in 1/8 .. 8), mirrored by `flip` and their centre put `offset` =
        (dy, dx) away (ints or floats, quantised to half pixels): the map is warp_matrix(selection.box, scale, angle, offset,
        flip).  `matrix` = six ints gives the inverse map in Q16 itself and excludes scale, angle, offset and flip.  Everything
        happens on the device under ONE hold of the session's lock, in move_selection's steps:
          1. the LIFT of move_rect(box, (0, 0)) into a scratch slot;
          2. unless `keep_source`, the fill of the HOLE, the selection grown by `hole_grow` (0 .. 16), exactly as fill_selection
             fills (`window`, `margin`, `max_side`, the lock plane); `feather` applies to this fill only -- the drop's soft edge
             is the interpolation's;
          3. the DROP: ONE launch at frame scale whatever `max_side` is, bilinear taps of the lifted pixels blended by their
             coverage (include/sketchedit_warp.h) into warp_rect(box, m): integers only, the same bytes on every machine.  Below a
             scale of 1/2 the taps undersample; there is no prefilter and no claim of quality;
          4. the warped SELECTION: the plane through the same map, selected where the coverage is at least a half, with its box
             and count -- the call's one extra download.
        Locked source pixels are not filled; they are still copied.  Locked destination pixels never change.
        -> (patches, positions, info) in move_selection's shape over [fill window, destination rectangle] (the destination alone
        with `keep_source`); info = dict(windows, transform=True, matrix=the six ints, selected, selection=the warped Selection)
        plus work / undoable / locked / feather where `fill` reports them.  With history on the call is ONE undo step, the
        ordered entry of a move; a backend call that fails once the frame was written clears the history.
        TypeError / ValueError, all before the first backend call: a selection that is none, of another frame size or empty, a bad
        scale, angle, offset, flip or matrix, a matrix together with one of those four, a singular map, a map that puts nothing in
        the frame, a bad hole_grow, window, max_side, encode or feather."""
        encode = _check_encode(encode)
        feather = _check_feather(feather)
        self._check_selection(selection, "transform_selection")
        if selection.box is None:
            raise ValueError("empty selection: nothing to transform")
        box = selection.box
        if matrix is not None:
            try:
                alone = bool(scale == 1.0 and angle == 0.0 and flip is None and tuple(offset) == (0, 0))
            except (TypeError, ValueError):
                alone = False
            if not alone:
                raise ValueError("matrix excludes scale, angle, offset and flip")
            m = _check_warp_map(matrix)
        else:
            m = _check_warp_map(warp_matrix(box, scale, angle, offset, flip))
        hole_grow = _check_hole_grow(hole_grow)
        dst = warp_rect(box, m, self.frame_hw)
        if dst is None:
            raise ValueError("the map %r puts nothing of the selection in the frame" % (m,))
        be = self.backend
        return self._lift_fill_drop(
            selection, dst, window, margin, low_latency, max_side, encode, feather, keep_source, hole_grow,
            lambda lift, lift_rect: be.warp_drop(self._frame, lift, lift_rect, selection.plane, self._lock_plane, box, dst, m),
            lambda: be.warp(selection.plane, box, m), dict(transform=True, matrix=m), False)

    # ---- blur, sharpen or pixelate a selection --------------------------------------------------------------------------
    def filter_selection(self, selection, kind="blur", radius=None, amount=None, sigma=None, cell=None, feather=None, encode=None):
        """"Blur that face, pixelate that number plate, sharpen what I just scaled up" (DESIGN.md 6t): the selected pixels become a
        filter of the frame as it is now.  `kind`:
          "blur"      a Gaussian of `radius` (1 .. 32, default 8) and `sigma` (default max(radius / 3, 0.5), at most radius);
          "box"       the box filter of `radius` (default 8);
          "sharpen"   an unsharp mask: the pixel plus `amount` (a float in (0, 4], default 1.0) times its difference from the
                      Gaussian of `radius` (default 2) and `sigma`, clamped to 0 .. 255;
          "pixelate"  the mean of the pixel's `cell` x `cell` block (2 .. 64, default 16), the blocks anchored at the top left
                      corner of the selection's box and averaged over all their pixels, selected or not.
        An argument the kind does not take must be None.  `feather` = f (None or 0 .. 16) fades the filter in over f pixels at
        the selection's rim.  Integer arithmetic (include/sketchedit_filter.h): the same bytes on every machine.  Everything
        happens on the device under ONE hold of the session's lock:
          1. the LIFT: filter_rect(box, radius) of the frame -- the box with the taps' margin -- is saved into a slot;
          2. ONE launch filters the lifted pixels into the frame where the selection selects and the lock plane does not lock;
          3. with history on the lift IS the journal entry's slot -- everything that changed lies inside it -- so the call is one
             undo step of the single-window kind and makes no second save; a lift above `history_bytes` commits unjournalled
             and clears the history, and so does a backend call that fails once the filter was launched.
        The selection stays what it was; no new Selection is made.
        -> (patches, positions, info) in edit_regions' shape over ONE window, move_rect(box, (0, 0)); `encode` applies.
        info = dict(windows, filter=kind, radius, amount, cell, selected) plus undoable / locked / feather where `edit` reports
        them (radius or cell None where the kind has none; amount -1.0 but for "sharpen").
        TypeError / ValueError, all before the first backend call: a selection that is none, of another frame size or empty, a bad
        kind, radius, sigma, amount, cell, feather or encode, an argument the kind does not take."""
        encode = _check_encode(encode)
        feather = _check_feather(feather)
        self._check_selection(selection, "filter_selection")
        if selection.box is None:
            raise ValueError("empty selection: nothing to filter")
        if not isinstance(kind, str) or kind not in FILTER_KINDS:
            raise ValueError("kind is one of %s (got %r)" % (", ".join(repr(k) for k in FILTER_KINDS), kind))
        takes = dict(blur=("radius", "sigma"), box=("radius",), sharpen=("radius", "sigma", "amount"), pixelate=("cell",))[kind]
        for name, v in (("radius", radius), ("amount", amount), ("sigma", sigma), ("cell", cell)):
            if v is not None and name not in takes:
                raise ValueError("kind %r takes no %s (got %r)" % (kind, name, v))
        q8, taps = -256, None
        if kind == "pixelate":
            cell = _filter_int(16 if cell is None else cell, 2, FILTER_MAX_CELL, "cell")
        else:
            radius = _filter_int((2 if kind == "sharpen" else 8) if radius is None else radius, 1, FILTER_MAX_RADIUS, "radius")
            taps = filter_taps("box" if kind == "box" else "gauss", radius, sigma)
        if kind == "sharpen":
            amount = 1.0 if amount is None else amount
            if (isinstance(amount, (bool, np.bool_)) or not isinstance(amount, (int, float, np.integer, np.floating))
                    or not 0 < amount <= FILTER_MAX_AMOUNT):
                raise ValueError("amount is a number in (0, %g] (got %r)" % (FILTER_MAX_AMOUNT, amount))
            amount = float(amount)
            q8 = int(round(256 * amount))
            if q8 < 1:
                raise ValueError("amount %r rounds to no sharpening at all" % (amount,))
        else:
            amount = -1.0
        box = selection.box
        lift_rect = filter_rect(box, radius or 0, self.frame_hw)
        wins = [move_rect(box, (0, 0), self.frame_hw)]
        be = self.backend

        def apply(lift):
            if kind == "pixelate":
                be.filter_mosaic(self._frame, lift, lift_rect, selection.plane, self._lock_plane, box, cell, q8, feather or 0)
            else:
                be.filter_blur(self._frame, lift, lift_rect, selection.plane, self._lock_plane, box, taps, q8, feather or 0)
        return self._lift_apply(selection, lift_rect, wins, apply, encode, dict(filter=kind, radius=radius, amount=amount, cell=cell), feather)

    # ---- adjust a selection's tone and colour ---------------------------------------------------------------------------
    def adjust_selection(self, selection, lut=None, matrix=None, auto=None, reference=None, which="luma", clip=0, amount=1.0, feather=None,
                         encode=None):
        """"Brighten that face, desaturate the background, make what I just dropped match the place it landed in" (DESIGN.md 6u):
        the selected pixels become a pointwise function of the frame as it is now -- a table, then a matrix.
          `lut`     a (3, 256) or (256,) table of ints 0 .. 255 (adjust_lut makes them), or
          `auto`    a table made ON THE DEVICE from histograms of the frame, nothing coming down: "levels" (the selection's range
                    stretched to 0 .. 255, `clip` per mille, 0 .. 200, of its pixels cut off at either end), "equalize", or "match"
                    (the selection's distribution made that of `reference`: a Selection of this session -- "make this look like
                    that" -- or ("rim", r), r = 1 .. 16: the ring of pixels within r of the selection and outside it -- "match
                    where it landed").  `which`: "luma" (one table from the luma of the pixels, for all three channels) or
                    "channels" (a table per channel).  `auto` excludes `lut`; `reference` and `clip` go with their mode only;
          `matrix`  12 ints (adjust_matrix makes them), applied AFTER the table, with either of the above or alone;
          `amount`  0.0 .. 1.0, the opacity of the adjustment; `feather` = f (None or 0 .. 16) fades it in over f pixels at the rim.
        Integer arithmetic (include/sketchedit_adjust.h): the same bytes on every machine.  Everything happens on the device under
        ONE hold of the session's lock:
          1. the LIFT: move_rect(box, (0, 0)) of the frame is saved into a slot;
          2. with `auto`: the ring, if one is asked for (grow and combine); the histogram of the selection and, for "match", of
             the reference; the table made of them -- no download between them;
          3. ONE launch adjusts the lifted pixels into the frame where the selection selects and the lock plane does not lock;
          4. with history on the lift IS the journal entry's slot, so the call is one undo step of the single-window kind and makes
             no second save; a lift above `history_bytes` commits unjournalled and clears the history, and so does a backend call
             that fails once the adjustment was launched.
        The selection stays what it was.  -> (patches, positions, info) in edit_regions' shape over ONE window, the lift's;
        `encode` applies.  info = dict(windows, adjust="lut" | "auto" | "matrix" | "lut+matrix" | "auto+matrix", auto, which,
        amount, selected) plus undoable / locked / feather where `edit` reports them (which None without `auto`).
        TypeError / ValueError, all before the first backend call: a selection that is none, of another frame size or empty,
        nothing to apply, a bad lut, matrix, auto, reference, which, clip, amount, feather or encode."""
        encode = _check_encode(encode)
        feather = _check_feather(feather)
        self._check_selection(selection, "adjust_selection")
        if selection.box is None:
            raise ValueError("empty selection: nothing to adjust")
        if auto is not None and (not isinstance(auto, str) or auto not in ADJUST_AUTO):
            raise ValueError("auto is None or one of %s (got %r)" % (", ".join(repr(k) for k in ADJUST_AUTO), auto))
        if lut is not None and auto is not None:
            raise ValueError("auto makes the table: it excludes lut")
        if lut is None and auto is None and matrix is None:
            raise ValueError("nothing to adjust: give lut, auto or matrix")
        if lut is not None:
            lut = _check_adjust_lut(lut)
        if matrix is not None:
            matrix = _check_adjust_matrix(matrix)
        if not isinstance(which, str) or which not in ADJUST_WHICH:
            raise ValueError("which is one of %s (got %r)" % (", ".join(repr(k) for k in ADJUST_WHICH), which))
        clip = _filter_int(clip, 0, ADJUST_MAX_CLIP, "clip")
        if clip and auto != "levels":
            raise ValueError("clip goes with auto='levels' only (got %r)" % (clip,))
        rim = None
        if auto == "match":
            if isinstance(reference, Selection):
                self._check_selection(reference, "adjust_selection: reference")
                if reference.box is None:
                    raise ValueError("empty reference: nothing to match")
            elif isinstance(reference, tuple) and len(reference) == 2 and isinstance(reference[0], str) and reference[0] == "rim":
                rim = _filter_int(reference[1], 1, SELECT_MAX_GROW, "the rim's width")
            else:
                raise TypeError("auto='match' takes reference=<a Selection> or ('rim', r) (got %r)" % (reference,))
        elif reference is not None:
            raise ValueError("reference goes with auto='match' only")
        amount = _adjust_number(amount, 0, 1, "amount")
        q8 = int(round(256 * amount))
        box = selection.box
        lift_rect = move_rect(box, (0, 0), self.frame_hw)
        wins = [lift_rect]
        be = self.backend

        def table():                             # after the lift, in front of the launch's `try`: a failure here leaves the history alone
            if auto is None:
                return (be.upload(lut) if lut is not None else None,)
            ref = None
            if rim is not None:
                ring, rbox, _ = be.combine(be.grow(selection.plane, rim), selection.plane, COMBINE_OPS["subtract"])
                ref = (ring, rbox or box)                    # no ring at all (the selection is the frame): an empty record, the identity
            elif auto == "match":
                ref = (reference.plane, reference.box)
            src = be.hist(self._frame, selection.plane, box)
            ref = be.hist(self._frame, ref[0], ref[1]) if ref is not None else None
            return (be.hist_lut(src, ref, ADJUST_AUTO[auto], ADJUST_WHICH[which], clip),)
        what = "+".join(k for k, on in (("lut", lut is not None), ("auto", auto is not None), ("matrix", matrix is not None)) if on)
        return self._lift_apply(
            selection, lift_rect, wins,
            lambda lift, tb: be.adjust(self._frame, lift, lift_rect, selection.plane, self._lock_plane, box, tb, matrix, q8, feather or 0),
            encode, dict(adjust=what, auto=auto, which=which if auto is not None else None, amount=amount), feather, prepare=table)

    def histogram(self, selection=None):
        """The histogram of the frame (`selection` None) or of a selection's pixels, for a front end's display: a
        (4, 256) uint32 array on the host, rows R, G, B and luma Y = (77 R + 150 G + 29 B + 128) >> 8.  Counted on the device; ONE
        download of 4 KB.  The lock plays no part.  An empty selection gives zeros without a backend call."""
        if selection is not None:
            self._check_selection(selection, "histogram")
            if selection.box is None:
                return np.zeros((4, 256), np.uint32)
        with self._lock:
            box = selection.box if selection is not None else (0, 0) + self.frame_hw
            rec = self.backend.hist(self._frame, selection.plane if selection is not None else None, box)
            return np.ascontiguousarray(self.backend.download(rec)).view(np.uint32).reshape(4, 256)

    # ---- the canvas: crop, extend, rotate and flip ---------------------------------------------------------------------
    def _canvas_args(self, orient, rect, pad, selections):
        """what every canvas call refuses, all before the first backend call -> (o, (Hn, Wn), (oy, ox), pad mode, colour, selections)"""
        o = canvas_orient(orient)
        new_hw, origin = canvas_size(self.frame_hw, orient, rect)
        mode, rgb = canvas_pad(pad)
        try:
            selections = list(selections)
        except TypeError:
            raise TypeError("selections is a sequence of Selections (got %s)" % type(selections).__name__)
        for sel in selections:
            self._check_selection(sel, "canvas")
        if not callable(getattr(self.backend, "canvas", None)):
            raise NotImplementedError("this session's backend (%s) has no `canvas` (DESIGN.md 6y)" % type(self.backend).__name__)
        return o, new_hw, origin, mode, rgb, selections

    def _canvas_steps(self, o, new_hw, origin, mode, rgb, selections):
        """The launches of a canvas step, with the session's lock held: ONE for the new frame, one per carried plane -- the lock
        plane, if any, and each selection, with the constant 0: new area is neither locked nor selected.  The session's fields
        are not touched.  -> (frame, lock plane or None, the carried Selections)"""
        be, hw = self.backend, self.frame_hw
        frame = be.canvas(self._frame, hw, new_hw, origin, o, mode, rgb)
        lock = None if self._lock_plane is None else be.canvas(self._lock_plane, hw, new_hw, origin, o, CANVAS_CONSTANT, 0)
        made = []
        for sel in selections:
            plane, box, count = be.canvas(sel.plane, hw, new_hw, origin, o, CANVAS_CONSTANT, 0, tiles=True)
            made.append(Selection(be, plane, box, count, new_hw))
        return frame, lock, made

    def _canvas(self, orient, rect, pad, selections, fill=None):
        """canvas and extend_canvas(fill="network") once the wrappers' own arguments are checked.  `fill`: None, or the outpaint's
        (window, margin, low_latency, max_side, feather, encode, seamless), checked"""
        o, new_hw, origin, mode, rgb, selections = self._canvas_args(orient, rect, pad, selections)
        be = self.backend
        if fill is not None:
            window, margin, low_latency, max_side, feather, encode, seamless = fill
            Ho, Wo = (self.frame_hw[1], self.frame_hw[0]) if o & 4 else self.frame_hw
            box = canvas_new_box((Ho, Wo), new_hw, origin)
            if box is None:
                raise ValueError("fill='network' fills the new area: the rectangle adds none")
            if window is not None:
                y0, x0, h, w = (int(v) for v in window)
                scaled = max_side is not None
                if h < 16 or w < 16 or (not scaled and (h % 8 or w % 8)) or y0 < 0 or x0 < 0 or y0 + h > new_hw[0] or x0 + w > new_hw[1]:
                    raise ValueError("window %r: sides are multiples of 8, >= 16, and the window lies inside the new %dx%d frame"
                                     % (window, new_hw[1], new_hw[0]))
                win = (y0, x0, h, w)
            else:
                win = choose_window(box, new_hw, margin=margin)
            if max_side is not None:
                choose_working_size(win[2:], max_side)
            cut = _blend_box(box, win) if seamless else None
        with self._lock:
            previous = self.frame_hw
            held = [self._frame, self.frame_hw, self._lock_plane]
            frame, lock, made = self._canvas_steps(o, new_hw, origin, mode, rgb, selections)
            patch, pos, extra = None, (0, 0), {}
            if fill is None:
                self._frame, self.frame_hw, self._lock_plane = frame, new_hw, lock
            else:
                # the plane of the new area, made on the device: the input is NULL, the constant 255
                new_area = be.canvas(None, (Ho, Wo), new_hw, origin, 0, CANVAS_CONSTANT, 255)
                self._frame, self.frame_hw, self._lock_plane = frame, new_hw, lock
                try:
                    if cut is None:
                        _, work, _ = self._fill_steps(new_area, None, win, low_latency, max_side, feather, False)
                    else:
                        _, work, _ = self._fill_steps(new_area, None, win, low_latency, max_side, feather, False, cut)
                    patch = be.crop(self._frame, *win) if encode is None else _encoded(be, encode, [self._frame], [win])[0]
                except Exception:                # out of place: the state the call found is still whole
                    self._frame, self.frame_hw, self._lock_plane = held
                    raise
                pos = (win[1], win[0])
                extra = _edit_info(dict(window=win, fill=True), False, work, None, feather)
                if cut is not None:
                    extra["blend"] = "seamless"
            undoable = self._record_canvas(held)
        info = dict(canvas=new_hw, previous=previous, orient=orient, rect=origin + new_hw, undoable=undoable, selections=made,
                    locked=lock is not None, **extra)
        return patch, pos, info

    def canvas(self, orient=None, rect=None, pad="edge", selections=()):
        """Changes the frame's rectangle: "straighten it, crop it, add room".  The frame is ORIENTED -- `orient` None,
        "cw", "ccw" (quarter turns), "180", "h", "v" (mirrors), "transpose" or "transverse" -- and then cut or extended to `rect` =
        (y0, x0, h, w) in oriented coordinates, which may reach outside (None: the whole oriented frame); what lies outside is
        filled by `pad`: "edge" (the nearest pixel), "reflect" (numpy's "reflect") or an (r, g, b) colour.  Made on the device,
        out of place, under ONE hold of the session's lock: ONE launch makes the new frame, one each carries the lock plane, if
        any, and every Selection in `selections` -- new area is neither locked nor selected -- and the session's frame, frame_hw
        and lock plane are replaced.  Nothing frame-sized crosses the bus; a carried selection's tile records are its one
        download.  Selections that are not handed in keep the old frame_hw and are refused afterwards where the size changed.
        -> (None, (0, 0), info): info = dict(canvas=(H, W), previous=(H, W), orient, rect, undoable, selections=[the carried
        Selections, NEW objects of the new frame_hw whose box and count are what the step left of them], locked).
        With history on the step is ONE undo entry that holds the old frame and lock plane whole (3 H W + H W bytes): undo and
        redo exchange them with the session's, without a kernel, and return (None, (0, 0), dict(canvas, undo_depth,
        redo_depth)); older entries are valid again exactly when the stack reaches them.  A step whose entry does not fit
        `history_bytes` clears the history (undoable = False): older entries name the old geometry.
        ValueError / TypeError, all before the first backend call: an unknown orient or pad, a rect that is not four ints, a side
        outside 1 .. 32768, an origin above 2^20, a new frame below a session's minimum, a selection of another frame size."""
        return self._canvas(orient, rect, pad, selections)

    def crop_canvas(self, rect, selections=()):
        """canvas(rect=rect) with a `rect` = (y0, x0, h, w) that lies inside the frame: ValueError otherwise."""
        canvas_size(self.frame_hw, None, rect)
        y0, x0, h, w = (int(v) for v in rect)
        if y0 < 0 or x0 < 0 or y0 + h > self.frame_hw[0] or x0 + w > self.frame_hw[1]:
            raise ValueError("rect %r: a crop lies inside the %dx%d frame" % (tuple(rect), self.frame_hw[1], self.frame_hw[0]))
        return self._canvas(None, (y0, x0, h, w), "edge", selections)

    def extend_canvas(self, top=0, bottom=0, left=0, right=0, pad="edge", fill=None, selections=(), window=None, margin=0.5,
                      low_latency=None, max_side=None, feather=None, encode=None, blend=None):
        """canvas(rect=(-top, -left, H + top + bottom, W + left + right), pad=pad): room on each side, four ints >= 0 of which one
        at least is > 0.
        fill="network" is the outpaint, "add room and let the network fill it": DEFINED as this call without `fill` followed by
        fill(the plane of the new area, window=..., margin=..., low_latency=..., max_side=..., feather=..., encode=...) on the
        extended frame, in ONE undo step and under one hold of the lock.  The plane of the new area is made on the device;
        the window is choose_window of its box at `margin` unless given; the lock plane, carried first, is respected as every
        fill respects it; `pad` is what the generator sees under the hole's rim and what stays where the window does not
        reach.  -> (patch, (x0, y0), info): the window after the paste as `fill` returns it, info as canvas' plus window,
        fill=True and work / feather where `fill` reports them.  No quality claim is made, as for `fill`.
        `blend` = "seamless" (with fill="network" only): DEFINED as the extension followed by fill(the plane of the
        new area, blend="seamless", ...) -- the new area takes the local colour of the old frame along the seam; its box is the
        new area's.  Refused as `fill` refuses it, before the first backend call."""
        if not all(_canvas_int(v) and v >= 0 for v in (top, bottom, left, right)) or not (top or bottom or left or right):
            raise ValueError("top, bottom, left, right are ints >= 0, one of them > 0 (got %r)" % ((top, bottom, left, right),))
        if not (fill is None or isinstance(fill, str)) or fill not in CANVAS_FILLS:
            raise ValueError("fill is None or 'network' (got %r)" % (fill,))
        rect = (-int(top), -int(left), self.frame_hw[0] + int(top) + int(bottom), self.frame_hw[1] + int(left) + int(right))
        if fill is None:
            if blend is not None:
                raise ValueError("blend is the paste of the outpaint's fill: it needs fill='network' (got blend=%r)" % (blend,))
            return self._canvas(None, rect, pad, selections)
        feather = _check_feather(feather)
        return self._canvas(None, rect, pad, selections, (window, margin, low_latency, max_side, feather, _check_encode(encode),
                                                          _check_blend(blend, feather, self.backend)))

    def orient_canvas(self, op, selections=()):
        """canvas(orient=op): "cw", "ccw", "180", "h", "v", "transpose" or "transverse" (DESIGN.md 6y)."""
        if op is None:
            raise ValueError("op is one of %s" % ", ".join(repr(k) for k in CANVAS_ORIENTS if k is not None))
        return self._canvas(op, None, "edge", selections)

    def frame(self):
        """The whole frame as an (H,W,3) uint8 array (a download of the frame)."""
        with self._lock:
            return self.backend.download(self._frame)

    def _rect(self, rect):
        """frame_png's and frame_jpg's rectangle, checked: (y0, x0, h, w), the whole frame for None"""
        Hi, Wi = self.frame_hw
        y0, x0, h, w = (0, 0, Hi, Wi) if rect is None else (int(v) for v in rect)
        if not (PNG_SIDE_MIN <= h <= PNG_SIDE_MAX and PNG_SIDE_MIN <= w <= PNG_SIDE_MAX) or y0 < 0 or x0 < 0 or y0 + h > Hi or x0 + w > Wi:
            raise ValueError("rectangle %r: sides are %d .. %d and the rectangle lies inside the %dx%d frame"
                             % ((y0, x0, h, w), PNG_SIDE_MIN, PNG_SIDE_MAX, Wi, Hi))
        return (y0, x0, h, w)

    def frame_png(self, rect=None):
        """The frame, or its rectangle `rect` = (y0, x0, h, w), as the bytes of a PNG file encoded on the device (DESIGN.md
        6j): only the compressed stream comes down.  The sides lie in [16, 8192] and the rectangle inside the frame."""
        with self._lock:
            return self.backend.crop_png([self._frame], [self._rect(rect)])[0]

    def frame_jpg(self, rect=None, quality=90, subsampling="444", optimize=False):
        """The frame, or its rectangle `rect` = (y0, x0, h, w), as the bytes of a baseline JPEG file at `quality` 1 .. 100,
        encoded on the device: a lossy preview, several times smaller than frame_png's file; the resident frame
        is not touched.  The sides lie in [16, 8192] and the rectangle inside the frame.  subsampling="420" stores chroma at
        half resolution and optimize=True codes with four Huffman tables made for this image: smaller files,
        the same decoder."""
        q = int(quality)
        if not 1 <= q <= 100:
            raise ValueError("quality is 1 .. 100 (got %r)" % (quality,))
        _check_subsampling(subsampling)
        if not isinstance(optimize, bool):
            raise ValueError("optimize is a bool (got %r)" % (optimize,))
        win = self._rect(rect)
        with self._lock:
            if subsampling == "444" and not optimize:
                return self.backend.crop_jpg([self._frame], [win], q)[0]
            return self.backend.crop_jpg([self._frame], [win], q, subsampling=subsampling, optimize=optimize)[0]


def create_models_for_gpus(opt, gpu_ids=None):
    """One EditLine2Model per GPU of this node (weights replicated, one se_ctx / stream / workspace each): the worker set
    of a multi-GPU BatchingServer.  `gpu_ids` defaults to every visible device."""
    import copy
    import torch
    from . import models
    ids = list(range(torch.cuda.device_count())) if gpu_ids is None else list(gpu_ids)
    out = []
    for i in ids:
        o = copy.copy(opt)
        o.gpu_ids = [i]
        with torch.cuda.device(i):
            out.append(models.create_model(o).eval())
    return out


class BatchingServer:
    """Concurrent `submit(img, mask)` calls are grouped by working size and run as one forward per group
    (up to `max_batch` requests, waiting at most `max_wait_s` for company).  The forward treats the images of a
    batch independently and an image's result is bit-identical across batch positions WITHIN one
    execution mode of the library (include/sketchedit_hip.h: default vs SE_FLAG_LOW_LATENCY run different kernels that
    agree to fp32 rounding -- enough to flip a soft-mask value sitting on the 0.5 threshold).  `mode_policy`:
      "pinned" (default): the mode is a function of the request's working size and `max_batch` only -- low-latency iff
          even a full group of this size (`max_batch` images) is a small call -- so a request's result does NOT depend
          on what it was batched with;
      "by_size": the Engine picks the mode from each group's actual size (lowest latency for a lone request; results
          may differ at fp32 rounding level between a lone and a batched run of the same request).

    `models` = one model per GPU (create_models_for_gpus): every model gets its own worker thread, all workers pull
    groups from the one shared queue -- dynamic batching across the GPUs of the node; an idle GPU
    takes the next group, so the load balances itself.  `model` = the single-GPU form.

    device_io=True (EditLine2Model workers): `submit` only decodes the request to uint8 arrays (_device_inputs); the worker
    uploads them, resizes and normalises each request into its slot of the group's batch on the device
    (Engine.prepare_u8), runs one forward with fused output quantisation for the group and resizes each result back to its
    raw size on the device (Engine.resize_u8).  Byte-identical to the host steps; a request whose sketch mode the device
    path does not take is prepared on the host and joins the same group.

    window=True (one EditLine2Model): the server batches edits of editing sessions instead -- `submit(session, sketch)` ->
    what `EditSession.edit` returns.  The group key is the WINDOW size (choose_window's buckets), so sessions whose frames
    differ in size share a forward; the mode policy is the same, by window size and `max_batch`.  A group is one gather,
    one forward, one border and one paste launch (Engine.edit_window_u8 / window_paste_u8).  Growing is per request: a
    request whose mask reaches its window's border is not pasted but queued again under its larger window's size (at most
    `max_grow` times); a group never holds two requests of one session (the second waits for the next group: it must
    see the first's result).  `max_side` (with window=True): every edit runs at
    choose_working_size(window, max_side), as EditSession.edit(max_side=...) does; the group key is then
    (hs, ws, H, W) and the mode policy goes by the working size, the size of the forward.
    Sessions bring their own `history`: the saves of a group's journalled requests are ONE launch, in front of
    the run when the group commits in the call, else in front of the paste for the requests that stay.  `undo(session)` /
    `redo(session)` block and return like `submit`; they are queued like an edit of that session, so an undo submitted after
    two edits undoes the second; undo / redo requests of different sessions share a group, one swap launch per window size.
    Sessions bring their own lock planes too; the group keys do not know about them.  A group with at least one
    locked session runs the locked entry, with no plane for the others (whose results are what they get alone); a group
    with none runs the entries above.
    `feather` (with window=True): server-wide like `max_side`, the radius of EditSession.edit(feather=...).  A
    group always runs uncommitted; the requests that stay are pasted with ONE feathered paste launch, behind the one save
    launch.  The group key does not change."""

    def __init__(self, model=None, max_batch=32, max_wait_s=0.005, models=None, mode_policy="pinned", device_io=False,
                 window=False, max_grow=2, max_side=None, feather=None):
        if mode_policy not in ("pinned", "by_size"):
            raise ValueError(mode_policy)
        self.mode_policy = mode_policy
        self.device_io = bool(device_io)
        self.models = list(models) if models is not None else [model]
        if not self.models or any(m is None for m in self.models):
            raise ValueError("BatchingServer needs a model (or a list of models, one per GPU)")
        if self.device_io and not all(hasattr(m, "engine") and hasattr(m, "inference_u8") for m in self.models):
            raise ValueError("device_io=True needs EditLine2Model workers (their library engine runs the request steps)")
        self.window, self.max_grow = bool(window), int(max_grow)
        if self.window and (self.device_io or len(self.models) != 1):
            raise ValueError("window=True serves the sessions of ONE model (a session's frame lives on that model's GPU) and "
                             "has no device_io variant")
        if max_side is not None and not self.window:
            raise ValueError("max_side is the working-size cap of window edits: it needs window=True")
        self.max_side = None if max_side is None else int(max_side)
        self.feather = _check_feather(feather)
        if self.feather is not None and not self.window:
            raise ValueError("feather is the soft edge of window edits' paste: it needs window=True")
        self.model = self.models[0]
        self._has_knob = [_accepts_low_latency(m) for m in self.models]
        self.max_batch, self.max_wait_s = max_batch, max_wait_s
        self._lock = threading.Condition()
        self._queue = []          # (working shape (1,3,H,W), request, size_raw, slot, arrival time); request = (x, m) fp32
        #                           tensors prepared on the host, or the uint8 arrays (image, sketch) of the device path
        self._stop = False
        self.batches = []         # sizes of the batches that were run (observability / tests)
        self.batches_by_model = [0] * len(self.models)
        self._collecting = set()  # working sizes some worker is waiting out a deadline for (one collector per size)
        self._workers = [threading.Thread(target=self._run, args=(k,), daemon=True) for k in range(len(self.models))]
        for t in self._workers:
            t.start()

    def _window_key(self, win):
        """group key of a window: ("window", 3, h, w), with max_side ("window", 3, hs, ws, H, W) -- the forward's size last"""
        key = ("window", 3, win[2], win[3])
        return key if self.max_side is None else key + choose_working_size(win[2:], self.max_side)

    def _submit_window(self, session, sketch):
        """key: _window_key; request = dict(session, sketch, bbox, window, margin, reruns)"""
        if session.model is not self.model:
            raise ValueError("the session belongs to another model than this server's")
        sk, bbox = session._request(sketch)
        win = choose_window(bbox, session.frame_hw)
        return self._window_key(win), dict(session=session, sketch=sk, bbox=bbox, window=win, margin=0.5, reruns=0), None

    def _submit_history(self, session, op):
        if not self.window:
            raise ValueError("undo / redo are requests of editing sessions: they need window=True")
        if session.model is not self.model:
            raise ValueError("the session belongs to another model than this server's")
        return self._enqueue(("history",), dict(session=session, op=op), None)

    def undo(self, session):
        """`session.undo()` in the session's queue order -> what it returns"""
        return self._submit_history(session, "undo")

    def redo(self, session):
        return self._submit_history(session, "redo")

    def submit(self, img, mask):
        arrays = _device_inputs(img, mask) if self.device_io and not self.window else None
        if self.window:
            key, req, size_raw = self._submit_window(img, mask)
        elif arrays is not None:
            h_raw, w_raw = arrays[0].shape[:2]
            key, req, size_raw = (1, 3, h_raw // 8 * 8, w_raw // 8 * 8), arrays, (w_raw, h_raw)
        else:
            x, m, size_raw = _to_tensors(img, mask)
            key, req = tuple(x.shape), (x, m)
        return self._enqueue(key, req, size_raw)

    def _enqueue(self, key, req, size_raw):
        slot = {"done": threading.Event(), "out": None, "err": None}
        with self._lock:
            if self._stop:
                raise RuntimeError("server is closed")
            self._queue.append((key, req, size_raw, slot, time.monotonic()))
            self._lock.notify_all()
        slot["done"].wait()
        if slot["err"] is not None:
            raise slot["err"]
        return slot["out"]

    def close(self):
        with self._lock:
            self._stop = True
            self._lock.notify_all()
        for t in self._workers:
            t.join()

    def _take_group(self):
        """A worker becomes the collector of the OLDEST queued request whose working size no other worker is collecting, and
        waits for company of that size until the group is full or `max_wait_s` after that oldest request ARRIVED (not after
        collection started).  Several workers collect at once, one per distinct size, so an idle GPU never sits out a
        deadline for size S1 while requests of size S2 are queued; with k sizes queued the waits overlap
        instead of stacking."""
        with self._lock:
            while True:
                head = next((q for q in self._queue if q[0] not in self._collecting), None)
                if head is None:
                    if self._stop and not self._queue:
                        return None                   # stopped and drained
                    self._lock.wait(0.05 if self._stop else None)
                    continue
                shape = head[0]
                self._collecting.add(shape)
                try:
                    deadline = head[4] + self.max_wait_s
                    while True:
                        n = len(self._candidates(shape))
                        left = deadline - time.monotonic()
                        if n >= self.max_batch or left <= 0 or self._stop:
                            break
                        self._lock.wait(left)
                    group = self._candidates(shape)[:self.max_batch]
                    taken = {id(q) for q in group}    # (list.remove would compare the tensors inside the tuples)
                    self._queue = [q for q in self._queue if id(q) not in taken]
                finally:
                    self._collecting.discard(shape)
                    self._lock.notify_all()           # requests of this size that did not fit may be collected now
                return group

    def _candidates(self, shape):
        """Queued requests of one working size, oldest first.  Window mode: only a session's OLDEST queued request, whatever its
        size, is eligible -- a session's edits run in the order they were submitted, one per group."""
        if not self.window:
            return [q for q in self._queue if q[0] == shape]
        seen, out = set(), []
        for q in self._queue:
            if id(q[1]["session"]) not in seen:
                seen.add(id(q[1]["session"]))
                if q[0] == shape:
                    out.append(q)
        return out

    def _run_window(self, k, group):
        """One group of window edits of one window size.  -> one entry per request: its result, or None for a request that
        was queued again under a larger window."""
        reqs = [q[1] for q in group]
        be = reqs[0]["session"].backend
        h, w = group[0][0][2:4]
        work = group[0][0][4:6] if self.max_side is not None else None
        low_latency = self._mode(group[0][0]) if self._has_knob[k] else None
        grown = [None if r["reruns"] >= self.max_grow else r["session"]._grown(r["bbox"], r["window"], r["margin"]) for r in reqs]
        # no request can grow: the counts decide nothing (a feathered paste is a call of its own: no group commits)
        commit = all(g is None for g in grown) and self.feather is None
        frames = [r["session"]._frame for r in reqs]
        origins = [r["window"][:2] for r in reqs]
        journalled = [i for i, r in enumerate(reqs) if r["session"]._journals(h, w)]
        slots = {}
        lks = [r["session"]._lock_plane for r in reqs]
        locked = any(t is not None for t in lks)          # (then the whole list travels, its Nones included)

        def save(idx):                                    # one launch for the group's journalled requests
            if idx:
                slots.update(zip(idx, be.save([frames[i] for i in idx], [origins[i] for i in idx], (h, w))))
        locks = sorted({id(r["session"]): r["session"]._lock for r in reqs}.items())
        for _, lk in locks:
            lk.acquire()
        try:
            crops = [be.upload(r["sketch"][y0:y0 + h, x0:x0 + w]) for r, (y0, x0) in zip(reqs, origins)]
            if commit:
                save(journalled)
            rgb, m8, counts = _run_windows(be, frames, origins, crops, (h, w), work, lks if locked else None, commit, low_latency)
            stay = [i for i in range(len(reqs)) if grown[i] is None or not any(counts[i])]
            if not commit:
                save([i for i in stay if i in journalled])          # (a request that is queued again journals nothing yet)
            if self.feather is not None and stay:
                be.paste_feather([frames[i] for i in stay], [origins[i] for i in stay], [lks[i] for i in stay] if locked else None,
                                 (h, w), self.feather, be.select(rgb, stay), be.select(m8, stay))
            elif not commit and stay:
                _paste_windows(be, [frames[i] for i in stay], [origins[i] for i in stay], (h, w), work,
                               [lks[i] for i in stay] if locked else None, be.select(rgb, stay), be.select(m8, stay))
            outs = [None] * len(reqs)
            for i in stay:
                r = reqs[i]
                y0, x0 = origins[i]
                info = dict(window=r["window"], counts=list(counts[i]), reruns=r["reruns"], margin=r["margin"])
                undoable = r["session"]._record(r["window"], slots.get(i)) if r["session"].history > 0 else None
                _edit_info(info, lks[i] is not None, None if work is None else tuple(work), undoable, self.feather)
                outs[i] = (be.crop(frames[i], y0, x0, h, w), (x0, y0), info)
        finally:
            for _, lk in locks:
                lk.release()
        again = []
        for i, q in enumerate(group):
            if outs[i] is None:
                r = dict(reqs[i])
                r["window"], r["margin"] = grown[i]
                r["reruns"] += 1
                again.append((self._window_key(r["window"]), r, None, q[3], q[4]))
        if again:
            with self._lock:
                self._queue = again + self._queue     # in front: they are older than what arrived since, and their sessions' next edits wait for them
                self._lock.notify_all()
        return outs

    def _run_history(self, group):
        """One group of undo / redo requests, each of another session (_candidates): one swap launch per window size; a region
        edit's, a move's or a canvas step's entry takes the session's own exchange.  A request with nothing to undo / redo fails alone
        (IndexError)."""
        reqs = [q[1] for q in group]
        be = reqs[0]["session"].backend
        outs = [None] * len(reqs)
        locks = sorted({id(r["session"]): r["session"]._lock for r in reqs}.items())
        for _, lk in locks:
            lk.acquire()
        try:
            stacks, by_size = [], {}
            for i, r in enumerate(reqs):
                s = r["session"]
                stacks.append((s._undo, s._redo) if r["op"] == "undo" else (s._redo, s._undo))
                if not stacks[i][0]:
                    group[i][3]["err"] = IndexError("nothing to " + r["op"])
                    outs[i] = False
                elif isinstance(stacks[i][0][-1][0], _Canvas):       # a canvas step's entry: the session's own pointer exchange
                    outs[i] = s._exchange_canvas(*stacks[i])
                elif isinstance(stacks[i][0][-1][0], _Sequence):     # a move's entry: the session's own ordered exchange
                    outs[i] = s._exchange_sequence(*stacks[i], r["op"] == "undo")
                elif isinstance(stacks[i][0][-1][0], _Regions):      # a region edit's entry: the session's own exchange
                    outs[i] = s._exchange_regions(*stacks[i])
                else:
                    by_size.setdefault(stacks[i][0][-1][0][2:], []).append(i)
            for hw, idx in by_size.items():
                tops = [stacks[i][0][-1] for i in idx]
                be.swap([reqs[i]["session"]._frame for i in idx], [t[0][:2] for t in tops], hw, [t[1] for t in tops])
                for i in idx:
                    outs[i] = reqs[i]["session"]._exchanged(*stacks[i])
        finally:
            for _, lk in locks:
                lk.release()
        return outs

    def _mode(self, shape):
        """Execution mode of a group of requests of working size `shape` (1,3,H,W) -- see the class docstring.  (A group key
        ends in the size its forward runs at: the window's, or the working size of a scaled window edit.)"""
        if self.mode_policy == "by_size":
            return None
        from ._lib import Engine
        return Engine.is_low_latency(self.max_batch, shape[-2], shape[-1])

    def _run_device(self, k, group):
        """device_io: every request prepared into its slot of one (B,3,H,W) / (B,1,H,W) pair on the device, one forward with
        fused quantisation (the group's execution mode as _forward's), each result resized back to its raw size there."""
        import torch
        from PIL import Image
        model = self.models[k]
        eng = model.engine()
        _, _, H, W = group[0][0]
        dev = torch.device("cuda", eng.device)
        image = torch.empty((len(group), 3, H, W), dtype=torch.float32, device=dev)
        sketch = torch.empty((len(group), 1, H, W), dtype=torch.float32, device=dev)
        for i, q in enumerate(group):
            req = q[1]
            if isinstance(req[0], np.ndarray):
                eng.prepare_u8(_lib.upload_u8(req[0], dev), _lib.upload_u8(req[1], dev), H, W, out=(image[i:i + 1], sketch[i:i + 1]))
            else:                                      # a sketch mode the device path does not take: prepared on the host
                image[i:i + 1].copy_(req[0])
                sketch[i:i + 1].copy_(req[1])
        low_latency = self._mode(group[0][0]) if self._has_knob[k] else None
        rgb, _ = model.inference_u8({"image": image, "mask": sketch}, low_latency=low_latency)
        outs = []
        for i, q in enumerate(group):
            w_raw, h_raw = q[2]
            outs.append(Image.fromarray(eng.resize_u8(rgb[i:i + 1], (h_raw, w_raw))[0].cpu().numpy()))
        return outs

    def _forward(self, k, x, m):
        model = self.models[k]
        if self._has_knob[k]:
            return model({"image": x, "mask": m}, mode="inference", low_latency=self._mode(tuple(x.shape)))
        return model({"image": x, "mask": m}, mode="inference")   # a model object without the execution-mode knob

    def _run(self, k):
        import torch
        while True:
            group = self._take_group()
            if group is None:
                return
            if not group:                 # another worker took the requests this one was waiting with
                continue
            ran = len(group)
            try:
                if self.window and group[0][0] == ("history",):
                    outs = self._run_history(group)
                elif self.window:
                    outs = self._run_window(k, group)
                    done = [(q, out) for q, out in zip(group, outs) if out is not None]     # the others were queued again
                    group, outs = [q for q, _ in done], [out for _, out in done]
                elif self.device_io:
                    outs = self._run_device(k, group)
                else:
                    x = torch.cat([q[1][0] for q in group], 0)
                    m = torch.cat([q[1][1] for q in group], 0)
                    with torch.no_grad():
                        generated, _ = self._forward(k, x, m)
                    outs = [_to_image(generated[i:i + 1], q[2]) for i, q in enumerate(group)]
                with self._lock:
                    self.batches.append(ran)
                    self.batches_by_model[k] += 1
                for q, out in zip(group, outs):
                    q[3]["out"] = out
            except Exception as e:      # deliver the failure to every waiting caller
                for q in group:
                    q[3]["err"] = e
            for q in group:
                q[3]["done"].set()
