"""The lasso and the algebra of selections of DESIGN.md 6p (include/sketchedit_lasso.h) in plain numpy / Python integers -- the
statement the kernels of se_lasso.hip and the sessions' select_lasso / combine / fill_lasso are compared with, byte for byte --
the kernel's tile-by-tile algorithm restated in Python integers, and the test shapes."""
import math

import numpy as np

from select_util import spec_grow

LIM = 4 * 8192                                   # what the kernel clamps a loaded coordinate to
ADD, SUBTRACT, INTERSECT, XOR, INVERT = range(5)


def clamp_edges(edges):
    return np.clip(np.asarray(edges, np.int64).reshape(-1, 4), 0, LIM)


def spec_lasso(edges, Hi, Wi):
    """selected[y, x] = 255 iff an odd number of edges span the scanline of the centre (4x + 2, 4y + 2) and cross it strictly
    left of the centre; int64 throughout, loaded values clamped as the kernel clamps them"""
    py = 4 * np.arange(Hi, dtype=np.int64)[:, None] + 2
    px = 4 * np.arange(Wi, dtype=np.int64)[None, :] + 2
    odd = np.zeros((Hi, Wi), bool)
    for ax, ay, bx, by in clamp_edges(edges).tolist():
        spans = (ay <= py) != (by <= py)
        s = (px - ax) * (by - ay) - (py - ay) * (bx - ax)
        odd ^= spans & ((s > 0) if by > ay else (s < 0))
    return np.where(odd, 255, 0).astype(np.uint8)


def spec_combine(a, b, op):
    sa = np.asarray(a) != 0
    sb = None if b is None else np.asarray(b) != 0
    out = {ADD: lambda: sa | sb, SUBTRACT: lambda: sa & ~sb, INTERSECT: lambda: sa & sb, XOR: lambda: sa ^ sb, INVERT: lambda: ~sa}[op]()
    return np.where(out, 255, 0).astype(np.uint8)


def spec_edges(rings, frame_hw):
    """rings of float points in frame pixels -> (N,4) int32 edges: floor(4 v + 0.5), clamped to the frame's rectangle, every
    ring closed"""
    Hi, Wi = frame_hw
    out = []
    for ring in rings:
        q = [(min(max(math.floor(4 * x + 0.5), 0), 4 * Wi), min(max(math.floor(4 * y + 0.5), 0), 4 * Hi)) for x, y in ring]
        out += [q[i] + q[(i + 1) % len(q)] for i in range(len(q))]
    return np.asarray(out, np.int32).reshape(-1, 4)


def spec_select_lasso(rings, frame_hw, grow):
    """the whole definition of EditSession.select_lasso: the (Hi,Wi) uint8 plane of 0 / 255"""
    return spec_grow(spec_lasso(spec_edges(rings, frame_hw), *frame_hw) == 255, grow)


def box_count(plane):
    """(tight half-open box or None, count) of plane > 0"""
    ys, xs = np.nonzero(plane)
    if ys.size == 0:
        return None, 0
    return (int(ys.min()), int(xs.min()), int(ys.max()) + 1, int(xs.max()) + 1), int(ys.size)


# ---- the kernel's algorithm, tile by tile, in Python integers -----------------------------------------------------------------------
def tiled_lasso(edges, Hi, Wi, fold_left=False, stats=None):
    """lasso_fill_kernel as it is written: 64 x 16 tiles, the edges in chunks of 256, the cull predicate (the half-open y-span
    holds a py of the tile's rows; min(ax, bx) below the tile's largest px), kept edges oriented upwards and tested as
    ay <= py < ay + dy and (px - ax) dy - (py - ay) dx > 0.  fold_left: the optional per-row parity of edges wholly left of the
    tile (not what the kernel does; kept to show it is the same plane)."""
    e = clamp_edges(edges).tolist()
    out = np.zeros((Hi, Wi), np.uint8)
    for ty0 in range(0, Hi, 16):
        for tx0 in range(0, Wi, 64):
            tx1, ty1 = min(tx0 + 64, Wi), min(ty0 + 16, Hi)
            cx0, cx1 = 4 * tx0 + 2, 4 * (tx1 - 1) + 2
            odd = [[False] * (tx1 - tx0) for _ in range(ty1 - ty0)]
            for base in range(0, len(e), 256):
                kept = []
                for ax, ay, bx, by in e[base:base + 256]:
                    lo, hi = min(ay, by), max(ay, by)
                    r = max(ty0, (lo + 1) >> 2)
                    assert (lo + 1) >> 2 == -((-(lo - 2)) // 4)
                    if r < ty1 and 4 * r + 2 < hi and min(ax, bx) < cx1:
                        kept.append((ax, ay, bx - ax, by - ay) if by > ay else (bx, by, ax - bx, ay - by))
                if stats is not None:
                    stats.append(len(kept))
                for ax, ay, dx, dy in kept:
                    assert dy > 0
                    whole_row = fold_left and max(ax, ax + dx) < cx0
                    for y in range(ty0, ty1):
                        ey = 4 * y + 2 - ay
                        if ey < 0 or ey >= dy:
                            continue
                        if whole_row:                                     # the crossing lies left of every centre of the tile
                            odd[y - ty0] = [not v for v in odd[y - ty0]]
                            continue
                        t = ey * dx
                        row = odd[y - ty0]
                        for x in range(tx0, tx1):
                            if (4 * x + 2 - ax) * dy - t > 0:
                                row[x - tx0] = not row[x - tx0]
            out[ty0:ty1, tx0:tx1] = np.where(np.array(odd), 255, 0)
    return out


# ---- shapes: each -> (N,4) int32 edges in quarter pixels of an (Hi,Wi) frame ---------------------------------------------------------
def ring_edges(*rings):
    out = []
    for q in rings:
        q = [(int(x), int(y)) for x, y in q]
        out += [q[i] + q[(i + 1) % len(q)] for i in range(len(q))]
    return np.asarray(out, np.int32).reshape(-1, 4)


def _ellipse(Hi, Wi, n, fx=0.45, fy=0.45, cx=None, cy=None):
    cx, cy = 2 * Wi if cx is None else cx, 2 * Hi if cy is None else cy
    return [(round(cx + 4 * fx * Wi * math.cos(2 * math.pi * k / n)), round(cy + 4 * fy * Hi * math.sin(2 * math.pi * k / n))) for k in range(n)]


def rect_on_centres(Hi, Wi):
    """vertices on pixel centres: ties on all four sides"""
    return ring_edges([(6, 6), (4 * (Wi - 2) + 2, 6), (4 * (Wi - 2) + 2, 4 * (Hi - 2) + 2), (6, 4 * (Hi - 2) + 2)])


def triangle_on_scanlines(Hi, Wi):
    """every vertex has ay = 2 mod 4: exactly on a scanline"""
    return ring_edges([(9, 4 * 2 + 2), (4 * Wi - 7, 4 * (Hi // 2) + 2), (4 * (Wi // 3) + 1, 4 * (Hi - 2) + 2)])


def star(Hi, Wi):
    """a self-crossing five-pointed star: its middle is a hole"""
    p = _ellipse(Hi, Wi, 5, 0.48, 0.48)
    return ring_edges([p[(2 * k) % 5] for k in range(5)])


def ring_in_ring(Hi, Wi):
    return ring_edges([(5, 7), (4 * Wi - 6, 11), (4 * Wi - 9, 4 * Hi - 5), (3, 4 * Hi - 10)],
                      [(Wi, Hi + 1), (3 * Wi - 2, Hi + 3), (3 * Wi + 1, 3 * Hi), (Wi + 3, 3 * Hi - 2)])


def horizontal_and_zero_length(Hi, Wi):
    """horizontal edges (some on scanlines, some doubling back), repeated points"""
    y0, y1 = 4 * 3 + 2, 4 * (Hi - 4) + 2
    return ring_edges([(10, y0), (2 * Wi, y0), (2 * Wi, y0), (Wi, y0), (4 * Wi - 10, y0), (4 * Wi - 10, 2 * Hi), (4 * Wi - 10, 2 * Hi),
                       (4 * Wi - 20, y1), (3 * Wi, y1), (10, y1), (10, y1)])


def collinear(Hi, Wi):
    """points on one line: nothing is selected"""
    return ring_edges([(6, 10), (4 * min(Hi, Wi) - 6, 4 * min(Hi, Wi) - 2), (2 * min(Hi, Wi) + 2, 2 * min(Hi, Wi) + 6)])


def whole_frame(Hi, Wi):
    return ring_edges([(0, 0), (4 * Wi, 0), (4 * Wi, 4 * Hi), (0, 4 * Hi)])


def sliver(Hi, Wi):
    """a diagonal strip of width 2 around the line x - y = 2: centres have x - y = 0 mod 4, so it holds none, though its box does"""
    t0, t1 = 4, 4 * min(Hi, Wi) - 8
    return ring_edges([(2 + t0 - 1, t0), (2 + t0 + 1, t0), (2 + t1 + 1, t1), (2 + t1 - 1, t1)])


def left_and_right(Hi, Wi):
    """a diamond over the frame, a small ring at its left side and one at its right: in the multi-tile sizes some edges lie
    wholly left of a tile and others wholly right of it"""
    return ring_edges([(2 * Wi, 3), (4 * Wi - 3, 2 * Hi + 1), (2 * Wi + 1, 4 * Hi - 3), (3, 2 * Hi - 1)],
                      [(9, 9), (45, 13), (41, 4 * Hi - 9), (7, 4 * Hi - 15)],
                      [(4 * Wi - 9, 9), (4 * Wi - 45, 13), (4 * Wi - 41, 4 * Hi - 9), (4 * Wi - 7, 4 * Hi - 15)])


def polygon_300(Hi, Wi):
    return ring_edges(_ellipse(Hi, Wi, 300))


def polygon_600(Hi, Wi):
    """two rings of 300: an annulus"""
    return ring_edges(_ellipse(Hi, Wi, 300, 0.47, 0.47), _ellipse(Hi, Wi, 300, 0.2, 0.25))


def no_edges(Hi, Wi):
    return np.zeros((0, 4), np.int32)


def out_of_range(Hi, Wi):
    """a buffer of other contents: negative, beyond the frame, beyond int16 and at int32's ends -- the clamped rule applies"""
    rng = np.random.RandomState(Hi * 1000 + Wi)
    e = rng.randint(-40, 4 * max(Hi, Wi) + 40, (40, 4)).astype(np.int64)
    e[::7, 0] = -2 ** 31
    e[3::7, 2] = 2 ** 31 - 1
    e[5::7, 1] = 70000
    e[6::7, 3] = -70000
    return e.astype(np.int32)


SHAPES = [rect_on_centres, triangle_on_scanlines, star, ring_in_ring, horizontal_and_zero_length, collinear, whole_frame, sliver,
          left_and_right, polygon_300, polygon_600, no_edges, out_of_range]
SIZES = [(16, 16), (37, 53), (64, 64), (65, 129), (100, 90), (130, 70)]
