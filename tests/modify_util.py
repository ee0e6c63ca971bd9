"""The modification of a selection's shape of DESIGN.md 6w (include/sketchedit_modify.h) in plain numpy -- the statement the
kernels of se_modify.hip and the sessions' modify_selection are compared with, byte for byte: brute force over the offsets of the
disc, a padded plane shifted and OR-ed or summed (3209 shifts at most) -- the kernels' tile-by-tile algorithm restated in Python
integers, and the test patterns."""
import functools
import math

import numpy as np

MAX_RADIUS = 32
EXPAND, CONTRACT, SMOOTH = range(3)
SUBTRACT = 1                                         # SE_COMBINE_SUBTRACT
DISC_COUNTS = {1: 5, 2: 13, 3: 29, 4: 49, 5: 81, 8: 197, 16: 797, 31: 3001, 32: 3209}      # the header's known answers


@functools.lru_cache(maxsize=None)
def disc(r):
    """the offsets (dy, dx) with dy^2 + dx^2 <= r^2, in integers"""
    return tuple((dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dy * dy + dx * dx <= r * r)


def _count(sel, r):
    """per pixel p: the number of True pixels of `sel` (a bool plane) among the in-frame pixels of p + D(r)"""
    Hi, Wi = sel.shape
    pad = np.zeros((Hi + 2 * r, Wi + 2 * r), np.int32)
    pad[r:r + Hi, r:r + Wi] = sel
    c = np.zeros((Hi, Wi), np.int32)
    for dy, dx in disc(r):
        c += pad[r + dy:r + dy + Hi, r + dx:r + dx + Wi]
    return c


def _u8(b):
    return np.where(b, 255, 0).astype(np.uint8)


def spec_expand(plane, r):
    return _u8(_count(np.asarray(plane) != 0, r) > 0)


def spec_contract(plane, r):
    sel = np.asarray(plane) != 0
    return _u8(sel & (_count(~sel, r) == 0))


def spec_smooth(plane, r):
    sel = np.asarray(plane) != 0
    c, n = _count(sel, r), _count(np.ones_like(sel), r)
    return _u8((2 * c > n) | ((2 * c == n) & sel))


def spec_modify(plane, op, r):
    assert 1 <= r <= MAX_RADIUS
    return {EXPAND: spec_expand, CONTRACT: spec_contract, SMOOTH: spec_smooth}[op](plane, r)


def spec_border(plane, r, side):
    sel = np.asarray(plane) != 0
    outer = sel if side == "inside" else spec_expand(plane, r) != 0
    inner = sel if side == "outside" else spec_contract(plane, r) != 0
    return _u8(outer & ~inner)


def spec_kind(plane, kind, r, side="both"):
    """the whole definition of EditSession.modify_selection"""
    if kind == "border":
        return spec_border(plane, r, side)
    return spec_modify(plane, dict(expand=EXPAND, contract=CONTRACT, smooth=SMOOTH)[kind], r)


def box_count(plane):
    """(tight half-open box or None, count) of plane > 0"""
    ys, xs = np.nonzero(plane)
    if ys.size == 0:
        return None, 0
    return (int(ys.min()), int(xs.min()), int(ys.max()) + 1, int(xs.max()) + 1), int(ys.size)


# ---- the kernels' algorithm, tile by tile, in Python integers ------------------------------------------------------------------------
def _isqrt_loop(v):
    s = 0
    while (s + 1) * (s + 1) <= v:
        s += 1
    return s


def _stage(plane, tx0, ty0, r, invert):
    """the staged row masks of a tile (Python ints of 64 + 2r bits) and the exit class: 0 mixed, 1 no bit, 2 every in-frame bit"""
    Hi, Wi = plane.shape
    masks, any_, full = [], False, True
    for i in range(16 + 2 * r):
        y, m, f = ty0 - r + i, 0, 0
        if 0 <= y < Hi:
            for c in range(64 + 2 * r):
                x = tx0 - r + c
                if 0 <= x < Wi:
                    f |= 1 << c
                    if (plane[y, x] != 0) != invert:
                        m |= 1 << c
        any_, full = any_ or m != 0, full and m == f
        masks.append(m)
    return masks, (1 if not any_ else 2 if full else 0)


def _store(out, base, tx0, ty0, rows):
    """store_tile: the aligned dwords of each row of the tile; `base` = the plane's first byte address mod 4.  Counts the writers
    of every byte in out[1]."""
    plane, writers = out
    Hi, Wi = plane.shape
    tw = min(64, Wi - tx0)
    for item in range(16 * 17):
        j, k = divmod(item, 17)
        y = ty0 + j
        if y >= Hi:
            continue
        p0 = 4 * k - (base + y * Wi + tx0) % 4
        if p0 >= tw:
            continue
        for e in range(4):
            if 0 <= p0 + e < tw:
                plane[y, tx0 + p0 + e] = 255 if (rows[j] >> (p0 + e)) & 1 else 0
                writers[y, tx0 + p0 + e] += 1


def tiled_modify(plane, op, r, base=0):
    """modify_disc_kernel / modify_vote_kernel as they are written: 64 x 16 tiles, the staged masks, the column distances read off
    two words, the byte-parallel compare, the exclusive prefix counts, the closed-form n, the early exits, the dword slots of
    the store.  Asserts that every byte has exactly one writer."""
    plane = np.asarray(plane)
    Hi, Wi = plane.shape
    out = (np.full((Hi, Wi), 0x5C, np.uint8), np.zeros((Hi, Wi), np.int32))
    lim = [_isqrt_loop(r * r - d * d) for d in range(r + 1)]
    assert lim == [math.isqrt(r * r - d * d) for d in range(r + 1)]
    M64 = (1 << 64) - 1
    for ty0 in range(0, Hi, 16):
        for tx0 in range(0, Wi, 64):
            invert = op == CONTRACT
            masks, flat = _stage(plane, tx0, ty0, r, invert)
            if flat:
                rows = [M64 if (flat == 2) != invert else 0] * 16
                _store(out, base, tx0, ty0, rows)
                continue
            rows = []
            if op != SMOOTH:
                g = [[0] * (64 + 2 * r) for _ in range(16)]
                for c in range(64 + 2 * r):
                    col = sum(((m >> c) & 1) << i for i, m in enumerate(masks))
                    c0, c1 = col & M64, col >> 64
                    for j in range(16):
                        i = j + r
                        below = ((c0 >> i) | (c1 << (64 - i))) & M64
                        above = (c0 << (63 - i)) & M64
                        dd = (below & -below).bit_length() - 1 if below else 64
                        du = 64 - above.bit_length() if above else 64
                        g[j][c] = min(dd, du, r + 1)
                for j in range(16):
                    m = 0
                    for x in range(64):
                        acc = 0
                        for dx in range(-r, r + 1):
                            acc |= (0x80 + lim[abs(dx)] - g[j][x + r + dx]) & 0xFF
                        m |= (acc >> 7) << x
                    rows.append(m ^ M64 if invert else m)
            else:
                pre = [[bin(m & ((1 << c) - 1)).count("1") for c in range(64 + 2 * r + 1)] for m in masks]
                for j in range(16):
                    m, y, i = 0, ty0 + j, j + r
                    for lane in range(64):
                        x, cc, c, n = tx0 + lane, lane + r, 0, 0
                        for d in range(r + 1):
                            L = lim[d]
                            run = min(x + L, Wi - 1) - max(x - L, 0) + 1
                            for s in ((d, -d) if d else (0,)):
                                c += pre[i + s][cc + L + 1] - pre[i + s][cc - L]
                                n += run if 0 <= y + s < Hi else 0
                        if x < Wi and y < Hi and (2 * c > n or (2 * c == n and (masks[i] >> cc) & 1)):
                            m |= 1 << lane
                    rows.append(m)
            _store(out, base, tx0, ty0, rows)
    assert (out[1] == 1).all()
    return out[0]


# ---- patterns: each (Hi, Wi, r) -> an (Hi,Wi) uint8 plane ----------------------------------------------------------------------------
def _blank(Hi, Wi, v=0):
    return np.full((Hi, Wi), v, np.uint8)


def points(Hi, Wi, pts, selected=True, value=255):
    """single pixels (those inside the frame), selected on an empty plane or unselected on a full one"""
    p = _blank(Hi, Wi, 0 if selected else value)
    for y, x in pts:
        if 0 <= y < Hi and 0 <= x < Wi:
            p[y, x] = value if selected else 0
    return p


def corners(Hi, Wi):
    return [(0, 0), (0, Wi - 1), (Hi - 1, 0), (Hi - 1, Wi - 1)]


FOUR_TILES = [(15, 63), (16, 64), (15, 64), (16, 63)]      # around the corner that four tiles share


def clamp_points(Hi, Wi, pts):
    return [(min(y, Hi - 1), min(x, Wi - 1)) for y, x in pts]


def checkerboard(Hi, Wi):
    yy, xx = np.mgrid[0:Hi, 0:Wi]
    return _u8((yy + xx) % 2 == 0)


def random_plane(Hi, Wi, density, seed, values=(255,)):
    rng = np.random.RandomState(seed)
    vals = np.asarray(values, np.uint8)
    return np.where(rng.random_sample((Hi, Wi)) < density, vals[rng.randint(0, len(vals), (Hi, Wi))], 0).astype(np.uint8)


def half_plane(Hi, Wi):
    """columns 0 .. Wi / 2 - 1 selected: on an even width the boundary columns see 2c == n under smooth"""
    p = _blank(Hi, Wi)
    p[:, :Wi // 2] = 255
    return p


def cross(Hi, Wi, half=20):
    """a horizontal and a vertical bar, 2 * half wide, through the middle: they meet all four frame edges head on"""
    p = _blank(Hi, Wi)
    p[max(Hi // 2 - half, 0):Hi // 2 + half, :] = 255
    p[:, max(Wi // 2 - half, 0):Wi // 2 + half] = 255
    return p


def blob(Hi, Wi):
    """an ellipse that touches all four frame edges, with a hole"""
    yy, xx = np.mgrid[0:Hi, 0:Wi]
    cy, cx = (Hi - 1) / 2.0, (Wi - 1) / 2.0
    d = ((yy - cy) / (Hi / 2.0)) ** 2 + ((xx - cx) / (Wi / 2.0)) ** 2
    return _u8((d <= 1.0) & (d >= 0.1))
