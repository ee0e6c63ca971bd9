"""The outline of a selection of DESIGN.md 6q (include/sketchedit_outline.h) in plain numpy / Python integers -- the statement the
kernels of se_outline.hip and the sessions' rings() are compared with, record for record -- the kernels' mask arithmetic restated
in Python integers, the rings traced straight from the pixels (no records, no tiles), and the test planes."""
import numpy as np

TILE = 64
M64 = (1 << 64) - 1


# ---- the statement ---------------------------------------------------------------------------------------------------------------
def _runs(side):
    """side: (h, w) bool, runs along the LAST axis -> (row, first, end) arrays, sorted by (row, first)"""
    z = np.zeros((side.shape[0], 1), bool)
    d = np.diff(np.concatenate([z, side, z], axis=1).astype(np.int8), axis=1)
    r0, c0 = np.nonzero(d == 1)
    r1, c1 = np.nonzero(d == -1)                     # (row-major: the k-th end closes the k-th start)
    assert (r0 == r1).all()
    return r0, c0, c1


def spec_outline(plane):
    """-> (total, 4) int32 records of the plane in the definition's order: tiles row-major; in a tile N, S (by (y, x)), E, W (by
    (x, y)); a pixel is selected iff its byte is non-zero, outside the frame nothing is"""
    sel = np.asarray(plane) != 0
    Hi, Wi = sel.shape
    p = np.pad(sel, 1)
    c = p[1:-1, 1:-1]
    sides = [c & ~p[:-2, 1:-1], c & ~p[2:, 1:-1], c & ~p[1:-1, 2:], c & ~p[1:-1, :-2]]       # N S E W
    out = []
    for ty0 in range(0, Hi, TILE):
        for tx0 in range(0, Wi, TILE):
            n, s, e, w = (m[ty0:ty0 + TILE, tx0:tx0 + TILE] for m in sides)
            y, x0, x1 = _runs(n)
            out.append(np.stack([4 * (tx0 + x0), 4 * (ty0 + y), 4 * (tx0 + x1), 4 * (ty0 + y)], 1))
            y, x0, x1 = _runs(s)
            out.append(np.stack([4 * (tx0 + x1), 4 * (ty0 + y) + 4, 4 * (tx0 + x0), 4 * (ty0 + y) + 4], 1))
            x, y0, y1 = _runs(e.T)
            out.append(np.stack([4 * (tx0 + x) + 4, 4 * (ty0 + y0), 4 * (tx0 + x) + 4, 4 * (ty0 + y1)], 1))
            x, y0, y1 = _runs(w.T)
            out.append(np.stack([4 * (tx0 + x), 4 * (ty0 + y1), 4 * (tx0 + x), 4 * (ty0 + y0)], 1))
    return np.concatenate(out).astype(np.int32).reshape(-1, 4)


# ---- the kernels' arithmetic, tile by tile, in Python integers ---------------------------------------------------------------------
def _mask_runs(m):
    """the runs of a 64-bit mask as emit_runs walks them: starts m & ~(m << 1), lowest first; the length from the first zero of
    m >> a (64 when there is none) -> [(a, a + len)]"""
    st = m & ~(m << 1) & M64
    out = []
    while st:
        a = (st & -st).bit_length() - 1
        st &= st - 1
        r = ~(m >> a) & M64
        out.append((a, a + ((r & -r).bit_length() - 1 if r else 64)))
    return out


def tiled_outline(plane, cap=None):
    """outline_tile_kernel / outline_scan_kernel as they are written: per 64 x 64 tile the row masks S_y by 'ballots', the halo as
    two row masks and two column masks (zero outside the frame), N = S & ~up, S = S & ~dn, the transpose by 64 'ballots', E = C & ~rt,
    W = C & ~lf; count = popcount of the starts; the exclusive scan of the 4 counts per tile in 256 chunks; a record's index =
    the scanned count + the lane's exclusive prefix + its rank.  -> (info [total, written], records (written, 4))"""
    v = np.asarray(plane) != 0
    Hi, Wi = v.shape
    ntx, nty = (Wi + 63) // 64, (Hi + 63) // 64
    bit = lambda a: sum(1 << i for i, b in enumerate(a) if b)
    tiles, cnt = [], []
    for t in range(ntx * nty):
        ty0, tx0 = (t // ntx) * 64, (t % ntx) * 64
        th, tw = min(64, Hi - ty0), min(64, Wi - tx0)
        S = [bit(v[ty0 + y, tx0:tx0 + tw]) if y < th else 0 for y in range(64)]
        Sa = bit(v[ty0 - 1, tx0:tx0 + tw]) if ty0 > 0 else 0
        Sb = bit(v[ty0 + th, tx0:tx0 + tw]) if ty0 + th < Hi else 0
        Cl = bit(v[ty0:ty0 + th, tx0 - 1]) if tx0 > 0 else 0
        Cr = bit(v[ty0:ty0 + th, tx0 + tw]) if tx0 + tw < Wi else 0
        up = [Sa] + S[:63]
        dn = S[1:] + [Sb]
        mN = [S[y] & ~up[y] & M64 for y in range(64)]
        mS = [S[y] & ~dn[y] & M64 for y in range(64)]
        C = [sum(((S[y] >> x) & 1) << y for y in range(64)) for x in range(64)]
        lf = [Cl] + C[:63]
        rt = C[1:] + [Cr]
        mE = [C[x] & ~rt[x] & M64 for x in range(64)]
        mW = [C[x] & ~lf[x] & M64 for x in range(64)]
        masks = (mN, mS, mE, mW)
        tiles.append((ty0, tx0, masks))
        cnt += [sum(bin(m & ~(m << 1) & M64).count("1") for m in k) for k in masks]
    # the scan: 256 threads, a contiguous chunk each
    n = len(cnt)
    per = (n + 255) // 256
    sums = [sum(cnt[min(n, t * per):min(n, t * per + per)]) for t in range(256)]
    offs, at = list(cnt), 0
    for t in range(256):
        a = sum(sums[:t])
        assert a == at
        for i in range(min(n, t * per), min(n, t * per + per)):
            offs[i], at = at, at + cnt[i]
    total = at
    cap = total if cap is None else cap
    written = min(total, cap)
    rec = np.full((written, 4), -1, np.int64)
    for t, (ty0, tx0, masks) in enumerate(tiles):
        for k, lanes in enumerate(masks):
            pre = offs[4 * t + k]                    # + the lane's exclusive prefix of the popcounts
            for lane, m in enumerate(lanes):
                g, runs = pre, _mask_runs(m)
                pre += len(runs)
                f, t0 = 4 * ((ty0 if k < 2 else tx0) + lane), tx0 if k < 2 else ty0
                for a, b in runs:
                    if g >= cap:                     # (indices ascend within a lane)
                        break
                    p0, p1 = 4 * (t0 + a), 4 * (t0 + b)
                    rec[g] = [(p0, f, p1, f), (p1, f + 4, p0, f + 4), (f + 4, p0, f + 4, p1), (f, p1, f, p0)][k]
                    g += 1
    assert (rec >= 0).all()
    return [total, written], rec.astype(np.int32)


# ---- the rings, traced from the pixels ---------------------------------------------------------------------------------------------
def spec_rings(plane):
    """The outline's rings straight from the pixel set (no records, no tiles): every boundary side is ONE unit step between
    lattice corners, clockwise with the interior on its right; from the smallest corner in (y, x) order that still has a step
    -- the smallest corner of its ring, which only that ring's N side (a hole's: E side) still leaves -- steps are followed corner to corner, taking
    the RIGHT turn where two steps leave a corner (two selected pixels touching diagonally), until the corner is reached again;
    a corner is kept where the direction changes.  -> [[(x, y), ...], ...] in frame pixels, sorted by first corner"""
    sel = np.pad(np.asarray(plane) != 0, 1)
    nxt = {}                                         # corner (x, y) -> the directions (dx, dy) of the steps that leave it
    ys, xs = np.nonzero(sel)
    for y, x in zip(ys.tolist(), xs.tolist()):
        X, Y = x - 1, y - 1
        if not sel[y - 1, x]:
            nxt.setdefault((X, Y), []).append((1, 0))
        if not sel[y, x + 1]:
            nxt.setdefault((X + 1, Y), []).append((0, 1))
        if not sel[y + 1, x]:
            nxt.setdefault((X + 1, Y + 1), []).append((-1, 0))
        if not sel[y, x - 1]:
            nxt.setdefault((X, Y + 1), []).append((0, -1))
    rings = []
    for start in sorted(nxt, key=lambda c: (c[1], c[0])):
        if not nxt[start]:
            continue
        assert nxt[start] in ([(1, 0)], [(0, 1)])       # an outer ring leaves its smallest corner by an N side, a hole by an E side
        d, p, pts = nxt[start].pop(), start, [start]
        while True:
            p = (p[0] + d[0], p[1] + d[1])
            if p == start:
                break
            out = nxt[p]
            nd = next(t for t in ((-d[1], d[0]), d, (d[1], -d[0])) if t in out)      # right, straight, left
            out.remove(nd)
            if nd != d:
                pts.append(p)
            d = nd
        rings.append(pts)
    assert not any(nxt.values())
    return rings


def ring_area(ring):
    """the shoelace area with y down: positive for a clockwise ring on the screen"""
    return sum(x0 * y1 - x1 * y0 for (x0, y0), (x1, y1) in zip(ring, ring[1:] + ring[:1])) // 2


# ---- the test planes: each (Hi, Wi) -> (Hi,Wi) uint8 ----------------------------------------------------------------------------------
def empty(Hi, Wi):
    return np.zeros((Hi, Wi), np.uint8)


def full(Hi, Wi):
    return np.full((Hi, Wi), 255, np.uint8)


def checkerboard(Hi, Wi):
    y, x = np.mgrid[:Hi, :Wi]
    return np.where((y + x) % 2 == 0, 255, 0).astype(np.uint8)


def hstripes(Hi, Wi):
    return np.where((np.mgrid[:Hi, :Wi][0] // 3) % 2 == 0, 255, 0).astype(np.uint8)


def vstripes(Hi, Wi):
    return np.where((np.mgrid[:Hi, :Wi][1] // 5) % 2 == 1, 255, 0).astype(np.uint8)


def _dist2(Hi, Wi):
    y, x = np.mgrid[:Hi, :Wi]
    return (2 * y + 1 - Hi) ** 2 + (2 * x + 1 - Wi) ** 2, min(Hi, Wi) ** 2


def disc(Hi, Wi):
    d, m = _dist2(Hi, Wi)
    return np.where(d * 100 <= 81 * m, 255, 0).astype(np.uint8)


def annulus(Hi, Wi):
    d, m = _dist2(Hi, Wi)
    return np.where((d * 100 <= 90 * m) & (d * 100 >= 25 * m), 255, 0).astype(np.uint8)


def noise(Hi, Wi):
    """half the pixels selected, with every value 1 .. 255"""
    rng = np.random.RandomState(Hi * 1000 + Wi)
    return np.where(rng.rand(Hi, Wi) < 0.5, rng.randint(1, 256, (Hi, Wi)), 0).astype(np.uint8)


def corners(Hi, Wi):
    p = np.zeros((Hi, Wi), np.uint8)
    p[0, 0] = p[0, -1] = p[-1, 0] = p[-1, -1] = 255
    return p


def values(Hi, Wi):
    """0, 1, 7 and 255 in 3 x 3 blocks: only 0 is unselected"""
    y, x = np.mgrid[:Hi, :Wi]
    return np.array([0, 1, 7, 255], np.uint8)[((y // 3) + 2 * (x // 3)) % 4]


def tile_corners(Hi, Wi):
    """one selected pixel at each tile corner around (63, 63) / (64, 64) (those that lie in the frame)"""
    p = np.zeros((Hi, Wi), np.uint8)
    for y in (63, 64):
        for x in (63, 64):
            if y < Hi and x < Wi:
                p[y, x] = 255
    return p


def rect_60_70(Hi, Wi):
    """a solid rectangle over x = 60 .. 70, y = 60 .. 70, clipped to the frame: its runs are split at 64"""
    p = np.zeros((Hi, Wi), np.uint8)
    p[60:71, 60:71] = 255
    return p


PATTERNS = [empty, full, checkerboard, hstripes, vstripes, disc, annulus, noise, corners]
MORE_PATTERNS = [values, tile_corners, rect_60_70]
