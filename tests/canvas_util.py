"""The canvas of an editing session (include/sketchedit_canvas.h) restated in numpy: the eight orientations as
np.flip / np.rot90 / transpose, checked against the header's index formula; the fold of the three pad modes; the rectangle; and
lane-by-lane restatements of the two kernels of se_canvas.hip: canvas_turn tile by tile, saying which tiles take the LDS route and
counting the writers of every output byte, and canvas_map on a flat byte array whose every load is checked.  Host arithmetic only;
everything is exact."""
import numpy as np

MIRROR_X, MIRROR_Y, TRANSPOSE = 1, 2, 4
EDGE, REFLECT, CONSTANT = 0, 1, 2
MAX_SIDE, MAX_OFFSET = 32768, 1 << 20
ORIENTS = {None: 0, "h": 1, "v": 2, "180": 3, "transpose": 4, "ccw": 5, "cw": 6, "transverse": 7}
TURN_W, TURN_H = 32, 64                              # canvas_turn's tile: output columns, output rows


def _as3(img):
    a = np.asarray(img)
    return a[:, :, None] if a.ndim == 2 else a


def orient_formula(img, o):
    """the header's rule 1, index by index"""
    a3 = _as3(img)
    Hi, Wi = a3.shape[:2]
    Ho, Wo = (Wi, Hi) if o & TRANSPOSE else (Hi, Wi)
    out = np.empty((Ho, Wo, a3.shape[2]), a3.dtype)
    for y in range(Ho):
        for x in range(Wo):
            a, b = (x, y) if o & TRANSPOSE else (y, x)
            out[y, x] = a3[Hi - 1 - a if o & MIRROR_Y else a, Wi - 1 - b if o & MIRROR_X else b]
    return out if np.asarray(img).ndim == 3 else out[:, :, 0]


def orient(img, o):
    """the named orientations in numpy's own words"""
    a = np.asarray(img)
    if o == 0:
        r = a
    elif o == 1:
        r = np.flip(a, 1)
    elif o == 2:
        r = np.flip(a, 0)
    elif o == 3:
        r = np.rot90(a, 2)
    elif o == 4:
        r = a.transpose((1, 0) + tuple(range(2, a.ndim)))
    elif o == 5:
        r = np.rot90(a, 1)                           # counter-clockwise
    elif o == 6:
        r = np.rot90(a, -1)                          # clockwise
    elif o == 7:
        r = np.rot90(a, 2).transpose((1, 0) + tuple(range(2, a.ndim)))
    else:
        raise ValueError(o)
    return np.ascontiguousarray(r)


def fold(i, n, mode):
    """rule 3: the index of i in [0, n) -- None for a CONSTANT pixel"""
    if 0 <= i < n:
        return i
    if mode == EDGE:
        return min(max(i, 0), n - 1)
    if mode == CONSTANT:
        return None
    if n == 1:
        return 0
    p = 2 * n - 2
    j = i % p                                        # Python's modulus is the floor modulus
    return j if j < n else p - j


def fold_array(n, lo, count, mode):
    """fold of lo .. lo + count - 1 as an int array; -1 for a CONSTANT pixel"""
    return np.array([-1 if fold(i, n, mode) is None else fold(i, n, mode) for i in range(lo, lo + count)], np.int64)


def spec_canvas(img, hw, out_hw, origin, o, mode, rgb=0):
    """The statement.  img: (Hi,Wi) / (Hi,Wi,3) uint8, or None (a plane of zeros of size `hw`); -> (Hn,Wn[,3]) uint8.  rgb: the
    constant's colour as the entry takes it, byte c = (rgb >> 8 c) & 255"""
    Hi, Wi = hw
    plane = img is None or np.asarray(img).ndim == 2
    a = np.zeros((Hi, Wi), np.uint8) if img is None else np.asarray(img)
    assert a.shape[:2] == (Hi, Wi)
    O = _as3(orient(a, o))
    Ho, Wo, C = O.shape
    Hn, Wn = out_hw
    fy, fx = fold_array(Ho, origin[0], Hn, mode), fold_array(Wo, origin[1], Wn, mode)
    out = O[np.maximum(fy, 0)[:, None], np.maximum(fx, 0)[None, :]]
    colour = np.array([(rgb >> (8 * c)) & 255 for c in range(C)], np.uint8)
    out[(fy < 0)[:, None] | (fx < 0)[None, :]] = colour
    out = np.ascontiguousarray(out)
    return out[:, :, 0] if plane else out


def turn_routes(hw, out_hw, origin, o, has_input=True):
    """canvas_turn's tiles -> a (tiles_y, tiles_x) bool array: True where the tile takes the LDS route -- its rectangle is a plain
    rectangle of the oriented image"""
    assert o & TRANSPOSE
    Ho, Wo = hw[1], hw[0]
    Hn, Wn = out_hw
    ty, tx = (Hn + TURN_H - 1) // TURN_H, (Wn + TURN_W - 1) // TURN_W
    lds = np.zeros((ty, tx), bool)
    for j in range(ty):
        for i in range(tx):
            y0, x0 = j * TURN_H, i * TURN_W
            th, tw = min(TURN_H, Hn - y0), min(TURN_W, Wn - x0)
            lds[j, i] = (has_input and y0 + origin[0] >= 0 and y0 + th + origin[0] <= Ho and x0 + origin[1] >= 0
                         and x0 + tw + origin[1] <= Wo)
    return lds


def tiled_turn(img, hw, out_hw, origin, o, mode, rgb=0, misalign=0):
    """canvas_turn_kernel, tile by tile and lane by lane, on an output whose first byte lies `misalign` bytes past a 4-byte
    aligned address.  -> (out, writers, lds): the output, the number of stores that hit each of its bytes (a (C Hn Wn,) array),
    and turn_routes' array"""
    Hi, Wi = hw
    a = None if img is None else _as3(img)
    C = 1 if a is None else a.shape[2]
    Ho, Wo = Wi, Hi
    Hn, Wn = out_hw
    oy, ox = origin
    colour = [(rgb >> (8 * c)) & 255 for c in range(C)]
    flat = np.zeros(misalign + C * Hn * Wn + 8, np.uint8)               # the aligned dwords around the output
    writers = np.zeros(flat.shape, np.int64)

    def src(Y, X):
        if a is None:
            return [0] * C
        aa, bb = X, Y                                                    # the transpose
        return list(a[Hi - 1 - aa if o & MIRROR_Y else aa, Wi - 1 - bb if o & MIRROR_X else bb])

    def px(y, x):
        fy, fx = fold(y + oy, Ho, mode), fold(x + ox, Wo, mode)
        if fy is None or fx is None:
            return colour
        return src(fy, fx)

    lds = turn_routes(hw, out_hw, origin, o, a is not None)
    for j in range(lds.shape[0]):
        for i in range(lds.shape[1]):
            y0, x0 = j * TURN_H, i * TURN_W
            th, tw = min(TURN_H, Hn - y0), min(TURN_W, Wn - x0)
            s_px = {}
            if lds[j, i]:
                for t in range(TURN_W * TURN_H):
                    xl, yl = t >> 6, t & 63
                    if xl < tw and yl < th:
                        s_px[xl, yl] = src(y0 + yl + oy, x0 + xl + ox)
            ln = tw * C
            for t in range(TURN_H * 32):
                yl, k = t >> 5, t & 31
                if yl >= th:
                    break
                s0 = ((y0 + yl) * Wn + x0) * C
                m = (misalign + s0) & 3
                if 4 * k >= m + ln:
                    continue
                for e in range(4):
                    s = 4 * k + e - m
                    if s < 0 or s >= ln:
                        continue
                    xl, c = divmod(s, C)
                    pv = s_px[xl, yl] if lds[j, i] else px(y0 + yl, x0 + xl)
                    at = misalign + s0 - m + 4 * k + e
                    flat[at] = pv[c]
                    writers[at] += 1
    n = C * Hn * Wn
    assert not writers[:misalign].any() and not writers[misalign + n:].any()
    out = flat[misalign:misalign + n].reshape((Hn, Wn, C))
    return (out[:, :, 0] if a is None or np.asarray(img).ndim == 2 else out), writers[misalign:misalign + n], lds


def tiled_map(mem, ia, hw, C, oa, out_hw, origin, o, mode, rgb=0):
    """canvas_map_kernel, lane by lane, on a move_util.Memory whose every load is checked against the source row it may touch:
    the input at address `ia` (None: the NULL input), the output at `oa`.  -> the number of lanes that took the fast route"""
    assert not o & TRANSPOSE
    Hi, Wi = hw
    Hn, Wn = out_hw
    oy, ox = origin
    n, rb, mis = C * Hn * Wn, C * Wn, oa & 3
    colour = [(rgb >> (8 * c)) & 255 for c in range(C)]
    fast = 0

    def px(y, x, c):
        fy, fx = fold(y + oy, Hi, mode), fold(x + ox, Wi, mode)
        if fy is None or fx is None:
            return colour[c]
        if ia is None:
            return 0
        sy, sx = Hi - 1 - fy if o & MIRROR_Y else fy, Wi - 1 - fx if o & MIRROR_X else fx
        return int(mem.mem[ia + (sy * Wi + sx) * C + c])

    for q in range((n + mis + 3) // 4):
        p0 = 4 * q - mis
        first, last = max(p0, 0), min(p0 + 3, n - 1)
        y, b = divmod(first, rb)
        k, sh = last - first, 8 * (first - p0)
        xa, xb, Y = b // C, (b + k) // C, y + oy
        v = 0
        if ia is not None and b + k < rb and 0 <= Y < Hi and xa + ox >= 0 and xb + ox < Wi:
            fast += 1
            sy = Hi - 1 - Y if o & MIRROR_Y else Y
            row = ia + sy * Wi * C
            hi = row + Wi * C
            if not o & MIRROR_X:
                v = mem.load4_within(row + (xa + ox) * C + (b - xa * C), row, hi) << sh
            elif C == 1:
                sx = Wi - 1 - (xa + ox)
                v = int.from_bytes(mem.load4_within(row + sx - 3, row, hi).to_bytes(4, "little"), "big") << sh
            else:
                sx = Wi - 1 - (xa + ox)
                a = row + 3 * (sx - 1)
                w = mem.load4_within(a, row, hi) | mem.load4_within(a + 4, row, hi) << 32
                for j in range(k + 1):
                    x, c = divmod(b + j, 3)
                    v |= ((w >> (8 * ((3 if x == xa else 0) + c))) & 255) << (sh + 8 * j)
        else:
            for p in range(first, last + 1):
                py, pb = divmod(p, rb)
                x, c = divmod(pb, C)
                v |= px(py, x, c) << (8 * (p - p0))
        for e in range(4):                                                 # store_plane_dword: the bytes inside [0, n) only
            if 0 <= p0 + e < n:
                mem.mem[oa + p0 + e] = (v >> (8 * e)) & 255
    return fast


# ---- the cases of the tests: sizes, rectangles -------------------------------------------------------------------------------------------
SIZES = [(1, 70), (70, 1), (3, 5), (16, 16), (37, 53), (64, 64), (65, 129), (130, 70), (200, 150)]


def rects(oriented_hw):
    """the rectangles (y0, x0, h, w) every size is tried with, in oriented coordinates: identity, a crop to 1 x 1, an interior crop at
    an odd origin, an extension by 1, one by more than the side on each edge, a mix of crop and extension, one wholly in the pad area"""
    Ho, Wo = oriented_hw
    return [(0, 0, Ho, Wo), (Ho // 2, Wo // 3, 1, 1), (min(1, Ho - 1), min(3, Wo - 1), max(1, Ho - 2), max(1, Wo - 5)),
            (-1, -1, Ho + 2, Wo + 2), (-Ho - 3, -Wo - 2, 3 * Ho + 5, 3 * Wo + 7), (Ho // 2, -5, Ho, Wo + 2), (Ho + 3, -Wo - 9, 7, 6)]
