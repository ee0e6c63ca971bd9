"""The statement of DESIGN.md 6s (include/sketchedit_warp.h) in plain numpy, restated independently of sketchedit_amd.serve: the
drop of a lifted selection through an inverse affine map in Q16 with bilinear taps, the warp of its plane, the map a scale /
angle / offset / flip makes and the rectangle it lands in; and se_warp.hip's arithmetic lane by lane on checked memory."""
from fractions import Fraction
import math

import numpy as np

from move_util import Memory, slot_of, box_of  # noqa: F401  (the slot layout and the checked memory are 6r's)

MAX_COEF, MAX_TRANSLATION = 1 << 20, 1 << 40
ONE = 65536


def _taps(sel, box, m, ys, xs):
    """rules 1 .. 3 for the destination pixels ys x xs -> (a, [(ws, ty, tx)] * 4): the coverage and per tap its weight times s
    and its source pixel, clipped into the box where the tap does not count"""
    by0, bx0, by1, bx1 = box
    ayy, ayx, ay0, axy, axx, ax0 = (int(v) for v in m)
    Y, X = np.asarray(ys, np.int64)[:, None], np.asarray(xs, np.int64)[None, :]
    sy, sx = ayy * Y + ayx * X + ay0, axy * Y + axx * X + ax0
    iy, ix, fy, fx = sy >> 16, sx >> 16, (sy >> 8) & 255, (sx >> 8) & 255
    a, taps = np.zeros(sy.shape, np.int64), []
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        w = (fy if dy else 256 - fy) * (fx if dx else 256 - fx)
        ty, tx = iy + dy, ix + dx
        inbox = (ty >= by0) & (ty < by1) & (tx >= bx0) & (tx < bx1)
        cy, cx = np.clip(ty, by0, by1 - 1), np.clip(tx, bx0, bx1 - 1)
        ws = np.where(inbox & (np.asarray(sel)[cy, cx] != 0), w, 0)
        a += ws
        taps.append((ws, cy, cx))
    assert a.min() >= 0 and a.max() <= ONE
    return a, taps


def coverage(sel, box, m):
    """a(p) of rule 3 for every pixel of the frame"""
    Hi, Wi = sel.shape
    return _taps(sel, box, m, np.arange(Hi), np.arange(Wi))[0]


def spec_warp(sel, box, m):
    """rule 7: the (Hi,Wi) plane of 0 / 255, half coverage"""
    return np.where(coverage(sel, box, m) >= ONE // 2, np.uint8(255), np.uint8(0))


def spec_drop(frame, lift, lift_rect, sel, lock, box, rect, m):
    """rules 1 .. 6 -> the new frame (the arguments are only read)"""
    Hi, Wi = sel.shape
    ly0, lx0, lh, lw = lift_rect
    by0, bx0, by1, bx1 = box
    ry0, rx0, rh, rw = rect
    assert ly0 <= by0 < by1 <= ly0 + lh and lx0 <= bx0 < bx1 <= lx0 + lw
    assert 0 <= ry0 and 0 <= rx0 and rh > 0 and rw > 0 and ry0 + rh <= Hi and rx0 + rw <= Wi
    assert all(abs(int(v)) <= MAX_COEF for v in (m[0], m[1], m[3], m[4])) and all(abs(int(v)) <= MAX_TRANSLATION for v in (m[2], m[5]))
    a, taps = _taps(sel, box, m, np.arange(Hi), np.arange(Wi))
    P = np.asarray(lift)[:, :3 * lw].reshape(lh, lw, 3).astype(np.int64)
    acc = np.zeros((Hi, Wi, 3), np.int64)
    for ws, cy, cx in taps:
        acc += ws[..., None] * P[cy - ly0, cx - lx0]
    blend = acc + (ONE - a)[..., None] * np.asarray(frame).astype(np.int64) + ONE // 2
    assert blend.max() < 1 << 31
    target = a > 0
    inr = np.zeros((Hi, Wi), bool)
    inr[ry0:ry0 + rh, rx0:rx0 + rw] = True
    target &= inr
    if lock is not None:
        target &= np.asarray(lock) == 0
    out = np.array(frame)
    out[target] = (blend[target] >> 16).astype(np.uint8)
    return out


# ---- the host's map and rectangle --------------------------------------------------------------------------------------------------
def warp_matrix(box, scale, angle, offset, flip):
    """the inverse map of: turn the object by `angle` degrees (counter-clockwise on the screen) about the box's centre, scale it
    by `scale` = s or (sy, sx), mirror it by `flip` (bit 0: x, bit 1: y), put the centre `offset` = (dy, dx) away"""
    by0, bx0, by1, bx1 = box
    sy, sx = scale if isinstance(scale, tuple) else (scale, scale)
    q = angle % 360
    if q % 90 == 0:
        cos, sin = ((1, 0), (0, 1), (-1, 0), (0, -1))[int(q // 90)]
    else:
        cos, sin = math.cos(math.radians(angle)), math.sin(math.radians(angle))
    fy, fx = (-1 if flip & 2 else 1), (-1 if flip & 1 else 1)
    ayy, ayx = round(fy * (1.0 / sy) * cos * ONE), round(fy * (1.0 / sy) * sin * ONE)
    axy, axx = round(fx * (1.0 / sx) * -sin * ONE), round(fx * (1.0 / sx) * cos * ONE)
    cy2, cx2 = by0 + by1 - 1, bx0 + bx1 - 1
    dy2, dx2 = cy2 + round(2 * offset[0]), cx2 + round(2 * offset[1])
    return (ayy, ayx, (cy2 * ONE - (ayy * dy2 + ayx * dx2)) >> 1, axy, axx, (cx2 * ONE - (axy * dy2 + axx * dx2)) >> 1)


def warp_rect(box, m, frame_hw):
    """the rectangle that holds every pixel with a > 0: the forward image of the corners of [by0 - 1, by1] x [bx0 - 1, bx1],
    floor of its minimum to ceil of its maximum, clipped to the frame, sides widened to 16 as move_rect widens them"""
    by0, bx0, by1, bx1 = box
    ayy, ayx, ay0, axy, axx, ax0 = m
    det = ayy * axx - ayx * axy
    if det == 0:
        raise ValueError("singular")
    pys, pxs = [], []
    for qy in (by0 - 1, by1):
        for qx in (bx0 - 1, bx1):
            u, v = qy * ONE - ay0, qx * ONE - ax0
            pys.append(Fraction(axx * u - ayx * v, det))
            pxs.append(Fraction(ayy * v - axy * u, det))
    out = []
    for ps, extent in ((pys, frame_hw[0]), (pxs, frame_hw[1])):
        lo, hi = max(math.floor(min(ps)), 0), min(math.ceil(max(ps)) + 1, extent)
        if hi <= lo:
            return None
        side = hi - lo
        if side < 16:
            lo -= (16 - side) // 2
            if lo < 0:
                lo = 0
            if lo + 16 > extent:
                lo = extent - 16
            side = 16
        out.append((lo, side))
    return out[0][0], out[1][0], out[0][1], out[1][1]


# ---- the kernels' arithmetic (se_warp.hip), lane by lane on ONE flat byte array with every access checked ---------------------------
def _i32(v):
    assert -(1 << 31) <= v < 1 << 31, v
    return v


def _lane_taps(mem, sel, Wi, box, sy, sx):
    """warp_taps: -> (a, iy, ix, xlo, xhi, [w00, w01, w10, w11] each times s) for the source position (sy, sx), or None when no
    tap can count; S is read through load4_within bounded by the box's pixels of the row that the taps with weight touch"""
    by0, bx0, by1, bx1 = box
    iy, ix = sy >> 16, sx >> 16
    if iy + 1 < by0 or iy >= by1 or ix + 1 < bx0 or ix >= bx1:
        return None
    fy, fx = (sy >> 8) & 255, (sx >> 8) & 255
    xlo, xhi = max(ix, bx0), min(ix + (2 if fx else 1), bx1)
    if xlo >= xhi:
        return None
    w, a = [0, 0, 0, 0], 0
    for r in (0, 1):
        yy, wy = iy + r, (fy if r else 256 - fy)
        if wy == 0 or yy < by0 or yy >= by1:
            continue
        row = sel + yy * Wi
        u = mem.load4_within(row + ix, row + xlo, row + xhi)
        w[2 * r] = wy * (256 - fx) if u & 255 else 0
        w[2 * r + 1] = wy * fx if (u >> 8) & 255 else 0
        a += w[2 * r] + w[2 * r + 1]
    return a, iy, ix, xlo, xhi, w


def tiled_drop(mem, frame, Hi, Wi, lift, lift_rect, sel, lock, box, rect, m):
    """warp_drop_kernel on `mem`, addresses for pointers: the tiles of R, the tile's corners in int64 and its early return, each
    lane's int32 delta, taps, blend and byte stores.  -> (tiles launched, tiles that returned before any load)"""
    ly0, lx0, lh, lw = lift_rect
    lpitch = (3 * lw + 15) // 16 * 16
    by0, bx0, by1, bx1 = box
    ry0, rx0, rh, rw = rect
    ry1, rx1 = ry0 + rh, rx0 + rw
    ayy, ayx, ay0, axy, axx, ax0 = (int(v) for v in m)
    tiles = early = 0
    for ty0 in range(ry0, ry1, 16):
        for tx0 in range(rx0, rx1, 64):
            tiles += 1
            by, bx = ayy * ty0 + ayx * tx0 + ay0, axy * ty0 + axx * tx0 + ax0            # int64, once per tile
            assert abs(by) < 1 << 62 and abs(bx) < 1 << 62
            cys = [by + _i32(ayy * cy + ayx * cx) for cy in (0, 15) for cx in (0, 63)]
            cxs = [bx + _i32(axy * cy + axx * cx) for cy in (0, 15) for cx in (0, 63)]
            if (max(cys) >> 16) + 1 < by0 or (min(cys) >> 16) >= by1 or (max(cxs) >> 16) + 1 < bx0 or (min(cxs) >> 16) >= bx1:
                early += 1
                continue
            for tid in range(256):
                lx = tid & 63
                x = tx0 + lx
                if x >= rx1:
                    continue
                for k in range(4):
                    ly = (tid >> 6) + 4 * k
                    y = ty0 + ly
                    if y >= ry1:
                        continue
                    t = _lane_taps(mem, sel, Wi, box, by + _i32(ayy * ly + ayx * lx), bx + _i32(axy * ly + axx * lx))
                    if t is None or t[0] == 0:
                        continue
                    a, iy, ix, xlo, xhi, w = t
                    if lock is not None:
                        la = lock + y * Wi + x
                        if mem.load4_within(la, la, la + 1) & 255:
                            continue
                    acc = [0, 0, 0]
                    for r in (0, 1):
                        if not (w[2 * r] or w[2 * r + 1]):
                            continue
                        yy = iy + r
                        assert ly0 <= yy < ly0 + lh and lx0 <= xlo and xhi <= lx0 + lw
                        prow = lift + (yy - ly0) * lpitch
                        addr, lo, hi = prow + 3 * (ix - lx0), prow + 3 * (xlo - lx0), prow + 3 * (xhi - lx0)
                        assert prow <= lo and hi <= prow + 3 * lw
                        u = mem.load4_within(addr, lo, hi) | (mem.load4_within(addr + 4, lo, hi) << 32)
                        for ch in range(3):
                            acc[ch] += w[2 * r] * ((u >> (8 * ch)) & 255) + w[2 * r + 1] * ((u >> (8 * (3 + ch))) & 255)
                    dst = frame + (y * Wi + x) * 3
                    assert frame <= dst and dst + 3 <= frame + 3 * Hi * Wi
                    for ch in range(3):
                        v = acc[ch] + 32768
                        if a < ONE:
                            v += (ONE - a) * int(mem.mem[dst + ch])
                        assert v < 1 << 31
                        mem.mem[dst + ch] = v >> 16
    return tiles, early


def tiled_warp(mem, sel, Hi, Wi, box, m, out):
    """plane_warp_kernel on `mem`: one lane per aligned dword of the output, single bytes at the plane's two ends"""
    ayy, ayx, ay0, axy, axx, ax0 = (int(v) for v in m)
    n, mis = Hi * Wi, out & 3
    for q in range((n + mis + 3) // 4):
        p0 = 4 * q - mis
        v = 0
        for e in range(4):
            p = p0 + e
            if not 0 <= p < n:
                continue
            y, x = divmod(p, Wi)
            t = _lane_taps(mem, sel, Wi, box, ayy * y + ayx * x + ay0, axy * y + axx * x + ax0)
            if t is not None and t[0] >= ONE // 2:
                v |= 255 << (8 * e)
        for e in range(4):
            if 0 <= p0 + e < n:
                mem.mem[out + p0 + e] = (v >> (8 * e)) & 255
