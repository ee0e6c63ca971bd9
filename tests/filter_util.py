"""The statement of DESIGN.md 6t (include/sketchedit_filter.h) in plain numpy, restated independently of sketchedit_amd.serve: the
blur, unsharp mask and mosaic of a lifted selection, the taps and the rectangle a filter lifts; and the kernels' arithmetic
(se_filter.hip) lane by lane on move_util.Memory with every access checked against the span it may touch."""
import math

import numpy as np

import move_util
from move_util import slot_of  # noqa: F401  (the tests build their lifts with it)

ONE, MAX_RADIUS, MAX_CELL, MIN_AMOUNT, MAX_AMOUNT, MAX_FEATHER = 4096, 32, 64, -256, 1024, 16


def taps(kind, radius, sigma=None):
    """[t0 .. tR]: gauss -- floor(4096 w_k / sum + 0.5) for k >= 1, sigma = max(R / 3, 0.5) unless given; box -- 4096 // (2R + 1);
    t0 is the rest"""
    R = int(radius)
    if kind == "box":
        t = [ONE // (2 * R + 1)] * R
    else:
        s = max(R / 3.0, 0.5) if sigma is None else float(sigma)
        w = [math.exp(-k * k / (2.0 * s * s)) for k in range(R + 1)]
        tot = w[0] + 2.0 * sum(w[1:])
        t = [int(math.floor(ONE * w[k] / tot + 0.5)) for k in range(1, R + 1)]
    return [ONE - 2 * sum(t)] + t


def filter_rect(box, radius, frame_hw):
    """the box grown by the radius, clipped to the frame, sides widened to 16 as move_rect widens them"""
    return move_util.move_rect((box[0] - radius, box[1] - radius, box[2] + radius, box[3] + radius), (0, 0), frame_hw)


def _lifted(lift, lift_rect):
    _, _, lh, lw = lift_rect
    return np.asarray(lift)[:, :3 * lw].reshape(lh, lw, 3).astype(np.int64)


def blurred(lift, lift_rect, box, t, frame_hw):
    """B of the box's pixels, (bh, bw, 3) int64: the two passes, every tap asserted to lie in the lift"""
    Hi, Wi = frame_hw
    ly0, lx0, lh, lw = lift_rect
    by0, bx0, by1, bx1 = box
    R = len(t) - 1
    assert 1 <= R <= MAX_RADIUS and min(t) >= 0 and t[0] + 2 * sum(t[1:]) == ONE
    yy = np.clip(np.arange(by0 - R, by1 + R), 0, Hi - 1) - ly0
    xx = np.clip(np.arange(bx0 - R, bx1 + R), 0, Wi - 1) - lx0
    assert 0 <= yy.min() and yy.max() < lh and 0 <= xx.min() and xx.max() < lw
    N = _lifted(lift, lift_rect)[yy][:, xx]
    bh, bw = by1 - by0, bx1 - bx0
    full = [int(t[abs(k)]) for k in range(-R, R + 1)]
    H = sum(full[j] * N[:, j:j + bw] for j in range(2 * R + 1))
    assert H.max() <= 255 * ONE
    V = sum(full[j] * H[j:j + bh] for j in range(2 * R + 1))
    assert V.max() + (1 << 23) < 1 << 32                      # fits UNSIGNED 32 bits (and not signed ones at 255)
    return (V + (1 << 23)) >> 24


def mosaicked(lift, lift_rect, box, cell):
    """B of the box's pixels for the mosaic: (sum + cnt // 2) // cnt over every clipped cell, anchored at the box's origin"""
    ly0, lx0, _, _ = lift_rect
    by0, bx0, by1, bx1 = box
    assert 2 <= cell <= MAX_CELL
    P = _lifted(lift, lift_rect)[by0 - ly0:by1 - ly0, bx0 - lx0:bx1 - lx0]
    B = np.zeros_like(P)
    for y in range(0, by1 - by0, cell):
        for x in range(0, bx1 - bx0, cell):
            blk = P[y:y + cell, x:x + cell]
            cnt = blk.shape[0] * blk.shape[1]
            B[y:y + cell, x:x + cell] = (blk.reshape(cnt, 3).sum(axis=0) + cnt // 2) // cnt
    return B


def counts(sel, box, f):
    """c(p) of the box's pixels: S != 0 inside the box within f, the box's outside counting as 0"""
    by0, bx0, by1, bx1 = box
    m = np.pad((np.asarray(sel)[by0:by1, bx0:bx1] != 0).astype(np.int64), f)
    rows = sum(m[e:e + by1 - by0] for e in range(2 * f + 1))
    return sum(rows[:, e:e + bx1 - bx0] for e in range(2 * f + 1))


def mixed(P, B, amount):
    """O = clamp(P + ((a (P - B) + 128) >> 8), 0, 255)"""
    return np.clip(P + ((int(amount) * (P - B) + 128) >> 8), 0, 255)


def _finish(frame, lift, lift_rect, sel, lock, box, B, amount, f):
    assert MIN_AMOUNT <= amount <= MAX_AMOUNT and 0 <= f <= MAX_FEATHER
    ly0, lx0, lh, lw = lift_rect
    by0, bx0, by1, bx1 = box
    assert ly0 <= by0 < by1 <= ly0 + lh and lx0 <= bx0 < bx1 <= lx0 + lw
    P = _lifted(lift, lift_rect)[by0 - ly0:by1 - ly0, bx0 - lx0:bx1 - lx0]
    O = mixed(P, B, amount)
    target = np.asarray(sel)[by0:by1, bx0:bx1] != 0
    if lock is not None:
        target &= np.asarray(lock)[by0:by1, bx0:bx1] == 0
    n = (2 * f + 1) ** 2
    c = counts(sel, box, f)[..., None]
    blend = (c * O + (n - c) * P + (n - 1) // 2) // n
    out = np.array(frame)
    view = out[by0:by1, bx0:bx1]
    view[target] = blend[target].astype(np.uint8)
    return out


def spec_blur(frame, lift, lift_rect, sel, lock, box, t, amount=-256, f=0):
    """the rule for BLUR -> the new frame (the arguments are only read; the frame's own bytes play no part in what is stored)"""
    B = blurred(lift, lift_rect, box, [int(v) for v in t], np.asarray(sel).shape)
    return _finish(frame, lift, lift_rect, sel, lock, box, B, amount, f)


def spec_mosaic(frame, lift, lift_rect, sel, lock, box, cell, amount=-256, f=0):
    """the rule for MOSAIC -> the new frame"""
    return _finish(frame, lift, lift_rect, sel, lock, box, mosaicked(lift, lift_rect, box, cell), amount, f)


# ---- the kernels' arithmetic (se_filter.hip), lane by lane on ONE flat byte array with every access checked -------------------------
class Memory(move_util.Memory):
    """move_util.Memory that remembers the first byte that every load really read"""

    def __init__(self, size, fill=0xA5):
        super().__init__(size, fill)
        self.log = []

    def dword_within(self, p, lo, hi):
        if max(p, lo) < min(p + 4, hi):
            self.log.append(max(p, lo))
        if lo <= p and p + 4 <= hi:
            return int.from_bytes(self.mem[p:p + 4].tobytes(), "little")
        return super().dword_within(p, lo, hi)

    def byte(self, a, lo, hi):
        assert lo <= a < hi, (a, lo, hi)
        self.log.append(a)
        return int(self.mem[a])


def _only(mem, mark, spans):
    """every load since `mark` lies in one of `spans`"""
    return all(any(lo <= a < hi for lo, hi in spans) for a in mem.log[mark:])


def _sel4_in_box(mem, sel, Wi, box, y, x):
    by0, bx0, by1, bx1 = box
    if y < by0 or y >= by1 or x + 3 < bx0 or x >= bx1:
        return [0] * 4
    row = sel + y * Wi
    u = mem.load4_within(row + x, row + bx0, row + bx1)
    return [1 if (u >> (8 * p)) & 255 else 0 for p in range(4)]


def _blend(P, O, cp, n):
    if cp == n:
        return O
    v = cp * O + (n - cp) * P + (n - 1) // 2
    assert v < 1 << 19
    return (v * (((1 << 32) // n + 1) & 0xffffffff)) >> 32


def _mix(P, B, a):
    return min(max(P + ((a * (P - B) + 128) >> 8), 0), 255)


def tiled_blur(mem, frame, Hi, Wi, lift, lift_rect, sel, lock, box, t, amount, f):
    """filter_blur_kernel on `mem`, addresses for pointers: the box's tiles, each tile's select / stage / rows / blend.  Loads are
    bounded as the kernel bounds them and asserted to stay in the plane, the first 3 lw bytes of a slot row or -- never -- the
    frame; stores are asserted to lie in the box's row of the frame.  -> (tiles, tiles that returned having loaded S only,
    tiles that returned having loaded S and L only)"""
    ly0, lx0, lh, lw = lift_rect
    lpitch = (3 * lw + 15) // 16 * 16
    by0, bx0, by1, bx1 = box
    t = [int(v) for v in t]
    R, n = len(t) - 1, (2 * f + 1) ** 2
    S_span, L_span = (sel, sel + Hi * Wi), (lock, lock + Hi * Wi) if lock is not None else (0, 0)
    tiles = early_s = early_l = 0
    for ty0 in range(by0, by1, 16):
        for tx0 in range(bx0, bx1, 64):
            tiles += 1
            tx1, ty1 = min(tx0 + 64, bx1), min(ty0 + 16, by1)
            tw, th = tx1 - tx0, ty1 - ty0
            mark = len(mem.log)
            # ---- select
            tg = {}
            for ly in range(th):
                for lx in range(0, tw, 4):
                    npx = min(4, tw - lx)
                    a = sel + (ty0 + ly) * Wi + tx0 + lx
                    assert S_span[0] <= a and a + npx <= S_span[1]
                    u = mem.load4_within(a, a, a + npx)
                    tg[ly, lx] = [1 if (u >> (8 * p)) & 255 else 0 for p in range(4)]
            if not any(any(g) for g in tg.values()):
                early_s += 1
                assert _only(mem, mark, [S_span])
                continue
            if lock is not None:
                for (ly, lx), g in tg.items():
                    if any(g):
                        npx = min(4, tw - lx)
                        a = lock + (ty0 + ly) * Wi + tx0 + lx
                        assert L_span[0] <= a and a + npx <= L_span[1]
                        u = mem.load4_within(a, a, a + npx)
                        tg[ly, lx] = [g[p] if not (u >> (8 * p)) & 255 else 0 for p in range(4)]
                if not any(any(g) for g in tg.values()):
                    early_l += 1
                    assert _only(mem, mark, [S_span, L_span])
                    continue
            # ---- stage
            rows, cols = th + 2 * R, tw + 2 * R
            st = np.zeros((rows, 3 * cols), np.int64)
            xa, xb = max(tx0 - R, 0), min(tx1 + R, Wi)
            run = 3 * (xb - xa)
            nl, jr = xa - (tx0 - R), xb - (tx0 - R)
            for i in range(rows):
                fy = min(max(ty0 - R + i, 0), Hi - 1)
                assert ly0 <= fy < ly0 + lh
                prow = lift + (fy - ly0) * lpitch
                src = prow + 3 * (xa - lx0)
                assert prow <= src and src + run <= prow + 3 * lw
                for q in range((run + 3) >> 2):
                    v = mem.load4_within(src + 4 * q, src, src + run)
                    for e in range(min(4, run - 4 * q)):
                        st[i, 3 * nl + 4 * q + e] = (v >> (8 * e)) & 255
                for jc in range(nl + cols - jr):
                    j, cx = (jc, 0) if jc < nl else (jr + jc - nl, Wi - 1)
                    for ch in range(3):
                        st[i, 3 * j + ch] = mem.byte(prow + 3 * (cx - lx0) + ch, prow, prow + 3 * lw)
            if f:
                cols4 = (64 + 2 * f + 3) >> 2
                fs = np.zeros((16 + 2 * f, 4 * cols4), np.int64)
                for i in range(16 + 2 * f):
                    for j4 in range(cols4):
                        fs[i, 4 * j4:4 * j4 + 4] = _sel4_in_box(mem, sel, Wi, box, ty0 - f + i, tx0 - f + 4 * j4)
                frow = np.stack([fs[:, k:k + 2 * f + 1].sum(axis=1) for k in range(64)], axis=1)
            assert _only(mem, mark, [S_span, L_span, (lift, lift + lh * lpitch)])
            # ---- rows
            Hs = t[0] * st[:, 3 * R:3 * R + 3 * tw]
            for k in range(1, R + 1):
                Hs = Hs + t[k] * (st[:, 3 * (R - k):3 * (R - k) + 3 * tw] + st[:, 3 * (R + k):3 * (R + k) + 3 * tw])
            # ---- blend
            for (ly, lx), g in tg.items():
                if not any(g):
                    continue
                y, x = ty0 + ly, tx0 + lx
                w12 = min(12, 3 * (tw - lx))
                acc = t[0] * Hs[ly + R, 3 * lx:3 * lx + w12]
                for k in range(1, R + 1):
                    acc = acc + t[k] * (Hs[ly + R - k, 3 * lx:3 * lx + w12] + Hs[ly + R + k, 3 * lx:3 * lx + w12])
                assert acc.max() + (1 << 23) < 1 << 32
                c = [int(frow[ly:ly + 2 * f + 1, lx + p].sum()) for p in range(4)] if f else [n] * 4
                brow = frame + (y * Wi + bx0) * 3
                dst = frame + (y * Wi + x) * 3
                for p in range(4):
                    if g[p]:
                        assert brow <= dst + 3 * p and dst + 3 * p + 3 <= brow + 3 * (bx1 - bx0) and 1 <= c[p] <= n
                        for ch in range(3):
                            P = int(st[ly + R, 3 * (lx + R) + 3 * p + ch])
                            B = (int(acc[3 * p + ch]) + (1 << 23)) >> 24
                            mem.mem[dst + 3 * p + ch] = _blend(P, _mix(P, B, amount), c[p], n)
    return tiles, early_s, early_l


def tiled_mosaic(mem, frame, Hi, Wi, lift, lift_rect, sel, lock, box, cell, amount, f):
    """filter_mosaic_kernel on `mem`: a wave per cell, its lanes striding over the cell's pixels.  -> (cells, cells that returned
    having loaded S and L only)"""
    ly0, lx0, lh, lw = lift_rect
    lpitch = (3 * lw + 15) // 16 * 16
    by0, bx0, by1, bx1 = box
    n = (2 * f + 1) ** 2
    S_span, L_span = (sel, sel + Hi * Wi), (lock, lock + Hi * Wi) if lock is not None else (0, 0)
    ncx, ncy = -(-(bx1 - bx0) // cell), -(-(by1 - by0) // cell)
    early = 0
    for q in range(ncx * ncy):
        y0, x0 = by0 + q // ncx * cell, bx0 + q % ncx * cell
        cw = min(cell, bx1 - x0)
        cnt = min(cell, by1 - y0) * cw
        assert cnt <= 4096
        mark = len(mem.log)
        mine = [0] * 64
        for lane in range(min(64, cnt)):
            for it, idx in enumerate(range(lane, cnt, 64)):
                at = (y0 + idx // cw) * Wi + x0 + idx % cw
                if mem.byte(sel + at, *S_span) and not (lock is not None and mem.byte(lock + at, *L_span)):
                    mine[lane] |= 1 << it
        if not any(mine):
            early += 1
            assert _only(mem, mark, [S_span, L_span])
            continue
        s = np.zeros((64, 3), np.int64)
        for lane in range(min(64, cnt)):
            for idx in range(lane, cnt, 64):
                py, px = y0 + idx // cw, x0 + idx % cw
                prow = lift + (py - ly0) * lpitch
                assert ly0 <= py < ly0 + lh
                for ch in range(3):
                    s[lane, ch] += mem.byte(prow + 3 * (px - lx0) + ch, prow, prow + 3 * lw)
        tot = s.sum(axis=0)
        assert tot.max() <= 4096 * 255
        B = [(int(v) + cnt // 2) // cnt for v in tot]
        for lane in range(min(64, cnt)):
            for it, idx in enumerate(range(lane, cnt, 64)):
                if not (mine[lane] >> it) & 1:
                    continue
                py, px = y0 + idx // cw, x0 + idx % cw
                cp = n
                if f:
                    ya, yb, xa, xb = max(py - f, by0), min(py + f + 1, by1), max(px - f, bx0), min(px + f + 1, bx1)
                    cp = 0
                    for yy in range(ya, yb):                # the kernel's byte loads of [row + xa, row + xb), a row at a time
                        row = sel + yy * Wi
                        assert S_span[0] <= row + xa and row + xb <= S_span[1]
                        cp += int(np.count_nonzero(mem.mem[row + xa:row + xb]))
                    assert 1 <= cp <= n
                prow = lift + (py - ly0) * lpitch
                dst = frame + (py * Wi + px) * 3
                assert frame + (py * Wi + bx0) * 3 <= dst and dst + 3 <= frame + (py * Wi + bx1) * 3
                for ch in range(3):
                    P = mem.byte(prow + 3 * (px - lx0) + ch, prow, prow + 3 * lw)
                    mem.mem[dst + ch] = _blend(P, _mix(P, B[ch], amount), cp, n)
    return ncx * ncy, early
