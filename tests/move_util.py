"""The statement of DESIGN.md 6r (include/sketchedit_move.h) in plain numpy, restated independently of sketchedit_amd.serve: the
drop of a lifted selection, the shift of its plane, and the rectangle a move lands in."""
import numpy as np

MAX_OFFSET, MAX_RADIUS = 16384, 16


def slot_of(frame, rect, fill=0xEE):
    """the journal slot of `rect` = (y0, x0, h, w) of `frame`: h rows of round_up(3 w, 16) bytes, the padding `fill`"""
    y0, x0, h, w = rect
    pitch = (3 * w + 15) // 16 * 16
    slot = np.full((h, pitch), fill, np.uint8)
    slot[:, :3 * w] = frame[y0:y0 + h, x0:x0 + w].reshape(h, 3 * w)
    return slot


def _moved(sel, box, offset, flip, ys, xs):
    """moved(p) of rule 1 for the destination pixels ys x xs (any integers) -> (moved, qy, qx), qy / qx clipped where not moved"""
    by0, bx0, by1, bx1 = box
    qy = np.asarray(ys, np.int64) - offset[0]
    qx = np.asarray(xs, np.int64) - offset[1]
    if flip & 2:
        qy = by0 + by1 - 1 - qy
    if flip & 1:
        qx = bx0 + bx1 - 1 - qx
    iny, inx = (qy >= by0) & (qy < by1), (qx >= bx0) & (qx < bx1)
    cy, cx = np.clip(qy, by0, by1 - 1), np.clip(qx, bx0, bx1 - 1)
    moved = iny[:, None] & inx[None, :] & (np.asarray(sel)[cy[:, None], cx[None, :]] != 0)
    return moved, cy, cx


def spec_shift(sel, box, offset, flip):
    """rule 6: the (Hi,Wi) plane of 0 / 255"""
    Hi, Wi = sel.shape
    moved, _, _ = _moved(sel, box, offset, flip, np.arange(Hi), np.arange(Wi))
    return np.where(moved, np.uint8(255), np.uint8(0))


def spec_drop(frame, lift, lift_rect, sel, lock, box, offset, flip, r):
    """rules 1 .. 5 -> the new frame (the arguments are only read)"""
    Hi, Wi = sel.shape
    ly0, lx0, lh, lw = lift_rect
    by0, bx0, by1, bx1 = box
    assert ly0 <= by0 < by1 <= ly0 + lh and lx0 <= bx0 < bx1 <= lx0 + lw and 0 <= r <= MAX_RADIUS
    # moved on the frame and r pixels around it: the count knows neither the frame's edge nor the lock
    ys, xs = np.arange(-r, Hi + r), np.arange(-r, Wi + r)
    big, cy, cx = _moved(sel, box, offset, flip, ys, xs)
    m = big.astype(np.int64)
    rows = sum(m[ey:ey + Hi] for ey in range(2 * r + 1))                             # the box sum, one axis after the other
    c = sum(rows[:, ex:ex + Wi] for ex in range(2 * r + 1))
    n = (2 * r + 1) ** 2
    target = big[r:r + Hi, r:r + Wi].copy()
    if lock is not None:
        target &= np.asarray(lock) == 0
    P = np.asarray(lift)[:, :3 * lw].reshape(lh, lw, 3).astype(np.int64)
    src = P[(cy[r:r + Hi] - ly0)[:, None], (cx[r:r + Wi] - lx0)[None, :]]             # P[q], meaningful on targets only
    F = np.asarray(frame).astype(np.int64)
    blend = (c[..., None] * src + (n - c[..., None]) * F + (n - 1) // 2) // n
    assert not target.any() or (1 <= c[target].min() and c[target].max() <= n)
    out = np.array(frame)
    out[target] = blend[target].astype(np.uint8)
    return out


def move_rect(box, offset, frame_hw):
    """the shifted box clipped to the frame, each side widened to 16 inside the frame: half the missing pixels (rounded down) at
    the low end, the rest at the high end, shifted back into the frame where that leaves it; None when nothing lands in it"""
    out = []
    for lo, hi, d, extent in ((box[0], box[2], offset[0], frame_hw[0]), (box[1], box[3], offset[1], frame_hw[1])):
        lo, hi = max(lo + d, 0), min(hi + d, extent)
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


def box_of(sel):
    """the tight box (y0, x0, y1, x1) of sel != 0, or None"""
    rows, cols = np.flatnonzero((sel != 0).any(axis=1)), np.flatnonzero((sel != 0).any(axis=0))
    if rows.size == 0:
        return None
    return int(rows[0]), int(cols[0]), int(rows[-1]) + 1, int(cols[-1]) + 1


# ---- the kernels' arithmetic (se_move.hip), lane by lane on ONE flat byte array with every access checked ---------------------------
class Memory:
    """device memory as the kernels see it: buffers at chosen addresses of one byte array; a read or write outside the span it was
    allowed raises"""

    def __init__(self, size, fill=0xA5):
        self.mem = np.full(size, fill, np.uint8)

    def put(self, addr, a):
        b = np.ascontiguousarray(a, np.uint8).reshape(-1)
        self.mem[addr:addr + b.size] = b
        return addr

    def get(self, addr, shape):
        return self.mem[addr:addr + int(np.prod(shape))].reshape(shape).copy()

    def dword_within(self, p, lo, hi):
        assert p % 4 == 0
        return sum(int(self.mem[p + i]) << (8 * i) for i in range(4) if lo <= p + i < hi)

    def load4_within(self, a, lo, hi):
        a0, sh = a & ~3, (a & 3) * 8
        d0 = self.dword_within(a0, lo, hi)
        if not sh:
            return d0
        return ((d0 >> sh) | (self.dword_within(a0 + 4, lo, hi) << (32 - sh))) & 0xffffffff

    def load12_within(self, a, lo, hi):
        return [(self.load4_within(a + 4 * i, lo, hi) >> (8 * j)) & 255 for i in range(3) for j in range(4)]


def _nonzero(u):
    return sum(1 << (8 * i) for i in range(4) if (u >> (8 * i)) & 255)


def _bswap(u):
    return int.from_bytes(int(u).to_bytes(4, "little"), "big")


def _moved4(mem, sel, Wi, box, offset, flip, y, x):
    """MoveMap::moved4: a byte of {0, 1} for each of the destination pixels (y, x .. x + 3)"""
    by0, bx0, by1, bx1 = box
    sy = by0 + by1 - 1 - (y - offset[0]) if flip & 2 else y - offset[0]
    if not by0 <= sy < by1:
        return 0
    row = sel + sy * Wi
    if flip & 1:
        sx = bx0 + bx1 - 1 - (x - offset[1])
        if sx < bx0 or sx - 3 >= bx1:
            return 0
        return _nonzero(_bswap(mem.load4_within(row + sx - 3, row + bx0, row + bx1)))
    sx = x - offset[1]
    if sx + 3 < bx0 or sx >= bx1:
        return 0
    return _nonzero(mem.load4_within(row + sx, row + bx0, row + bx1))


def tiled_drop(mem, frame, Hi, Wi, lift, lift_rect, sel, lock, box, offset, flip, r):
    """move_drop_kernel on `mem`, addresses for pointers: the launch's tiles, each lane's stage / rows / blend.  Writes go through
    the ownership rule and are asserted to lie inside the destination rectangle's rows."""
    ly0, lx0, lh, lw = lift_rect
    lpitch = (3 * lw + 15) // 16 * 16
    by0, bx0, by1, bx1 = box
    ry0, rx0, ry1, rx1 = max(by0 + offset[0], 0), max(bx0 + offset[1], 0), min(by1 + offset[0], Hi), min(bx1 + offset[1], Wi)
    if ry0 >= ry1 or rx0 >= rx1:
        return 0
    n = (2 * r + 1) ** 2
    magic, half = ((1 << 32) // n + 1) & 0xffffffff, (n - 1) // 2
    tiles = 0
    for ty0 in range(ry0, ry1, 16):
        for tx0 in range(rx0, rx1, 64):
            tiles += 1
            if r:
                rows, cols4 = 16 + 2 * r, (64 + 2 * r + 3) >> 2
                st = np.zeros((rows, 4 * cols4), np.int64)
                for i in range(rows):
                    for j4 in range(cols4):
                        v = _moved4(mem, sel, Wi, box, offset, flip, ty0 - r + i, tx0 - r + 4 * j4)
                        st[i, 4 * j4:4 * j4 + 4] = [(v >> (8 * k)) & 1 for k in range(4)]
                if not st.any():
                    continue
                srow = np.stack([st[:, k:k + 2 * r + 1].sum(axis=1) for k in range(64)], axis=1)
            for ly in range(16):
                for lx in range(0, 64, 4):
                    y, x = ty0 + ly, tx0 + lx
                    if y >= ry1 or x >= rx1:
                        continue
                    npx = min(4, rx1 - x)
                    if r:
                        s4 = [int(st[ly + r, lx + r + p]) if p < npx else 0 for p in range(4)]
                    else:
                        v = _moved4(mem, sel, Wi, box, offset, flip, y, x)
                        s4 = [(v >> (8 * p)) & 1 if p < npx else 0 for p in range(4)]
                    if not any(s4):
                        continue
                    if lock is not None:
                        lrow = lock + y * Wi
                        lk = mem.load4_within(lrow + x, lrow + x, lrow + x + npx)
                        s4 = [s4[p] if not (lk >> (8 * p)) & 255 else 0 for p in range(4)]
                        if not any(s4):
                            continue
                    c = [int(srow[ly:ly + 2 * r + 1, lx + p].sum()) for p in range(4)] if r else [1] * 4
                    sy = by0 + by1 - 1 - (y - offset[0]) if flip & 2 else y - offset[0]
                    sx = bx0 + bx1 - 1 - (x - offset[1]) if flip & 1 else x - offset[1]
                    assert ly0 <= sy < ly0 + lh
                    prow = lift + (sy - ly0) * lpitch
                    s = mem.load12_within(prow + 3 * ((sx - 3 if flip & 1 else sx) - lx0), prow, prow + 3 * lw)
                    frow, dst = frame + (y * Wi + rx0) * 3, frame + (y * Wi + x) * 3
                    full = all(not s4[p] or c[p] == n for p in range(4))
                    f = [0] * 12 if full else mem.load12_within(dst, frow, frow + 3 * (rx1 - rx0))
                    o = []
                    for j in range(12):
                        a = s[3 * (3 - j // 3) + j % 3] if flip & 1 else s[j]
                        cp = c[j // 3]
                        v = cp * a + (n - cp) * f[j] + half
                        assert v < 1 << 19
                        o.append(a if not r or cp == n else (v * magic) >> 32)
                    for p in range(4):
                        if s4[p]:
                            assert frow <= dst + 3 * p and dst + 3 * p + 3 <= frow + 3 * (rx1 - rx0)
                            mem.mem[dst + 3 * p:dst + 3 * p + 3] = o[3 * p:3 * p + 3]
    return tiles


def tiled_shift(mem, sel, Hi, Wi, box, offset, flip, out):
    """plane_shift_kernel on `mem`: one lane per aligned dword of the output"""
    n, mis = Hi * Wi, out & 3
    for q in range((n + mis + 3) // 4):
        p0 = 4 * q - mis
        first, last = max(p0, 0), min(p0 + 3, n - 1)
        y, x = divmod(first, Wi)
        if x + (last - first) < Wi:
            v = (_moved4(mem, sel, Wi, box, offset, flip, y, x) * 255 << (8 * (first - p0))) & 0xffffffff
        else:
            v = 0
            for p in range(first, last + 1):
                py, px = divmod(p, Wi)
                v |= ((_moved4(mem, sel, Wi, box, offset, flip, py, px) & 1) * 255) << (8 * (p - p0))
        for e in range(4):
            if 0 <= p0 + e < n:
                mem.mem[out + p0 + e] = (v >> (8 * e)) & 255
