"""The statement of DESIGN.md 6u (include/sketchedit_adjust.h) in plain numpy, restated independently of sketchedit_amd.serve: the
pointwise adjustment of a lifted selection, the histogram of a selection and the three table builders; and the kernels' arithmetic
(se_adjust.hip) lane by lane on filter_util.Memory with every access checked against the span it may touch."""
import numpy as np

import filter_util
import move_util
from filter_util import Memory, _blend, _only, _sel4_in_box, counts  # noqa: F401  (the count and the blend are 6t's, word for word)
from move_util import slot_of  # noqa: F401  (the tests build their lifts with it)

MAX_COEF, MAX_OFFSET, ONE_AMOUNT, MAX_FEATHER, MAX_CLIP, HIST_GROUPS = 32768, 1 << 20, 256, 16, 200, 256
STRETCH, EQUALIZE, MATCH = 0, 1, 2
PER_CHANNEL, LUMA = 0, 1
GREY = [1225, 2404, 467] * 3 + [0, 0, 0]
IDENTITY = np.tile(np.arange(256, dtype=np.uint8), (3, 1))


def luma(rgb):
    """Y = (77 R + 150 G + 29 B + 128) >> 8 of an (..., 3) array"""
    v = np.asarray(rgb).astype(np.int64)
    return (77 * v[..., 0] + 150 * v[..., 1] + 29 * v[..., 2] + 128) >> 8


def adjusted(P, lut, matrix, amount):
    """O of an (..., 3) int64 array of lifted pixels: the table FIRST, then the matrix in int32, then the mix"""
    P = np.asarray(P).astype(np.int64)
    Q = P if lut is None else np.stack([np.asarray(lut).reshape(3, 256).astype(np.int64)[c][P[..., c]] for c in range(3)], axis=-1)
    if matrix is None:
        M = Q
    else:
        m = [int(v) for v in matrix]
        assert len(m) == 12 and max(abs(v) for v in m[:9]) <= MAX_COEF and max(abs(v) for v in m[9:]) <= MAX_OFFSET
        rows = []
        for c in range(3):
            acc = m[3 * c] * Q[..., 0] + m[3 * c + 1] * Q[..., 1] + m[3 * c + 2] * Q[..., 2] + m[9 + c] + 2048
            assert np.abs(acc).max() < 1 << 31                  # int32 holds it
            rows.append(np.clip(acc >> 12, 0, 255))
        M = np.stack(rows, axis=-1)
    return P + ((int(amount) * (M - P) + 128) >> 8)


def spec_adjust(frame, lift, lift_rect, sel, lock, box, lut=None, matrix=None, amount=256, f=0):
    """the rule for ADJUST -> the new frame (the arguments are only read; the frame's own bytes play no part in what is stored)"""
    assert 0 <= amount <= ONE_AMOUNT and 0 <= f <= MAX_FEATHER
    ly0, lx0, lh, lw = lift_rect
    by0, bx0, by1, bx1 = box
    assert ly0 <= by0 < by1 <= ly0 + lh and lx0 <= bx0 < bx1 <= lx0 + lw
    P = filter_util._lifted(lift, lift_rect)[by0 - ly0:by1 - ly0, bx0 - lx0:bx1 - lx0]
    O = adjusted(P, lut, matrix, amount)
    assert O.min() >= 0 and O.max() <= 255
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


def spec_hist(frame, sel, box):
    """HIST -> (4, 256) uint32: R, G, B and Y of the box's pixels with S != 0 (sel None: all of them)"""
    by0, bx0, by1, bx1 = box
    px = np.asarray(frame)[by0:by1, bx0:bx1].reshape(-1, 3)
    if sel is not None:
        px = px[np.asarray(sel)[by0:by1, bx0:bx1].reshape(-1) != 0]
    rows = [np.bincount(px[:, c], minlength=256) for c in range(3)] + [np.bincount(luma(px), minlength=256)]
    return np.stack(rows).astype(np.uint32)


def _row(mode, h, href, k):
    """one row of a table, in Python ints (unbounded, so nothing can wrap)"""
    ident = list(range(256))
    h = [int(v) for v in h]
    N, cdf = sum(h), list(np.cumsum(np.asarray(h, dtype=object)))
    if N == 0:
        return ident
    if mode == STRETCH:
        t = N * k // 1000
        lo = min(v for v in range(256) if cdf[v] > t)
        hi = max(v for v in range(256) if N - (cdf[v - 1] if v else 0) > t)
        assert lo <= hi
        if hi == lo:
            return ident
        return [0 if v < lo else min(((v - lo) * 255 + (hi - lo) // 2) // (hi - lo), 255) for v in range(256)]
    if mode == EQUALIZE:
        m = min(v for v in range(256) if h[v] > 0)
        c0 = cdf[m]
        if N == c0:
            return ident
        return [0 if v < m else ((cdf[v] - c0) * 255 + (N - c0) // 2) // (N - c0) for v in range(256)]
    href = [int(v) for v in href]
    Nr, cr = sum(href), list(np.cumsum(np.asarray(href, dtype=object)))
    if Nr == 0:
        return ident
    return [int(np.searchsorted(np.asarray([c * N for c in cr], dtype=object), cdf[v] * Nr, side="left")) for v in range(256)]


def spec_lut(hist_src, hist_ref, mode, which, clip=0):
    """LUT -> (3, 256) uint8"""
    assert mode in (STRETCH, EQUALIZE, MATCH) and which in (PER_CHANNEL, LUMA) and 0 <= clip <= MAX_CLIP
    assert (hist_ref is not None) == (mode == MATCH)
    rows = []
    for c in range(3):
        r = 3 if which == LUMA else c
        rows.append(_row(mode, np.asarray(hist_src).reshape(4, 256)[r], None if hist_ref is None else np.asarray(hist_ref).reshape(4, 256)[r], clip))
    out = np.asarray(rows, dtype=np.int64)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


# ---- the kernels' arithmetic (se_adjust.hip), lane by lane on ONE flat byte array with every access checked -------------------------
def tiled_adjust(mem, frame, Hi, Wi, lift, lift_rect, sel, lock, box, lut, matrix, amount, f):
    """adjust_kernel on `mem`, addresses for pointers (lut None: no table): the box's tiles, each tile's select / stage / point.
    Loads are bounded as the kernel bounds them and asserted to stay in the plane, the table's 768 bytes, the first 3 lw bytes of a
    slot row or -- never -- the frame; stores are asserted to lie in the box's row of the frame.  -> (tiles, tiles that returned
    having loaded S only, tiles that returned having loaded S and L only)"""
    ly0, lx0, lh, lw = lift_rect
    lpitch = (3 * lw + 15) // 16 * 16
    by0, bx0, by1, bx1 = box
    n = (2 * f + 1) ** 2
    m = None if matrix is None else [int(v) for v in matrix]
    S_span, L_span = (sel, sel + Hi * Wi), (lock, lock + Hi * Wi) if lock is not None else (0, 0)
    T_span = (lut, lut + 768) if lut is not None else (0, 0)
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
            # ---- stage: the table (a dword per lane of the first 192), S around the tile
            tb = None
            if lut is not None:
                tb = []
                for t in range(192):
                    u = mem.load4_within(lut + 4 * t, lut, lut + 768)
                    tb += [(u >> (8 * e)) & 255 for e in range(4)]
            if f:
                cols4 = (64 + 2 * f + 3) >> 2
                fs = np.zeros((16 + 2 * f, 4 * cols4), np.int64)
                for i in range(16 + 2 * f):
                    for j4 in range(cols4):
                        fs[i, 4 * j4:4 * j4 + 4] = _sel4_in_box(mem, sel, Wi, box, ty0 - f + i, tx0 - f + 4 * j4)
                frow = np.stack([fs[:, k:k + 2 * f + 1].sum(axis=1) for k in range(64)], axis=1)
            # ---- point
            for (ly, lx), g in tg.items():
                if not any(g):
                    continue
                y, x = ty0 + ly, tx0 + lx
                npx = min(4, tw - lx)
                assert ly0 <= y < ly0 + lh
                prow = lift + (y - ly0) * lpitch
                src = prow + 3 * (x - lx0)
                assert prow <= src and src + 3 * npx <= prow + 3 * lw
                pb = mem.load12_within(src, src, src + 3 * npx)
                c = [int(frow[ly:ly + 2 * f + 1, lx + p].sum()) for p in range(4)] if f else [n] * 4
                brow = frame + (y * Wi + bx0) * 3
                dst = frame + (y * Wi + x) * 3
                for p in range(4):
                    if not g[p]:
                        continue
                    assert brow <= dst + 3 * p and dst + 3 * p + 3 <= brow + 3 * (bx1 - bx0) and 1 <= c[p] <= n
                    P = pb[3 * p:3 * p + 3]
                    M = [tb[256 * ch + P[ch]] for ch in range(3)] if tb is not None else list(P)
                    if m is not None:
                        q = list(M)
                        for ch in range(3):
                            acc = m[3 * ch] * q[0] + m[3 * ch + 1] * q[1] + m[3 * ch + 2] * q[2] + m[9 + ch] + 2048
                            assert -(1 << 31) <= acc < 1 << 31
                            M[ch] = min(max(acc >> 12, 0), 255)
                    for ch in range(3):
                        O = P[ch] + ((amount * (M[ch] - P[ch]) + 128) >> 8)
                        assert 0 <= O <= 255
                        mem.mem[dst + 3 * p + ch] = _blend(P[ch], O, c[p], n)
            assert _only(mem, mark, [S_span, L_span, T_span, (lift, lift + lh * lpitch)])
    return tiles, early_s, early_l


def tiled_hist(mem, frame, Hi, Wi, sel, box, slabs, hist, groups=None):
    """hist_tiles_kernel and hist_sum_kernel on `mem` (sel None: no plane): `groups` workgroups (None: the launch's own number)
    stride over the box's tiles, a sub-histogram per wave, a wave whose active lanes hold one value adding their number once; each
    workgroup stores its 1024 words to its slab at `slabs`, the sum goes to `hist`.  Loads are asserted to stay in the plane and in
    the box's rows of the frame.  -> (workgroups, wave adds that were folded into one, adds made lane by lane)"""
    by0, bx0, by1, bx1 = box
    ntx, nty = -(-(bx1 - bx0) // 64), -(-(by1 - by0) // 16)
    G = min(ntx * nty, HIST_GROUPS) if groups is None else groups
    assert 1 <= G <= HIST_GROUPS and slabs % 4 == 0 and hist % 4 == 0
    folded = single = 0
    for g in range(G):
        sub = np.zeros((4, 1024), np.int64)
        for tile in range(g, ntx * nty, G):
            tx0, ty0 = bx0 + tile % ntx * 64, by0 + tile // ntx * 16
            tx1, ty1 = min(tx0 + 64, bx1), min(ty0 + 16, by1)
            lanes = []
            for tid in range(256):
                lx, ly = 4 * (tid & 15), tid >> 4
                x, y = tx0 + lx, ty0 + ly
                on, pb = [0] * 4, [0] * 12
                if y < ty1 and x < tx1:
                    npx = min(4, tx1 - x)
                    if sel is not None:
                        a = sel + y * Wi + x
                        assert sel <= a and a + npx <= sel + Hi * Wi
                        u = mem.load4_within(a, a, a + npx)
                        on = [1 if (u >> (8 * p)) & 255 else 0 for p in range(4)]
                    else:
                        on = [1 if p < npx else 0 for p in range(4)]
                    if any(on):
                        src = frame + (y * Wi + x) * 3
                        assert frame + (y * Wi + bx0) * 3 <= src and src + 3 * npx <= frame + (y * Wi + bx1) * 3
                        pb = mem.load12_within(src, src, src + 3 * npx)
                lanes.append((on, pb))
            for wave in range(4):
                for p in range(4):
                    act = [ln for ln in range(64) if lanes[64 * wave + ln][0][p]]
                    if not act:
                        continue
                    px = [lanes[64 * wave + ln][1][3 * p:3 * p + 3] for ln in act]
                    for ch in range(4):
                        vals = [v[ch] if ch < 3 else (77 * v[0] + 150 * v[1] + 29 * v[2] + 128) >> 8 for v in px]
                        if all(v == vals[0] for v in vals):
                            sub[wave, 256 * ch + vals[0]] += len(vals)
                            folded += 1
                        else:
                            for v in vals:
                                sub[wave, 256 * ch + v] += 1
                            single += len(vals)
        total = sub.sum(axis=0)
        assert total.max() < 1 << 32
        mem.put(slabs + 4096 * g, total.astype("<u4").view(np.uint8))
    acc = np.zeros(1024, np.int64)
    for g in range(G):
        acc += mem.mem[slabs + 4096 * g:slabs + 4096 * (g + 1)].view("<u4")
    mem.put(hist, (acc & 0xffffffff).astype("<u4").view(np.uint8))
    return G, folded, single


def _scan256(x):
    """scan256: the 8 doubling steps over 256 lanes, unsigned 64 bits"""
    x = [int(v) for v in x]
    d = 1
    while d < 256:
        x = [(x[v] + (x[v - d] if v >= d else 0)) & 0xffffffffffffffff for v in range(256)]
        d <<= 1
    return x


def lanes_lut(hist_src, hist_ref, mode, which, clip):
    """adjust_lut_kernel, a lane per value: the scans, the two lanes that find lo and hi, the binary search; every product and sum
    asserted to fit unsigned 64 bits.  -> (3, 256) uint8"""
    M64 = 1 << 64
    hs = np.asarray(hist_src).reshape(4, 256)
    hr = None if hist_ref is None else np.asarray(hist_ref).reshape(4, 256)
    out = np.zeros((3, 256), np.uint8)
    for r in range(1 if which == LUMA else 3):
        row = 3 if which == LUMA else r
        sa = _scan256(hs[row])
        N = sa[255]
        o = list(range(256))
        if mode == MATCH:
            sb = _scan256(hr[row])
            Nr = sb[255]
            if N and Nr:
                for v in range(256):
                    want = sa[v] * Nr
                    assert want < M64
                    lo, hi, steps = 0, 255, 0
                    while lo < hi:
                        mid = (lo + hi) >> 1
                        assert sb[mid] * N < M64
                        if sb[mid] * N >= want:
                            hi = mid
                        else:
                            lo = mid + 1
                        steps += 1
                    assert steps <= 8
                    o[v] = lo
        elif N:
            assert N * clip < M64
            t = N * clip // 1000 if mode == STRETCH else 0
            los = [v for v in range(256) if sa[v] > t and (sa[v - 1] if v else 0) <= t]
            his = [v for v in range(256) if N - (sa[v - 1] if v else 0) > t and (v == 255 or not N - sa[v] > t)]
            assert len(los) == 1 and len(his) == 1                # one writer each
            lo, hi = los[0], his[0]
            if mode == STRETCH:
                if hi != lo:
                    o = [0 if v < lo else min(((v - lo) * 255 + (hi - lo) // 2) // (hi - lo), 255) for v in range(256)]
            else:
                c0 = sa[lo]
                if N != c0:
                    assert (N - c0) * 255 + (N - c0) // 2 < M64
                    o = [0 if v < lo else ((sa[v] - c0) * 255 + (N - c0) // 2) // (N - c0) for v in range(256)]
        if which == LUMA:
            out[:] = np.asarray(o, np.uint8)
        else:
            out[r] = np.asarray(o, np.uint8)
    return out
