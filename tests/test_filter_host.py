"""Blur, sharpen or pixelate a selection, without a GPU: the statement's properties, the taps, the kernels'
arithmetic lane by lane with every access checked, the session against a scripted backend that really edits a frame, the ABI."""
import os
import re

import numpy as np
import pytest

from sketchedit_amd import _lib, serve
import abi_util
import filter_util as F
import move_util as M
import select_util as U
from test_fill_host import _names
from test_move_host import BOX, HW, RING, _Stub as _MoveStub, _lock_array
from test_warp_host import _Stub as _WarpStub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the statement ----------------------------------------------------------------------------------------------------------------------
def _known():
    P = np.full((16, 16, 3), 10, np.uint8)
    P[:, 8:] = 200
    whole = (0, 0, 16, 16)
    return P, M.slot_of(P, whole), whole, np.full((16, 16), 255, np.uint8)


def test_known_answers_of_the_header():
    P, slot, whole, sel = _known()
    frame = np.full((16, 16, 3), 99, np.uint8)                        # the frame's own bytes play no part
    for a, want in ((-256, (10, 58, 153, 200)), (-128, (10, 34, 177, 200)), (256, (10, 0, 247, 200)), (1024, (10, 0, 255, 200)), (0, (10, 10, 200, 200))):
        out = F.spec_blur(frame, slot, whole, sel, None, (0, 0, 16, 16), (2048, 1024), a)
        for row in (0, 7, 15):
            assert tuple(out[row, 6:10, 1]) == want, a
        assert (out[..., 0] == out[..., 2]).all() and (out[:, :6] == 10).all() and (out[:, 10:] == 200).all()
    out = F.spec_mosaic(frame, slot, whole, sel, None, (0, 0, 16, 16), 3)
    assert (out[:, 6:9] == 73).all() and (out[:, 15] == 200).all() and (out[:, :6] == 10).all() and (out[:, 9:15] == 200).all()
    hdr = open(os.path.join(ROOT, "include", "sketchedit_filter.h")).read()
    for text in ("B = 10, 58, 153, 200", "a = -128: 10, 34, 177, 200", "a = 256: 10, 0, 247, 200", "a = 1024: 10, 0, 255, 200", "(660 + 4) / 9 = 73"):
        assert text in hdr


def test_taps_for_every_radius_and_kind():
    assert serve.filter_taps("gauss", 1) == [3224, 436] and serve.filter_taps("gauss", 2) == [2450, 796, 27]
    for kind in ("gauss", "box"):
        for R in range(1, 33):
            for sigma in ((None, 0.3, R, R / 2.0) if kind == "gauss" else (None,)):
                t = serve.filter_taps(kind, R, sigma)
                assert t == F.taps(kind, R, sigma) and all(type(v) is int for v in t), (kind, R, sigma)
                assert len(t) == R + 1 and min(t) >= 0 and t[0] > 0 and t[0] + 2 * sum(t[1:]) == 4096
                assert all(t[k] >= t[k + 1] for k in range(1, R))         # (t[0] may lie a unit or two below t[1] for a wide sigma)
    assert serve.filter_taps("box", 32)[1:] == [63] * 32 and serve.filter_taps("box", 32)[0] == 4096 - 64 * 63
    for bad in (lambda: serve.filter_taps("sinc", 2), lambda: serve.filter_taps("gauss", 0), lambda: serve.filter_taps("gauss", 33),
                lambda: serve.filter_taps("gauss", 2.0), lambda: serve.filter_taps("gauss", True), lambda: serve.filter_taps("gauss", 2, 0),
                lambda: serve.filter_taps("gauss", 2, 2.5), lambda: serve.filter_taps("gauss", 2, "1"), lambda: serve.filter_taps("box", 2, 1.0),
                lambda: serve.filter_taps(None, 2)):
        with pytest.raises(ValueError):
            bad()


def test_filter_rect():
    for box, r, hw in (((5, 5, 8, 8), 3, (100, 100)), ((0, 0, 20, 20), 32, (36, 40)), ((200, 300, 230, 340), 8, (400, 600)),
                       ((90, 90, 100, 100), 0, (100, 100)), ((40, 2, 43, 5), 1, (64, 64))):
        got = serve.filter_rect(box, r, hw)
        assert got == F.filter_rect(box, r, hw)
        y0, x0, h, w = got
        assert h >= 16 and w >= 16 and 0 <= y0 and y0 + h <= hw[0] and 0 <= x0 and x0 + w <= hw[1]
        assert y0 <= max(box[0] - r, 0) and x0 <= max(box[1] - r, 0) and y0 + h >= min(box[2] + r, hw[0]) and x0 + w >= min(box[3] + r, hw[1])
    assert serve.filter_rect((200, 300, 230, 340), 8, (400, 600)) == (192, 292, 46, 56)
    assert serve.filter_rect((200, 300, 230, 340), 0, (400, 600)) == serve.move_rect((200, 300, 230, 340), (0, 0), (400, 600))


def _case(seed, hw=(37, 53), box=None, R=0, density=0.7):
    """noise: a frame (what is there now), another frame as it was when lifted, a selection, a lock, the lift of the box grown by R"""
    rng = np.random.RandomState(seed)
    Hi, Wi = hw
    frame = rng.randint(0, 256, (Hi, Wi, 3)).astype(np.uint8)
    before = rng.randint(0, 256, (Hi, Wi, 3)).astype(np.uint8)
    sel = np.where(rng.rand(Hi, Wi) < density, rng.randint(1, 256, (Hi, Wi)), 0).astype(np.uint8)
    lock = np.where(rng.rand(Hi, Wi) < 0.2, 255, 0).astype(np.uint8)
    box = box or (1, 2, Hi - 3, Wi - 1)
    rect = F.filter_rect(box, R, hw)
    return frame, before, sel, lock, box, rect, M.slot_of(before, rect)


@pytest.mark.parametrize("value", [0, 255])
def test_a_constant_frame_stays_constant(value):
    """every taps and amount; at 255 and R = 32 the vertical sum is 255 * 2^24 + 2^23, which only UNSIGNED 32 bits hold"""
    hw, box = (37, 53), (0, 0, 37, 53)
    P = np.full(hw + (3,), value, np.uint8)
    rect = (0, 0) + hw
    slot, sel = M.slot_of(P, rect), np.full(hw, 1, np.uint8)
    frame = np.full(hw + (3,), 123, np.uint8)
    for t in (F.taps("gauss", 32), F.taps("box", 32), F.taps("gauss", 1), F.taps("gauss", 32, 0.3), [0] * 32 + [2048], [4096] + [0] * 32):
        assert (F.blurred(slot, rect, box, t, hw) == value).all()
        for a in (-256, -128, 0, 256, 1024):
            for f in (0, 3):
                assert (F.spec_blur(frame, slot, rect, sel, None, box, t, a, f) == value).all()
    assert 255 * (1 << 24) + (1 << 23) >= 1 << 31
    for cell in (2, 5, 64):
        for a in (-256, 1024):
            assert (F.spec_mosaic(frame, slot, rect, sel, None, box, cell, a, 2) == value).all()


def test_amount_zero_is_the_lift_and_minus_one_is_the_blur():
    frame, before, sel, lock, box, rect, slot = _case(1, R=7)
    t = F.taps("gauss", 7)
    by0, bx0, by1, bx1 = box
    tg = np.zeros(sel.shape, bool)
    tg[by0:by1, bx0:bx1] = sel[by0:by1, bx0:bx1] != 0
    out = F.spec_blur(frame, slot, rect, sel, None, box, t, 0)
    assert np.array_equal(out[tg], before[tg]) and np.array_equal(out[~tg], frame[~tg])
    out = F.spec_blur(frame, slot, rect, sel, None, box, t, -256)
    B = F.blurred(slot, rect, box, t, sel.shape)
    assert np.array_equal(out[by0:by1, bx0:bx1][tg[by0:by1, bx0:bx1]], B[tg[by0:by1, bx0:bx1]].astype(np.uint8))
    out = F.spec_mosaic(frame, slot, rect, sel, None, box, 5, 0)
    assert np.array_equal(out[tg], before[tg])
    sharp = F.spec_blur(frame, slot, rect, sel, None, box, t, 1024)
    assert (sharp[tg] == 0).sum() > 500 and (sharp[tg] == 255).sum() > 500            # the clamp works at both ends


def test_nothing_but_unlocked_targets_changes():
    frame, before, sel, lock, box, rect, slot = _case(2, R=7)
    by0, bx0, by1, bx1 = box
    inbox = np.zeros(sel.shape, bool)
    inbox[by0:by1, bx0:bx1] = True
    for f in (0, 4):
        for out in (F.spec_blur(frame, slot, rect, sel, lock, box, F.taps("box", 7), -256, f),
                    F.spec_mosaic(frame, slot, rect, sel, lock, box, 5, -256, f)):
            tg = inbox & (sel != 0) & (lock == 0)
            assert np.array_equal(out[~tg], frame[~tg]) and (out[tg] != frame[tg]).any()
            assert np.array_equal(out[lock != 0], frame[lock != 0])


def test_only_the_lift_within_the_radius_matters():
    hw, box, R = (65, 129), (20, 30, 40, 80), 7
    frame, before, sel, lock, _, _, _ = _case(3, hw, box, R)
    wide = F.filter_rect(box, 16, hw)                                   # a lift larger than the filter needs
    t = F.taps("gauss", R)
    want = F.spec_blur(frame, M.slot_of(before, wide), wide, sel, None, box, t)
    far = before.copy()
    near = np.zeros(hw, bool)
    near[box[0] - R:box[2] + R, box[1] - R:box[3] + R] = True
    far[~near] ^= 0xFF
    assert np.array_equal(F.spec_blur(frame, M.slot_of(far, wide), wide, sel, None, box, t), want)
    # ... and the corner tap at exactly the radius does: R = 1, taps (2048, 1024), the pixel up and left of the box's first moved by
    # 128 moves that B by 1024 * 1024 * 128 >> 24 = 8
    sel[box[0], box[1]] = 1
    near1 = before.copy()
    near1[box[0] - 1, box[1] - 1] = (near1[box[0] - 1, box[1] - 1].astype(int) + 128) % 256
    a = F.spec_blur(frame, M.slot_of(before, wide), wide, sel, None, box, (2048, 1024))
    b = F.spec_blur(frame, M.slot_of(near1, wide), wide, sel, None, box, (2048, 1024))
    assert (np.abs(a[box[0], box[1]].astype(int) - b[box[0], box[1]]) == 8).all() and np.array_equal(a[box[0] + 1:], b[box[0] + 1:])
    # the mosaic's mean runs over unselected pixels too: changing one changes the cell
    sel2 = sel.copy()
    sel2[20:25, 30:35] = 0
    sel2[20, 30] = 255
    rect0 = F.filter_rect(box, 0, hw)
    a = F.spec_mosaic(frame, M.slot_of(before, rect0), rect0, sel2, None, box, 5)
    other = before.copy()
    other[24, 34] = (255 - other[24, 34].astype(np.int64) // 128 * 255).astype(np.uint8)      # an unselected pixel of the first cell, moved by >= 127
    b = F.spec_mosaic(frame, M.slot_of(other, rect0), rect0, sel2, None, box, 5)
    assert not np.array_equal(a[20, 30], b[20, 30]) and np.array_equal(a[25:], b[25:])


def test_feather_counts_the_selection_in_the_box_alone():
    hw, box = (37, 53), (0, 0, 20, 30)                                  # the box touches the frame's top left corner
    frame, before, _, _, _, _, _ = _case(4, hw, box, 2)
    sel = np.zeros(hw, np.uint8)
    sel[0:12, 0:14] = 200                                               # a block in that corner
    sel[30:, 40:] = 255                                                 # selected, outside the box: never counted, never written
    rect = F.filter_rect(box, 2, hw)
    slot = M.slot_of(before, rect)
    t, f = F.taps("gauss", 2), 3
    n = (2 * f + 1) ** 2
    c = F.counts(sel, box, f)
    assert c[5, 5] == n and c[0, 0] == 16 and c[11, 13] == 16 and c[5, 13] == 4 * 7 and c[12, 5] == 3 * 7        # the frame's corner fades like any other
    hard = F.spec_blur(frame, slot, rect, sel, None, box, t, -256, 0)
    soft = F.spec_blur(frame, slot, rect, sel, None, box, t, -256, f)
    P = before.astype(int)
    assert np.array_equal(soft[3:9, 3:11], hard[3:9, 3:11])             # c == n stores O
    rim = np.zeros(hw, bool)
    rim[0:12, 11:14] = True
    lo, hi = np.minimum(P, hard.astype(int)), np.maximum(P, hard.astype(int))
    between = (lo <= soft) & (soft <= hi)
    assert between[rim].all() and ((soft != hard) & (soft != before))[rim].any()
    strictly = rim[..., None] & (hi - lo > n)
    assert strictly.any() and ((soft > lo) & (soft < hi))[strictly].all()
    assert np.array_equal(soft[sel == 0], frame[sel == 0]) and np.array_equal(soft[30:], frame[30:])
    # the lock takes pixels out of the targets, not out of the count
    lock = np.zeros(hw, np.uint8)
    lock[0:12, 0:7] = 255
    locked = F.spec_blur(frame, slot, rect, sel, lock, box, t, -256, f)
    assert np.array_equal(locked[lock != 0], frame[lock != 0]) and np.array_equal(locked[:, 7:], soft[:, 7:])


def test_a_box_at_every_edge_and_a_radius_beyond_the_frame():
    """the clamp: against a brute-force evaluation of the rule, pixel by pixel"""
    def brute(before, box, t, hw):
        R = len(t) - 1
        Hi, Wi = hw
        P = before.astype(np.int64)
        out = {}
        for y in range(box[0], box[2]):
            for x in range(box[1], box[3]):
                v = np.zeros(3, np.int64)
                for ky in range(-R, R + 1):
                    yy = min(max(y + ky, 0), Hi - 1)
                    h = np.zeros(3, np.int64)
                    for kx in range(-R, R + 1):
                        h += t[abs(kx)] * P[yy, min(max(x + kx, 0), Wi - 1)]
                    v += t[abs(ky)] * h
                out[y, x] = (v + (1 << 23)) >> 24
        return out

    hw = (16, 16)
    rng = np.random.RandomState(7)
    before = rng.randint(0, 256, hw + (3,)).astype(np.uint8)
    whole = (0, 0, 16, 16)
    slot = M.slot_of(before, whole)
    for box, t in (((0, 0, 3, 16), F.taps("gauss", 3)), ((13, 0, 16, 4), F.taps("box", 5)), ((0, 12, 16, 16), F.taps("gauss", 2)),
                   ((6, 6, 9, 9), F.taps("gauss", 32, 20.0)), ((0, 0, 2, 2), F.taps("box", 32))):
        assert F.filter_rect(box, len(t) - 1, hw) == whole
        B = F.blurred(slot, whole, box, t, hw)
        for (y, x), v in brute(before, box, t, hw).items():
            assert np.array_equal(B[y - box[0], x - box[1]], v), (box, y, x)


# ---- the kernels' arithmetic, lane by lane -----------------------------------------------------------------------------------------------------
def _place(k, frame, sel, lock, slot):
    Hi, Wi = sel.shape
    mem = F.Memory(16384 + 5 * Hi * Wi + slot.size)
    fa = mem.put(1024 + k % 4, frame)
    sa = mem.put(fa + 3 * Hi * Wi + 1031, sel)
    la = mem.put(sa + Hi * Wi + 1033, lock)
    pa = mem.put((la + Hi * Wi + 1024 + 15) // 16 * 16, slot)
    return mem, fa, sa, la, pa


def _only_the_frame_changed(mem, clean, fa, n):
    changed = np.flatnonzero(mem.mem != clean)
    return changed.size > 0 and fa <= changed.min() and changed.max() < fa + n


SIZES = [(16, 16), (37, 53), (65, 129)]


@pytest.mark.parametrize("hw", SIZES, ids=lambda hw: "%dx%d" % hw)
@pytest.mark.parametrize("R", [1, 7, 16, 32])
def test_tiled_blur_is_the_statement(hw, R):
    """every feather, locked and not, the frame at each byte offset mod 4: 12 runs per size and radius, the amount cycling"""
    Hi, Wi = hw
    k = 0
    for f in (0, 1, 16):
        for locked in (False, True):
            for kind in ("gauss", "box"):
                box = (0, 0, Hi, Wi) if (k % 3 == 0 or Hi == 16) else (1, 2, Hi - 3, Wi - 1)
                frame, before, sel, lock, box, rect, slot = _case(100 * R + k, hw, box, R)
                mem, fa, sa, la, pa = _place(k, frame, sel, lock, slot)
                clean = mem.mem.copy()
                t, a = F.taps(kind, R), (-256, -128, 256, 1024)[k % 4]
                tiles, es, el = F.tiled_blur(mem, fa, Hi, Wi, pa, rect, sa, la if locked else None, box, t, a, f)
                want = F.spec_blur(frame, slot, rect, sel, lock if locked else None, box, t, a, f)
                assert np.array_equal(mem.get(fa, frame.shape), want), (hw, R, f, locked, kind)
                assert _only_the_frame_changed(mem, clean, fa, 3 * Hi * Wi)
                assert tiles == -(-(box[2] - box[0]) // 16) * -(-(box[3] - box[1]) // 64) and es + el < tiles
                k += 1


@pytest.mark.parametrize("hw", SIZES, ids=lambda hw: "%dx%d" % hw)
@pytest.mark.parametrize("cell", [2, 3, 5, 16, 64])
def test_tiled_mosaic_is_the_statement(hw, cell):
    Hi, Wi = hw
    k = 0
    for f in (0, 1, 16):
        for locked in (False, True):
            box = (0, 0, Hi, Wi) if (k % 3 == 0 or Hi == 16) else (1, 2, Hi - 3, Wi - 1)
            frame, before, sel, lock, box, rect, slot = _case(100 * cell + k, hw, box, 0)
            mem, fa, sa, la, pa = _place(k, frame, sel, lock, slot)
            clean = mem.mem.copy()
            a = (-256, -128, 256, 1024)[k % 4]
            cells, early = F.tiled_mosaic(mem, fa, Hi, Wi, pa, rect, sa, la if locked else None, box, cell, a, f)
            want = F.spec_mosaic(frame, slot, rect, sel, lock if locked else None, box, cell, a, f)
            assert np.array_equal(mem.get(fa, frame.shape), want), (hw, cell, f, locked)
            assert _only_the_frame_changed(mem, clean, fa, 3 * Hi * Wi)
            assert cells == -(-(box[2] - box[0]) // cell) * -(-(box[3] - box[1]) // cell)
            k += 1


def test_a_tile_without_targets_loads_nothing_but_the_planes():
    """the selection in one corner of a 65 x 129 box of 15 tiles: the others read their part of S and return; a tile whose selected
    pixels are all locked reads S and L and returns; the statement holds all the same"""
    hw = (65, 129)
    frame, before, _, _, box, rect, slot = _case(9, hw, (0, 0, 65, 129), 16)
    sel = np.zeros(hw, np.uint8)
    sel[3:9, 5:30] = 7                                                  # tile (0, 0)
    sel[40:44, 70:90] = 9                                               # tile (2, 1), locked whole
    lock = np.zeros(hw, np.uint8)
    lock[38:48, 64:128] = 255
    t = F.taps("gauss", 16)
    for f in (0, 5):
        mem, fa, sa, la, pa = _place(1, frame, sel, lock, slot)
        tiles, es, el = F.tiled_blur(mem, fa, 65, 129, pa, rect, sa, la, box, t, -256, f)
        assert (tiles, es, el) == (15, 13, 1)
        assert np.array_equal(mem.get(fa, frame.shape), F.spec_blur(frame, slot, rect, sel, lock, box, t, -256, f))
        mem, fa, sa, la, pa = _place(2, frame, sel, lock, slot)
        tiles, es, el = F.tiled_blur(mem, fa, 65, 129, pa, rect, sa, None, box, t, -256, f)
        assert (tiles, es, el) == (15, 13, 0)
        mem, fa, sa, la, pa = _place(3, frame, sel, lock, slot)
        cells, early = F.tiled_mosaic(mem, fa, 65, 129, pa, rect, sa, la, box, 16, -256, f)
        assert cells == 5 * 9 and early == 45 - 2                         # columns 5 .. 29 of rows 3 .. 8: cells (0, 0) and (0, 1)
        assert np.array_equal(mem.get(fa, frame.shape), F.spec_mosaic(frame, slot, rect, sel, lock, box, 16, -256, f))


def test_the_all_255_frame_at_radius_32_through_the_tiles():
    hw, box = (37, 53), (0, 0, 37, 53)
    P = np.full(hw + (3,), 255, np.uint8)
    slot, sel = M.slot_of(P, (0, 0) + hw), np.full(hw, 255, np.uint8)
    mem, fa, sa, la, pa = _place(0, np.zeros(hw + (3,), np.uint8), sel, sel, slot)
    F.tiled_blur(mem, fa, 37, 53, pa, (0, 0) + hw, sa, None, box, F.taps("box", 32), -256, 0)
    assert (mem.get(fa, hw + (3,)) == 255).all()


# ---- the sessions against a scripted backend -------------------------------------------------------------------------------------------------
class _Stub(_WarpStub):
    """... with the two calls of DESIGN.md 6t, which are the statement"""

    def filter_blur(self, frame, lift, lift_rect, plane, lock, box, taps, amount, feather):
        self.calls.append(("filter_blur", tuple(lift_rect), id(plane), None if lock is None else id(lock), tuple(box), tuple(taps), amount, feather))
        self.lift = lift.copy()
        frame[...] = F.spec_blur(frame, lift, lift_rect, plane, lock, box, taps, amount, feather)

    def filter_mosaic(self, frame, lift, lift_rect, plane, lock, box, cell, amount, feather):
        self.calls.append(("filter_mosaic", tuple(lift_rect), id(plane), None if lock is None else id(lock), tuple(box), cell, amount, feather))
        self.lift = lift.copy()
        frame[...] = F.spec_mosaic(frame, lift, lift_rect, plane, lock, box, cell, amount, feather)


def _session(stub, lock=False, **kw):
    f = U._noise(HW, 5)
    s = serve.EditSession(None, f, backend=stub, **kw)
    if lock:
        s.set_lock(_lock_array())
    sel = s.select_lasso([RING])
    stub.calls.clear()
    return s, sel, f


KINDS = [("blur", {}, 8, "gauss", -256, -1.0), ("blur", dict(radius=32, sigma=20.0), 32, "gauss", -256, -1.0), ("box", dict(radius=3), 3, "box", -256, -1.0),
         ("sharpen", {}, 2, "gauss", 256, 1.0), ("sharpen", dict(radius=5, amount=2.5, sigma=1.0), 5, "gauss", 640, 2.5),
         ("pixelate", {}, 0, None, -256, -1.0), ("pixelate", dict(cell=5), 0, None, -256, -1.0)]


@pytest.mark.parametrize("case", KINDS, ids=lambda c: c[0] + "".join("-%s" % v for v in c[1].values()))
@pytest.mark.parametrize("lock", [False, True])
@pytest.mark.parametrize("history", [0, 2])
@pytest.mark.parametrize("feather", [None, 4])
def test_filter_issues_one_save_and_one_launch(case, lock, history, feather):
    kind, kw, R, tk, q8, amount = case
    stub = _Stub()
    s, sel, f = _session(stub, lock, history=history)
    plane0 = sel.plane.copy()
    patches, positions, info = s.filter_selection(sel, kind, feather=feather, **kw)
    lift_rect = F.filter_rect(BOX, R, HW)
    win = M.move_rect(BOX, (0, 0), HW)
    assert stub.calls[0] == ("save", [lift_rect[:2]], lift_rect[2:])
    lk = s._lock_plane
    if kind == "pixelate":
        cell = kw.get("cell", 16)
        assert _names(stub) == ["save", "filter_mosaic", "crop"]
        assert stub.calls[1] == ("filter_mosaic", lift_rect, id(sel.plane), None if lk is None else id(lk), BOX, cell, -256, feather or 0)
        want = F.spec_mosaic(f, M.slot_of(f, lift_rect), lift_rect, plane0, _lock_array() if lock else None, BOX, cell, -256, feather or 0)
    else:
        cell = None
        t = F.taps(tk, R, kw.get("sigma"))
        assert _names(stub) == ["save", "filter_blur", "crop"]
        assert stub.calls[1] == ("filter_blur", lift_rect, id(sel.plane), None if lk is None else id(lk), BOX, tuple(t), q8, feather or 0)
        want = F.spec_blur(f, M.slot_of(f, lift_rect), lift_rect, plane0, _lock_array() if lock else None, BOX, t, q8, feather or 0)
    assert stub.calls[2] == ("crop", win)
    y0, x0, h, w = lift_rect
    assert np.array_equal(stub.lift[:, :3 * w].reshape(h, w, 3), f[y0:y0 + h, x0:x0 + w])
    assert np.array_equal(s._frame, want) and not np.array_equal(want, f)
    assert positions == [(win[1], win[0])] and len(patches) == 1 and np.array_equal(patches[0], want[win[0]:win[0] + win[2], win[1]:win[1] + win[3]])
    expect = dict(windows=[win], filter=kind, radius=R or None, amount=amount, cell=cell, selected=1200)
    if lock:
        expect["locked"] = True
        assert np.array_equal(want[_lock_array() != 0], f[_lock_array() != 0])
    if history:
        expect["undoable"] = True
    if feather:
        expect["feather"] = 4
    assert info == expect
    assert np.array_equal(sel.plane, plane0) and sel.box == BOX and sel.count == 1200          # the selection stays what it was
    if history:
        # the lift is the undo slot: a single-window entry over the lift rectangle
        assert s.can_undo and len(s._undo) == 1 and s._undo[0][0] == lift_rect and not isinstance(s._undo[0][0], (serve._Sequence, serve._Regions))
        assert s.history_bytes_used == serve.window_saved_bytes(lift_rect[2], lift_rect[3])
    else:
        assert not s.can_undo


def test_undo_and_redo_restore_every_byte_also_through_a_server():
    stub = _Stub()
    srv = serve.BatchingServer(object(), max_batch=4, max_wait_s=0.01, window=True, max_grow=0)
    f = U._noise(HW, 5)
    s = serve.EditSession(srv.model, f, backend=stub, history=3)
    try:
        sel = s.select_lasso([RING])
        s.filter_selection(sel, "blur", radius=8, feather=2)
        one = s._frame.copy()
        s.filter_selection(sel, "pixelate", cell=7)
        two = s._frame.copy()
        assert not np.array_equal(one, f) and not np.array_equal(two, one) and len(s._undo) == 2
        r8, r0 = F.filter_rect(BOX, 8, HW), F.filter_rect(BOX, 0, HW)
        for _ in range(2):
            stub.calls.clear()
            patch, pos, u = s.undo()
            assert stub.calls[0] == ("swap", [r0[:2]], r0[2:]) and u == dict(window=r0, undo_depth=1, redo_depth=1) and np.array_equal(s._frame, one)
            s.undo()
            assert np.array_equal(s._frame, f) and not s.can_undo
            stub.calls.clear()
            s.redo()
            assert stub.calls[0] == ("swap", [r8[:2]], r8[2:]) and np.array_equal(s._frame, one)
            s.redo()
            assert np.array_equal(s._frame, two) and not s.can_redo
        srv.undo(s)
        assert np.array_equal(s._frame, one)
        srv.undo(s)
        assert np.array_equal(s._frame, f)
        srv.redo(s)
        srv.redo(s)
        assert np.array_equal(s._frame, two)
    finally:
        srv.close()


def test_history_bytes_a_failing_call_a_lock_and_encode():
    # the lift's slot is what history_bytes is checked against: R = 8 lifts 46 x 56, R = 0 lifts 30 x 40
    small = serve.window_saved_bytes(30, 40)
    assert serve.window_saved_bytes(46, 56) > small
    stub = _Stub()
    s, sel, f = _session(stub, history=3, history_bytes=small)
    _, _, info = s.filter_selection(sel, "pixelate")
    assert info["undoable"] is True and len(s._undo) == 1
    _, _, info = s.filter_selection(sel, "blur")                       # commits unjournalled, clears the history
    assert info["undoable"] is False and not s.can_undo and not s.can_redo and _names(stub).count("save") == 2
    _, _, info = s.filter_selection(sel, "sharpen", radius=1)          # R = 1 lifts 32 x 42: too large as well
    assert info["undoable"] is False

    class _No(_Stub):
        def filter_blur(self, *a):
            raise RuntimeError("the device said no")

    s, sel, f = _session(_No(), history=3)
    sk = np.zeros(HW, np.uint8)
    sk[50:60, 50:80] = 255
    s.edit(sk, max_grow=0)
    assert s.can_undo
    with pytest.raises(RuntimeError, match="said no"):
        s.filter_selection(sel)
    assert not s.can_undo and not s.can_redo
    # encode: one encoder call over the one window
    stub = _Stub()
    s, sel, f = _session(stub, lock=True, history=1)
    win = M.move_rect(BOX, (0, 0), HW)
    patches, positions, info = s.filter_selection(sel, "box", encode="png")
    assert patches == [b"png"] and _names(stub) == ["save", "filter_blur", "crop_png"] and stub.calls[2] == ("crop_png", [win]) and info["locked"]
    patches, _, _ = s.filter_selection(sel, "pixelate", encode=("jpg", 80))
    assert patches == [b"jpg"] and stub.calls[-1][:3] == ("crop_jpg", [win], 80)
    patches, _, _ = s.filter_selection(sel, "sharpen", encode=("jpg", 80, "420", True))
    assert patches == [b"jpg"] and stub.calls[-1] == ("crop_jpg", [win], 80, dict(subsampling="420", optimize=True))


def test_refusals_make_no_backend_call():
    stub = _Stub()
    s, sel, f = _session(stub, history=1)
    other = serve.EditSession(None, np.zeros((64, 64, 3), np.uint8), backend=_Stub()).select_lasso([[(1, 1), (30, 1), (15, 30)]])
    empty = s.combine(sel, sel, "subtract")
    stub.calls.clear()
    T = s.filter_selection
    bad = [lambda: T(other), lambda: T(sel.plane), lambda: T(None), lambda: T(empty), lambda: T(sel, "gauss"), lambda: T(sel, None), lambda: T(sel, 3),
           lambda: T(sel, radius=0), lambda: T(sel, radius=33), lambda: T(sel, radius=2.0), lambda: T(sel, radius=True), lambda: T(sel, radius="2"),
           lambda: T(sel, sigma=0), lambda: T(sel, sigma=-1.0), lambda: T(sel, sigma=8.5), lambda: T(sel, sigma="1"), lambda: T(sel, sigma=float("nan")),
           lambda: T(sel, amount=1.0), lambda: T(sel, cell=4), lambda: T(sel, "box", sigma=1.0), lambda: T(sel, "box", amount=-1.0), lambda: T(sel, "box", cell=2),
           lambda: T(sel, "sharpen", amount=0), lambda: T(sel, "sharpen", amount=-1.0), lambda: T(sel, "sharpen", amount=4.01),
           lambda: T(sel, "sharpen", amount="1"), lambda: T(sel, "sharpen", amount=True), lambda: T(sel, "sharpen", amount=float("nan")),
           lambda: T(sel, "sharpen", amount=0.001), lambda: T(sel, "sharpen", cell=4), lambda: T(sel, "sharpen", radius=40),
           lambda: T(sel, "pixelate", cell=1), lambda: T(sel, "pixelate", cell=65), lambda: T(sel, "pixelate", cell=4.0), lambda: T(sel, "pixelate", cell=True),
           lambda: T(sel, "pixelate", radius=2), lambda: T(sel, "pixelate", sigma=1.0), lambda: T(sel, "pixelate", amount=-1.0),
           lambda: T(sel, feather=17), lambda: T(sel, feather=2.5), lambda: T(sel, feather=-1), lambda: T(sel, encode="gif"), lambda: T(sel, encode=("jpg", 0))]
    for k, call in enumerate(bad):
        with pytest.raises((ValueError, TypeError)):
            call()
        assert stub.calls == [] and not s.can_undo, k
    with pytest.raises(ValueError, match="empty selection: nothing to filter"):
        T(empty)
    with pytest.raises(TypeError):
        T(sel.plane)
    with pytest.raises(ValueError, match="takes no cell"):
        T(sel, "blur", cell=4)
    assert stub.calls == []


def test_existing_calls_issue_what_they_issued():
    """every method of before, transform_selection included, on a backend WITH the two new calls never uses them and issues the
    very calls it issues on the backend of before, leaving the same frame"""
    sk = np.zeros(HW, np.uint8)
    sk[200:210, 300:330] = 255
    mask = np.zeros(HW, np.uint8)
    mask[200:230, 300:340] = 1
    f = U._noise(HW, 5)
    f[200:230, 300:340] = U.REGION
    seqs, frames = {}, {}
    for k, cls in enumerate((_WarpStub, _Stub)):
        for lock in (False, True):
            stub = cls()
            s = serve.EditSession(None, f, backend=stub, history=3)
            if lock:
                s.set_lock(mask)
            stub.calls.clear()
            s.edit(sk, max_grow=0)
            s.edit_strokes([([(30, 20), (60, 30)], 3), ([(500, 300), (520, 310)], 3)])
            s.fill(mask)
            s.fill_strokes([([(30, 20), (60, 30)], 3)])
            a = s.select_similar((210, 320))
            s.fill_similar((210, 320))
            b = s.select_lasso([RING], grow=2)
            c = s.combine(a, b, "xor")
            s.invert(c)
            s.fill_selection(b)
            s.fill_lasso([RING])
            _, _, info = s.move_selection(b, (10, 25), flip="h", feather=2)
            s.clone_selection(info["selection"], (-100, -200))
            s.transform_selection(b, scale=1.5, angle=30.0, offset=(10, 25.5))
            s.set_lock(b)
            b.rings()
            s.undo()
            s.undo()
            s.redo()
            seqs[k, lock], frames[k, lock] = list(stub.calls), s._frame.copy()
            assert stub.calls and not {"filter_blur", "filter_mosaic"} & set(_names(stub))
    for lock in (False, True):
        assert [c[0] for c in seqs[0, lock]] == [c[0] for c in seqs[1, lock]] and np.array_equal(frames[0, lock], frames[1, lock])
    # a backend of before cannot filter, and says so only when asked to
    s = serve.EditSession(None, f, backend=_WarpStub(), history=1)
    sel = s.select_lasso([RING])
    with pytest.raises(AttributeError):
        s.filter_selection(sel)
    assert not issubclass(_MoveStub, _Stub)


def test_model_backend_filter_calls():
    """_ModelBackend's two calls on a scripted model: one model call each, nothing downloaded"""
    class _Model:
        def __init__(self):
            self.calls = []

        def filter_blur_u8(self, frame, lift, lift_rect, sel, lock, box, taps, amount, feather):
            self.calls.append(("filter_blur_u8", tuple(lift_rect), tuple(box), tuple(taps), amount, feather))

        def filter_mosaic_u8(self, frame, lift, lift_rect, sel, lock, box, cell, amount, feather):
            self.calls.append(("filter_mosaic_u8", tuple(lift_rect), tuple(box), cell, amount, feather))

    be = serve._ModelBackend.__new__(serve._ModelBackend)
    be.model = _Model()
    assert be.filter_blur(None, None, (0, 0, 16, 23), None, None, (5, 7, 10, 20), [2048, 1024], -256, 3) is None
    assert be.filter_mosaic(None, None, (0, 0, 16, 23), None, None, (5, 7, 10, 20), 4, 256, 0) is None
    assert be.model.calls == [("filter_blur_u8", (0, 0, 16, 23), (5, 7, 10, 20), (2048, 1024), -256, 3), ("filter_mosaic_u8", (0, 0, 16, 23), (5, 7, 10, 20), 4, 256, 0)]


# ---- the C-ABI -------------------------------------------------------------------------------------------------------------
def test_abi_has_two_new_symbols_in_a_header_of_their_own():
    hdr = open(os.path.join(ROOT, "include", "sketchedit_filter.h")).read()
    declared = re.findall(r"^(?:int|size_t)\s+(se_\w+)\(", hdr, re.M)
    assert declared == _lib.abi_names("sketchedit_filter.h") == ["se_filter_blur_u8", "se_filter_mosaic_u8"]
    others = [n for n in _lib.abi_names() if n not in declared]
    for name in others:                                               # the header refers to other families by DESIGN section
        assert not re.search(r"\b%s\b" % name, hdr), name
    for name in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if name != "sketchedit_filter.h":
            assert "se_filter" not in open(os.path.join(ROOT, "include", name)).read(), name
    assert "se_filter.hip" in _lib.SOURCES and _lib.SOURCES[-1] == "se_api.hip"
    for define, value in (("SE_FILTER_MAX_RADIUS", "32"), ("SE_FILTER_ONE", "4096"), ("SE_FILTER_MAX_CELL", "64"), ("SE_FILTER_MIN_AMOUNT", r"\(-256\)"),
                          ("SE_FILTER_MAX_AMOUNT", "1024"), ("SE_FILTER_MAX_FEATHER", "16")):
        assert re.search(r"#define %s %s$" % (define, value), hdr, re.M), define
    assert (_lib.FILTER_MAX_RADIUS, _lib.FILTER_ONE, _lib.FILTER_MAX_CELL, _lib.FILTER_MIN_AMOUNT, _lib.FILTER_MAX_AMOUNT, _lib.FILTER_MAX_FEATHER) == \
        (32, 4096, 64, -256, 1024, 16) == (F.MAX_RADIUS, F.ONE, F.MAX_CELL, F.MIN_AMOUNT, F.MAX_AMOUNT, F.MAX_FEATHER)
    assert (serve.FILTER_MAX_RADIUS, serve.FILTER_ONE, serve.FILTER_MAX_CELL, serve.FILTER_MAX_AMOUNT * 256) == (32, 4096, 64, 1024)
    import ctypes
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    lib = ctypes.CDLL(_lib.LIB_PATH)                                    # the built library, as the other host tests load it
    for s in declared:
        getattr(lib, s)
    from sketchedit_amd import kernel_labels
    assert kernel_labels.label_of("void se::filter_blur_kernel<8>(unsigned char*, int)") == "filter_blur"
    for rc in (8, 16, 32):
        assert kernel_labels.label_of("filter_blur_kernel<%d>(unsigned char*, int)" % rc) == "filter_blur"
    assert kernel_labels.label_of("filter_mosaic_kernel(unsigned char*, int)") == "filter_mosaic"
    names, labels = abi_util.prof_labels()
    assert len(names) == len(labels) - 1 and labels[-1] == "PL_COUNT"
    i = names.index("filter_blur")
    assert names[i - 1:i + 3] == ["outline_emit", "filter_blur", "filter_mosaic", "move_drop"]                  # in front of move_drop, not appended
    assert labels[i - 1:i + 3] == ["PL_OUTLINE_EMIT", "PL_FILTER_BLUR", "PL_FILTER_MOSAIC", "PL_MOVE_DROP"]
    assert names[-2:] == ["warp_drop", "plane_warp"] and labels[-3:] == ["PL_WARP_DROP", "PL_PLANE_WARP", "PL_COUNT"]
    for label in ("filter_blur", "filter_mosaic"):
        assert label in set(kernel_labels.KERNEL_LABELS.values())
    from sketchedit_amd.models.editline2_model import EditLine2Model
    for name in ("filter_blur_u8", "filter_mosaic_u8"):
        assert callable(getattr(_lib.Engine, name)) and callable(getattr(EditLine2Model, name))
    for name in ("filter_blur", "filter_mosaic"):
        assert callable(getattr(serve._ModelBackend, name))


def test_the_kernels_cross_compile_for_gfx950(tmp_path):
    import shutil
    import subprocess
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc on this machine")
    obj = str(tmp_path / "se_filter.o")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(_lib.CSRC, "se_filter.hip"), "-o", obj])
    assert os.path.getsize(obj) > 0
