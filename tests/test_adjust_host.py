"""Adjust a selection's tone and colour, without a GPU: the statement's properties, the histogram and the table
builders against brute force, the kernels' arithmetic lane by lane with every access checked, the host helpers, the session against a
scripted backend that really edits a frame, the ABI."""
import os
import re

import numpy as np
import pytest

from sketchedit_amd import _lib, serve
import abi_util
import adjust_util as A
import lasso_util as L
import move_util as M
import select_util as U
from test_fill_host import _names
from test_filter_host import _Stub as _FilterStub
from test_move_host import BOX, HW, RING, _lock_array

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVERT = np.tile(np.arange(255, -1, -1, dtype=np.uint8), (3, 1))
EXTREME = [32768] * 9 + [1 << 20] * 3


# ---- the statement: ADJUST ----------------------------------------------------------------------------------------------------------------------
def test_known_answers_of_the_header():
    P = np.array([[200, 100, 50]])
    assert A.adjusted(P, None, A.GREY, 256).tolist() == [[124, 124, 124]] and A.adjusted(P, A.IDENTITY, A.GREY, 256).tolist() == [[124, 124, 124]]
    assert A.adjusted(P, A.IDENTITY, A.GREY, 128)[0, 0] == 162 and A.luma(P).tolist() == [124]
    h = np.zeros((4, 256), np.uint32)
    h[:, 50] = h[:, 150] = 10
    for which in (A.PER_CHANNEL, A.LUMA):
        lut = A.spec_lut(h, None, A.STRETCH, which, 0)
        assert [int(lut[c][v]) for c in range(3) for v in (50, 100, 150, 200)] == [0, 128, 255, 255] * 3
    h = np.zeros((4, 256), np.uint32)
    h[:, 10], h[:, 20], h[:, 30] = 1, 1, 2
    lut = A.spec_lut(h, None, A.EQUALIZE, A.LUMA)
    assert [int(lut[1][v]) for v in (10, 15, 20, 30)] == [0, 0, 85, 255]
    s, r = np.zeros((4, 256), np.uint32), np.zeros((4, 256), np.uint32)
    s[:, 10] = s[:, 20] = 2
    r[:, 100], r[:, 200] = 1, 3
    lut = A.spec_lut(s, r, A.MATCH, A.PER_CHANNEL)
    assert [int(lut[2][v]) for v in (5, 10, 20)] == [0, 200, 200]
    hdr = open(os.path.join(ROOT, "include", "sketchedit_adjust.h")).read()
    for text in ("(1225, 2404, 467)", "M = 124 in every channel", "a = 128 gives O[0] = 162", "Y(200, 100, 50) = 124", "lut[50] = 0, lut[100] = 128",
                 "lut[150] = lut[200] = 255", "lut[10] = lut[15] = 0, lut[20] = 85, lut[30] = 255", "lut[5] = 0, lut[10] = lut[20] = 200",
                 "26 118 144 < 2^31"):
        assert text in hdr, text
    assert 3 * 255 * 32768 + (1 << 20) + 2048 == 26118144


def _case(seed, hw=(37, 53), box=None, density=0.7):
    """noise: a frame (what is there now), another frame as it was when lifted, a selection, a lock, the lift of the box"""
    rng = np.random.RandomState(seed)
    Hi, Wi = hw
    frame = rng.randint(0, 256, (Hi, Wi, 3)).astype(np.uint8)
    before = rng.randint(0, 256, (Hi, Wi, 3)).astype(np.uint8)
    sel = np.where(rng.rand(Hi, Wi) < density, rng.randint(1, 256, (Hi, Wi)), 0).astype(np.uint8)
    lock = np.where(rng.rand(Hi, Wi) < 0.2, 255, 0).astype(np.uint8)
    box = box or (1, 2, Hi - 3, Wi - 1)
    rect = M.move_rect(box, (0, 0), hw)
    return frame, before, sel, lock, box, rect, M.slot_of(before, rect)


def _random_lut(seed):
    return np.random.RandomState(seed).randint(0, 256, (3, 256)).astype(np.uint8)


def _targets(sel, lock, box):
    tg = np.zeros(sel.shape, bool)
    tg[box[0]:box[2], box[1]:box[3]] = sel[box[0]:box[2], box[1]:box[3]] != 0
    return tg if lock is None else tg & (lock == 0)


def test_the_identity_and_the_two_ends_of_the_amount():
    frame, before, sel, lock, box, rect, slot = _case(1)
    tg = _targets(sel, None, box)
    for lut, mx, a in ((A.IDENTITY, None, 256), (None, serve.adjust_matrix(), 256), (_random_lut(2), A.GREY, 0), (A.IDENTITY, None, 0), (A.IDENTITY, None, 77)):
        out = A.spec_adjust(frame, slot, rect, sel, None, box, lut, mx, a)
        assert np.array_equal(out[tg], before[tg]) and np.array_equal(out[~tg], frame[~tg])
    lut = _random_lut(3)
    out = A.spec_adjust(frame, slot, rect, sel, None, box, lut, None, 256)                     # a = 256 gives M exactly
    want = np.stack([lut[c][before[..., c]] for c in range(3)], axis=-1)
    assert np.array_equal(out[tg], want[tg]) and not np.array_equal(out[tg], before[tg])


def test_the_table_comes_before_the_matrix():
    P = np.array([[200, 100, 50]])
    lut = np.array(A.IDENTITY)
    lut[0] = 0                                                          # red to 0, THEN grey: (2404 * 100 + 467 * 50 + 2048) >> 12 = 64
    assert A.adjusted(P, lut, A.GREY, 256).tolist() == [[64, 64, 64]]
    grey_then_table = [[0, 124, 124]]                                   # the other order would zero the grey's red
    assert A.adjusted(A.adjusted(P, None, A.GREY, 256), lut, None, 256).tolist() == grey_then_table
    swap = [0, 4096, 0, 4096, 0, 0, 0, 0, 4096, 0, 0, 0]                # red <-> green: the table's rows follow the INPUT channel
    lut2 = np.array(A.IDENTITY)
    lut2[0] = 7
    assert A.adjusted(P, lut2, swap, 256).tolist() == [[100, 7, 50]]


def test_both_clamps_and_int32_at_the_extreme_matrix():
    frame, before, sel, lock, box, rect, slot = _case(4)
    tg = _targets(sel, None, box)
    hot = [12288, 0, 0, 0, 12288, 0, 0, 0, 12288, -255 * 4096, -255 * 4096, -255 * 4096]       # 3 x - 255: 0 below 85, 255 from 170
    out = A.spec_adjust(frame, slot, rect, sel, None, box, None, hot, 256)
    assert (out[tg] == 0).sum() > 500 and (out[tg] == 255).sum() > 500
    P = np.full((1, 3), 255)
    assert A.adjusted(P, None, EXTREME, 256).tolist() == [[255] * 3] and A.adjusted(P, None, [-v for v in EXTREME], 256).tolist() == [[0] * 3]
    acc = 3 * 255 * 32768 + (1 << 20) + 2048
    assert acc < 1 << 31 and -acc + 4096 > -(1 << 31) and (-acc + 4096) >> 12 < 0        # the arithmetic shift keeps the sign
    assert A.adjusted(np.array([[10, 10, 10]]), None, [0] * 9 + [-2049, -2048, 2047], 256).tolist() == [[0, 0, 0]]       # (-1) >> 12 = -1 -> 0; 0; 4095 >> 12 = 0
    assert A.adjusted(np.array([[100, 100, 100]]), None, [0] * 9 + [4096 * 3 + 2047, 4096 * 3 + 2048, 0], 256).tolist() == [[3, 4, 0]]
    # the mix rounds half up and its shift is arithmetic: M below P
    assert A.adjusted(np.array([[3, 3, 3]]), np.zeros((3, 256), np.uint8), None, 128).tolist() == [[2, 2, 2]]          # 3 + ((128 * -3 + 128) >> 8) = 3 - 1
    assert A.adjusted(np.array([[0, 0, 0]]), np.full((3, 256), 3, np.uint8), None, 128).tolist() == [[2, 2, 2]]        # 0 + ((384 + 128) >> 8)


def test_nothing_but_unlocked_targets_changes():
    frame, before, sel, lock, box, rect, slot = _case(5)
    for f in (0, 4):
        out = A.spec_adjust(frame, slot, rect, sel, lock, box, INVERT, A.GREY, 256, f)
        tg = _targets(sel, lock, box)
        assert np.array_equal(out[~tg], frame[~tg]) and (out[tg] != frame[tg]).any()
        assert np.array_equal(out[lock != 0], frame[lock != 0])
    other = frame ^ 0xFF                                                # the frame's own bytes play no part in what is stored
    a, b = A.spec_adjust(frame, slot, rect, sel, lock, box, INVERT), A.spec_adjust(other, slot, rect, sel, lock, box, INVERT)
    assert np.array_equal(a[tg], b[tg])


def test_feather_follows_6t():
    hw, box = (37, 53), (0, 0, 20, 30)                                  # the box touches the frame's top left corner
    frame, before, _, _, _, _, _ = _case(6, hw, box)
    sel = np.zeros(hw, np.uint8)
    sel[0:12, 0:14] = 200
    sel[30:, 40:] = 255                                                 # selected, outside the box: never counted, never written
    rect = M.move_rect(box, (0, 0), hw)
    slot = M.slot_of(before, rect)
    f = 3
    n = (2 * f + 1) ** 2
    c = A.counts(sel, box, f)
    assert c[5, 5] == n and c[0, 0] == 16 and c[11, 13] == 16 and c[5, 13] == 4 * 7
    hard = A.spec_adjust(frame, slot, rect, sel, None, box, INVERT, None, 256, 0)
    soft = A.spec_adjust(frame, slot, rect, sel, None, box, INVERT, None, 256, f)
    assert np.array_equal(soft[3:9, 3:11], hard[3:9, 3:11])             # c == n stores O
    rim = np.zeros(hw, bool)
    rim[0:12, 11:14] = True
    P = before.astype(int)
    lo, hi = np.minimum(P, hard.astype(int)), np.maximum(P, hard.astype(int))
    strictly = rim[..., None] & (hi - lo > n)
    assert strictly.any() and ((soft > lo) & (soft < hi))[strictly].all()          # a rim pixel lies strictly between P and O
    assert np.array_equal(soft[sel == 0], frame[sel == 0]) and np.array_equal(soft[30:], frame[30:])
    lock = np.zeros(hw, np.uint8)
    lock[0:12, 0:7] = 255                                               # the lock takes pixels out of the targets, not out of the count
    locked = A.spec_adjust(frame, slot, rect, sel, lock, box, INVERT, None, 256, f)
    assert np.array_equal(locked[lock != 0], frame[lock != 0]) and np.array_equal(locked[:, 7:], soft[:, 7:])


# ---- the statement: HIST and LUT ------------------------------------------------------------------------------------------------------------------
def test_hist_against_bincount_on_boxes_at_every_edge():
    hw = (37, 53)
    frame, _, sel, _, _, _, _ = _case(7, hw)
    for box in ((0, 0, 37, 53), (0, 0, 5, 7), (30, 40, 37, 53), (0, 46, 37, 53), (10, 0, 11, 53), (36, 52, 37, 53), (9, 9, 20, 31)):
        for s in (sel, None):
            got = A.spec_hist(frame, s, box)
            assert got.shape == (4, 256) and got.dtype == np.uint32
            px = [frame[y, x] for y in range(box[0], box[2]) for x in range(box[1], box[3]) if s is None or s[y, x]]
            for ch in range(3):
                assert np.array_equal(got[ch], np.bincount([int(p[ch]) for p in px], minlength=256))
            assert np.array_equal(got[3], np.bincount([(77 * int(p[0]) + 150 * int(p[1]) + 29 * int(p[2]) + 128) >> 8 for p in px], minlength=256))
            assert got.sum() == 4 * len(px)
    assert A.spec_hist(frame, np.zeros(hw, np.uint8), (0, 0, 37, 53)).sum() == 0
    assert A.luma([[255, 255, 255]]).tolist() == [255] and A.luma([[0, 0, 0]]).tolist() == [0] and 77 + 150 + 29 == 256


def _brute_row(mode, h, href, k):
    """the rule read literally, value by value, in Python ints"""
    h = [int(v) for v in h]
    N = sum(h)
    sums = {}

    def cdf(hh, v):                                             # hh[0] + .. + hh[v], added up once per row
        if id(hh) not in sums:
            sums[id(hh)] = [sum(hh[:u + 1]) for u in range(256)]
        return sums[id(hh)][v] if v >= 0 else 0

    ident = list(range(256))
    if N == 0:
        return ident
    if mode == A.STRETCH:
        t = N * k // 1000
        lo = next(v for v in range(256) if cdf(h, v) > t)
        hi = next(v for v in range(255, -1, -1) if N - cdf(h, v - 1) > t)
        if hi == lo:
            return ident
        return [0 if v < lo else max(0, min(255, ((v - lo) * 255 + (hi - lo) // 2) // (hi - lo))) for v in range(256)]
    if mode == A.EQUALIZE:
        m = next(v for v in range(256) if h[v] > 0)
        c0 = cdf(h, m)
        if N == c0:
            return ident
        return [0 if v < m else ((cdf(h, v) - c0) * 255 + (N - c0) // 2) // (N - c0) for v in range(256)]
    href = [int(v) for v in href]
    Nr = sum(href)
    if Nr == 0:
        return ident
    return [next(u for u in range(256) if cdf(href, u) * N >= cdf(h, v) * Nr) for v in range(256)]


def _hists():
    rng = np.random.RandomState(8)
    frame = rng.randint(0, 256, (40, 50, 3)).astype(np.uint8)
    dark = (frame // 3 + 20).astype(np.uint8)
    flat = np.zeros((4, 256), np.uint32)
    flat[0, 17], flat[1, 200], flat[2, 0], flat[3, 255] = 1200, 1200, 1200, 1200
    two = np.zeros((4, 256), np.uint32)
    two[:, 50] = 999
    two[:, 150] = 1
    ends = np.zeros((4, 256), np.uint32)
    ends[:, 0] = ends[:, 255] = 5
    return dict(random=A.spec_hist(frame, None, (0, 0, 40, 50)), dark=A.spec_hist(dark, None, (0, 0, 40, 50)), flat=flat,
                empty=np.zeros((4, 256), np.uint32), two=two, ends=ends)


@pytest.mark.parametrize("mode", [A.STRETCH, A.EQUALIZE, A.MATCH], ids=["stretch", "equalize", "match"])
@pytest.mark.parametrize("which", [A.PER_CHANNEL, A.LUMA], ids=["channels", "luma"])
def test_lut_against_brute_force(mode, which):
    hs = _hists()
    for name, h in hs.items():
        for rname, href in (hs.items() if mode == A.MATCH else [(None, None)]):
            for k in ((0, 1, 10, 200) if mode == A.STRETCH else (0,)):
                got = A.spec_lut(h, href, mode, which, k)
                for c in range(3):
                    r = 3 if which == A.LUMA else c
                    assert got[c].tolist() == _brute_row(mode, h[r], None if href is None else href[r], k), (name, rname, k, c)
                assert np.array_equal(got, A.lanes_lut(h, href, mode, which, k)), (name, rname, k)
                if name == "empty" or rname == "empty" or (name == "flat" and mode != A.MATCH):
                    assert np.array_equal(got, A.IDENTITY)
                if mode == A.MATCH:
                    assert (np.diff(got.astype(int), axis=1) >= 0).all()          # monotone
                    if name == rname and name in ("random", "dark"):               # onto itself: every value that occurs stays
                        for c in range(3):
                            occ = np.flatnonzero(h[3 if which == A.LUMA else c])
                            assert np.array_equal(got[c][occ], occ)
    if mode == A.EQUALIZE:
        assert A.spec_lut(hs["ends"], None, mode, which)[0].tolist() == [0] + [0] * 254 + [255]
        assert A.spec_lut(hs["two"], None, mode, which)[0][150] == 255
    if mode == A.STRETCH:
        assert A.spec_lut(hs["two"], None, mode, which, 0)[0][100] == 128 and np.array_equal(A.spec_lut(hs["two"], None, mode, which, 1), A.IDENTITY)


def test_lo_never_passes_hi_for_any_clip():
    hs = _hists()
    one = np.zeros((4, 256), np.uint32)
    one[:, 9] = 1
    three = np.zeros((4, 256), np.uint32)
    three[:, 3] = three[:, 4] = three[:, 250] = 1
    for h in list(hs.values()) + [one, three]:
        for k in range(0, 201):
            N = int(h[3].sum())
            assert 2 * (N * k // 1000) < N or N == 0
            A.spec_lut(h, None, A.STRETCH, A.LUMA, k)                   # asserts lo <= hi
            A.lanes_lut(h, None, A.STRETCH, A.LUMA, k)                  # asserts one writer of lo and one of hi


def test_the_products_fit_64_bits_at_2_to_the_25_pixels():
    n = 1 << 25
    a, b = np.zeros((4, 256), np.uint32), np.zeros((4, 256), np.uint32)
    a[:, 255] = n                                                       # cdf[255] N_ref = 2^50
    b[:, 0], b[:, 255] = n // 2, n // 2
    assert n * n == 1 << 50
    for src, ref in ((a, b), (b, a), (a, a)):
        got = A.lanes_lut(src, ref, A.MATCH, A.PER_CHANNEL, 0)          # asserts every product < 2^64
        assert np.array_equal(got, A.spec_lut(src, ref, A.MATCH, A.PER_CHANNEL))
    for mode in (A.STRETCH, A.EQUALIZE):
        assert np.array_equal(A.lanes_lut(b, None, mode, A.LUMA, 200), A.spec_lut(b, None, mode, A.LUMA, 200))
    big = np.full((4, 256), (1 << 32) - 1, np.uint32)                   # the words' own limit: 2^40 in all, and (N - c0) 255 still fits
    assert np.array_equal(A.lanes_lut(big, None, A.EQUALIZE, A.LUMA, 0), A.spec_lut(big, None, A.EQUALIZE, A.LUMA))


# ---- the kernels' arithmetic, lane by lane -----------------------------------------------------------------------------------------------------
def _place(k, frame, sel, lock, slot, lut):
    Hi, Wi = sel.shape
    mem = A.Memory(32768 + 5 * Hi * Wi + slot.size + 4096 * 257)
    fa = mem.put(1024 + k % 4, frame)
    sa = mem.put(fa + 3 * Hi * Wi + 1031, sel)
    la = mem.put(sa + Hi * Wi + 1033, lock)
    pa = mem.put((la + Hi * Wi + 1024 + 15) // 16 * 16, slot)
    ta = mem.put(pa + slot.size + 1021 + k % 3, lut)
    return mem, fa, sa, la, pa, ta


def _only_changed(mem, clean, lo, n):
    changed = np.flatnonzero(mem.mem != clean)
    return changed.size > 0 and lo <= changed.min() and changed.max() < lo + n


SIZES = [(16, 16), (37, 53), (65, 129)]
MIX = [3000, 1500, -404, -700, 5000, -204, 100, -900, 4896, 4096 * 9, -4096 * 14, 2000]


@pytest.mark.parametrize("hw", SIZES, ids=lambda hw: "%dx%d" % hw)
@pytest.mark.parametrize("group", ["table", "matrix", "both", "feather"])
def test_tiled_adjust_is_the_statement(hw, group):
    """locked and not, the frame at every byte offset mod 4, the table at every offset mod 3 (so mod 4 too over the runs)"""
    Hi, Wi = hw
    runs = dict(table=[(True, False, 256, 0)], matrix=[(False, True, 256, 0)], both=[(True, True, a, 0) for a in (1, 128, 256)],
                feather=[(True, True, 200, f) for f in (1, 7, 16)])[group]
    k = 0
    for with_lut, with_mx, a, f in runs:
        for locked in (False, True):
            for off in range(4 if len(runs) == 1 else 2):
                box = (0, 0, Hi, Wi) if (k % 3 == 0 or Hi == 16) else (1, 2, Hi - 3, Wi - 1)
                frame, before, sel, lock, box, rect, slot = _case(100 + k, hw, box)
                lut = _random_lut(k)
                mem, fa, sa, la, pa, ta = _place(k, frame, sel, lock, slot, lut)
                clean = mem.mem.copy()
                tiles, es, el = A.tiled_adjust(mem, fa, Hi, Wi, pa, rect, sa, la if locked else None, box, ta if with_lut else None,
                                               MIX if with_mx else None, a, f)
                want = A.spec_adjust(frame, slot, rect, sel, lock if locked else None, box, lut if with_lut else None, MIX if with_mx else None, a, f)
                assert np.array_equal(mem.get(fa, frame.shape), want) and not np.array_equal(want, frame), (hw, group, a, f, locked)
                assert _only_changed(mem, clean, fa, 3 * Hi * Wi)
                assert tiles == -(-(box[2] - box[0]) // 16) * -(-(box[3] - box[1]) // 64) and es + el < tiles
                k += 1
    assert {(1024 + i % 4) % 4 for i in range(k)} == {0, 1, 2, 3}


def test_a_tile_without_targets_loads_nothing_but_the_planes():
    hw = (65, 129)
    frame, before, _, _, box, rect, slot = _case(9, hw, (0, 0, 65, 129))
    sel = np.zeros(hw, np.uint8)
    sel[3:9, 5:30] = 7                                                  # tile (0, 0)
    sel[40:44, 70:90] = 9                                               # tile (2, 1), locked whole
    lock = np.zeros(hw, np.uint8)
    lock[38:48, 64:128] = 255
    for f in (0, 5):
        mem, fa, sa, la, pa, ta = _place(1, frame, sel, lock, slot, INVERT)
        assert A.tiled_adjust(mem, fa, 65, 129, pa, rect, sa, la, box, ta, A.GREY, 256, f) == (15, 13, 1)
        assert np.array_equal(mem.get(fa, frame.shape), A.spec_adjust(frame, slot, rect, sel, lock, box, INVERT, A.GREY, 256, f))
        mem, fa, sa, la, pa, ta = _place(2, frame, sel, lock, slot, INVERT)
        assert A.tiled_adjust(mem, fa, 65, 129, pa, rect, sa, None, box, ta, None, 256, f) == (15, 13, 0)


@pytest.mark.parametrize("hw", SIZES, ids=lambda hw: "%dx%d" % hw)
def test_tiled_hist_is_the_statement(hw):
    """noise and a flat frame, with and without S, boxes at the edges, the frame at every byte offset mod 4, several grids: the same
    1024 words; a flat selection folds every wave's adds"""
    Hi, Wi = hw
    k = 0
    for flat in (False, True):
        for with_sel in (True, False):
            for box in ((0, 0, Hi, Wi), (1, 2, Hi - 3, Wi - 1), (Hi - 1, Wi - 1, Hi, Wi), (0, Wi - 5, Hi, Wi)):
                frame, _, sel, lock, _, _, slot = _case(200 + k, hw)
                if flat:
                    frame[...] = (200, 100, 50)
                mem, fa, sa, la, pa, ta = _place(k, frame, sel, lock, slot, INVERT)
                slabs, hist = (ta + 768 + 1027) // 256 * 256, (ta + 768 + 1027) // 256 * 256 + 4096 * 256 + 4
                mem.mem[slabs:hist + 4096] = 0x5A                       # garbage: every word that is read is written first
                clean = mem.mem.copy()
                tiles = -(-(box[2] - box[0]) // 16) * -(-(box[3] - box[1]) // 64)
                want = A.spec_hist(frame, sel if with_sel else None, box)
                for groups in sorted({None, 1, min(tiles, 3)}, key=str):
                    G, folded, single = A.tiled_hist(mem, fa, Hi, Wi, sa if with_sel else None, box, slabs, hist, groups)
                    got = mem.mem[hist:hist + 4096].view("<u4").reshape(4, 256)
                    assert np.array_equal(got, want), (hw, flat, with_sel, box, groups)
                    assert G == (groups or min(tiles, 256))
                    if flat:
                        assert single == 0 and (folded > 0) == (want.sum() > 0) and got[3, 124] == got.sum() // 4          # (the one pixel may be unselected)
                assert _only_changed(mem, clean, slabs, hist + 4096 - slabs)
                k += 1


# ---- the host helpers ---------------------------------------------------------------------------------------------------------------------------
def test_adjust_lut_rows_and_its_order():
    at = lambda **kw: [int(serve.adjust_lut(**kw)[0][v]) for v in (0, 1, 50, 100, 128, 200, 255)]       # noqa: E731
    assert at() == [0, 1, 50, 100, 128, 200, 255] and np.array_equal(serve.adjust_lut(), A.IDENTITY)
    assert at(brightness=20) == [20, 21, 70, 120, 148, 220, 255]
    assert at(contrast=50) == [0, 0, 11, 86, 128, 236, 255]
    assert at(gamma=2.0) == [0, 16, 113, 160, 181, 226, 255]
    assert at(levels=(50, 150)) == [0, 0, 0, 128, 199, 255, 255]
    assert at(invert=True) == [255, 254, 205, 155, 127, 55, 0]
    assert at(posterize=4) == [0, 0, 0, 85, 170, 255, 255]
    assert at(curve=[(0, 0), (128, 192), (255, 255)]) == [0, 2, 75, 150, 192, 228, 255]
    assert at(levels=(10, 240, 20, 230), gamma=0.5, brightness=-10, contrast=-20, curve=[(0, 10), (255, 200)], posterize=8, invert=True) == \
        [255, 255, 255, 219, 219, 146, 109]
    # the order: levels before brightness (the other order would give min(255, (v + 100 - 50) * 2.55)), invert last
    assert at(levels=(50, 150), brightness=100)[2] == 100 and at(brightness=100, invert=True)[0] == 155
    assert at(posterize=2, invert=True) == [255, 255, 255, 255, 0, 0, 0]
    t = serve.adjust_lut(contrast=-100)
    assert t.shape == (3, 256) and t.dtype == np.uint8 and (t == 128).all() and np.array_equal(t[0], t[1]) and np.array_equal(t[0], t[2])
    for bad in (dict(brightness=256), dict(brightness="1"), dict(contrast=101), dict(contrast=True), dict(gamma=0), dict(gamma=11), dict(gamma=None),
                dict(levels=(5,)), dict(levels=(9, 9)), dict(levels=(10, 5)), dict(levels=(0, 256)), dict(levels=(0.0, 255)), dict(levels=5),
                dict(curve=[(0, 0)]), dict(curve=[(5, 0), (5, 9)]), dict(curve=[(9, 0), (5, 9)]), dict(curve=[(0, 0), (300, 9)]), dict(curve=7),
                dict(curve=[(0, 0), (1.5, 2)]), dict(invert=1), dict(posterize=1), dict(posterize=257), dict(posterize=4.0), dict(gamma=float("nan"))):
        with pytest.raises(ValueError):
            serve.adjust_lut(**bad)


def test_adjust_matrix_rows_sum_to_one():
    assert serve.adjust_matrix(saturation=0) == A.GREY == list(serve.ADJUST_GREY) * 3 + [0, 0, 0]
    assert serve.adjust_matrix() == [4096, 0, 0, 0, 4096, 0, 0, 0, 4096, 0, 0, 0]
    assert serve.adjust_matrix(1.5, 30) == [4694, -2522, 1924, 1147, 4572, -1623, -2401, 1025, 5472, 0, 0, 0]
    assert serve.adjust_matrix(mix=[[1, 0, 0, 10], [0, 1, 0, 0], [0, 0, .5, -3]]) == [4096, 0, 0, 0, 4096, 0, 0, 0, 2048, 40960, 0, -12288]
    for s in (0, 0.3, 1, 1.7, 4):
        for h in (-360, -95.5, 0, 30, 120, 180, 359):
            m = serve.adjust_matrix(s, h)
            assert all(type(v) is int for v in m) and m[9:] == [0, 0, 0]
            assert [sum(m[3 * c:3 * c + 3]) for c in range(3)] == [4096] * 3          # a grey pixel stays what it is
            assert max(abs(v) for v in m) <= serve.ADJUST_MAX_COEF
            assert A.adjusted(np.array([[77, 77, 77]]), None, m, 256).tolist() == [[77, 77, 77]]
    third = serve.adjust_matrix(1, 120)                                  # a third of a turn about the grey axis permutes the channels
    assert A.adjusted(np.array([[200, 100, 50]]), None, third, 256).tolist() in ([[50, 200, 100]], [[100, 50, 200]])
    assert serve.adjust_matrix(1, 360) == serve.adjust_matrix()
    for bad in (dict(saturation=-0.1), dict(saturation=4.1), dict(saturation="1"), dict(hue=361), dict(hue=None), dict(mix=[[1, 0, 0]] * 2),
                dict(mix=[[1, 0]] * 3), dict(mix=[[9, 0, 0]] * 3), dict(mix=[[1, 0, 0, 257]] * 3), dict(mix=[[1, 0, 0], [0, 1, 0, 0], [0, 0, 1]]),
                dict(mix=5), dict(mix=[[1, 0, 0]] * 3, saturation=0.5), dict(mix=[[1, 0, 0]] * 3, hue=10), dict(mix=[["a", 0, 0]] * 3)):
        with pytest.raises(ValueError):
            serve.adjust_matrix(**bad)


# ---- the sessions against a scripted backend -------------------------------------------------------------------------------------------------
class _Stub(_FilterStub):
    """... with the three calls of DESIGN.md 6u, which are the statement; a hist record and a table "on the device" are arrays"""

    def adjust(self, frame, lift, lift_rect, plane, lock, box, lut, matrix, amount, feather):
        self.calls.append(("adjust", tuple(lift_rect), id(plane), None if lock is None else id(lock), tuple(box), None if lut is None else id(lut),
                           None if matrix is None else tuple(matrix), amount, feather))
        self.lift, self.lut = lift.copy(), None if lut is None else np.array(lut)
        frame[...] = A.spec_adjust(frame, lift, lift_rect, plane, lock, box, lut, matrix, amount, feather)

    def hist(self, frame, plane, box):
        self.calls.append(("hist", None if plane is None else id(plane), tuple(box)))
        return A.spec_hist(frame, plane, box).view(np.int32)

    def hist_lut(self, src, ref, mode, which, clip):
        self.calls.append(("hist_lut", id(src), None if ref is None else id(ref), mode, which, clip))
        self.table = A.spec_lut(src.view(np.uint32), None if ref is None else ref.view(np.uint32), mode, which, clip)
        return self.table

    def download(self, t):
        self.calls.append(("download", tuple(t.shape)))
        return t.copy()


RING2 = [(100, 50), (160, 50), (160, 90), (100, 90)]                     # a second selection: rows 50 .. 89, columns 100 .. 159


def _session(stub, lock=False, **kw):
    f = U._noise(HW, 5)
    f[BOX[0]:BOX[2], BOX[1]:BOX[3]] //= 2                              # a dark object: levels and match have something to do
    s = serve.EditSession(None, f, backend=stub, **kw)
    if lock:
        s.set_lock(_lock_array())
    sel = s.select_lasso([RING])
    stub.calls.clear()
    return s, sel, f


WIN = (200, 300, 30, 40)
CASES = [("lut", dict(lut=INVERT), ["save", "adjust", "crop"]),
         ("matrix", dict(matrix=A.GREY, amount=0.5), ["save", "adjust", "crop"]),
         ("lut+matrix", dict(lut=INVERT[0], matrix=MIX), ["save", "adjust", "crop"]),
         ("levels", dict(auto="levels", clip=10, which="channels"), ["save", "hist", "hist_lut", "adjust", "crop"]),
         ("equalize", dict(auto="equalize", matrix=A.GREY), ["save", "hist", "hist_lut", "adjust", "crop"]),
         ("match", dict(auto="match", reference="OTHER"), ["save", "hist", "hist", "hist_lut", "adjust", "crop"]),
         ("rim", dict(auto="match", reference=("rim", 8), which="channels"), ["save", "grow", "combine", "hist", "hist", "hist_lut", "adjust", "crop"])]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
@pytest.mark.parametrize("lock", [False, True])
@pytest.mark.parametrize("history", [0, 2])
@pytest.mark.parametrize("feather", [None, 4])
def test_adjust_issues_one_save_and_one_launch(case, lock, history, feather):
    name, kw, names = case
    kw = dict(kw)
    stub = _Stub()
    s, sel, f = _session(stub, lock, history=history)
    other = None
    if kw.get("reference") == "OTHER":
        other = kw["reference"] = s.select_lasso([RING2])
        stub.calls.clear()
    plane0 = sel.plane.copy()
    patches, positions, info = s.adjust_selection(sel, feather=feather, **kw)
    assert _names(stub) == names and stub.calls[0] == ("save", [WIN[:2]], WIN[2:])
    lk, lka = s._lock_plane, _lock_array() if lock else None
    # the table the statement makes of the ORIGINAL frame (the lock plays no part in a histogram)
    auto, which = kw.get("auto"), A.LUMA if kw.get("which", "luma") == "luma" else A.PER_CHANNEL
    if auto is None:
        table = None if "lut" not in kw else np.broadcast_to(kw["lut"], (3, 256))
    else:
        src = A.spec_hist(f, plane0, BOX)
        ref = None
        if name == "match":
            ref = A.spec_hist(f, other.plane, other.box)
        elif name == "rim":
            ring = L.spec_combine(U.spec_grow(plane0 != 0, 8), plane0, 1)
            rbox = L.box_count(ring)[0]
            assert rbox == (192, 292, 238, 348) and stub.calls[1][2] == 8 and stub.calls[2][3] == 1
            ref = A.spec_hist(f, ring, rbox)
            hists = [c for c in stub.calls if c[0] == "hist"]
            assert hists[0] == ("hist", id(sel.plane), BOX) and hists[1][2] == rbox
        table = A.spec_lut(src, ref, dict(levels=0, equalize=1, match=2)[auto], which, kw.get("clip", 0))
        lut_call = [c for c in stub.calls if c[0] == "hist_lut"][0]
        assert lut_call[3:] == (dict(levels=0, equalize=1, match=2)[auto], which, kw.get("clip", 0)) and (lut_call[2] is None) == (auto != "match")
        assert np.array_equal(stub.table, table) and not np.array_equal(table, A.IDENTITY)
        assert "download" not in [c[0] for c in stub.calls]               # nothing comes down between the histograms and the launch
    q8 = int(round(256 * kw.get("amount", 1.0)))
    call = [c for c in stub.calls if c[0] == "adjust"][0]
    assert call[1:5] == (WIN, id(sel.plane), None if lk is None else id(lk), BOX) and call[6:] == (None if "matrix" not in kw else tuple(kw["matrix"]), q8, feather or 0)
    assert (call[5] is None) == (table is None) and (table is None or np.array_equal(stub.lut, table))
    want = A.spec_adjust(f, M.slot_of(f, WIN), WIN, plane0, lka, BOX, table, kw.get("matrix"), q8, feather or 0)
    assert stub.calls[-1] == ("crop", WIN)
    assert np.array_equal(stub.lift[:, :120].reshape(30, 40, 3), f[200:230, 300:340])
    assert np.array_equal(s._frame, want) and not np.array_equal(want, f)
    assert positions == [(300, 200)] and len(patches) == 1 and np.array_equal(patches[0], want[200:230, 300:340])
    what = "+".join(k for k in ("lut", "auto", "matrix") if k in kw)
    expect = dict(windows=[WIN], adjust=what, auto=auto, which=kw.get("which", "luma") if auto else None, amount=kw.get("amount", 1.0), selected=1200)
    if lock:
        expect["locked"] = True
        assert np.array_equal(want[lka != 0], f[lka != 0])
    if history:
        expect["undoable"] = True
    if feather:
        expect["feather"] = 4
    assert info == expect
    assert np.array_equal(sel.plane, plane0) and sel.box == BOX and sel.count == 1200          # the selection stays what it was
    if history:
        assert s.can_undo and len(s._undo) == 1 and s._undo[0][0] == WIN and not isinstance(s._undo[0][0], (serve._Sequence, serve._Regions))
        assert s.history_bytes_used == serve.window_saved_bytes(30, 40)
        s.undo()
        assert np.array_equal(s._frame, f)
        s.redo()
        assert np.array_equal(s._frame, want)
    else:
        assert not s.can_undo


def test_match_makes_the_object_look_like_its_surroundings():
    stub = _Stub()
    s, sel, f = _session(stub)
    before = f[200:230, 300:340].astype(float).mean()
    around = A.luma(f[192:238, 292:348]).astype(float)
    s.adjust_selection(sel, auto="match", reference=("rim", 8))
    after = s._frame[200:230, 300:340].astype(float).mean()
    assert before < 70 and abs(after - 127.5) < 6 and abs(around.mean() - 127.5) > 6       # the dark object came up to the noise around it
    # a selection that is the whole frame has no rim: the identity, and still one launch
    stub = _Stub()
    s = serve.EditSession(None, f, backend=stub, history=1)
    whole = s.invert(s.combine(sel2 := s.select_lasso([RING]), sel2, "subtract"))
    assert whole.count == HW[0] * HW[1]
    stub.calls.clear()
    _, _, info = s.adjust_selection(whole, auto="match", reference=("rim", 3))
    assert np.array_equal(s._frame, f) and np.array_equal(stub.table, A.IDENTITY) and _names(stub).count("adjust") == 1 and info["undoable"] is True


def test_undo_and_redo_restore_every_byte_also_through_a_server():
    stub = _Stub()
    srv = serve.BatchingServer(object(), max_batch=4, max_wait_s=0.01, window=True, max_grow=0)
    s, sel, f = _session(stub, history=3)
    s = serve.EditSession(srv.model, f, backend=stub, history=3)
    try:
        sel = s.select_lasso([RING])
        s.adjust_selection(sel, lut=serve.adjust_lut(brightness=40), feather=2)
        one = s._frame.copy()
        s.adjust_selection(sel, auto="equalize", matrix=serve.adjust_matrix(saturation=0))
        two = s._frame.copy()
        assert not np.array_equal(one, f) and not np.array_equal(two, one) and len(s._undo) == 2
        for _ in range(2):
            stub.calls.clear()
            patch, pos, u = s.undo()
            assert stub.calls[0] == ("swap", [WIN[:2]], WIN[2:]) and u == dict(window=WIN, undo_depth=1, redo_depth=1) and np.array_equal(s._frame, one)
            s.undo()
            assert np.array_equal(s._frame, f) and not s.can_undo
            s.redo()
            assert np.array_equal(s._frame, one)
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


def test_history_bytes_a_failing_call_and_encode():
    small = serve.window_saved_bytes(30, 40)
    stub = _Stub()
    s, sel, f = _session(stub, history=3, history_bytes=small)
    _, _, info = s.adjust_selection(sel, lut=INVERT)
    assert info["undoable"] is True and len(s._undo) == 1
    s, sel, f = _session(stub, history=3, history_bytes=small - 1)      # a lift above history_bytes commits unjournalled
    sk = np.zeros(HW, np.uint8)
    _, _, info = s.adjust_selection(sel, lut=INVERT)
    assert info["undoable"] is False and not s.can_undo and not s.can_redo and np.array_equal(s._frame[200:230, 300:340], 255 - f[200:230, 300:340])

    class _No(_Stub):
        def adjust(self, *a):
            raise RuntimeError("the device said no")

    class _NoHist(_Stub):
        def hist_lut(self, *a):
            raise RuntimeError("no table")

    s, sel, f = _session(_No(), history=3)
    sk[50:60, 50:80] = 255
    s.edit(sk, max_grow=0)
    assert s.can_undo
    with pytest.raises(RuntimeError, match="said no"):
        s.adjust_selection(sel, lut=INVERT)
    assert not s.can_undo and not s.can_redo                            # the adjustment may be in the frame
    s, sel, f = _session(_NoHist(), history=3)
    s.edit(sk, max_grow=0)
    with pytest.raises(RuntimeError, match="no table"):
        s.adjust_selection(sel, auto="levels")
    assert s.can_undo                                                   # nothing was launched: the history stands
    stub = _Stub()
    s, sel, f = _session(stub, lock=True, history=1)
    patches, positions, info = s.adjust_selection(sel, lut=INVERT, encode="png")
    assert patches == [b"png"] and _names(stub) == ["save", "adjust", "crop_png"] and stub.calls[-1] == ("crop_png", [WIN]) and info["locked"]
    patches, _, _ = s.adjust_selection(sel, auto="levels", encode=("jpg", 80))
    assert patches == [b"jpg"] and stub.calls[-1][:3] == ("crop_jpg", [WIN], 80)
    patches, _, _ = s.adjust_selection(sel, matrix=A.GREY, encode=("jpg", 80, "420", True))
    assert patches == [b"jpg"] and stub.calls[-1] == ("crop_jpg", [WIN], 80, dict(subsampling="420", optimize=True))


def test_histogram_is_one_download():
    stub = _Stub()
    s, sel, f = _session(stub, lock=True)
    got = s.histogram(sel)
    assert got.dtype == np.uint32 and got.shape == (4, 256) and np.array_equal(got, A.spec_hist(f, sel.plane, BOX)) and got.sum() == 4 * 1200
    assert stub.calls == [("hist", id(sel.plane), BOX), ("download", (4, 256))]
    stub.calls.clear()
    assert np.array_equal(s.histogram(), A.spec_hist(f, None, (0, 0) + HW)) and stub.calls[0] == ("hist", None, (0, 0) + HW)
    empty = s.combine(sel, sel, "subtract")
    stub.calls.clear()
    assert s.histogram(empty).sum() == 0 and stub.calls == []
    with pytest.raises(TypeError):
        s.histogram(sel.plane)
    other = serve.EditSession(None, np.zeros((64, 64, 3), np.uint8), backend=_Stub()).select_lasso([[(1, 1), (30, 1), (15, 30)]])
    with pytest.raises(ValueError):
        s.histogram(other)
    assert stub.calls == []


def test_refusals_make_no_backend_call():
    stub = _Stub()
    s, sel, f = _session(stub, history=1)
    other = serve.EditSession(None, np.zeros((64, 64, 3), np.uint8), backend=_Stub()).select_lasso([[(1, 1), (30, 1), (15, 30)]])
    empty = s.combine(sel, sel, "subtract")
    ref = s.select_lasso([RING2])
    stub.calls.clear()
    T = s.adjust_selection
    ok = dict(lut=INVERT)
    bad = [lambda: T(other, **ok), lambda: T(sel.plane, **ok), lambda: T(None, **ok), lambda: T(empty, **ok), lambda: T(sel),
           lambda: T(sel, lut=INVERT, auto="levels"), lambda: T(sel, lut=np.zeros((3, 255), np.uint8)), lambda: T(sel, lut=np.zeros((3, 256))),
           lambda: T(sel, lut=np.full((3, 256), 256)), lambda: T(sel, lut=np.full(256, -1)), lambda: T(sel, lut="invert"), lambda: T(sel, lut=5),
           lambda: T(sel, matrix=[4096] * 11), lambda: T(sel, matrix=[1.0] * 12), lambda: T(sel, matrix=[32769] + [0] * 11),
           lambda: T(sel, matrix=[0] * 9 + [0, 0, (1 << 20) + 1]), lambda: T(sel, matrix=[True] * 12), lambda: T(sel, matrix=7), lambda: T(sel, matrix="grey"),
           lambda: T(sel, auto="auto"), lambda: T(sel, auto=1), lambda: T(sel, auto="match"), lambda: T(sel, auto="match", reference=sel.plane),
           lambda: T(sel, auto="match", reference=other), lambda: T(sel, auto="match", reference=empty), lambda: T(sel, auto="match", reference=("rim", 0)),
           lambda: T(sel, auto="match", reference=("rim", 17)), lambda: T(sel, auto="match", reference=("rim", 2.0)), lambda: T(sel, auto="match", reference=("ring", 2)),
           lambda: T(sel, auto="match", reference=("rim",)), lambda: T(sel, auto="levels", reference=ref), lambda: T(sel, lut=INVERT, reference=("rim", 2)),
           lambda: T(sel, auto="levels", which="y"), lambda: T(sel, auto="levels", which=1), lambda: T(sel, lut=INVERT, which=None),
           lambda: T(sel, auto="levels", clip=201), lambda: T(sel, auto="levels", clip=-1), lambda: T(sel, auto="levels", clip=1.0),
           lambda: T(sel, auto="equalize", clip=5), lambda: T(sel, lut=INVERT, clip=5), lambda: T(sel, auto="match", reference=ref, clip=5),
           lambda: T(sel, amount=1.01, **ok), lambda: T(sel, amount=-0.1, **ok), lambda: T(sel, amount="1", **ok), lambda: T(sel, amount=True, **ok),
           lambda: T(sel, amount=float("nan"), **ok), lambda: T(sel, feather=17, **ok), lambda: T(sel, feather=2.5, **ok), lambda: T(sel, feather=-1, **ok),
           lambda: T(sel, encode="gif", **ok), lambda: T(sel, encode=("jpg", 0), **ok)]
    for k, call in enumerate(bad):
        with pytest.raises((ValueError, TypeError)):
            call()
        assert stub.calls == [] and not s.can_undo, k
    with pytest.raises(ValueError, match="empty selection: nothing to adjust"):
        T(empty, **ok)
    with pytest.raises(TypeError):
        T(sel.plane, **ok)
    with pytest.raises(ValueError, match="excludes lut"):
        T(sel, lut=INVERT, auto="levels")
    with pytest.raises(TypeError, match="rim"):
        T(sel, auto="match")
    assert stub.calls == []


def test_existing_calls_issue_what_they_issued():
    """every method of before, filter_selection included, on a backend WITH the three new calls never uses them and issues the very
    calls it issues on the backend of before, leaving the same frame"""
    sk = np.zeros(HW, np.uint8)
    sk[200:210, 300:330] = 255
    mask = np.zeros(HW, np.uint8)
    mask[200:230, 300:340] = 1
    f = U._noise(HW, 5)
    f[200:230, 300:340] = U.REGION
    seqs, frames = {}, {}
    for k, cls in enumerate((_FilterStub, _Stub)):
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
            s.filter_selection(b, "blur", radius=3, feather=2)
            s.filter_selection(b, "pixelate", cell=5)
            s.set_lock(b)
            b.rings()
            s.undo()
            s.undo()
            s.redo()
            seqs[k, lock], frames[k, lock] = [c for c in stub.calls if c[0] != "download"], s._frame.copy()
            assert stub.calls and not {"adjust", "hist", "hist_lut"} & set(_names(stub))
    for lock in (False, True):
        assert [c[0] for c in seqs[0, lock]] == [c[0] for c in seqs[1, lock]] and np.array_equal(frames[0, lock], frames[1, lock])
    # a backend of before cannot adjust, and says so only when asked to
    s = serve.EditSession(None, f, backend=_FilterStub(), history=1)
    sel = s.select_lasso([RING])
    with pytest.raises(AttributeError):
        s.adjust_selection(sel, lut=INVERT)
    with pytest.raises(AttributeError):
        s.histogram(sel)


def test_model_backend_adjust_calls():
    """_ModelBackend's three calls on a scripted model: one model call each, nothing downloaded"""
    class _Model:
        def __init__(self):
            self.calls = []

        def adjust_u8(self, frame, lift, lift_rect, sel, lock, box, lut, matrix, amount, feather):
            self.calls.append(("adjust_u8", tuple(lift_rect), tuple(box), lut, matrix, amount, feather))

        def adjust_hist_u8(self, frame, sel, box):
            self.calls.append(("adjust_hist_u8", sel, tuple(box)))
            return "record"

        def adjust_lut_u8(self, src, ref, mode, which, clip):
            self.calls.append(("adjust_lut_u8", src, ref, mode, which, clip))
            return "table"

    be = serve._ModelBackend.__new__(serve._ModelBackend)
    be.model = _Model()
    assert be.adjust(None, None, (0, 0, 16, 23), None, None, (5, 7, 10, 20), "t", [1] * 12, 200, 3) is None
    assert be.hist(None, "plane", (5, 7, 10, 20)) == "record" and be.hist_lut("a", "b", 2, 1, 0) == "table"
    assert be.model.calls == [("adjust_u8", (0, 0, 16, 23), (5, 7, 10, 20), "t", [1] * 12, 200, 3), ("adjust_hist_u8", "plane", (5, 7, 10, 20)),
                              ("adjust_lut_u8", "a", "b", 2, 1, 0)]


# ---- the C-ABI -------------------------------------------------------------------------------------------------------------
def test_abi_has_four_new_symbols_in_a_header_of_their_own():
    hdr = open(os.path.join(ROOT, "include", "sketchedit_adjust.h")).read()
    declared = re.findall(r"^(?:int|size_t)\s+(se_\w+)\(", hdr, re.M)
    assert declared == _lib.abi_names("sketchedit_adjust.h") == ["se_adjust_u8", "se_adjust_hist_u8_workspace_bytes", "se_adjust_hist_u8", "se_adjust_lut_u8"]
    others = [n for n in _lib.abi_names() if n not in declared]
    for name in others:                                               # the header refers to other families by DESIGN section
        assert not re.search(r"\b%s\b" % name, hdr), name
    for fam in ("se_filter", "se_move", "se_warp", "se_outline", "se_lasso", "se_select", "se_window"):
        assert fam not in hdr, fam
    for name in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if name != "sketchedit_adjust.h":
            assert "se_adjust" not in open(os.path.join(ROOT, "include", name)).read(), name
    assert "se_adjust.hip" in _lib.SOURCES and _lib.SOURCES[-1] == "se_api.hip"
    for define, value in (("SE_ADJUST_MAX_COEF", "32768"), ("SE_ADJUST_MAX_OFFSET", "1048576"), ("SE_ADJUST_ONE_AMOUNT", "256"), ("SE_ADJUST_MAX_FEATHER", "16"),
                          ("SE_ADJUST_MAX_CLIP", "200"), ("SE_ADJUST_STRETCH", "0"), ("SE_ADJUST_EQUALIZE", "1"), ("SE_ADJUST_MATCH", "2"),
                          ("SE_ADJUST_PER_CHANNEL", "0"), ("SE_ADJUST_LUMA", "1"), ("SE_ADJUST_HIST_GROUPS", "256")):
        assert re.search(r"#define %s %s$" % (define, value), hdr, re.M), define
    assert (_lib.ADJUST_MAX_COEF, _lib.ADJUST_MAX_OFFSET, _lib.ADJUST_ONE_AMOUNT, _lib.ADJUST_MAX_FEATHER, _lib.ADJUST_MAX_CLIP, _lib.ADJUST_HIST_GROUPS) == \
        (32768, 1 << 20, 256, 16, 200, 256) == (A.MAX_COEF, A.MAX_OFFSET, A.ONE_AMOUNT, A.MAX_FEATHER, A.MAX_CLIP, A.HIST_GROUPS)
    assert (_lib.ADJUST_STRETCH, _lib.ADJUST_EQUALIZE, _lib.ADJUST_MATCH, _lib.ADJUST_PER_CHANNEL, _lib.ADJUST_LUMA) == (0, 1, 2, 0, 1) == \
        (A.STRETCH, A.EQUALIZE, A.MATCH, A.PER_CHANNEL, A.LUMA)
    assert serve.ADJUST_AUTO == dict(levels=0, equalize=1, match=2) and serve.ADJUST_WHICH == dict(channels=0, luma=1)
    assert (serve.ADJUST_MAX_COEF, serve.ADJUST_MAX_OFFSET, serve.ADJUST_MAX_CLIP, serve.ADJUST_ONE) == (32768, 1 << 20, 200, 4096)
    import ctypes
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    lib = ctypes.CDLL(_lib.LIB_PATH)                                    # the built library, as the other host tests load it
    for s in declared:
        getattr(lib, s)
    lib.se_adjust_hist_u8_workspace_bytes.restype = ctypes.c_size_t      # host only: no device is touched
    ws = lambda h, w: lib.se_adjust_hist_u8_workspace_bytes(h, w)       # noqa: E731
    assert ws(15, 100) == 0 and ws(100, 15) == 0 and ws(16, 16) == 4096 and ws(16, 65) == 8192 and ws(17, 64) == 8192
    assert ws(272, 1040) == 256 * 4096 and ws(1081, 1921) == 256 * 4096 and ws(256, 1024) == 256 * 4096 and ws(256, 960) == 240 * 4096
    from sketchedit_amd import kernel_labels
    for kernel, label in (("adjust_kernel", "adjust"), ("hist_tiles_kernel", "hist_tiles"), ("hist_sum_kernel", "hist_sum"), ("adjust_lut_kernel", "adjust_lut")):
        assert kernel_labels.label_of("void se::%s(unsigned char*, int)" % kernel) == label
        assert kernel_labels.label_of("%s(unsigned char*, int)" % kernel) == label
        assert label in set(kernel_labels.KERNEL_LABELS.values())
    names, labels = abi_util.prof_labels()
    assert len(names) == len(labels) - 1 and labels[-1] == "PL_COUNT"
    i = names.index("adjust")
    assert names[i - 1:i + 5] == ["plane_combine", "adjust", "hist_tiles", "hist_sum", "adjust_lut", "outline_count"]      # between the two, not appended
    assert labels[i - 1:i + 5] == ["PL_PLANE_COMBINE", "PL_ADJUST", "PL_HIST_TILES", "PL_HIST_SUM", "PL_ADJUST_LUT", "PL_OUTLINE_COUNT"]
    assert names[-4:] == ["move_drop", "plane_shift", "warp_drop", "plane_warp"] and labels[-3:] == ["PL_WARP_DROP", "PL_PLANE_WARP", "PL_COUNT"]
    j = names.index("filter_blur")
    assert names[j - 1:j + 3] == ["outline_emit", "filter_blur", "filter_mosaic", "move_drop"]
    from sketchedit_amd.models.editline2_model import EditLine2Model
    for name in ("adjust_u8", "adjust_hist_u8", "adjust_lut_u8"):
        assert callable(getattr(_lib.Engine, name)) and callable(getattr(EditLine2Model, name))
    for name in ("adjust", "hist", "hist_lut"):
        assert callable(getattr(serve._ModelBackend, name))
    for name in ("adjust_selection", "histogram"):
        assert callable(getattr(serve.EditSession, name))


def test_the_kernels_cross_compile_for_gfx950(tmp_path):
    import shutil
    import subprocess
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc on this machine")
    obj = str(tmp_path / "se_adjust.o")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(_lib.CSRC, "se_adjust.hip"), "-o", obj])
    assert os.path.getsize(obj) > 0


def test_the_selection_tile_is_written_once():
    """What the operators on a selection share on the device lives in one file under csrc/ (se_seltile.h, se_device.h): an operator
    that copied its predecessor's text instead of calling it would define one of these a second time."""
    texts = {name: open(os.path.join(_lib.CSRC, name)).read() for name in sorted(os.listdir(_lib.CSRC))}
    for piece in ("bytes_nonzero(unsigned", "load12_within(const", "sel4_in_box(const", "struct Lift", "in1 = z =="):
        holders = [name for name, text in texts.items() if piece in text]
        assert len(holders) == 1 and texts[holders[0]].count(piece) == 1, (piece, holders)
