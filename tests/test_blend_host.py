"""Host tests of the seamless move and clone: the statement's own properties and the header's known answers, its
agreement with the hard drop where no rim exists, the kernels of se_blend.hip restated on one checked byte array against the
statement, EditSession.move_selection(..., blend="seamless") against a scripted backend, and the new entries' place in the
C-ABI.  CPU only; every comparison is exact."""
import os
import re

import numpy as np
import pytest

from sketchedit_amd import _lib, serve
import abi_util
import blend_util as B
import move_util as M
import select_util as U
from test_fill_host import _names
from test_move_host import BOX, HW, OFF, _Stub as _MoveStub, _lock_array, _session

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _grown_rect(box, hw):
    """the lift rectangle of a seamless move: move_rect of the box grown by one pixel and clipped to the frame"""
    g = (max(box[0] - 1, 0), max(box[1] - 1, 0), min(box[2] + 1, hw[0]), min(box[3] + 1, hw[1]))
    return M.move_rect(g, (0, 0), hw)


def _disc(hw, frac=0.4):
    yy, xx = np.mgrid[0:hw[0], 0:hw[1]]
    return np.where(((yy - hw[0] / 2.0) / (hw[0] * frac)) ** 2 + ((xx - hw[1] / 2.0) / (hw[1] * frac)) ** 2 < 1, 200, 0).astype(np.uint8)


def _case(seed, hw=(37, 53), sel=None, lock_p=0.2):
    rng = np.random.RandomState(seed)
    frame = rng.randint(0, 256, hw + (3,)).astype(np.uint8)
    before = rng.randint(0, 256, hw + (3,)).astype(np.uint8)
    sel = _disc(hw) if sel is None else sel
    lock = np.where(rng.rand(*hw) < lock_p, 255, 0).astype(np.uint8)
    box = M.box_of(sel)
    rect = _grown_rect(box, hw)
    return frame, before, M.slot_of(before, rect), rect, sel, lock, box


# ---- the statement ----------------------------------------------------------------------------------------------------------------------
def test_known_answers_of_the_header():
    hdr = open(os.path.join(ROOT, "include", "sketchedit_blend.h")).read()
    assert "become 30" in hdr and "become 0 (the clamp)" in hdr and "#define SE_BLEND_MAX_SIDE 2048" in hdr
    sel = np.zeros((16, 16), np.uint8)
    sel[2:4, 2:5] = 1
    for frame_v, around, obj, want_v in ((10, 180, 200, 30), (10, 250, 100, 0)):
        frame = np.full((16, 16, 3), frame_v, np.uint8)
        before = np.full((16, 16, 3), around, np.uint8)
        before[2:4, 2:5] = obj
        got = B.spec_blend(frame, M.slot_of(before, (0, 0, 16, 16)), (0, 0, 16, 16), sel, None, (2, 2, 4, 5), (1, 3), 0)
        want = frame.copy()
        want[3:5, 5:8] = want_v
        assert np.array_equal(got, want) and int((got != frame).sum()) == 18


@pytest.mark.parametrize("flip", range(4))
def test_a_constant_rim_difference_is_added_exactly(flip):
    """F = P + c around the object: the membrane is c everywhere, whatever the object's own detail is"""
    frame, before, _, rect, sel, _, box = _case(flip)
    for c, off in ((-37, (0, 0)), (90, (2, -3)), (-200, (-4, 5))):
        # the place it lands in: the lift's own pixels, moved, plus c (the lift is kept in a range that leaves F a byte)
        lo, hi = max(0, -c), min(255, 255 - c)
        P = np.clip(before, lo, hi)
        slot = M.slot_of(P, rect)
        Hi, Wi = sel.shape
        ys, xs = np.arange(Hi), np.arange(Wi)
        qy, qx = B._src(box, off, flip, ys, xs)
        held = ((qy >= rect[0]) & (qy < rect[0] + rect[2]))[:, None] & ((qx >= rect[1]) & (qx < rect[1] + rect[3]))[None, :]
        f = np.where(held[..., None], P[np.clip(qy, 0, Hi - 1)[:, None], np.clip(qx, 0, Wi - 1)[None, :]].astype(int) + c, 128).astype(np.uint8)
        got, e, levels = B.spec_blend(f, slot, rect, sel, None, box, off, flip, want_levels=True)
        hard = M.spec_drop(f, slot, rect, sel, None, box, off, flip, 0)
        moved = M.spec_shift(sel, box, off, flip) == 255
        assert moved.any() and np.array_equal(got[moved], np.clip(hard[moved].astype(int) + c, 0, 255).astype(np.uint8)), (c, off)
        assert np.array_equal(got[~moved], f[~moved])
        for state, u in levels:
            assert (u[state != B.OUT] == 16 * c + 4096).all()


def test_every_value_lies_between_the_least_and_greatest_known_value_and_channels_are_independent():
    frame, _, slot, rect, sel, lock, box = _case(5)
    got, e, levels = B.spec_blend(frame, slot, rect, sel, lock, box, (3, -2), 1, want_levels=True)
    state0, u0 = levels[0]
    for ch in range(3):
        known = u0[..., ch][state0 == B.KNOWN]
        assert known.min() >= 16 and known.max() <= 8176
        for state, u in levels:
            live = u[..., ch][state != B.OUT]
            assert live.min() >= known.min() and live.max() <= known.max()
    # a channel's result depends on that channel alone
    for ch in range(3):
        f2, s2 = frame.copy(), slot.copy()
        for other in range(3):
            if other != ch:
                f2[..., other] = 255 - f2[..., other]
                s2[:, other:3 * rect[3]:3] = 255 - s2[:, other:3 * rect[3]:3]
        assert np.array_equal(B.spec_blend(f2, s2, rect, sel, lock, box, (3, -2), 1)[..., ch], got[..., ch])
    # it is not the hard drop, and only unlocked moved pixels change
    hard = M.spec_drop(frame, slot, rect, sel, lock, box, (3, -2), 1, 0)
    target = (M.spec_shift(sel, box, (3, -2), 1) == 255) & (lock == 0)
    assert not np.array_equal(got, hard) and np.array_equal(got[~target], frame[~target]) and (got[target] != frame[target]).any()


@pytest.mark.parametrize("flip", range(4))
def test_flips_and_a_lock_follow_a_pixel_by_pixel_restatement(flip):
    """level 0 by loops over pixels, as the header words it"""
    frame, before, slot, rect, sel, lock, box = _case(20 + flip, hw=(24, 31))
    Hi, Wi = sel.shape
    off = (2, -3)
    by0, bx0, by1, bx1 = box

    def src(y, x):
        return (by0 + by1 - 1 - (y - off[0]) if flip & 2 else y - off[0]), (bx0 + bx1 - 1 - (x - off[1]) if flip & 1 else x - off[1])

    def target(y, x):
        qy, qx = src(y, x)
        return 0 <= y < Hi and 0 <= x < Wi and by0 <= qy < by1 and bx0 <= qx < bx1 and sel[qy, qx] != 0 and lock[y, x] == 0

    e, state, u = B.level0(frame, slot, rect, sel, lock, box, off, flip)
    d, e2 = B.rects(box, off, (Hi, Wi))
    assert e == e2 == (max(d[0] - 1, 0), max(d[1] - 1, 0), min(d[2] + 1, Hi), min(d[3] + 1, Wi))
    kinds = set()
    for y in range(e[0], e[2]):
        for x in range(e[1], e[3]):
            qy, qx = src(y, x)
            if target(y, x):
                want = B.UNKNOWN
            elif (rect[0] <= qy < rect[0] + rect[2] and rect[1] <= qx < rect[1] + rect[3] and
                  (target(y - 1, x) or target(y + 1, x) or target(y, x - 1) or target(y, x + 1))):
                want = B.KNOWN
                assert np.array_equal(u[y - e[0], x - e[1]], 16 * (frame[y, x].astype(int) - before[qy, qx]) + 4096)
                kinds.add("locked" if lock[y, x] else "rim")
            else:
                want = B.OUT
            assert state[y - e[0], x - e[1]] == want, (y, x)
    assert kinds == {"locked", "rim"}                                   # a locked destination pixel next to the object is KNOWN


# ---- agreement with the hard drop ------------------------------------------------------------------------------------------------------
def test_without_a_known_cell_it_is_the_hard_drop():
    """the full frame selected and moved by (0, 0): no rim anywhere"""
    hw = (20, 33)
    frame, _, slot, rect, sel, _, box = _case(7, hw=hw, sel=np.full(hw, 255, np.uint8))
    for flip in range(4):
        got, e, levels = B.spec_blend(frame, slot, rect, sel, None, box, (0, 0), flip, want_levels=True)
        assert not (levels[0][0] == B.KNOWN).any()
        assert np.array_equal(got, M.spec_drop(frame, slot, rect, sel, None, box, (0, 0), flip, 0))
        assert not np.array_equal(got, frame)


@pytest.mark.parametrize("off", [(-14, 0), (14, 1), (0, -20), (-1, 20), (-14, -20), (14, 20)], ids=str)
def test_an_object_over_an_edge_has_a_neumann_side_there(off):
    """the rim the frame's edge cuts away is OUT, not a value: a constant difference on the rest of the rim is still added exactly"""
    hw = (37, 53)
    _, before, _, rect, sel, _, box = _case(3, hw=hw)
    P = np.clip(before, 40, 255)
    slot = M.slot_of(P, rect)
    ys, xs = np.arange(hw[0]), np.arange(hw[1])
    qy, qx = B._src(box, off, 0, ys, xs)
    f = np.clip(P[np.clip(qy, 0, hw[0] - 1)[:, None], np.clip(qx, 0, hw[1] - 1)[None, :]].astype(int) - 40, 0, 255).astype(np.uint8)
    got, e, levels = B.spec_blend(f, slot, rect, sel, None, box, off, 0, want_levels=True)
    moved = M.spec_shift(sel, box, off, 0) == 255
    d, _ = B.rects(box, off, hw)
    assert moved.any() and (d[0] == 0 or d[1] == 0 or d[2] == hw[0] or d[3] == hw[1])
    assert 0 < moved.sum() < (sel != 0).sum()                             # partly out
    hard = M.spec_drop(f, slot, rect, sel, None, box, off, 0, 0)
    assert np.array_equal(got[moved], hard[moved] - 40) and np.array_equal(got[~moved], f[~moved])
    # wholly out: nothing changes
    assert np.array_equal(B.spec_blend(f, slot, rect, sel, None, box, (hw[0], 0), 0), f)
    assert B.launches(box, (hw[0], 0), hw) == 0


# ---- the kernels, restated ----------------------------------------------------------------------------------------------------------------
def _run_tiled(frame, slot, rect, sel, lock, box, off, flip, fa_mis):
    Hi, Wi = sel.shape
    wsb = B.workspace_bytes(box[2] - box[0], box[3] - box[1])
    mem = B.Memory(3 * Hi * Wi + 2 * Hi * Wi + slot.size + wsb + 8192)
    fa = mem.put(1024 + fa_mis, frame)
    sa = mem.put(fa + frame.size + 101, sel)
    la = None if lock is None else mem.put(sa + sel.size + 203, lock)
    pa = mem.put(((la or sa) + sel.size + 300) // 16 * 16, slot)
    wa = (pa + slot.size + 500) // 16 * 16
    assert wa + wsb <= mem.mem.size
    before = mem.mem.copy()
    n = B.tiled_blend(mem, fa, Hi, Wi, pa, rect, sa, la, box, off, flip, wa, wsb)
    after = mem.mem.copy()
    got = mem.get(fa, frame.shape)
    after[fa:fa + frame.size] = before[fa:fa + frame.size]
    after[wa:wa + wsb] = before[wa:wa + wsb]
    assert np.array_equal(after, before)                                 # nothing but the frame and the workspace is written
    return got, n, mem.writers[fa:fa + frame.size].reshape(frame.shape)


@pytest.mark.parametrize("hw", [(16, 16), (37, 53), (65, 129)], ids=lambda hw: "%dx%d" % hw)
def test_the_tiled_kernels_equal_the_statement(hw):
    """classification with its halo, pull, relax with halo 8 in split launches and in one workgroup, apply's store slots"""
    full = np.full(hw, 255, np.uint8)
    line = np.zeros(hw, np.uint8)
    line[hw[0] // 2, 1:hw[1] - 1] = 9
    k, seen = 0, set()
    for name, sel in (("disc", None), ("full", full), ("line", line)):
        frame, _, slot, rect, sel, lock, box = _case(hw[0] + k, hw=hw, sel=sel)
        h, w = box[2] - box[0], box[3] - box[1]
        for off in ((0, 0), (1, -1), (h // 3, -(w // 3)), (-box[0] - h // 2, 3), (hw[0] - box[0] - h // 2, hw[1] - box[1] - w // 2), (0, hw[1])):
            flip, lk = k % 4, lock if k % 2 else None
            want = B.spec_blend(frame, slot, rect, sel, lk, box, off, flip)
            got, n, writers = _run_tiled(frame, slot, rect, sel, lk, box, off, flip, k % 4)
            assert np.array_equal(got, want), (name, hw, off, flip, k % 2)
            assert n == B.launches(box, off, hw)
            target = M.spec_shift(sel, box, off, flip) == 255
            if lk is not None:
                target &= lk == 0
            assert np.array_equal(writers, np.repeat(target[..., None], 3, axis=2).astype(np.int32))      # ONE writer per target byte, none elsewhere
            l0 = B.level0(frame, slot, rect, sel, lk, box, off, flip)
            hard = M.spec_drop(frame, slot, rect, sel, lk, box, off, flip, 0)
            if l0 is None or not (l0[1] == B.KNOWN).any():               # no rim (the full frame: the lift holds no source around it)
                assert np.array_equal(want, hard) and (name == "full" or l0 is None)
            else:
                assert not np.array_equal(want, hard) and not np.array_equal(want, frame)
                seen.add(name)
            k += 1
    assert seen == {"disc", "full", "line"}                               # (the full frame has a rim where a lock cuts into it)
    # the schedule: 65 x 129's full frame has a level of 33 x 65 cells that takes two launches of four sweeps, double buffered
    if hw == (65, 129):
        assert B.level_sizes(65, 129)[1] == (33, 65) and B.sweeps_of(1) == 8 and B.launches((0, 0, 65, 129), (0, 0), hw) == 1 + 8 + (1 + 2 + 7) + 1


def test_workspace_and_schedule_are_functions_of_the_size_alone():
    assert B.workspace_bytes(0, 5) == B.workspace_bytes(5, 2049) == 0
    assert B.workspace_bytes(1, 1) == 16 * (9 + 4 + 1) and B.workspace_bytes(2048, 2048) < 96 << 20
    assert [B.sweeps_of(l) for l in range(6)] == [4, 8, 16, 32, 64, 64]
    assert B.level_sizes(5, 3) == [(5, 3), (3, 2), (2, 1), (1, 1)]
    # section 6r's disc of 253 x 253: 255 x 255 cells, 9 levels; 23 launches
    assert B.launches((100, 100, 353, 353), (300, 300), (1024, 1024)) == 1 + 8 + (1 + 2 + 4 + 6) + 1


def test_deviation_from_the_harmonic_membrane_is_recorded(capsys):
    """printed, not asserted: the statement against scipy's exact solve, where scipy is installed (DESIGN.md 6x holds the figures)"""
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.linalg import spsolve
    for radius, step, noise in ((30, 0, 6), (30, 100, 20)):
        n = 2 * radius + 6
        yy, xx = np.mgrid[0:n, 0:n]
        sel = np.where((yy - n / 2.0) ** 2 + (xx - n / 2.0) ** 2 < radius ** 2, 255, 0).astype(np.uint8)
        rng = np.random.RandomState(radius + step)
        ramp = 40.0 * (xx - n / 2.0) / radius if not step else np.where(xx < n / 2, -step, step)
        diff = np.rint(ramp + rng.uniform(-noise, noise, (n, n))).astype(int)
        P = np.full((n, n, 3), 128, np.uint8)
        frame = np.clip(128 + diff, 0, 255).astype(np.uint8)[..., None].repeat(3, axis=2)
        box = M.box_of(sel)
        rect = (0, 0, n, n)
        got = B.spec_blend(frame, M.slot_of(P, rect), rect, sel, None, box, (0, 0), 0)[..., 0].astype(float) - 128
        inside = sel != 0
        idx = -np.ones((n, n), int)
        idx[inside] = np.arange(inside.sum())
        A = sp.lil_matrix((inside.sum(), inside.sum()))
        b = np.zeros(inside.sum())
        for y, x in zip(*np.nonzero(inside)):
            A[idx[y, x], idx[y, x]] = 4
            for ny, nx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                if inside[ny, nx]:
                    A[idx[y, x], idx[ny, nx]] = -1
                else:
                    b[idx[y, x]] += frame[ny, nx, 0].astype(float) - 128
        exact = spsolve(A.tocsr(), b)
        dev = np.abs(got[inside] - exact)
        with capsys.disabled():
            print("\nblend deviation radius=%d step=%d noise=%d: max %.2f mean %.2f p99 %.2f grey levels" %
                  (radius, step, noise, dev.max(), dev.mean(), np.percentile(dev, 99)))


# ---- the sessions against a scripted backend -------------------------------------------------------------------------------------------------
class _Stub(_MoveStub):
    """test_move_host's backend with the seamless drop: the statement"""

    def move_blend(self, frame, lift, lift_rect, plane, lock, box, offset, flip):
        self.calls.append(("move_blend", tuple(lift_rect), id(plane), None if lock is None else id(lock), tuple(box), tuple(offset), flip))
        self.lift = lift.copy()
        frame[...] = B.spec_blend(frame, lift, lift_rect, plane, lock, box, offset, flip)


LIFT = (199, 299, 32, 42)                                                # BOX grown by one pixel


def _expect(f, sel, lock, offset, flip, hole_grow, win, keep_source):
    after = f.copy()
    if not keep_source:
        hole = U.spec_grow(sel != 0, hole_grow) != 0
        if lock is not None:
            hole &= lock == 0
        y0, x0, h, w = win
        inwin = np.zeros(HW, bool)
        inwin[y0:y0 + h, x0:x0 + w] = True
        after[hole & inwin] = _Stub.FILL
    return B.spec_blend(after, M.slot_of(f, LIFT), LIFT, sel, lock, BOX, offset, flip)


@pytest.mark.parametrize("keep_source", [False, True])
@pytest.mark.parametrize("lock", [False, True])
@pytest.mark.parametrize("history", [0, 2])
@pytest.mark.parametrize("max_side,feather", [(None, None), (128, 4)])
def test_seamless_move_issues_lift_fill_save_blend_shift_in_that_order(keep_source, lock, history, max_side, feather):
    stub = _Stub()
    s, sel, f = _session(stub, lock, history=history)
    plane0 = sel.plane.copy()
    assert _grown_rect(BOX, HW) == LIFT
    call = s.clone_selection if keep_source else s.move_selection
    patches, positions, info = call(sel, OFF, flip="h", max_side=max_side, feather=feather, low_latency=True, blend="seamless")
    win = serve.choose_window((198, 298, 232, 342), HW, margin=0.5)
    dst = (210, 325, 30, 40)
    wins = ([] if keep_source else [win]) + [dst]
    paste = "paste_feather" if feather else "paste_locked"
    fill = [] if keep_source else ["grow", "fill_keep", "run_fill"] + (["save"] if history else []) + [paste]
    assert _names(stub) == ["save"] + fill + (["save"] if history else []) + ["move_blend", "shift"] + ["crop"] * len(wins)
    saves = [c for c in stub.calls if c[0] == "save"]
    assert saves[0] == ("save", [LIFT[:2]], LIFT[2:])                  # the GROWN lift: the rim's sources are in it
    if history:
        assert saves[1:] == [("save", [w[:2]], w[2:]) for w in wins]
    calls = {c[0]: c for c in stub.calls}
    lk = s._lock_plane
    assert calls["move_blend"] == ("move_blend", LIFT, id(sel.plane), None if lk is None else id(lk), BOX, OFF, 1)
    assert calls["shift"] == ("shift", id(sel.plane), BOX, OFF, 1)
    assert np.array_equal(stub.lift[:, :126].reshape(32, 42, 3), f[199:231, 299:341])
    moved = info.pop("selection")
    want = dict(windows=wins, move=True, offset=OFF, flip="h", blend="seamless", selected=1200)
    if lock:
        want["locked"] = True
    if max_side and not keep_source:
        want["work"] = serve.choose_working_size(win[2:], max_side)
    if history:
        want["undoable"] = True
    if feather and not keep_source:                                   # the feather is the fill's alone
        want["feather"] = 4
    assert info == want
    assert moved.box == (210, 325, 240, 365) and moved.count == 1200 and np.array_equal(moved.plane, M.spec_shift(plane0, BOX, OFF, 1))
    after = _expect(f, plane0, _lock_array() if lock else None, OFF, 1, 2, win, keep_source)
    assert np.array_equal(s._frame, after) and not np.array_equal(after, f)
    hard = s._frame.copy()
    hard[...] = M.spec_drop(hard, M.slot_of(f, LIFT), LIFT, plane0, _lock_array() if lock else None, BOX, OFF, 1, 0)
    assert not np.array_equal(after, hard)                            # the membrane is not 0
    for p, w in zip(patches, wins):
        assert np.array_equal(p, after[w[0]:w[0] + w[2], w[1]:w[1] + w[3]])
    if lock:
        assert np.array_equal(after[_lock_array() != 0], f[_lock_array() != 0])
    if history:
        # ONE undo step, byte for byte both ways
        s.undo()
        assert np.array_equal(s._frame, f) and not s.can_undo
        s.redo()
        assert np.array_equal(s._frame, after) and not s.can_redo
    else:
        assert not s.can_undo


def test_the_lift_of_a_box_at_the_frames_corner_is_clipped():
    stub = _Stub()
    f = U._noise(HW, 5)
    s = serve.EditSession(None, f, backend=stub)
    sel = s.select_lasso([[(0, 0), (30, 0), (30, 20), (0, 20)]])
    assert sel.box == (0, 0, 20, 30)
    stub.calls.clear()
    s.clone_selection(sel, (50, 60), blend="seamless")
    assert [c for c in stub.calls if c[0] == "save"][0] == ("save", [(0, 0)], (21, 31))
    assert np.array_equal(s._frame, B.spec_blend(f, M.slot_of(f, (0, 0, 21, 31)), (0, 0, 21, 31), sel.plane, None, sel.box, (50, 60), 0))


def test_refusals_come_before_the_first_backend_call():
    stub = _Stub()
    s, sel, f = _session(stub, history=1)
    for bad in ("poisson", "", 1, True, ("seamless",), b"seamless"):
        with pytest.raises(ValueError, match="blend"):
            s.move_selection(sel, OFF, blend=bad)
    with pytest.raises(ValueError, match="out of the frame"):
        s.move_selection(sel, (400, 0), blend="seamless")
    with pytest.raises(ValueError, match="feather"):
        s.move_selection(sel, OFF, blend="seamless", feather=17)
    old = _MoveStub()                                                 # a backend without the new call
    s2, sel2, f2 = _session(old, history=1)
    with pytest.raises(NotImplementedError, match="move_blend"):
        s2.move_selection(sel2, OFF, blend="seamless")
    with pytest.raises(NotImplementedError, match="move_blend"):
        s2.clone_selection(sel2, OFF, blend="seamless")
    assert stub.calls == [] and old.calls == [] and np.array_equal(s._frame, f) and np.array_equal(s2._frame, f2) and not s.can_undo
    # a box above the limit
    assert serve.BLEND_MAX_SIDE == _lib.BLEND_MAX_SIDE == B.MAX_SIDE == 2048
    wide = serve.EditSession(None, np.zeros((32, 2100, 3), np.uint8), backend=stub)
    big = wide.select_lasso([[(10, 5), (2059, 5), (2059, 9), (10, 9)]])
    assert big.box == (5, 10, 9, 2059)
    stub.calls.clear()
    with pytest.raises(ValueError, match="2048"):
        wide.clone_selection(big, (1, 1), blend="seamless")
    assert stub.calls == []
    wide.clone_selection(big, (1, 1))                                 # the plain clone takes it


@pytest.mark.parametrize("with_new_call", [False, True])
def test_blend_none_issues_the_old_sequence(with_new_call):
    """on backends with and without move_blend: the same calls with the same arguments, the lift rectangle included"""
    logs = []
    for kw in (dict(), dict(blend=None)):
        stub = _Stub() if with_new_call else _MoveStub()
        s, sel, f = _session(stub, True, history=2)
        _, _, info = s.move_selection(sel, OFF, flip="v", feather=3, **kw)
        assert "blend" not in info and info["feather"] == 3
        assert [c for c in stub.calls if c[0] == "save"][0] == ("save", [(200, 300)], (30, 40))
        assert "move_blend" not in _names(stub) and "move_drop" in _names(stub)
        logs.append((_names(stub), [c for c in stub.calls if c[0] in ("save", "grow", "shift")], s._frame.copy()))
    assert logs[0][0] == logs[1][0] and logs[0][1][0] == logs[1][1][0] and np.array_equal(logs[0][2], logs[1][2])
    assert logs[0][0] == ["save", "grow", "fill_keep", "run_fill", "save", "paste_feather", "save", "move_drop", "shift", "crop", "crop"]


# ---- the C-ABI -----------------------------------------------------------------------------------------------------------------------------
def test_abi_has_two_new_symbols_in_a_header_of_their_own():
    hdr = open(os.path.join(ROOT, "include", "sketchedit_blend.h")).read()
    declared = re.findall(r"^(?:int|size_t)\s+(\w+)\(", hdr, re.M)
    assert declared == _lib.abi_names("sketchedit_blend.h") == ["se_move_blend_u8_workspace_bytes", "se_move_blend_u8"]
    assert [n for n in _lib.abi_names() if "blend" in n] == declared
    for name in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if name != "sketchedit_blend.h":
            assert "move_blend" not in open(os.path.join(ROOT, "include", name)).read(), name
    i = _lib.SOURCES.index("se_blend.hip")
    assert _lib.SOURCES[i - 1] == "se_move.hip" and "se_api_move.hip" in _lib.SOURCES and _lib.SOURCES[-1] == "se_api.hip"
    import ctypes
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in declared:
        getattr(lib, s)
    lib.se_move_blend_u8_workspace_bytes.restype = ctypes.c_size_t
    for h, w in ((1, 1), (30, 40), (253, 253), (2048, 2048), (0, 4), (2049, 4), (4, 2049)):
        assert lib.se_move_blend_u8_workspace_bytes(h, w) == B.workspace_bytes(h, w), (h, w)
    from sketchedit_amd import kernel_labels
    for kernel in ("blend_init", "blend_pull", "blend_relax", "blend_apply"):
        assert kernel_labels.label_of("void se::%s_kernel(uint2 const*, int)" % kernel) == kernel
        assert kernel_labels.label_of("%s_kernel(uint2 const*, int)" % kernel) == kernel
    names, labels = abi_util.prof_labels()
    assert len(names) == len(labels) - 1 and labels[-1] == "PL_COUNT"
    i = names.index("blend_init")
    assert names[i:i + 4] == ["blend_init", "blend_pull", "blend_relax", "blend_apply"]
    assert labels[i:i + 4] == ["PL_BLEND_INIT", "PL_BLEND_PULL", "PL_BLEND_RELAX", "PL_BLEND_APPLY"]
    src = open(os.path.join(_lib.CSRC, "se_blend.hip")).read()
    assert "atomic" not in src.replace("no atomics", "") and "while" not in src      # a fixed schedule: nothing polled
    from sketchedit_amd.models.editline2_model import EditLine2Model
    assert callable(_lib.Engine.move_blend_u8) and callable(EditLine2Model.move_blend_u8) and callable(serve._ModelBackend.move_blend)
    assert serve.MOVE_BLENDS == (None, "seamless")
