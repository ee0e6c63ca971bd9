"""Host tests of moving and cloning a selection: the statement's own properties and the header's known answer,
serve.move_rect against its restatement, EditSession.move_selection / clone_selection and the ordered journal entry against a
scripted backend that logs every call and, where it matters, really edits a numpy frame, and the new entries' place in the
C-ABI.  CPU only; every comparison is exact."""
import os
import re

import numpy as np
import pytest

from sketchedit_amd import _lib, serve
import lasso_util as L
import move_util as M
import select_util as U
from test_fill_host import _names
from test_outline_host import _Stub as _OutlineStub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HW = (400, 600)


# ---- the statement ----------------------------------------------------------------------------------------------------------------------
def _random_case(seed, hw=(37, 53)):
    rng = np.random.RandomState(seed)
    Hi, Wi = hw
    frame = rng.randint(0, 256, (Hi, Wi, 3)).astype(np.uint8)
    before = rng.randint(0, 256, (Hi, Wi, 3)).astype(np.uint8)
    sel = np.where(rng.rand(Hi, Wi) < 0.6, rng.randint(1, 256, (Hi, Wi)), 0).astype(np.uint8)
    lock = np.where(rng.rand(Hi, Wi) < 0.2, 255, 0).astype(np.uint8)
    box = (5, 7, 29, 40)
    rect = M.move_rect(box, (0, 0), hw)
    return frame, before, M.slot_of(before, rect), rect, sel, lock, box


def test_known_answer_of_the_header():
    hdr = open(os.path.join(ROOT, "include", "sketchedit_move.h")).read()
    assert "become 200" in hdr and "= 94" in hdr and "= 137" in hdr and "row 3, column 7" in hdr
    frame = np.full((16, 16, 3), 10, np.uint8)
    lift = M.slot_of(np.full((16, 16, 3), 200, np.uint8), (0, 0, 16, 16))
    sel = np.zeros((16, 16), np.uint8)
    sel[2:4, 2:5] = 1
    box, off = (2, 2, 4, 5), (1, 3)
    got = M.spec_drop(frame, lift, (0, 0, 16, 16), sel, None, box, off, 0, 0)
    want = frame.copy()
    want[3:5, 5:8] = 200
    assert np.array_equal(got, want) and int((got != frame).sum()) == 18
    got = M.spec_drop(frame, lift, (0, 0, 16, 16), sel, None, box, off, 0, 1)
    want = frame.copy()
    want[3:5, 5:8] = 94
    want[3:5, 6] = 137
    assert np.array_equal(got, want)
    shifted = M.spec_shift(sel, box, off, 0)
    assert int((shifted == 255).sum()) == 6 and (shifted[3:5, 5:8] == 255).all()
    sel[2, 2] = 0
    shifted = M.spec_shift(sel, box, off, 1)
    assert shifted[3, 7] == 0 and int((shifted == 255).sum()) == 5 and (shifted[4, 5:8] == 255).all()


@pytest.mark.parametrize("flip", range(4))
def test_radius_zero_is_a_masked_copy_and_a_full_count_gives_the_lift(flip):
    frame, before, lift, rect, sel, lock, box = _random_case(flip)
    by0, bx0, by1, bx1 = box
    for off in ((0, 0), (3, -4), (-9, 30)):
        for lk in (None, lock):
            got = M.spec_drop(frame, lift, rect, sel, lk, box, off, flip, 0)
            want = frame.copy()
            for y in range(37):
                for x in range(53):
                    qy = by0 + by1 - 1 - (y - off[0]) if flip & 2 else y - off[0]
                    qx = bx0 + bx1 - 1 - (x - off[1]) if flip & 1 else x - off[1]
                    if by0 <= qy < by1 and bx0 <= qx < bx1 and sel[qy, qx] and (lk is None or lk[y, x] == 0):
                        want[y, x] = before[qy, qx]
            assert np.array_equal(got, want), (flip, off, lk is None)
            moved = M.spec_shift(sel, box, off, flip) == 255
            assert not ((got != frame).any(axis=2) & ~moved).any()              # only moved pixels change
    # c == n: a solid selection's interior takes the lift's bytes exactly, its rim a blend that is neither
    solid = np.ones_like(sel)
    r = 3
    got = M.spec_drop(np.zeros_like(frame), lift, rect, solid, None, box, (2, 5), flip, r)
    hard = M.spec_drop(np.zeros_like(frame), lift, rect, solid, None, box, (2, 5), flip, 0)
    inner = np.zeros(sel.shape, bool)
    inner[by0 + 2 + r:by1 + 2 - r, bx0 + 5 + r:bx1 + 5 - r] = True
    assert inner.any() and np.array_equal(got[inner], hard[inner])
    rim = (M.spec_shift(solid, box, (2, 5), flip) == 255) & ~inner
    assert (got[rim].astype(int) <= hard[rim].astype(int)).all() and (got[rim] != hard[rim]).any()
    assert not got[M.spec_shift(solid, box, (2, 5), flip) == 0].any()         # nothing outside the moved selection is written


def test_the_count_ignores_the_frame_edge_and_the_lock():
    frame, before, lift, rect, sel, lock, box = _random_case(9)
    solid = np.ones_like(sel)
    # pushed over the top-left corner: the pixels at the frame's edge are interior pixels of the object and take the lift's bytes
    got = M.spec_drop(frame, lift, rect, solid, None, box, (-15, -20), 0, 4)
    assert np.array_equal(got[0:5, 0:10], before[15:20, 20:30])
    # a lock next to a pixel does not change the pixel's own blend
    lk = np.zeros_like(lock)
    lk[10, :] = 255
    a = M.spec_drop(frame, lift, rect, solid, None, box, (1, 1), 0, 2)
    b = M.spec_drop(frame, lift, rect, solid, lk, box, (1, 1), 0, 2)
    assert np.array_equal(b[10], frame[10]) and np.array_equal(np.delete(a, 10, axis=0), np.delete(b, 10, axis=0))


@pytest.mark.parametrize("flip", range(4))
def test_a_flip_applied_twice_is_the_identity(flip):
    _, _, _, _, sel, _, box = _random_case(11 + flip)
    inside = np.zeros_like(sel)
    inside[box[0]:box[2], box[1]:box[3]] = sel[box[0]:box[2], box[1]:box[3]]
    once = M.spec_shift(sel, box, (0, 0), flip)
    assert np.array_equal(M.spec_shift(once, box, (0, 0), flip), np.where(inside != 0, 255, 0))
    assert np.array_equal(once[box[0]:box[2], box[1]:box[3]],
                          np.where(inside != 0, 255, 0)[box[0]:box[2], box[1]:box[3]][::-1 if flip & 2 else 1, ::-1 if flip & 1 else 1])
    # there and back again
    there = M.spec_shift(sel, box, (4, -6), flip)
    tb = (box[0] + 4, box[1] - 6, box[2] + 4, box[3] - 6)
    assert np.array_equal(M.spec_shift(there, tb, (-4, 6), flip), np.where(inside != 0, 255, 0))
    # wholly out: zeros, and the drop changes nothing
    assert not M.spec_shift(sel, box, (40, 0), flip).any() and not M.spec_shift(sel, box, (0, -41), flip).any()


# ---- move_rect ------------------------------------------------------------------------------------------------------------------------
def test_move_rect_corners():
    hw = (100, 200)
    cases = {((10, 20, 50, 70), (0, 0)): (10, 20, 40, 50),
             ((10, 20, 50, 70), (5, -7)): (15, 13, 40, 50),
             ((10, 20, 50, 70), (-30, 0)): (0, 20, 20, 50),                # clipped at the top
             ((10, 20, 50, 70), (70, 0)): (80, 20, 20, 50),                # at the bottom
             ((10, 20, 50, 70), (0, -40)): (10, 0, 40, 30),                # on the left
             ((10, 20, 50, 70), (0, 150)): (10, 170, 40, 30),              # on the right
             ((10, 20, 50, 70), (-45, 0)): (0, 20, 16, 50),                # 5 rows left at the top edge: widened downwards
             ((10, 20, 50, 70), (85, 0)): (84, 20, 16, 50),                # 5 rows left at the bottom edge: widened upwards
             ((10, 20, 50, 70), (0, -66)): (10, 0, 40, 16),                # 4 columns at the left edge
             ((10, 20, 50, 70), (0, 178)): (10, 184, 40, 16),              # 2 columns at the right edge
             ((40, 60, 44, 70), (0, 0)): (34, 57, 16, 16),                 # a small box in the middle: centred
             ((40, 60, 45, 71), (0, 0)): (35, 58, 16, 16),                 # odd sides: the extra pixel at the high end
             ((0, 0, 1, 1), (0, 0)): (0, 0, 16, 16), ((99, 199, 100, 200), (0, 0)): (84, 184, 16, 16),
             ((10, 20, 50, 70), (-50, 0)): None, ((10, 20, 50, 70), (90, 0)): None, ((10, 20, 50, 70), (0, -70)): None,
             ((10, 20, 50, 70), (0, 180)): None, ((10, 20, 50, 70), (-16384, 16384)): None}
    for (box, off), want in cases.items():
        assert serve.move_rect(box, off, hw) == want == M.move_rect(box, off, hw), (box, off)
    rng = np.random.RandomState(3)
    for _ in range(2000):
        Hi, Wi = int(rng.randint(16, 80)), int(rng.randint(16, 80))
        y0, x0 = int(rng.randint(0, Hi)), int(rng.randint(0, Wi))
        box = (y0, x0, int(rng.randint(y0 + 1, Hi + 1)), int(rng.randint(x0 + 1, Wi + 1)))
        off = (int(rng.randint(-90, 91)), int(rng.randint(-90, 91)))
        got = serve.move_rect(box, off, (Hi, Wi))
        assert got == M.move_rect(box, off, (Hi, Wi))
        cy0, cx0, cy1, cx1 = max(box[0] + off[0], 0), max(box[1] + off[1], 0), min(box[2] + off[0], Hi), min(box[3] + off[1], Wi)
        if cy0 >= cy1 or cx0 >= cx1:
            assert got is None
            continue
        y, x, h, w = got
        assert 0 <= y <= cy0 and cy1 <= y + h <= Hi and 0 <= x <= cx0 and cx1 <= x + w <= Wi      # inside the frame, around the clipped box
        assert h == max(cy1 - cy0, 16) and w == max(cx1 - cx0, 16)
    assert (serve.MOVE_MAX_OFFSET, _lib.MOVE_MAX_OFFSET, M.MAX_OFFSET) == (16384,) * 3 and serve.MOVE_FLIPS == {None: 0, "h": 1, "v": 2, "hv": 3}


# ---- the sessions against a scripted backend -------------------------------------------------------------------------------------------------
class _Stub(_OutlineStub):
    """... with the three calls of DESIGN.md 6r, and a frame that is really edited: save / swap copy and exchange rectangles,
    the fill's pastes write FILL where the keep plane is 0, the drop is the statement"""
    FILL = 77

    def grow(self, plane, grow):
        self.calls.append(("grow", id(plane), grow))
        return U.spec_grow(plane != 0, grow)

    def move_drop(self, frame, lift, lift_rect, plane, lock, box, offset, flip, radius):
        self.calls.append(("move_drop", tuple(lift_rect), id(plane), None if lock is None else id(lock), tuple(box), tuple(offset), flip, radius))
        self.lift = lift.copy()
        frame[...] = M.spec_drop(frame, lift, lift_rect, plane, lock, box, offset, flip, radius)

    def shift(self, plane, box, offset, flip):
        self.calls.append(("shift", id(plane), tuple(box), tuple(offset), flip))
        out = M.spec_shift(plane, box, offset, flip)
        self.plane = out
        return (out,) + L.box_count(out)

    def save(self, frames, origins, window_hw):
        self.calls.append(("save", [tuple(o) for o in origins], tuple(window_hw)))
        return [M.slot_of(f, tuple(o) + tuple(window_hw)) for f, o in zip(frames, origins)]

    def swap(self, frames, origins, window_hw, slots):
        self.calls.append(("swap", [tuple(o) for o in origins], tuple(window_hw)))
        h, w = window_hw
        for f, (y0, x0), slot in zip(frames, origins, slots):
            now = f[y0:y0 + h, x0:x0 + w].reshape(h, 3 * w).copy()
            f[y0:y0 + h, x0:x0 + w] = slot[:, :3 * w].reshape(h, w, 3)
            slot[:, :3 * w] = now

    def fill_keep(self, frames, origins, holes, locks, window_hw):
        super().fill_keep(frames, origins, holes, locks, window_hw)
        self.keeps = [np.where((h == 0) | (False if locks is None else locks[i] != 0), 255, 0).astype(np.uint8) for i, h in enumerate(holes)]
        return self.keeps

    def _paste(self, frames, origins, keeps, window_hw):
        h, w = window_hw
        for f, (y0, x0), k in zip(frames, origins, keeps):
            f[y0:y0 + h, x0:x0 + w][k[y0:y0 + h, x0:x0 + w] == 0] = self.FILL

    def paste_locked(self, frames, origins, locks, window_hw, rgb, m8):
        super().paste_locked(frames, origins, locks, window_hw, rgb, m8)
        self._paste(frames, origins, locks, window_hw)

    def paste_feather(self, frames, origins, locks, window_hw, radius, rgb, m8):
        super().paste_feather(frames, origins, locks, window_hw, radius, rgb, m8)
        self._paste(frames, origins, locks, window_hw)


RING = [(300, 200), (340, 200), (340, 230), (300, 230)]                  # rows 200 .. 229, columns 300 .. 339
BOX = (200, 300, 230, 340)


def _lock_array():
    plane = np.zeros(HW, np.uint8)
    plane[0:8, 0:8] = 255
    plane[215:225, 310:330] = 255                                        # inside the source
    plane[222:232, 350:360] = 255                                        # inside the destination of OFF
    return plane


def _session(stub, lock=False, **kw):
    f = U._noise(HW, 5)
    s = serve.EditSession(None, f, backend=stub, **kw)
    if lock:
        s.set_lock(_lock_array())
    sel = s.select_lasso([RING])
    stub.calls.clear()
    return s, sel, f


OFF = (10, 25)                                                           # smaller than the object: source and destination overlap


def _expect(f, sel, lock, offset, flip, feather, hole_grow, win, keep_source):
    """the frame after the scripted backend's move: the fill's FILL in the window, then the statement's drop of the original pixels"""
    after = f.copy()
    if not keep_source:
        hole = U.spec_grow(sel != 0, hole_grow) != 0
        if lock is not None:
            hole &= lock == 0
        y0, x0, h, w = win
        inwin = np.zeros(HW, bool)
        inwin[y0:y0 + h, x0:x0 + w] = True
        after[hole & inwin] = _Stub.FILL
    rect = M.move_rect(BOX, (0, 0), HW)
    return M.spec_drop(after, M.slot_of(f, rect), rect, sel, lock, BOX, offset, flip, feather or 0)


@pytest.mark.parametrize("keep_source", [False, True])
@pytest.mark.parametrize("lock", [False, True])
@pytest.mark.parametrize("history", [0, 2])
@pytest.mark.parametrize("max_side", [None, 128])
@pytest.mark.parametrize("feather", [None, 4])
def test_move_issues_lift_fill_save_drop_shift_in_that_order(keep_source, lock, history, max_side, feather):
    stub = _Stub()
    s, sel, f = _session(stub, lock, history=history)
    plane0 = sel.plane.copy()
    patches, positions, info = s.move_selection(sel, OFF, flip="h", keep_source=keep_source, max_side=max_side, feather=feather, low_latency=True)
    grown = (198, 298, 232, 342)                                     # hole_grow = 2 is the default
    win = serve.choose_window(grown, HW, margin=0.5)
    dst = (210, 325, 30, 40)
    wins = ([] if keep_source else [win]) + [dst]
    paste = "paste_feather" if feather else "paste_locked"
    fill = [] if keep_source else ["grow", "fill_keep", "run_fill"] + (["save"] if history else []) + [paste]
    assert _names(stub) == ["save"] + fill + (["save"] if history else []) + ["move_drop", "shift"] + ["crop"] * len(wins)
    assert not [c for c in stub.calls if c[0] == "upload"]            # nothing goes up
    saves = [c for c in stub.calls if c[0] == "save"]
    assert saves[0] == ("save", [(200, 300)], (30, 40))               # the lift: move_rect(box, (0, 0))
    if history:
        assert saves[1:] == [("save", [w[:2]], w[2:]) for w in wins]  # each rectangle in front of its own step
    calls = {c[0]: c for c in stub.calls}
    lk = s._lock_plane
    assert calls["move_drop"] == ("move_drop", (200, 300, 30, 40), id(sel.plane), None if lk is None else id(lk), BOX, OFF, 1, feather or 0)
    assert calls["shift"] == ("shift", id(sel.plane), BOX, OFF, 1)
    assert np.array_equal(stub.lift[:, :120].reshape(30, 40, 3), f[200:230, 300:340])       # the lift holds the ORIGINAL pixels
    work = None
    if not keep_source:
        work = serve.choose_working_size(win[2:], max_side) if max_side else None
        assert calls["grow"] == ("grow", id(sel.plane), 2)
        assert calls["fill_keep"] == ("fill_keep", [win[:2]], [HW], 1 if lock else None, win[2:])
        assert calls["run_fill"] == ("run_fill", [win[:2]], [None], 1 if lock else None, win[2:], work, True)
        assert np.array_equal(stub.holes[0], U.spec_grow(plane0 != 0, 2))
    assert [c[1] for c in stub.calls if c[0] == "crop"] == wins
    assert positions == [(w[1], w[0]) for w in wins] and [p.shape for p in patches] == [w[2:] + (3,) for w in wins]
    moved = info.pop("selection")
    want = dict(windows=wins, move=True, offset=OFF, flip="h", selected=1200)
    if lock:
        want["locked"] = True
    if work:
        want["work"] = work
    if history:
        want["undoable"] = True
    if feather:
        want["feather"] = 4
    assert info == want
    assert isinstance(moved, serve.Selection) and moved is not sel and moved.box == (210, 325, 240, 365) and moved.count == 1200
    assert np.array_equal(moved.plane, M.spec_shift(plane0, BOX, OFF, 1)) and np.array_equal(sel.plane, plane0) and sel.box == BOX
    after = _expect(f, plane0, _lock_array() if lock else None, OFF, 1, feather, 2, win, keep_source)
    assert np.array_equal(s._frame, after) and not np.array_equal(after, f)
    for p, w in zip(patches, wins):
        assert np.array_equal(p, after[w[0]:w[0] + w[2], w[1]:w[1] + w[3]])
    if lock:                                                          # locked source pixels are not filled, locked destination pixels never change
        assert np.array_equal(after[_lock_array() != 0], f[_lock_array() != 0])
    if history:
        assert s.can_undo and len(s._undo) == 1 and isinstance(s._undo[0][0], serve._Sequence)
        assert s.history_bytes_used == sum(serve.window_saved_bytes(w[2], w[3]) for w in wins)
    else:
        assert not s.can_undo


def test_undo_swaps_in_reverse_and_redo_forward_and_both_restore_every_byte():
    stub = _Stub()
    s, sel, f = _session(stub, history=3)
    _, _, info = s.move_selection(sel, OFF, feather=2)
    win, dst = info["windows"]
    assert serve._windows_intersect(win, dst)                         # the case region entries could not hold
    after = s._frame.copy()
    assert np.array_equal(after, _expect(f, sel.plane, None, OFF, 0, 2, 2, win, False))
    for _ in range(2):                                                # twice: the slots are exchanged, not used up
        stub.calls.clear()
        patches, positions, u = s.undo()
        assert stub.calls[:2] == [("swap", [dst[:2]], dst[2:]), ("swap", [win[:2]], win[2:])]          # REVERSE order
        assert _names(stub) == ["swap", "swap", "crop", "crop"] and [c[1] for c in stub.calls[2:]] == [win, dst]
        assert u == dict(windows=[win, dst], undo_depth=0, redo_depth=1) and positions == [(win[1], win[0]), (dst[1], dst[0])]
        assert np.array_equal(s._frame, f) and np.array_equal(patches[1], f[dst[0]:dst[0] + dst[2], dst[1]:dst[1] + dst[3]])
        stub.calls.clear()
        patches, positions, r = s.redo()
        assert stub.calls[:2] == [("swap", [win[:2]], win[2:]), ("swap", [dst[:2]], dst[2:])]          # forward order
        assert r == dict(windows=[win, dst], undo_depth=1, redo_depth=0)
        assert np.array_equal(s._frame, after) and np.array_equal(patches[0], after[win[0]:win[0] + win[2], win[1]:win[1] + win[3]])
    # the wrong order would not have restored the frame: the second slot holds the bytes the fill left
    g = after.copy()
    wins, slots, _ = s._undo[-1]
    copies = [x.copy() for x in slots]
    for i in (0, 1):
        stub.swap([g], [wins[i][:2]], wins[i][2:], [copies[i]])
    assert not np.array_equal(g, f)
    # a clone is one rectangle, one swap; it sits on the journal with every other kind
    sk = np.zeros(HW, np.uint8)
    sk[50:60, 50:80] = 255
    s.edit(sk, max_grow=0)
    before_clone = s._frame.copy()
    _, _, info = s.clone_selection(info["selection"], (-100, -200), flip="hv")
    assert info["windows"] == [(110, 125, 30, 40)] and s.history_bytes_used > 0 and len(s._undo) == 3
    stub.calls.clear()
    patches, positions, u = s.undo()
    assert _names(stub) == ["swap", "crop"] and u["windows"] == [(110, 125, 30, 40)] and isinstance(patches, list) and len(patches) == 1
    assert np.array_equal(s._frame, before_clone)
    s.undo()                                                          # the edit: the kind it always was
    assert _names(stub)[-2:] == ["swap", "crop"]
    s.undo()
    assert np.array_equal(s._frame, f) and not s.can_undo and len(s._redo) == 3
    s.redo()
    assert np.array_equal(s._frame, after)
    s.move_selection(sel, (0, 1), keep_source=True)                   # a new step drops the redo entries
    assert not s.can_redo


def test_server_undo_and_redo_take_a_move_back_in_order():
    """moves are not batched by the server, but a session that made one is undone through it as session.undo() does it -- alone
    and in a group with sessions whose tops are of the other kinds, none of which fails"""
    stub = _Stub()
    srv = serve.BatchingServer(object(), max_batch=4, max_wait_s=0.01, window=True, max_grow=0)
    try:
        s = serve.EditSession(srv.model, U._noise(HW, 5), backend=stub, history=4)
        f = s.frame()
        sel = s.select_lasso([RING])
        _, _, info = s.move_selection(sel, OFF, feather=2)
        win, dst = info["windows"]
        after = s.frame()
        stub.calls.clear()
        patches, positions, u = srv.undo(s)
        assert stub.calls[:2] == [("swap", [dst[:2]], dst[2:]), ("swap", [win[:2]], win[2:])]          # REVERSE order
        assert u == dict(windows=[win, dst], undo_depth=0, redo_depth=1) and len(patches) == 2 and positions == [(win[1], win[0]), (dst[1], dst[0])]
        assert np.array_equal(s.frame(), f)
        stub.calls.clear()
        _, _, r = srv.redo(s)
        assert stub.calls[:2] == [("swap", [win[:2]], win[2:]), ("swap", [dst[:2]], dst[2:])]          # forward order
        assert r == dict(windows=[win, dst], undo_depth=1, redo_depth=0) and np.array_equal(s.frame(), after)
        with pytest.raises(IndexError):
            srv.redo(s)
        # a mixed group: a move, a plain edit of the same window size as another, a region edit, and a session with nothing to undo
        sk = np.zeros(HW, np.uint8)
        sk[50:60, 50:80] = 255
        others = [serve.EditSession(srv.model, U._noise(HW, 6 + k), backend=stub, history=2) for k in range(4)]
        before = [o.frame() for o in others]
        others[0].edit(sk, max_grow=0)
        others[1].edit(sk, max_grow=0)
        others[2].edit_strokes([([(30, 20), (60, 30)], 3), ([(500, 300), (520, 310)], 3)])
        group = [(("history",), dict(session=x, op="undo"), None, {}) for x in [s] + others]
        outs = srv._run_history(group)
        assert [isinstance(o, tuple) for o in outs] == [True, True, True, True, False] and isinstance(group[4][3]["err"], IndexError)
        assert all("err" not in g[3] for g in group[:4])
        assert np.array_equal(s.frame(), f) and all(np.array_equal(o.frame(), b) for o, b in zip(others, before))
        assert outs[0][2]["windows"] == [win, dst] and "window" in outs[1][2] and len(outs[3][2]["windows"]) == 2
    finally:
        srv.close()


def test_a_shift_that_fails_leaves_no_entry_for_a_selection_nobody_got():
    class _NoShift(_Stub):
        def shift(self, plane, box, offset, flip):
            raise RuntimeError("the device said no")

    stub = _NoShift()
    s, sel, f = _session(stub, history=3)
    sk = np.zeros(HW, np.uint8)
    sk[50:60, 50:80] = 255
    s.edit(sk, max_grow=0)
    assert s.can_undo
    with pytest.raises(RuntimeError, match="said no"):
        s.move_selection(sel, OFF)
    assert not s.can_undo and not s.can_redo and s.history_bytes_used == 0        # the frame was written: no entry restores a state it was in
    assert not np.array_equal(s._frame, f)


def test_history_bytes_caps_the_sum_of_the_slots():
    stub = _Stub()
    win = serve.choose_window((198, 298, 232, 342), HW, margin=0.5)
    a, b = serve.window_saved_bytes(*win[2:]), serve.window_saved_bytes(30, 40)
    s, sel, f = _session(stub, history=4, history_bytes=a + b - 1)    # each slot fits, the two together do not
    sk = np.zeros(HW, np.uint8)
    sk[50:60, 50:80] = 255
    s.edit(sk, max_grow=0)
    assert s.can_undo
    stub.calls.clear()
    _, _, info = s.move_selection(sel, OFF)
    assert info["undoable"] is False and not s.can_undo and not s.can_redo and s.history_bytes_used == 0
    assert [c for c in stub.calls if c[0] == "save"] == [("save", [(200, 300)], (30, 40))]                # the lift alone
    s, sel, f = _session(stub, history=4, history_bytes=a + b)
    _, _, info = s.move_selection(sel, OFF)
    assert info["undoable"] is True and s.history_bytes_used == a + b
    _, _, info = s.clone_selection(sel, OFF)                          # over the cap together: the OLDEST entry goes
    assert info["undoable"] is True and len(s._undo) == 1 and s.history_bytes_used == b
    s, sel, f = _session(stub, history=1)                             # history counts steps: a move is one
    s.move_selection(sel, OFF)
    s.move_selection(sel, (-5, 0))
    assert len(s._undo) == 1


def test_hole_grow_window_encode_and_moving_again():
    stub = _Stub()
    s, sel, f = _session(stub, history=1)
    _, _, info = s.move_selection(sel, (0, 50), hole_grow=0)
    assert "grow" not in _names(stub) and stub.holes[0] is sel.plane  # the selection's plane as it is
    assert info["windows"][0] == serve.choose_window(BOX, HW, margin=0.5)
    stub.calls.clear()
    _, _, info = s.move_selection(sel, (0, 50), hole_grow=np.int64(16), window=(180, 280, 96, 128), flip="v")
    assert info["windows"] == [(180, 280, 96, 128), (200, 350, 30, 40)] and {c[0]: c for c in stub.calls}["grow"][2] == 16
    assert {c[0]: c for c in stub.calls}["move_drop"][6] == 2
    _, _, info = s.move_selection(sel, (0, 50), window=(180, 280, 99, 131), max_side=64, margin=0.25)
    assert info["windows"][0] == (180, 280, 99, 131) and info["work"] == serve.choose_working_size((99, 131), 64)
    stub.calls.clear()
    patches, _, info = s.move_selection(sel, (0, 50), encode="png")
    assert patches == [b"png", b"png"] and stub.calls[-1] == ("crop_png", info["windows"]) and "crop" not in _names(stub)
    patches, _, info = s.clone_selection(sel, (0, 50), encode=("jpg", 80))
    assert patches == [b"jpg"] and stub.calls[-1][:3] == ("crop_jpg", info["windows"], 80)
    # pushed partly over the edge: the destination rectangle is clipped, the moved selection too; and it moves again
    _, _, info = s.move_selection(sel, (-215, -320))
    assert info["windows"][1] == (0, 0, 16, 20) and info["selection"].box == (0, 0, 15, 20) and info["selection"].count == 300
    _, _, again = s.move_selection(info["selection"], (100, 100))
    assert again["selection"].box == (100, 100, 115, 120) and again["selected"] == 300
    # a clone with keep_source spelled either way is the same call
    stub.calls.clear()
    s.clone_selection(sel, OFF, keep_source=False)
    assert "run_fill" not in _names(stub)


def test_refusals_make_no_backend_call():
    stub = _Stub()
    s, sel, f = _session(stub, history=1)
    other = serve.EditSession(None, np.zeros((64, 64, 3), np.uint8), backend=_Stub()).select_lasso([[(1, 1), (30, 1), (15, 30)]])
    empty = s.combine(sel, sel, "subtract")
    stub.calls.clear()
    bad = [lambda: s.move_selection(other, OFF),
           lambda: s.move_selection(sel.plane, OFF),
           lambda: s.move_selection(None, OFF),
           lambda: s.move_selection(empty, OFF),
           lambda: s.move_selection(sel, 5),
           lambda: s.move_selection(sel, (1, 2, 3)),
           lambda: s.move_selection(sel, (1.0, 2)),
           lambda: s.move_selection(sel, (True, 2)),
           lambda: s.move_selection(sel, (16385, 0)),
           lambda: s.move_selection(sel, (0, -16385)),
           lambda: s.move_selection(sel, (400, 0)),                   # wholly out
           lambda: s.move_selection(sel, (0, -340)),
           lambda: s.move_selection(sel, (-16384, 16384)),
           lambda: s.move_selection(sel, OFF, flip="x"),
           lambda: s.move_selection(sel, OFF, flip=1),
           lambda: s.move_selection(sel, OFF, flip=["h"]),
           lambda: s.move_selection(sel, OFF, hole_grow=-1),
           lambda: s.move_selection(sel, OFF, hole_grow=17),
           lambda: s.move_selection(sel, OFF, hole_grow=1.5),
           lambda: s.move_selection(sel, OFF, hole_grow=True),
           lambda: s.move_selection(sel, OFF, window=(0, 0, 100, 128)),
           lambda: s.move_selection(sel, OFF, window=(350, 0, 64, 64)),
           lambda: s.move_selection(sel, OFF, margin=-1.0),
           lambda: s.move_selection(sel, OFF, max_side=8),
           lambda: s.move_selection(sel, OFF, encode="gif"),
           lambda: s.move_selection(sel, OFF, feather=17),
           lambda: s.move_selection(sel, OFF, feather=-1),
           lambda: s.clone_selection(sel, OFF, feather=2.5),
           lambda: s.clone_selection(sel, OFF, max_side=8),
           lambda: s.clone_selection(sel, (400, 0)),
           lambda: s.clone_selection(other, OFF)]
    for k, call in enumerate(bad):
        with pytest.raises((ValueError, TypeError)):
            call()
        assert stub.calls == [] and not s.can_undo, k
    with pytest.raises(ValueError, match="moves the whole selection out of the frame"):
        s.move_selection(sel, (-230, 0))
    with pytest.raises(ValueError, match="empty selection: nothing to move"):
        s.clone_selection(empty, OFF)
    s.move_selection(sel, (-229, 0), keep_source=True)                # one row stays: valid
    doc = serve.EditSession.move_selection.__doc__
    for phrase in ("Locked source pixels are not filled; they are still copied", "Locked destination pixels never change",
                   "clone_selection(...) is move_selection(..., keep_source=True)"):
        assert phrase in doc


def test_existing_calls_issue_what_they_issued():
    """edit, fill, select_*, combine, undo and redo on a backend WITH the move's calls never use them, and issue the very calls
    they issue on the backend of before"""
    sk = np.zeros(HW, np.uint8)
    sk[200:210, 300:330] = 255
    mask = np.zeros(HW, np.uint8)
    mask[200:230, 300:340] = 1
    f = U._noise(HW, 5)
    f[200:230, 300:340] = U.REGION
    new = {"grow", "move_drop", "shift"}

    seqs = {}
    for k, cls in enumerate((_OutlineStub, _Stub)):
        for lock in (False, True):
            stub = cls()
            s = serve.EditSession(None, f, backend=stub, history=3)
            if lock:
                s.set_lock(mask)
            stub.calls.clear()
            s.edit(sk, max_grow=0)
            s.edit_strokes([([(30, 20), (60, 30)], 3), ([(500, 300), (520, 310)], 3)])
            s.fill(mask)
            s.fill_strokes([([(300.5, 200.0), (340.0, 230.25)], 12.0)], feather=2, max_side=128)
            a = s.select_similar((210, 320))
            b = s.select_lasso([RING], grow=2)
            c = s.combine(a, b, "xor")
            s.invert(c)
            s.fill_selection(b)
            s.fill_similar((210, 320))
            s.fill_lasso([RING])
            s.set_lock(b)
            b.rings()
            s.undo()
            s.undo()
            s.redo()
            seqs[k, lock] = _names(stub)
            assert stub.calls and not new & set(_names(stub))
            assert [e for e in s._undo + s._redo if isinstance(e[0], serve._Sequence)] == []
    assert seqs[0, False] == seqs[1, False] and seqs[0, True] == seqs[1, True]
    # the fill's calls, spelled out: the split of _fill changed none
    stub = _Stub()
    s = serve.EditSession(None, f, backend=stub, history=1)
    stub.calls.clear()
    s.fill(mask, feather=3)
    assert _names(stub) == ["fill_keep", "run_fill", "save", "paste_feather", "crop"]
    s.undo()
    assert _names(stub)[-2:] == ["swap", "crop"] and not isinstance(s._redo[0][0], (serve._Sequence, serve._Regions))
    # a backend of before cannot move, and says so only when asked to
    stub = _OutlineStub()
    s = serve.EditSession(None, f, backend=stub, history=1)
    sel = s.select_lasso([RING])
    with pytest.raises(AttributeError):
        s.move_selection(sel, OFF)


def test_model_backend_grow_drop_and_shift():
    """_ModelBackend's three calls on a scripted model: one model call each, and the shift's tile records are the one download"""
    from sketch_tiles_util import sketch_tiles as spec_tiles

    class _T:
        def __init__(self, a):
            self.a, self.n = a, 0

        def cpu(self):
            self.n += 1
            return self

        def numpy(self):
            return self.a

    class _Model:
        def __init__(self):
            self.calls, self.tiles = [], []

        def select_grow_u8(self, plane, grow):
            self.calls.append(("select_grow_u8", grow))
            return U.spec_grow(plane != 0, grow)

        def move_drop_u8(self, frame, lift, lift_rect, sel, lock, box, offset, flip=0, radius=0):
            self.calls.append(("move_drop_u8", tuple(lift_rect), tuple(box), tuple(offset), flip, radius))

        def plane_shift_u8(self, sel, box, offset, flip=0):
            self.calls.append(("plane_shift_u8", tuple(box), tuple(offset), flip))
            return M.spec_shift(sel, box, offset, flip)

        def sketch_tiles_u8(self, plane, tile):
            self.calls.append(("sketch_tiles_u8", tile))
            self.tiles.append(_T(spec_tiles(plane, tile)))
            return self.tiles[-1]

    be = serve._ModelBackend.__new__(serve._ModelBackend)
    be.model = _Model()
    sel = np.zeros((37, 53), np.uint8)
    sel[5:20, 7:30] = 255
    assert np.array_equal(be.grow(sel, 3), U.spec_grow(sel != 0, 3))
    be.move_drop(None, None, (5, 7, 16, 23), sel, None, (5, 7, 20, 30), (3, -4), 2, 5)
    plane, box, count = be.shift(sel, (5, 7, 20, 30), (3, -10), 1)
    assert np.array_equal(plane, M.spec_shift(sel, (5, 7, 20, 30), (3, -10), 1)) and box == (8, 0, 23, 20) and count == 15 * 20
    assert be.model.calls == [("select_grow_u8", 3), ("move_drop_u8", (5, 7, 16, 23), (5, 7, 20, 30), (3, -4), 2, 5),
                              ("plane_shift_u8", (5, 7, 20, 30), (3, -10), 1), ("sketch_tiles_u8", 32)]
    assert [t.n for t in be.model.tiles] == [1]
    plane, box, count = be.shift(sel, (5, 7, 20, 30), (40, 0), 0)     # wholly out: the empty selection
    assert box is None and count == 0 and not plane.any()


# ---- the C-ABI -------------------------------------------------------------------------------------------------------------
def test_abi_has_two_new_symbols_in_a_header_of_their_own():
    hdr = open(os.path.join(ROOT, "include", "sketchedit_move.h")).read()
    declared = re.findall(r"^(?:int|size_t)\s+(se_\w+)\(", hdr, re.M)
    assert declared == _lib.abi_names("sketchedit_move.h") == ["se_move_drop_u8", "se_plane_shift_u8"]
    others = [n for n in _lib.abi_names() if n not in declared]
    for name in others:                                               # the header refers to other families by DESIGN section
        assert not re.search(r"\b%s\b" % name, hdr), name
    for name in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if name != "sketchedit_move.h":
            text = open(os.path.join(ROOT, "include", name)).read()
            assert "se_move" not in text.replace("se_move_blend_u8", "") and "se_plane_shift" not in text, name      # (the seamless drop's two apart)
    assert "se_move.hip" in _lib.SOURCES and "se_api_move.hip" in _lib.SOURCES and _lib.SOURCES[-1] == "se_api.hip"
    assert re.search(r"#define SE_MOVE_MAX_OFFSET 16384\b", hdr) and re.search(r"#define SE_MOVE_MAX_RADIUS 16\b", hdr)
    assert re.search(r"#define SE_MOVE_FLIP_X 1\b", hdr) and re.search(r"#define SE_MOVE_FLIP_Y 2\b", hdr)
    assert (_lib.MOVE_MAX_RADIUS, _lib.MOVE_FLIP_X, _lib.MOVE_FLIP_Y, M.MAX_RADIUS, serve.FEATHER_MAX_RADIUS) == (16, 1, 2, 16, 16)
    import ctypes
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    lib = ctypes.CDLL(_lib.LIB_PATH)                                    # the built library, as the other host tests load it
    for s in declared:
        getattr(lib, s)
    from sketchedit_amd import kernel_labels
    assert kernel_labels.label_of("void se::move_drop_kernel<true>(unsigned char*, int)") == "move_drop"
    assert kernel_labels.label_of("move_drop_kernel<false>(unsigned char*, int)") == "move_drop"
    assert kernel_labels.label_of("plane_shift_kernel(unsigned char*, long, long)") == "plane_shift"
    misc = open(os.path.join(_lib.CSRC, "se_misc.hip")).read()
    for label in ("move_drop", "plane_shift"):
        assert '"%s"' % label in misc and label in set(kernel_labels.KERNEL_LABELS.values())
    from sketchedit_amd.models.editline2_model import EditLine2Model
    for name in ("move_drop_u8", "plane_shift_u8"):
        assert callable(getattr(_lib.Engine, name)) and callable(getattr(EditLine2Model, name))


def test_the_kernels_cross_compile_for_gfx950(tmp_path):
    import shutil
    import subprocess
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc on this machine")
    obj = str(tmp_path / "se_move.o")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(_lib.CSRC, "se_move.hip"), "-o", obj])
    assert os.path.getsize(obj) > 0


# ---- the kernels' arithmetic, lane by lane -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(16, 16), (37, 53), (65, 129)], ids=lambda hw: "%dx%d" % hw)
def test_tiled_arithmetic_is_the_statement(hw):
    """se_move.hip's gather through aligned dwords, its byte swap under the x flip, the staged counts, the division by multiply
    and the store ownership, on one flat byte array in which every access is checked against the span the kernel may touch"""
    Hi, Wi = hw
    rng = np.random.RandomState(Hi)
    frame = rng.randint(0, 256, (Hi, Wi, 3)).astype(np.uint8)
    before = rng.randint(0, 256, (Hi, Wi, 3)).astype(np.uint8)
    sel = np.where(rng.rand(Hi, Wi) < 0.7, rng.randint(1, 256, (Hi, Wi)), 0).astype(np.uint8)
    lock = np.where(rng.rand(Hi, Wi) < 0.2, 255, 0).astype(np.uint8)
    box = (1, 2, Hi - 3, Wi - 1)
    rect = M.move_rect(box, (0, 0), hw)
    slot = M.slot_of(before, rect)
    cases = [((0, 0), 0, 0, False), ((1, -1), 1, 1, True), ((-5, 7), 2, 3, False), ((Hi - 6, 3 - Wi), 3, 16, True), ((2, 3), 3, 0, True),
             ((0, -Wi), 1, 2, False)]
    for k, (off, flip, r, locked) in enumerate(cases):
        mem = M.Memory(16384 + 5 * Hi * Wi + slot.size)
        fa = mem.put(1024 + k % 4, frame)
        sa = mem.put(fa + 3 * Hi * Wi + 1031, sel)
        la = mem.put(sa + Hi * Wi + 1033, lock)
        pa = mem.put((la + Hi * Wi + 1024 + 15) // 16 * 16, slot)
        oa = pa + slot.size + 1024 + (k + 1) % 4
        clean = mem.mem.copy()
        tiles = M.tiled_drop(mem, fa, Hi, Wi, pa, rect, sa, la if locked else None, box, off, flip, r)
        want = M.spec_drop(frame, slot, rect, sel, lock if locked else None, box, off, flip, r)
        assert np.array_equal(mem.get(fa, frame.shape), want), (hw, off, flip, r)
        changed = np.flatnonzero(mem.mem != clean)
        assert changed.size == 0 or (fa <= changed.min() and changed.max() < fa + 3 * Hi * Wi)
        assert (tiles == 0) == (off == (0, -Wi)) and (tiles == 0 or changed.size > 0)
        mem.mem[:] = clean
        M.tiled_shift(mem, sa, Hi, Wi, box, off, flip, oa)
        assert np.array_equal(mem.get(oa, hw), M.spec_shift(sel, box, off, flip)), (hw, off, flip)
        changed = np.flatnonzero(mem.mem != clean)
        assert oa <= changed.min() and changed.max() < oa + Hi * Wi
