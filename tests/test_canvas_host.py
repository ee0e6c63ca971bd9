"""Host tests of the canvas of an editing session: the statement of tests/canvas_util.py against numpy's own flips,
turns and pads and against the header's known answers, serve's pure helpers and every refusal, EditSession.canvas and its wrappers,
the new journal entry kind and the outpaint against a scripted backend that logs every call and really edits numpy frames, the
tile-by-tile restatement of canvas_turn, and the new entry's place in the C-ABI.  CPU only; every comparison is exact."""
import os
import re

import numpy as np
import pytest

from sketchedit_amd import _lib, serve
import abi_util
import canvas_util as C
import lasso_util as L
import select_util as U
from test_fill_host import _names
from test_move_host import BOX, HW, OFF, RING, _Stub as _MoveStub, _lock_array

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PADS = {C.EDGE: "edge", C.REFLECT: "reflect"}


# ---- the statement --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("o", range(8))
def test_the_eight_orientations_are_numpy_flips_and_turns(o):
    for hw, ch in (((3, 5), 3), ((1, 7), 1), ((6, 1), 3), ((4, 4), 1)):
        rng = np.random.RandomState(o + hw[0])
        a = rng.randint(0, 256, hw + ((3,) if ch == 3 else ())).astype(np.uint8)
        got, want = C.orient(a, o), C.orient_formula(a, o)
        assert got.shape == want.shape and np.array_equal(got, want), (o, hw)
        assert got.shape[:2] == ((hw[1], hw[0]) if o & 4 else hw)
    a = np.arange(6, dtype=np.uint8).reshape(2, 3)
    named = {0: a, 1: np.fliplr(a), 2: np.flipud(a), 3: np.rot90(a, 2), 4: a.T, 5: np.rot90(a), 6: np.rot90(a, -1), 7: np.rot90(a, 2).T}
    assert np.array_equal(C.orient(a, o), named[o])
    assert serve.CANVAS_ORIENTS == C.ORIENTS == {None: 0, "h": 1, "v": 2, "180": 3, "transpose": 4, "ccw": 5, "cw": 6, "transverse": 7}
    inverse = {0: 0, 1: 1, 2: 2, 3: 3, 4: 4, 5: 6, 6: 5, 7: 7}
    assert np.array_equal(C.orient(C.orient(a, o), inverse[o]), a)


@pytest.mark.parametrize("n", [1, 2, 3, 7])
def test_fold_is_numpy_pad(n):
    row = np.arange(10, 10 + n)
    for before, after in ((0, 0), (1, 1), (n, n + 1), (5 * n + 3, 4 * n + 1)):     # several periods
        idx = [C.fold(i, n, C.EDGE) for i in range(-before, n + after)]
        assert np.array_equal(row[idx], np.pad(row, (before, after), mode="edge"))
        idx = [C.fold(i, n, C.REFLECT) for i in range(-before, n + after)]
        assert np.array_equal(row[idx], np.pad(row, (before, after), mode="reflect"))
        idx = [C.fold(i, n, C.CONSTANT) for i in range(-before, n + after)]
        got = np.array([99 if i is None else row[i] for i in idx])
        assert np.array_equal(got, np.pad(row, (before, after), mode="constant", constant_values=99))


@pytest.mark.parametrize("mode", [C.EDGE, C.REFLECT, C.CONSTANT])
def test_the_rectangle_is_numpy_pad_then_a_slice(mode):
    rng = np.random.RandomState(mode)
    for hw in ((5, 7), (1, 4), (6, 1)):
        img = rng.randint(0, 256, hw + (3,)).astype(np.uint8)
        for o in (0, 3, 5):
            O = C.orient(img, o)
            Ho, Wo = O.shape[:2]
            py, px = 2 * Ho + 3, 2 * Wo + 1
            kw = dict(mode="constant", constant_values=0) if mode == C.CONSTANT else dict(mode=PADS[mode])
            big = np.pad(O, ((py, py), (px, px), (0, 0)), **kw)
            if mode == C.CONSTANT:
                inside = np.zeros(big.shape[:2], bool)
                inside[py:py + Ho, px:px + Wo] = True
                big[~inside] = (9, 200, 31)
            for y0, x0, h, w in ((0, 0, Ho, Wo), (-py, -px, Ho + 2 * py, Wo + 2 * px), (Ho - 1, -2, 3, Wo + 1), (Ho + 1, Wo, 2, 1)):
                got = C.spec_canvas(img, hw, (h, w), (y0, x0), o, mode, 9 | 200 << 8 | 31 << 16)
                assert np.array_equal(got, big[py + y0:py + y0 + h, px + x0:px + x0 + w]), (hw, o, (y0, x0, h, w))


def test_known_answers_of_the_header():
    hdr = open(os.path.join(ROOT, "include", "sketchedit_canvas.h")).read()
    img = np.array([[1, 2, 3], [4, 5, 6]], np.uint8)
    cases = [((3, 2), (0, 0), 6, C.EDGE, 0, [[4, 1], [5, 2], [6, 3]]), ((3, 2), (0, 0), 5, C.EDGE, 0, [[3, 6], [2, 5], [1, 4]]),
             ((2, 5), (0, -1), 1, C.EDGE, 0, [[3, 3, 2, 1, 1], [6, 6, 5, 4, 4]]), ((1, 9), (1, -4), 0, C.REFLECT, 0, [[4, 5, 6, 5, 4, 5, 6, 5, 4]]),
             ((3, 4), (-1, 1), 0, C.CONSTANT, 9, [[9, 9, 9, 9], [2, 3, 9, 9], [5, 6, 9, 9]])]
    for out_hw, origin, o, mode, rgb, want in cases:
        assert np.array_equal(C.spec_canvas(img, (2, 3), out_hw, origin, o, mode, rgb), np.array(want, np.uint8)), (o, mode)
        assert str(want) in hdr, want
    want = [[255, 255, 255, 255], [0, 0, 255, 255], [0, 0, 255, 255]]
    assert np.array_equal(C.spec_canvas(None, (2, 3), (3, 4), (-1, 1), 0, C.CONSTANT, 255), np.array(want, np.uint8)) and str(want) in hdr
    # what follows: a crop of an extension by its margins gives the input back; the x mirror reverses pixels, not bytes
    rgb = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3)
    big = C.spec_canvas(rgb, (2, 3), (8, 9), (-3, -4), 0, C.REFLECT)
    assert np.array_equal(C.spec_canvas(big, (8, 9), (2, 3), (3, 4), 0, C.EDGE), rgb)
    assert np.array_equal(C.spec_canvas(rgb, (2, 3), (2, 3), (0, 0), 1, C.EDGE)[0, 0], rgb[0, 2])


# ---- serve's pure helpers ---------------------------------------------------------------------------------------------------------------------
def test_canvas_size_orient_pad_and_the_new_area():
    assert serve.canvas_size((120, 104), None, None) == ((120, 104), (0, 0))
    assert serve.canvas_size((120, 104), "cw", None) == ((104, 120), (0, 0)) == serve.canvas_size((120, 104), "transverse", None)
    assert serve.canvas_size((120, 104), "180", (-3, 5, 40, 17)) == ((40, 17), (-3, 5))
    assert serve.canvas_size((120, 104), "ccw", (0, 0, 104, 120)) == ((104, 120), (0, 0))
    assert [serve.canvas_orient(k) for k in (None, "h", "v", "180", "transpose", "ccw", "cw", "transverse")] == list(range(8))
    assert serve.canvas_pad("edge") == (0, 0) and serve.canvas_pad("reflect") == (1, 0)
    assert serve.canvas_pad((1, 2, 3)) == (2, 1 | 2 << 8 | 3 << 16) and serve.canvas_pad([255, 0, np.uint8(7)]) == (2, 255 | 7 << 16)
    assert (serve.CANVAS_CONSTANT, serve.CANVAS_MAX_SIDE, serve.CANVAS_MAX_OFFSET) == (C.CONSTANT, C.MAX_SIDE, C.MAX_OFFSET) == (2, 32768, 1 << 20)
    assert (_lib.CANVAS_EDGE, _lib.CANVAS_REFLECT, _lib.CANVAS_CONSTANT, _lib.CANVAS_MAX_SIDE, _lib.CANVAS_MAX_OFFSET) == (0, 1, 2, 32768, 1 << 20)
    # the new area's box in closed form = the box of the statement's plane
    for hw, out_hw, origin in (((20, 30), (25, 30), (-5, 0)), ((20, 30), (25, 30), (0, 0)), ((20, 30), (20, 37), (0, -7)), ((20, 30), (20, 37), (0, 0)),
                               ((20, 30), (26, 36), (-3, -3)), ((20, 30), (22, 31), (-2, 0)), ((20, 30), (10, 10), (40, 40)), ((20, 30), (30, 30), (-5, 0)),
                               ((20, 30), (10, 10), (3, 3)), ((20, 30), (20, 30), (0, 0)), ((20, 30), (10, 12), (15, 3)), ((20, 30), (10, 12), (3, 25))):
        plane = C.spec_canvas(None, hw, out_hw, origin, 0, C.CONSTANT, 255)
        assert serve.canvas_new_box(hw, out_hw, origin) == serve.sketch_bbox(plane), (hw, out_hw, origin)


@pytest.mark.parametrize("bad", [
    lambda: serve.canvas_orient("left"), lambda: serve.canvas_orient(6), lambda: serve.canvas_orient(["cw"]),
    lambda: serve.canvas_pad("wrap"), lambda: serve.canvas_pad((1, 2)), lambda: serve.canvas_pad((1, 2, 256)), lambda: serve.canvas_pad((1, 2.0, 3)),
    lambda: serve.canvas_pad(None), lambda: serve.canvas_pad((True, 0, 0)),
    lambda: serve.canvas_size((120, 104), "cw", (0, 0, 16)), lambda: serve.canvas_size((120, 104), None, (0, 0, 16.0, 16)),
    lambda: serve.canvas_size((120, 104), None, (0, 0, 0, 16)), lambda: serve.canvas_size((120, 104), None, (0, 0, 32769, 16)),
    lambda: serve.canvas_size((120, 104), None, (0, 0, 32768, 32768)), lambda: serve.canvas_size((120, 104), None, ((1 << 20) + 1, 0, 16, 16)),
    lambda: serve.canvas_size((120, 104), None, (0, -(1 << 20) - 1, 16, 16)), lambda: serve.canvas_size((120, 104), None, (0, 0, 15, 40)),
    lambda: serve.canvas_size((120, 104), None, (0, 0, 40, 15)), lambda: serve.canvas_size((120, 104), "diag", None),
    lambda: serve.canvas_size((120, 104), None, "abcd")])
def test_the_pure_helpers_refuse(bad):
    with pytest.raises(ValueError):
        bad()


# ---- the sessions against a scripted backend ---------------------------------------------------------------------------------------------------
class _Stub(_MoveStub):
    """... with the one call of DESIGN.md 6y: the statement, on numpy frames and planes"""

    def canvas(self, src, src_hw, out_hw, origin, orient, pad, rgb, tiles=False):
        self.calls.append(("canvas", "none" if src is None else ("plane" if src.ndim == 2 else "frame"), tuple(src_hw), tuple(out_hw), tuple(origin),
                           orient, pad, rgb, tiles))
        out = C.spec_canvas(src, tuple(src_hw), tuple(out_hw), tuple(origin), orient, pad, rgb)
        return (out,) + L.box_count(out) if tiles else out


def _session(stub, lock=False, **kw):
    f = U._noise(HW, 5)
    s = serve.EditSession(None, f, backend=stub, **kw)
    if lock:
        s.set_lock(_lock_array())
    sel = s.select_lasso([RING])
    stub.calls.clear()
    return s, sel, f


def _canvas_calls(stub):
    return [c for c in stub.calls if c[0] == "canvas"]


def _mask(hw=HW):
    m = np.zeros(hw, np.uint8)
    m[50:70, 80:120] = 255
    return m


@pytest.mark.parametrize("lock", [False, True])
def test_each_wrapper_is_one_launch_per_array_and_the_statement(lock):
    H, W = HW
    cases = [("orient_canvas", ("cw",), {}, 6, (W, H), (0, 0), 0, 0), ("orient_canvas", ("h",), {}, 1, HW, (0, 0), 0, 0),
             ("crop_canvas", ((30, 41, 217, 333),), {}, 0, (217, 333), (30, 41), 0, 0),
             ("extend_canvas", (), dict(top=3, right=50, pad="reflect"), 0, (H + 3, W + 50), (-3, 0), 1, 0),
             ("extend_canvas", (), dict(bottom=8, left=1, pad=(1, 2, 3)), 0, (H + 8, W + 1), (0, -1), 2, 1 | 2 << 8 | 3 << 16),
             ("canvas", (), dict(orient="ccw", rect=(-5, 100, 300, 200), pad="edge"), 5, (300, 200), (-5, 100), 0, 0)]
    for name, args, kw, o, new_hw, origin, mode, rgb in cases:
        stub = _Stub()
        s, sel, f = _session(stub, lock, history=2)
        other = s.select_lasso([[(10, 10), (40, 10), (40, 60)]])
        stub.calls.clear()
        lk = s.lock()
        patch, pos, info = getattr(s, name)(*args, selections=[sel, other], **kw)
        want = [("canvas", "frame", HW, new_hw, origin, o, mode, rgb, False)]
        want += [("canvas", "plane", HW, new_hw, origin, o, 2, 0, False)] if lock else []
        want += [("canvas", "plane", HW, new_hw, origin, o, 2, 0, True)] * 2
        assert stub.calls == want, name                                            # nothing else: no upload, no download, no save
        assert patch is None and pos == (0, 0)
        assert s.frame_hw == new_hw and np.array_equal(s.frame(), C.spec_canvas(f, HW, new_hw, origin, o, mode, rgb))
        assert s.locked == lock and (not lock or np.array_equal(s.lock(), C.spec_canvas(lk, HW, new_hw, origin, o, C.CONSTANT, 0)))
        assert info["canvas"] == new_hw and info["previous"] == HW and info["rect"] == origin + new_hw and info["undoable"] is True
        assert info["locked"] == lock and info["orient"] == kw.get("orient", args[0] if name == "orient_canvas" else None)
        for old, new in zip((sel, other), info["selections"]):
            plane = C.spec_canvas(old.plane, HW, new_hw, origin, o, C.CONSTANT, 0)
            assert new is not old and new.frame_hw == new_hw and np.array_equal(new.plane, plane)
            assert (new.box, new.count) == L.box_count(plane)
            assert old.frame_hw == HW                                              # the one handed in stays what it was
        if new_hw != HW:
            with pytest.raises(ValueError):
                s.fill_selection(sel)                                              # ... and is refused as a selection of another size is


def test_a_crop_cuts_a_selection_and_can_empty_it():
    stub = _Stub()
    s, sel, _ = _session(stub)
    _, _, info = s.crop_canvas((210, 320, 100, 100), selections=[sel])
    cut = info["selections"][0]
    assert cut.box == (0, 0, 20, 20) and cut.count == 400 and sel.count == 30 * 40
    s2, sel2, _ = _session(_Stub())
    gone = s2.crop_canvas((0, 0, 100, 100), selections=(sel2,))[2]["selections"][0]
    assert gone.box is None and gone.count == 0 and not gone.plane.any() and gone.frame_hw == (100, 100)


def test_the_journal_holds_the_other_state_whole():
    H, W = HW
    # history 0: nothing is kept
    s, _, f = _session(_Stub(), True)
    info = s.orient_canvas("cw")[2]
    assert info["undoable"] is False and not s.can_undo and s.history_bytes_used == 0
    # history 3: 3 H W of the frame, and H W more with a lock plane
    for lock in (False, True):
        s, _, f = _session(_Stub(), lock, history=3)
        assert s.extend_canvas(left=10)[2]["undoable"] is True
        assert s.history_bytes_used == (4 if lock else 3) * H * W
        assert isinstance(s._undo[-1][0], serve._Canvas) and tuple(s._undo[-1][0]) == HW
        s.undo()
        assert s.history_bytes_used == (4 if lock else 3) * H * (W + 10) and s.frame_hw == HW      # the slot now holds the extended state
    # history_bytes: an entry that fits, and one that does not -- which clears the older entries too
    s, _, f = _session(_Stub(), history=3, history_bytes=3 * H * W + 10 ** 5)
    s.fill(_mask())
    assert len(s._undo) == 1
    assert s.crop_canvas((0, 0, 200, 200))[2]["undoable"] is True and len(s._undo) == 1       # the oldest entry went: over the cap
    assert isinstance(s._undo[0][0], serve._Canvas)
    s, _, f = _session(_Stub(), history=3, history_bytes=3 * H * W - 1)
    s.fill(_mask())
    s.fill(_mask())
    s.undo()
    assert s.can_undo and s.can_redo
    before = s.frame()
    info = s.orient_canvas("180")[2]
    assert info["undoable"] is False and not s.can_undo and not s.can_redo and s.history_bytes_used == 0
    assert np.array_equal(s.frame(), before[::-1, ::-1]) and s.frame_hw == HW
    # a lock plane that makes the entry too large
    s, _, f = _session(_Stub(), True, history=3, history_bytes=3 * H * W)
    s.fill(_mask())
    assert s.orient_canvas("v")[2]["undoable"] is False and not s.can_undo


def test_undo_and_redo_through_edit_canvas_edit():
    stub = _Stub()
    s, sel, f0 = _session(stub, True, history=4)
    lock0 = s.lock()
    s.fill(_mask())
    f1 = s.frame()
    s.canvas(orient="cw", rect=(-4, 10, 300, 260), pad=(9, 8, 7))
    f2, lock2 = s.frame(), s.lock()
    assert f2.shape == (300, 260, 3) and lock2.shape == (300, 260)
    s.fill(_mask((300, 260)))
    f3 = s.frame()
    assert not np.array_equal(f3, f2) and not np.array_equal(f1, f0)
    stub.calls.clear()
    assert s.undo()[2]["undo_depth"] == 2 and np.array_equal(s.frame(), f2)
    stub.calls.clear()
    got = s.undo()                                                                 # the canvas step: a pointer exchange
    assert stub.calls == [] and got == (None, (0, 0), dict(canvas=HW, undo_depth=1, redo_depth=2))
    assert s.frame_hw == HW and np.array_equal(s.frame(), f1) and np.array_equal(s.lock(), lock0)
    s.undo()                                                                       # the older entry is valid again
    assert np.array_equal(s.frame(), f0) and not s.can_undo
    s.redo()
    assert np.array_equal(s.frame(), f1)
    stub.calls.clear()
    got = s.redo()
    assert stub.calls == [] and got == (None, (0, 0), dict(canvas=(300, 260), undo_depth=2, redo_depth=1))
    assert s.frame_hw == (300, 260) and np.array_equal(s.frame(), f2) and np.array_equal(s.lock(), lock2)
    s.redo()
    assert np.array_equal(s.frame(), f3) and not s.can_redo
    with pytest.raises(IndexError):
        s.redo()


def test_set_lock_after_a_canvas_step_then_undo():
    """the one place where undo touches the lock: each geometry keeps the lock plane it had"""
    s, _, _ = _session(_Stub(), True, history=2)
    lock0 = s.lock()
    s.orient_canvas("ccw")
    turned = s.lock()
    assert np.array_equal(turned, np.rot90(lock0))
    s.set_lock(None)
    assert not s.locked
    s.undo()
    assert s.locked and np.array_equal(s.lock(), lock0)
    s.redo()
    assert not s.locked and s.frame_hw == (HW[1], HW[0])                           # what set_lock left on that geometry
    s.undo()
    new = np.zeros(HW, np.uint8)
    new[:5] = 255
    s.set_lock(new)
    s.redo()
    s.undo()
    assert np.array_equal(s.lock(), new)


@pytest.mark.parametrize("lock,max_side,feather,encode", [(False, None, None, None), (True, 128, 3, "png"), (True, None, None, ("jpg", 80))])
def test_the_outpaint_is_extend_then_fill_in_one_entry(lock, max_side, feather, encode):
    H, W = HW
    stub = _Stub()
    s, sel, f = _session(stub, lock, history=3)
    s.fill(_mask())
    stub.calls.clear()
    patch, pos, info = s.extend_canvas(right=40, bottom=3, pad="reflect", fill="network", max_side=max_side, feather=feather, encode=encode,
                                       selections=[sel])
    new_hw = (H + 3, W + 40)
    win = serve.choose_window((0, 0) + new_hw, new_hw, margin=0.5)
    want = ["canvas"] * (3 if lock else 2) + ["canvas", "fill_keep", "run_fill", "paste_feather" if feather else "paste_locked",
                                              "crop" if encode is None else "crop_" + (encode if isinstance(encode, str) else encode[0])]
    assert _names(stub) == want                                                    # no save: the entry holds the old frame
    assert _canvas_calls(stub)[-1] == ("canvas", "none", HW, new_hw, (0, 0), 0, 2, 255, False)
    assert "upload" not in [c[0] for c in stub.calls]                              # nothing frame-sized goes up
    assert pos == (win[1], win[0]) and info["window"] == win and info["fill"] is True and info["canvas"] == new_hw and info["undoable"] is True
    assert info.get("work") == (None if max_side is None else serve.choose_working_size(win[2:], max_side)) and info.get("feather") == feather
    assert info["locked"] == lock and info["selections"][0].frame_hw == new_hw
    assert len(s._undo) == 2 and isinstance(s._undo[-1][0], serve._Canvas)         # ONE entry
    # against the definition: a twin that extends, then fills the plane of the new area
    twin_stub = _Stub()
    t, _, _ = _session(twin_stub, lock, history=3)
    t.fill(_mask())
    t.extend_canvas(right=40, bottom=3, pad="reflect")
    area = np.zeros(new_hw, np.uint8)
    area[H:] = 255
    area[:, W:] = 255
    t.fill(area, max_side=max_side, feather=feather)
    assert np.array_equal(s.frame(), t.frame())
    if encode is None:
        assert np.array_equal(patch, t.frame()[win[0]:win[0] + win[2], win[1]:win[1] + win[3]])
    else:
        assert patch == (b"png" if encode == "png" else b"jpg")
    before = t.frame()
    s.undo()
    assert s.frame_hw == HW and len(s._undo) == 1
    s.redo()
    assert np.array_equal(s.frame(), before)


def test_an_outpaint_that_fails_leaves_the_session_as_it_was():
    class _NoFill(_Stub):
        def run_fill(self, *a, **k):
            raise RuntimeError("the device said no")
    s, _, f = _session(_NoFill(), True, history=2)
    lock = s.lock()
    with pytest.raises(RuntimeError):
        s.extend_canvas(top=16, fill="network")
    assert s.frame_hw == HW and np.array_equal(s.frame(), f) and np.array_equal(s.lock(), lock) and not s.can_undo


def test_server_undo_and_redo_take_a_canvas_step():
    stub = _Stub()
    srv = serve.BatchingServer(object(), max_batch=4, max_wait_s=0.01, window=True, max_grow=0)
    try:
        s = serve.EditSession(srv.model, U._noise(HW, 5), backend=stub, history=4)
        f = s.frame()
        s.orient_canvas("transpose")
        after = s.frame()
        stub.calls.clear()
        assert srv.undo(s) == (None, (0, 0), dict(canvas=HW, undo_depth=0, redo_depth=1)) and stub.calls == []
        assert np.array_equal(s.frame(), f)
        assert srv.redo(s) == (None, (0, 0), dict(canvas=(HW[1], HW[0]), undo_depth=1, redo_depth=0)) and np.array_equal(s.frame(), after)
        # a mixed group: a canvas entry beside a plain one and a session with nothing to undo
        other = serve.EditSession(srv.model, U._noise(HW, 6), backend=stub, history=2)
        before = other.frame()
        other.fill(_mask())
        empty = serve.EditSession(srv.model, U._noise(HW, 7), backend=stub, history=2)
        group = [(("history",), dict(session=x, op="undo"), None, {}) for x in (s, other, empty)]
        outs = srv._run_history(group)
        assert outs[0][2]["canvas"] == HW and "window" in outs[1][2] and outs[2] is False and isinstance(group[2][3]["err"], IndexError)
        assert np.array_equal(s.frame(), f) and np.array_equal(other.frame(), before)
    finally:
        srv.close()


def test_refusals_make_no_backend_call():
    stub = _Stub()
    s, sel, f = _session(stub, True, history=2)
    small = serve.EditSession(None, U._noise((64, 64), 1), backend=_Stub())
    foreign = small.select_lasso([[(1, 1), (30, 1), (30, 30)]])
    bad = [lambda: s.canvas(orient="left"), lambda: s.canvas(rect=(0, 0, 8, 100)), lambda: s.canvas(pad="wrap"), lambda: s.canvas(rect=(0, 0, 100)),
           lambda: s.canvas(selections=[foreign]), lambda: s.crop_canvas((-1, 0, 100, 100)), lambda: s.crop_canvas((0, 0, HW[0] + 1, 100)),
           lambda: s.crop_canvas((0, 500, 100, 101)), lambda: s.extend_canvas(), lambda: s.extend_canvas(top=-1), lambda: s.extend_canvas(top=1.5),
           lambda: s.extend_canvas(top=4, fill="magic"), lambda: s.extend_canvas(top=4, fill="network", feather=99),
           lambda: s.extend_canvas(top=4, fill="network", encode="gif"), lambda: s.extend_canvas(top=4, fill="network", window=(0, 0, 17, 64)),
           lambda: s.extend_canvas(top=4, fill="network", window=(0, 0, 64, 4096)), lambda: s.extend_canvas(top=4, fill="network", max_side=3),
           lambda: s.extend_canvas(top=1 << 16), lambda: s.orient_canvas(None), lambda: s.orient_canvas("upside")]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
        assert stub.calls == [], k
    for call in (lambda: s.canvas(selections=[sel.plane]), lambda: s.canvas(selections=5)):
        with pytest.raises(TypeError):
            call()
    assert stub.calls == [] and s.frame_hw == HW and np.array_equal(s.frame(), f) and not s.can_undo
    old = serve.EditSession(None, f, backend=_MoveStub())                           # a backend from before 6y
    with pytest.raises(NotImplementedError):
        old.orient_canvas("cw")


def test_a_session_without_a_canvas_call_issues_what_it_issued():
    """the same calls with the same arguments on backends with and without `canvas`"""
    logs = []
    for stub in (_Stub(), _MoveStub()):
        f = U._noise(HW, 5)
        s = serve.EditSession(None, f, backend=stub, history=2)
        s.set_lock(_lock_array())
        sel = s.select_lasso([RING])
        stub.calls.clear()
        s.move_selection(sel, OFF, flip="v", feather=3)
        s.fill(_mask())
        s.undo()
        s.undo()
        s.redo()
        logs.append(([c for c in stub.calls if c[0] not in ("move_drop", "shift", "grow", "paste_locked", "paste_feather")], _names(stub), s.frame()))
    assert logs[0][0] == logs[1][0] and logs[0][1] == logs[1][1] and np.array_equal(logs[0][2], logs[1][2])
    assert logs[0][1][:11] == ["save", "grow", "fill_keep", "run_fill", "save", "paste_feather", "save", "move_drop", "shift", "crop", "crop"]
    assert "canvas" not in logs[0][1] and logs[0][1].count("swap") == 5
    assert BOX == (200, 300, 230, 340)


# ---- the kernels' arithmetic, tile by tile -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", C.SIZES, ids=lambda hw: "%dx%d" % hw)
def test_tiled_turn_is_the_statement_with_one_writer_per_byte(hw):
    rng = np.random.RandomState(hw[0])
    imgs = {1: rng.randint(0, 256, hw).astype(np.uint8), 3: rng.randint(0, 256, hw + (3,)).astype(np.uint8)}
    oriented = (hw[1], hw[0])
    routes = set()
    k = 0
    for (y0, x0, h, w) in C.rects(oriented):
        if h * w > 40000:                                                          # the statement is tiled in Python: keep it quick
            h, w = min(h, 150), min(w, 260)
        for ch in (1, 3):
            o, mode = 4 + k % 4, k % 3
            rgb = 0x0a141e if ch == 3 else 0x5a
            out, writers, lds = C.tiled_turn(imgs[ch], hw, (h, w), (y0, x0), o, mode, rgb, misalign=k % 4)
            assert np.array_equal(out, C.spec_canvas(imgs[ch], hw, (h, w), (y0, x0), o, mode, rgb)), (hw, (y0, x0, h, w), o, mode, ch)
            assert (writers == 1).all()
            routes |= set(lds.reshape(-1).tolist())
            k += 1
    out, writers, lds = C.tiled_turn(None, hw, (9, 70), (-2, -3), 5, C.CONSTANT, 255, misalign=3)      # the NULL-input plane form
    assert np.array_equal(out, C.spec_canvas(None, hw, (9, 70), (-2, -3), 5, C.CONSTANT, 255)) and (writers == 1).all() and not lds.any()
    if hw in ((130, 70), (200, 150)):
        assert routes == {True, False}                                             # both routes occur


@pytest.mark.parametrize("hw", [(1, 70), (70, 1), (3, 5), (16, 16), (37, 53), (65, 129)], ids=lambda hw: "%dx%d" % hw)
def test_tiled_map_is_the_statement_and_stays_inside_the_two_arrays(hw):
    """se_canvas.hip's walk of the output's aligned dwords, its source bytes through dword loads bounded by the source row and its
    pixel-wise x mirror, on one flat byte array in which only the output's bytes may change"""
    import move_util as M
    rng = np.random.RandomState(hw[1])
    imgs = {1: rng.randint(0, 256, hw).astype(np.uint8), 3: rng.randint(0, 256, hw + (3,)).astype(np.uint8)}
    k = fast = 0
    for (y0, x0, h, w) in C.rects(hw):
        if h * w > 20000:
            h, w = min(h, 100), min(w, 200)
        for ch in (1, 3):
            for o in range(4):
                mode = (k + o) % 3
                rgb = 0x0a141e if ch == 3 else 0x5a
                mem = M.Memory(4096 + ch * hw[0] * hw[1] + 2048 + ch * h * w + 2048)
                ia = mem.put(1024 + 1 + k % 4, imgs[ch])                          # the input at odd offsets
                oa = ia + ch * hw[0] * hw[1] + 1024 + (k + o) % 4                  # the output at every offset mod 4
                clean = mem.mem.copy()
                fast += C.tiled_map(mem, ia, hw, ch, oa, (h, w), (y0, x0), o, mode, rgb)
                want = C.spec_canvas(imgs[ch], hw, (h, w), (y0, x0), o, mode, rgb)
                assert np.array_equal(mem.get(oa, want.shape), want), (hw, (y0, x0, h, w), ch, o, mode)
                changed = np.flatnonzero(mem.mem != clean)
                assert changed.size == 0 or (oa <= changed.min() and changed.max() < oa + want.size)
            k += 1
    assert fast > 0
    mem = M.Memory(8192)
    C.tiled_map(mem, None, hw, 1, 1027, (9, 70), (-2, -3), 3, C.CONSTANT, 255)     # the NULL-input plane form
    assert np.array_equal(mem.get(1027, (9, 70)), C.spec_canvas(None, hw, (9, 70), (-2, -3), 3, C.CONSTANT, 255))


@pytest.mark.parametrize("hw", [(130, 70), (200, 150)], ids=lambda hw: "%dx%d" % hw)
def test_both_routes_of_the_turn_occur_at_the_large_sizes(hw):
    oriented = (hw[1], hw[0])
    seen = set()
    for (y0, x0, h, w) in C.rects(oriented):
        seen |= set(C.turn_routes(hw, (h, w), (y0, x0), 6).reshape(-1).tolist())
    assert seen == {True, False}
    assert C.turn_routes(hw, oriented, (0, 0), 6).all()                            # the identity rectangle: every tile is interior
    mixed = C.turn_routes(hw, (oriented[0] + 2, oriented[1] + 2), (-1, -1), 5)
    assert not mixed.all() and (hw != (200, 150) or mixed.any())                   # an extension by 1: the rim's tiles gather


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_abi_has_one_new_entry_in_a_header_of_its_own():
    hdr = open(os.path.join(ROOT, "include", "sketchedit_canvas.h")).read()
    decl = re.search(r"^int\s+(\w+)\((.*?)\);", hdr, re.M | re.S)
    assert [decl.group(1)] == _lib.abi_names("sketchedit_canvas.h") == ["se_canvas_u8"] == re.findall(r"^(?:int|size_t)\s+(\w+)\(", hdr, re.M)
    args = [" ".join(a.split()) for a in decl.group(2).split(",")]
    assert args == ["se_ctx* ctx", "void* stream", "const unsigned char* in_or_NULL", "int Hi", "int Wi", "int C", "unsigned char* out", "int Hn", "int Wn",
                    "int oy", "int ox", "int orient", "int pad_mode", "unsigned pad_rgb"]
    name = decl.group(1)
    assert "move_blend" not in hdr and [n for n in _lib.abi_names() if "canvas" in n] == [name]
    i = _lib.SOURCES.index("se_blend.hip")
    assert _lib.SOURCES[i - 1] == "se_move.hip" and "se_canvas.hip" in _lib.SOURCES and _lib.SOURCES[-1] == "se_api.hip"
    for macro, value in (("MIRROR_X", 1), ("MIRROR_Y", 2), ("TRANSPOSE", 4), ("EDGE", 0), ("REFLECT", 1), ("CONSTANT", 2), ("MAX_SIDE", 32768),
                         ("MAX_OFFSET", 1048576)):
        assert re.search(r"#define SE_CANVAS_%s %d\b" % (macro, value), hdr), macro
    import ctypes
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    getattr(lib, name)
    from sketchedit_amd import kernel_labels
    assert kernel_labels.label_of("void se::canvas_map_kernel(se::CanvasMap, unsigned char*, int, long, long)") == "canvas_map"
    assert kernel_labels.label_of("canvas_turn_kernel(CanvasMap, unsigned char*, int, int)") == "canvas_turn"
    names, labels = abi_util.prof_labels()
    assert len(names) == len(labels) - 1 and labels[-1] == "PL_COUNT"
    i = names.index("canvas_map")
    assert names[i - 1:i + 3] == ["blend_apply", "canvas_map", "canvas_turn", "select_similar"]        # behind the blend, not appended
    assert labels[i - 1:i + 3] == ["PL_BLEND_APPLY", "PL_CANVAS_MAP", "PL_CANVAS_TURN", "PL_SELECT_SIMILAR"]
    src = open(os.path.join(_lib.CSRC, "se_canvas.hip")).read()
    assert "atomic" not in src.replace("no atomics", "") and "while" not in src and "float" not in src and "double" not in src.replace("(double)", "")
    assert "TURN_PITCH = 65" in src and C.TURN_W == 32 and C.TURN_H == 64 and "TURN_W = 32, TURN_H = 64" in src
    from sketchedit_amd.models.editline2_model import EditLine2Model
    assert callable(_lib.Engine.canvas_u8) and callable(EditLine2Model.canvas_u8) and callable(serve._ModelBackend.canvas)


def test_model_backend_canvas_forwards_and_takes_the_tiles():
    class _Model:
        def __init__(self):
            self.calls = []

        def engine(self):
            return self

        edit_window_u8 = None

        def canvas_u8(self, src, out_hw, origin=(0, 0), orient=0, pad=0, pad_rgb=0, src_hw=None):
            self.calls.append(("canvas_u8", None if src is None else src.shape, tuple(out_hw), tuple(origin), orient, pad, pad_rgb, tuple(src_hw)))
            return C.spec_canvas(src, tuple(src_hw), tuple(out_hw), tuple(origin), orient, pad, pad_rgb)

        def sketch_tiles_u8(self, plane, tile):
            self.calls.append(("sketch_tiles_u8", tile))

            class _T:
                def cpu(self):
                    return self

                def numpy(self):
                    ys, xs = np.nonzero(plane)
                    return np.array([[ys.size, ys.min(), xs.min(), ys.max() + 1, xs.max() + 1]] if ys.size else np.zeros((0, 5)), np.int64)
            return _T()
    be = serve._ModelBackend.__new__(serve._ModelBackend)
    be.model = _Model()
    plane = np.zeros((20, 30), np.uint8)
    plane[3:6, 4:9] = 255
    out = be.canvas(plane, (20, 30), (30, 20), (0, 0), 6, 2, 0)
    assert np.array_equal(out, np.rot90(plane, -1)) and be.model.calls == [("canvas_u8", (20, 30), (30, 20), (0, 0), 6, 2, 0, (20, 30))]
    out, box, count = be.canvas(plane, (20, 30), (30, 20), (0, 0), 6, 2, 0, tiles=True)
    assert box == (4, 14, 9, 17) and count == 15 and be.model.calls[-1] == ("sketch_tiles_u8", 32)
    area = be.canvas(None, (20, 30), (22, 30), (-2, 0), 0, 2, 255)
    assert be.model.calls[-1][1] is None and (area[:2] == 255).all() and not area[2:].any()
