"""Host tests of scaling and rotating a selection: the statement's known answers and its ties to the move of 6r,
serve.warp_matrix and serve.warp_rect against their restatement, EditSession.transform_selection against a scripted backend
that logs every call and really edits a numpy frame, se_warp.hip's arithmetic lane by lane on checked memory, and the new
entries' place in the C-ABI.  CPU only; every comparison is exact."""
import os
import re

import numpy as np
import pytest

from sketchedit_amd import _lib, serve
import lasso_util as L
import move_util as M
import select_util as U
import warp_util as W
from test_fill_host import _names
from test_move_host import BOX, HW, RING, _Stub as _MoveStub, _lock_array

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ID = 65536


# ---- the statement ----------------------------------------------------------------------------------------------------------------------
def _known():
    frame = np.full((16, 16, 3), 10, np.uint8)
    lift = M.slot_of(np.full((16, 16, 3), 200, np.uint8), (0, 0, 16, 16))
    sel = np.zeros((16, 16), np.uint8)
    sel[2:4, 2:4] = 1
    return frame, lift, sel, (2, 2, 4, 4), (0, 0, 16, 16)


def test_known_answers_of_the_header():
    hdr = open(os.path.join(ROOT, "include", "sketchedit_warp.h")).read()
    assert "105, 200, 105" in hdr and "58 105 58 / 105 200 105 / 58 105 58" in hdr
    frame, lift, sel, box, rect = _known()
    m = (ID, 0, 0, 0, ID, -32768)
    want = frame.copy()
    want[2:4, 2:5] = np.array([105, 200, 105], np.uint8)[None, :, None]
    assert np.array_equal(W.spec_drop(frame, lift, rect, sel, None, box, rect, m), want)
    plane = np.zeros((16, 16), np.uint8)
    plane[2:4, 2:5] = 255
    assert np.array_equal(W.spec_warp(sel, box, m), plane)
    m = (ID, 0, -32768, 0, ID, -32768)
    want = frame.copy()
    want[2:5, 2:5] = np.array([[58, 105, 58], [105, 200, 105], [58, 105, 58]], np.uint8)[..., None]
    assert np.array_equal(W.spec_drop(frame, lift, rect, sel, None, box, rect, m), want)
    plane = np.zeros((16, 16), np.uint8)
    plane[3, 2:5] = plane[2:5, 3] = 255
    assert np.array_equal(W.spec_warp(sel, box, m), plane)


def _random_case(seed, hw=(37, 53), box=(5, 7, 29, 40)):
    rng = np.random.RandomState(seed)
    Hi, Wi = hw
    frame = rng.randint(0, 256, (Hi, Wi, 3)).astype(np.uint8)
    before = rng.randint(0, 256, (Hi, Wi, 3)).astype(np.uint8)
    sel = np.where(rng.rand(Hi, Wi) < 0.6, rng.randint(1, 256, (Hi, Wi)), 0).astype(np.uint8)
    lock = np.where(rng.rand(Hi, Wi) < 0.2, 255, 0).astype(np.uint8)
    rect = M.move_rect(box, (0, 0), hw)
    return frame, before, M.slot_of(before, rect), rect, sel, lock, box


@pytest.mark.parametrize("flip", [None, "h", "v", "hv"])
def test_identity_scale_and_integer_offset_is_the_move(flip):
    """scale 1, angle 0, an integer offset: the drop is 6r's at r = 0 byte for byte and the plane is 6r's shift -- also where the
    object is pushed over each edge of the frame and over a corner"""
    frame, before, lift, rect, sel, lock, box = _random_case(3)
    bits = serve.MOVE_FLIPS[flip]
    whole = (0, 0, 37, 53)
    for off in ((0, 0), (3, -4), (-9, 6), (-20, 0), (25, 2), (1, -30), (0, 35), (-18, -25), (40, 0)):
        m = serve.warp_matrix(box, 1.0, 0.0, off, flip)
        assert m == W.warp_matrix(box, 1.0, 0.0, off, bits) and (m[0], m[1], m[3], m[4]) == (-ID if bits & 2 else ID, 0, 0, -ID if bits & 1 else ID)
        for lk in (None, lock):
            got = W.spec_drop(frame, lift, rect, sel, lk, box, whole, m)
            assert np.array_equal(got, M.spec_drop(frame, lift, rect, sel, lk, box, off, bits, 0)), (flip, off)
        assert np.array_equal(W.spec_warp(sel, box, m), M.spec_shift(sel, box, off, bits)), (flip, off)
        # the rectangle warp_rect gives holds move_rect's: the taps reach one pixel past the box
        wr, mr = serve.warp_rect(box, m, (37, 53)), M.move_rect(box, off, (37, 53))
        if mr is not None:
            assert wr[0] <= mr[0] and wr[1] <= mr[1] and wr[0] + wr[2] >= mr[0] + mr[2] and wr[1] + wr[3] >= mr[1] + mr[3]
            assert np.array_equal(W.spec_drop(frame, lift, rect, sel, None, box, wr, m), M.spec_drop(frame, lift, rect, sel, None, box, off, bits, 0))


@pytest.mark.parametrize("angle", [90, 180, 270, -90])
def test_a_quarter_turn_of_a_box_of_like_parity_is_a_permutation(angle):
    """sides of like parity: every source position is a pixel centre, a is 0 or 65 536, and the drop is np.rot90 of the masked
    object about the box's centre"""
    hw = (48, 50)
    for box in ((10, 12, 30, 36), (11, 12, 30, 35)):                                     # 20 x 24 and 19 x 23
        frame, before, lift, rect, sel, lock, box = _random_case(angle % 7, hw, box)
        m = serve.warp_matrix(box, 1.0, angle)
        a = W.coverage(sel, box, m)
        assert set(np.unique(a)) == {0, ID}
        k = (angle // 90) % 4
        inside = np.zeros(hw, bool)
        inside[box[0]:box[2], box[1]:box[3]] = sel[box[0]:box[2], box[1]:box[3]] != 0
        obj = np.rot90(np.where(inside[..., None], before, 0)[box[0]:box[2], box[1]:box[3]], k)
        msk = np.rot90(inside[box[0]:box[2], box[1]:box[3]], k)
        h, w = msk.shape
        y0, x0 = (box[0] + box[2] - h) // 2, (box[1] + box[3] - w) // 2
        want = frame.copy()
        want[y0:y0 + h, x0:x0 + w][msk] = obj[msk]
        got = W.spec_drop(frame, lift, rect, sel, None, box, (0, 0) + hw, m)
        assert np.array_equal(got, want) and not np.array_equal(got, frame)
        plane = np.zeros(hw, np.uint8)
        plane[y0:y0 + h, x0:x0 + w][msk] = 255
        assert np.array_equal(W.spec_warp(sel, box, m), plane)


def test_nothing_outside_the_rectangle_the_lock_or_the_coverage_changes():
    frame, before, lift, rect, sel, lock, box = _random_case(8)
    for m, R in ((serve.warp_matrix(box, 1.5, 30.0, (2, -3)), (4, 6, 20, 30)), (serve.warp_matrix(box, (0.5, 2.0), 45.0, (0.5, 0)), (0, 0, 37, 53)),
                 ((70000, 9000, -200000, -12000, 50000, 300000), (10, 0, 27, 16))):
        a = W.coverage(sel, box, m)
        assert ((a > 0) & (a < ID)).any() and (a == 0).any()
        inr = np.zeros(sel.shape, bool)
        inr[R[0]:R[0] + R[2], R[1]:R[1] + R[3]] = True
        for lk in (None, lock):
            got = W.spec_drop(frame, lift, rect, sel, lk, box, R, m)
            may = inr & (a > 0) & (True if lk is None else lk == 0)
            assert not (got != frame).any(axis=2)[~may].any() and (got != frame).any()
    # an unselected neighbour's colour never bleeds in: the result does not depend on the lift's bytes of unselected pixels
    m = serve.warp_matrix(box, 1.3, 20.0)
    other = before.copy()
    other[sel == 0] ^= 0x5A
    assert np.array_equal(W.spec_drop(frame, lift, rect, sel, None, box, (0, 0, 37, 53), m),
                          W.spec_drop(frame, M.slot_of(other, rect), rect, sel, None, box, (0, 0, 37, 53), m))


# ---- warp_matrix ------------------------------------------------------------------------------------------------------------------------
def test_warp_matrix_exact_values():
    box = (10, 20, 30, 50)                                               # cy2 = 39, cx2 = 69: sides of like parity (20, 30)
    assert serve.warp_matrix(box) == (ID, 0, 0, 0, ID, 0)
    assert serve.warp_matrix(box, angle=90) == (0, ID, (39 - 69) * 32768, -ID, 0, (69 + 39) * 32768)
    assert serve.warp_matrix(box, angle=180) == (-ID, 0, 39 * ID, 0, -ID, 69 * ID)
    assert serve.warp_matrix(box, angle=270) == (0, -ID, (39 + 69) * 32768, ID, 0, (69 - 39) * 32768)
    assert serve.warp_matrix(box, angle=-90) == serve.warp_matrix(box, angle=270) == serve.warp_matrix(box, angle=630.0)
    assert serve.warp_matrix(box, angle=360) == serve.warp_matrix(box)
    assert serve.warp_matrix(box, scale=2) == (32768, 0, 39 * 16384, 0, 32768, 69 * 16384)
    assert serve.warp_matrix(box, scale=(0.5, 4.0), flip="h") == (2 * ID, 0, -39 * 32768, 0, -16384, (69 * ID + 16384 * 69) >> 1)
    assert serve.warp_matrix(box, offset=(3, -4), flip="v") == (-ID, 0, (39 + 3) * ID, 0, ID, 4 * ID)
    # the half pixel: offsets are quantised to halves, and a half cancels what a quarter turn of unlike parity leaves
    assert serve.warp_matrix(box, offset=(0.5, -1.5)) == (ID, 0, -32768, 0, ID, 3 * 32768)
    assert serve.warp_matrix(box, offset=(0.26, 0.24)) == (ID, 0, -32768, 0, ID, 0)
    odd = (10, 20, 30, 51)                                               # 20 x 31
    m = serve.warp_matrix(odd, angle=90)
    assert m[2] % ID == 32768 and m[5] % ID == 32768
    m = serve.warp_matrix(odd, angle=90, offset=(0.5, 0.5))
    assert m[2] % ID == 0 and m[5] % ID == 0
    sel = np.zeros((64, 80), np.uint8)
    sel[10:30, 20:51] = 255
    assert set(np.unique(W.coverage(sel, odd, m))) == {0, ID}
    # 30 degrees: round(float64 * 65536)
    m = serve.warp_matrix(box, scale=1.5, angle=30.0)
    assert (m[0], m[1], m[3], m[4]) == (37837, 21845, -21845, 37837)
    rng = np.random.RandomState(2)
    for _ in range(300):
        b = (int(rng.randint(0, 40)), int(rng.randint(0, 40)))
        b += (b[0] + int(rng.randint(1, 40)), b[1] + int(rng.randint(1, 40)))
        sc = (float(rng.uniform(0.125, 8)), float(rng.uniform(0.125, 8)))
        ang, off, fl = float(rng.uniform(-400, 400)), (float(rng.uniform(-50, 50)), int(rng.randint(-50, 50))), [None, "h", "v", "hv"][rng.randint(4)]
        m = serve.warp_matrix(b, sc, ang, off, fl)
        assert m == W.warp_matrix(b, sc, ang, off, serve.MOVE_FLIPS[fl]) and all(isinstance(v, int) for v in m)
        assert max(abs(m[0]), abs(m[1]), abs(m[3]), abs(m[4])) <= 8 * ID <= W.MAX_COEF and max(abs(m[2]), abs(m[5])) <= W.MAX_TRANSLATION
    for bad in (dict(scale=0.1), dict(scale=8.5), dict(scale=(1, 2, 3)), dict(scale="2"), dict(scale=(1.0, 0.0)), dict(scale=float("nan")),
                dict(angle="90"), dict(angle=float("inf")), dict(angle=True), dict(offset=5), dict(offset=(1, 2, 3)), dict(offset=(1, "2")),
                dict(offset=(16385, 0)), dict(flip="x"), dict(flip=1)):
        with pytest.raises(ValueError):
            serve.warp_matrix(box, **bad)
    with pytest.raises(ValueError):
        serve.warp_matrix((10, 20, 10, 50))
    assert (serve.WARP_MAX_COEF, _lib.WARP_MAX_COEF, W.MAX_COEF) == (1 << 20,) * 3
    assert (serve.WARP_MAX_TRANSLATION, _lib.WARP_MAX_TRANSLATION, W.MAX_TRANSLATION) == (1 << 40,) * 3
    assert "undersample" in serve.warp_matrix.__doc__ and "undersample" in serve.EditSession.transform_selection.__doc__


# ---- warp_rect --------------------------------------------------------------------------------------------------------------------------
def test_warp_rect_holds_every_covered_pixel_on_random_maps():
    """no pixel outside the rectangle has a > 0: the drop over the rectangle is the drop over the frame"""
    rng = np.random.RandomState(11)
    hw = (37, 53)
    none = partial = maps = 0
    for k in range(1500):
        y0, x0 = int(rng.randint(0, 30)), int(rng.randint(0, 45))
        box = (y0, x0, int(rng.randint(y0 + 1, 38)), int(rng.randint(x0 + 1, 54)))
        sc = (float(2 ** rng.uniform(-3, 3)), float(2 ** rng.uniform(-3, 3)))
        off = (float(rng.uniform(-30, 30)), float(rng.uniform(-40, 40)))
        m = serve.warp_matrix(box, sc, float(rng.uniform(0, 360)), off, [None, "h", "v", "hv"][rng.randint(4)])
        if k % 5 == 0:                                                   # a raw map: sheared, up to the coefficient limit
            m = tuple(int(v) for v in rng.randint(-W.MAX_COEF, W.MAX_COEF + 1, 2)) + (int(rng.randint(-40, 80)) << 15,) + \
                tuple(int(v) for v in rng.randint(-3 * ID, 3 * ID + 1, 2)) + (int(rng.randint(-40, 80)) << 15,)
            if m[0] * m[4] - m[1] * m[3] == 0:
                continue
        maps += 1
        sel = np.ones(hw, np.uint8)
        a = W.coverage(sel, box, m)
        R = serve.warp_rect(box, m, hw)
        assert R == W.warp_rect(box, m, hw), (box, m)
        if R is None:
            none += 1
            assert not a.any(), (box, m)
            continue
        assert 0 <= R[0] and 0 <= R[1] and R[2] >= 16 and R[3] >= 16 and R[0] + R[2] <= 37 and R[1] + R[3] <= 53
        out = np.ones(hw, bool)
        out[R[0]:R[0] + R[2], R[1]:R[1] + R[3]] = False
        assert not a[out].any(), (box, m, R)
        partial += int(((a > 0) & (a < ID)).any())
    assert maps >= 1000 and none > 20 and partial > 800, (maps, none, partial)


def test_warp_rect_corners():
    hw = (100, 200)
    box = (10, 20, 50, 70)
    ident = lambda dy, dx: serve.warp_matrix(box, offset=(dy, dx))      # noqa: E731
    cases = {(0, 0): (9, 19, 42, 52), (5, -7): (14, 12, 42, 52), (-30, 0): (0, 19, 21, 52), (70, 0): (79, 19, 21, 52),
             (0, -40): (9, 0, 42, 31), (0, 150): (9, 169, 42, 31),
             (-45, 0): (0, 19, 16, 52),                                 # 6 rows left at the top edge: widened downwards
             (85, 0): (84, 19, 16, 52), (0, -66): (9, 0, 42, 16), (0, 178): (9, 184, 42, 16),
             (-51, 0): None, (91, 0): None, (0, -71): None, (0, 181): None,
             (-50, 0): (0, 19, 16, 52)}                                 # the tap row past the box's last row still reaches row 0
    for off, want in cases.items():
        assert serve.warp_rect(box, ident(*off), hw) == want == W.warp_rect(box, ident(*off), hw), off
    small = (40, 60, 44, 70)
    assert serve.warp_rect(small, serve.warp_matrix(small), hw) == (34, 57, 16, 16)          # 6 x 12 -> 16 x 16 around it
    assert serve.warp_rect(small, serve.warp_matrix(small, scale=2), hw) == W.warp_rect(small, serve.warp_matrix(small, scale=2), hw) == (34, 53, 16, 24)
    assert serve.warp_rect(box, serve.warp_matrix(box, scale=8), hw) == (0, 0, 100, 200)     # clipped on every side
    for m in ((0, 0, 0, 0, 0, 0), (ID, ID, 0, ID, ID, 0), (3, 6, 5, 1, 2, 9)):
        with pytest.raises(ValueError, match="singular"):
            serve.warp_rect(box, m, hw)


# ---- the sessions against a scripted backend -------------------------------------------------------------------------------------------------
class _Stub(_MoveStub):
    """... with the two calls of DESIGN.md 6s, which are the statement"""

    def warp_drop(self, frame, lift, lift_rect, plane, lock, box, rect, m):
        self.calls.append(("warp_drop", tuple(lift_rect), id(plane), None if lock is None else id(lock), tuple(box), tuple(rect), tuple(m)))
        self.lift = lift.copy()
        frame[...] = W.spec_drop(frame, lift, lift_rect, plane, lock, box, rect, m)

    def warp(self, plane, box, m):
        self.calls.append(("warp", id(plane), tuple(box), tuple(m)))
        out = W.spec_warp(plane, box, m)
        return (out,) + L.box_count(out)


def _session(stub, lock=False, **kw):
    f = U._noise(HW, 5)
    s = serve.EditSession(None, f, backend=stub, **kw)
    if lock:
        s.set_lock(_lock_array())
    sel = s.select_lasso([RING])
    stub.calls.clear()
    return s, sel, f


def _expect(f, sel, lock, m, hole_grow, win, keep_source):
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
    return W.spec_drop(after, M.slot_of(f, rect), rect, sel, lock, BOX, (0, 0) + HW, m)


ARGS = dict(scale=1.5, angle=30.0, offset=(10, 25.5), flip="h")          # the destination overlaps the source


@pytest.mark.parametrize("keep_source", [False, True])
@pytest.mark.parametrize("lock", [False, True])
@pytest.mark.parametrize("history", [0, 2])
@pytest.mark.parametrize("max_side", [None, 128])
@pytest.mark.parametrize("feather", [None, 4])
def test_transform_issues_lift_fill_save_drop_warp_in_that_order(keep_source, lock, history, max_side, feather):
    stub = _Stub()
    s, sel, f = _session(stub, lock, history=history)
    plane0 = sel.plane.copy()
    patches, positions, info = s.transform_selection(sel, keep_source=keep_source, max_side=max_side, feather=feather, low_latency=True, **ARGS)
    m = W.warp_matrix(BOX, 1.5, 30.0, (10, 25.5), 1)
    grown = (198, 298, 232, 342)
    win = serve.choose_window(grown, HW, margin=0.5)
    dst = W.warp_rect(BOX, m, HW)
    wins = ([] if keep_source else [win]) + [dst]
    paste = "paste_feather" if feather else "paste_locked"
    fill = [] if keep_source else ["grow", "fill_keep", "run_fill"] + (["save"] if history else []) + [paste]
    assert _names(stub) == ["save"] + fill + (["save"] if history else []) + ["warp_drop", "warp"] + ["crop"] * len(wins)
    assert not [c for c in stub.calls if c[0] in ("upload", "move_drop", "shift")]
    saves = [c for c in stub.calls if c[0] == "save"]
    assert saves[0] == ("save", [(200, 300)], (30, 40))               # the lift: move_rect(box, (0, 0))
    if history:
        assert saves[1:] == [("save", [w[:2]], w[2:]) for w in wins]
    calls = {c[0]: c for c in stub.calls}
    lk = s._lock_plane
    # ONE drop at frame scale whatever max_side is; the feather is the fill's alone
    assert calls["warp_drop"] == ("warp_drop", (200, 300, 30, 40), id(sel.plane), None if lk is None else id(lk), BOX, dst, m)
    assert calls["warp"] == ("warp", id(sel.plane), BOX, m)
    assert np.array_equal(stub.lift[:, :120].reshape(30, 40, 3), f[200:230, 300:340])
    work = None
    if not keep_source:
        work = serve.choose_working_size(win[2:], max_side) if max_side else None
        assert calls["grow"] == ("grow", id(sel.plane), 2)
        assert calls["run_fill"] == ("run_fill", [win[:2]], [None], 1 if lock else None, win[2:], work, True)
    assert [c[1] for c in stub.calls if c[0] == "crop"] == wins
    assert positions == [(w[1], w[0]) for w in wins] and [p.shape for p in patches] == [w[2:] + (3,) for w in wins]
    warped = info.pop("selection")
    want = dict(windows=wins, transform=True, matrix=m, selected=1200)
    if lock:
        want["locked"] = True
    if work:
        want["work"] = work
    if history:
        want["undoable"] = True
    if feather and not keep_source:
        want["feather"] = 4
    assert info == want
    spec = W.spec_warp(plane0, BOX, m)
    assert isinstance(warped, serve.Selection) and warped is not sel and (warped.box, warped.count) == L.box_count(spec)
    assert np.array_equal(warped.plane, spec) and np.array_equal(sel.plane, plane0) and sel.box == BOX and warped.count > 2000
    after = _expect(f, plane0, _lock_array() if lock else None, m, 2, win, keep_source)
    assert np.array_equal(s._frame, after) and not np.array_equal(after, f)
    for p, w in zip(patches, wins):
        assert np.array_equal(p, after[w[0]:w[0] + w[2], w[1]:w[1] + w[3]])
    if lock:
        assert np.array_equal(after[_lock_array() != 0], f[_lock_array() != 0])
    if history:
        assert s.can_undo and len(s._undo) == 1 and isinstance(s._undo[0][0], serve._Sequence)
        assert s.history_bytes_used == sum(serve.window_saved_bytes(w[2], w[3]) for w in wins)
    else:
        assert not s.can_undo


def test_undo_and_redo_restore_every_byte_where_the_rectangles_overlap():
    stub = _Stub()
    srv = serve.BatchingServer(object(), max_batch=4, max_wait_s=0.01, window=True, max_grow=0)
    f = U._noise(HW, 5)
    s = serve.EditSession(srv.model, f, backend=stub, history=3)
    sel = s.select_lasso([RING])
    try:
        _, _, info = s.transform_selection(sel, **ARGS)
    except Exception:
        srv.close()
        raise
    win, dst = info["windows"]
    assert serve._windows_intersect(win, dst)
    after = s._frame.copy()
    assert np.array_equal(after, _expect(f, sel.plane, None, info["matrix"], 2, win, False))
    for _ in range(2):
        stub.calls.clear()
        patches, positions, u = s.undo()
        assert stub.calls[:2] == [("swap", [dst[:2]], dst[2:]), ("swap", [win[:2]], win[2:])]          # REVERSE order
        assert u == dict(windows=[win, dst], undo_depth=0, redo_depth=1) and np.array_equal(s._frame, f)
        stub.calls.clear()
        s.redo()
        assert stub.calls[:2] == [("swap", [win[:2]], win[2:]), ("swap", [dst[:2]], dst[2:])]          # forward order
        assert np.array_equal(s._frame, after)
    # through a server, and the warped selection transforms again
    try:
        srv.undo(s)
        assert np.array_equal(s._frame, f)
        srv.redo(s)
        assert np.array_equal(s._frame, after)
    finally:
        srv.close()
    _, _, again = s.transform_selection(info["selection"], scale=0.5, angle=-30.0, keep_source=True)
    assert again["selected"] == info["selection"].count and 0 < again["selection"].count < info["selection"].count and len(s._undo) == 2
    s.undo()
    assert np.array_equal(s._frame, after)
    s.undo()
    assert np.array_equal(s._frame, f)


def test_matrix_window_encode_and_clipping():
    stub = _Stub()
    s, sel, f = _session(stub, history=1)
    m = (70000, 9000, -3000000, -12000, 50000, 9000000)
    patches, _, info = s.transform_selection(sel, matrix=list(np.array(m, np.int64)), hole_grow=0, window=(180, 280, 96, 128), encode="png")
    assert info["matrix"] == m and all(type(v) is int for v in info["matrix"]) and info["windows"] == [(180, 280, 96, 128), W.warp_rect(BOX, m, HW)]
    assert "grow" not in _names(stub) and patches == [b"png", b"png"] and {c[0]: c for c in stub.calls}["warp_drop"][6] == m
    # scaled up by 8 about its centre: the object is clipped by the frame, the rectangle and the selection too
    _, _, info = s.transform_selection(sel, scale=8, offset=(-150, 200), keep_source=True)
    y0, x0, h, w = info["windows"][0]
    assert info["windows"] == [W.warp_rect(BOX, info["matrix"], HW)] and y0 == 0 and x0 + w == 600 and h < 400 and w < 600
    spec = W.spec_warp(sel.plane, BOX, info["matrix"])
    assert (info["selection"].box, info["selection"].count) == L.box_count(spec) and info["selection"].box[0] == 0 and info["selection"].box[3] == 600
    assert 20000 < info["selection"].count < 64 * 1200
    # a failure after the frame was written clears the history

    class _NoWarp(_Stub):
        def warp(self, plane, box, m):
            raise RuntimeError("the device said no")

    s, sel, f = _session(_NoWarp(), history=3)
    sk = np.zeros(HW, np.uint8)
    sk[50:60, 50:80] = 255
    s.edit(sk, max_grow=0)
    with pytest.raises(RuntimeError, match="said no"):
        s.transform_selection(sel, angle=10)
    assert not s.can_undo and not s.can_redo and not np.array_equal(s._frame, f)


def test_refusals_make_no_backend_call():
    stub = _Stub()
    s, sel, f = _session(stub, history=1)
    other = serve.EditSession(None, np.zeros((64, 64, 3), np.uint8), backend=_Stub()).select_lasso([[(1, 1), (30, 1), (15, 30)]])
    empty = s.combine(sel, sel, "subtract")
    stub.calls.clear()
    good = (ID, 0, 0, 0, ID, 0)
    T = s.transform_selection
    bad = [lambda: T(other), lambda: T(sel.plane), lambda: T(None), lambda: T(empty),
           lambda: T(sel, scale=0.1), lambda: T(sel, scale=9), lambda: T(sel, scale=(1, 2, 3)), lambda: T(sel, scale="2"), lambda: T(sel, scale=(1, 0)),
           lambda: T(sel, angle="x"), lambda: T(sel, angle=float("nan")), lambda: T(sel, offset=5), lambda: T(sel, offset=(1, 2, 3)),
           lambda: T(sel, offset=(16385, 0)), lambda: T(sel, offset=("a", 0)), lambda: T(sel, flip="x"), lambda: T(sel, flip=1),
           lambda: T(sel, offset=(400, 0)), lambda: T(sel, offset=(0, -700)),                            # nothing in the frame
           lambda: T(sel, matrix=good, scale=2), lambda: T(sel, matrix=good, angle=1), lambda: T(sel, matrix=good, flip="h"),
           lambda: T(sel, matrix=good, offset=(1, 0)), lambda: T(sel, matrix=good[:5]), lambda: T(sel, matrix=5), lambda: T(sel, matrix=(1.0,) * 6),
           lambda: T(sel, matrix=(True,) * 6), lambda: T(sel, matrix=((1 << 20) + 1, 0, 0, 0, ID, 0)), lambda: T(sel, matrix=(ID, 0, 0, -(1 << 20) - 1, ID, 0)),
           lambda: T(sel, matrix=(ID, 0, (1 << 40) + 1, 0, ID, 0)), lambda: T(sel, matrix=(ID, 0, 0, 0, ID, -(1 << 40) - 1)),
           lambda: T(sel, matrix=(ID, ID, 0, ID, ID, 0)),                  # singular
           lambda: T(sel, matrix=(ID, 0, 1 << 40, 0, ID, 0)),              # valid, and nothing in the frame
           lambda: T(sel, hole_grow=-1), lambda: T(sel, hole_grow=17), lambda: T(sel, hole_grow=1.5), lambda: T(sel, hole_grow=True),
           lambda: T(sel, window=(0, 0, 100, 128)), lambda: T(sel, window=(350, 0, 64, 64)), lambda: T(sel, margin=-1.0), lambda: T(sel, max_side=8),
           lambda: T(sel, encode="gif"), lambda: T(sel, feather=17), lambda: T(sel, feather=2.5)]
    for k, call in enumerate(bad):
        with pytest.raises((ValueError, TypeError)):
            call()
        assert stub.calls == [] and not s.can_undo, k
    with pytest.raises(ValueError, match="puts nothing of the selection in the frame"):
        T(sel, offset=(0, 400))
    with pytest.raises(ValueError, match="empty selection: nothing to transform"):
        T(empty)
    with pytest.raises(ValueError, match="singular"):
        T(sel, matrix=(0,) * 6)
    assert stub.calls == []


def test_existing_calls_issue_what_they_issued():
    """every method of before, move_selection and clone_selection included, on a backend WITH the two new calls never uses them
    and issues the very calls it issues on the backend of before"""
    sk = np.zeros(HW, np.uint8)
    sk[200:210, 300:330] = 255
    mask = np.zeros(HW, np.uint8)
    mask[200:230, 300:340] = 1
    f = U._noise(HW, 5)
    f[200:230, 300:340] = U.REGION
    seqs, frames = {}, {}
    for k, cls in enumerate((_MoveStub, _Stub)):
        for lock in (False, True):
            stub = cls()
            s = serve.EditSession(None, f, backend=stub, history=3)
            if lock:
                s.set_lock(mask)
            stub.calls.clear()
            s.edit(sk, max_grow=0)
            s.edit_strokes([([(30, 20), (60, 30)], 3), ([(500, 300), (520, 310)], 3)])
            s.fill(mask)
            a = s.select_similar((210, 320))
            b = s.select_lasso([RING], grow=2)
            c = s.combine(a, b, "xor")
            s.invert(c)
            s.fill_selection(b)
            s.fill_lasso([RING])
            _, _, info = s.move_selection(b, (10, 25), flip="h", feather=2)
            s.clone_selection(info["selection"], (-100, -200))
            s.set_lock(b)
            b.rings()
            s.undo()
            s.undo()
            s.redo()
            seqs[k, lock], frames[k, lock] = _names(stub), s._frame.copy()
            assert stub.calls and not {"warp_drop", "warp"} & set(_names(stub))
    for lock in (False, True):
        assert seqs[0, lock] == seqs[1, lock] and np.array_equal(frames[0, lock], frames[1, lock])
    # a backend of before cannot transform, and says so only when asked to
    s = serve.EditSession(None, f, backend=_MoveStub(), history=1)
    sel = s.select_lasso([RING])
    with pytest.raises(AttributeError):
        s.transform_selection(sel, angle=5)


def test_model_backend_warp_drop_and_warp():
    """_ModelBackend's two calls on a scripted model: one model call each, and the warp's tile records are the one download"""
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

        def warp_drop_u8(self, frame, lift, lift_rect, sel, lock, box, rect, m):
            self.calls.append(("warp_drop_u8", tuple(lift_rect), tuple(box), tuple(rect), tuple(m)))

        def plane_warp_u8(self, sel, box, m):
            self.calls.append(("plane_warp_u8", tuple(box), tuple(m)))
            return W.spec_warp(sel, box, m)

        def sketch_tiles_u8(self, plane, tile):
            self.calls.append(("sketch_tiles_u8", tile))
            self.tiles.append(_T(spec_tiles(plane, tile)))
            return self.tiles[-1]

    be = serve._ModelBackend.__new__(serve._ModelBackend)
    be.model = _Model()
    sel = np.zeros((37, 53), np.uint8)
    sel[5:20, 7:30] = 255
    box = (5, 7, 20, 30)
    m = serve.warp_matrix(box, 1.25, 40.0, (3, -2.5))
    be.warp_drop(None, None, (5, 7, 16, 23), sel, None, box, (0, 0, 37, 53), m)
    plane, wbox, count = be.warp(sel, box, m)
    spec = W.spec_warp(sel, box, m)
    assert np.array_equal(plane, spec) and (wbox, count) == L.box_count(spec) and count > 15 * 23
    assert be.model.calls == [("warp_drop_u8", (5, 7, 16, 23), box, (0, 0, 37, 53), m), ("plane_warp_u8", box, m), ("sketch_tiles_u8", 32)]
    assert [t.n for t in be.model.tiles] == [1]
    plane, wbox, count = be.warp(sel, box, (ID, 0, 100 * ID, 0, ID, 0))   # nothing lands: the empty selection
    assert wbox is None and count == 0 and not plane.any()


# ---- the C-ABI -------------------------------------------------------------------------------------------------------------
def test_abi_has_two_new_symbols_in_a_header_of_their_own():
    hdr = open(os.path.join(ROOT, "include", "sketchedit_warp.h")).read()
    declared = re.findall(r"^(?:int|size_t)\s+(se_\w+)\(", hdr, re.M)
    assert declared == _lib.abi_names("sketchedit_warp.h") == ["se_warp_drop_u8", "se_plane_warp_u8"]
    others = [n for n in _lib.abi_names() if n not in declared]
    for name in others:                                               # the header refers to other families by DESIGN section
        assert not re.search(r"\b%s\b" % name, hdr), name
    for word in ("se_move", "se_plane_shift", "se_outline"):
        assert word not in hdr
    for name in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if name != "sketchedit_warp.h":
            text = open(os.path.join(ROOT, "include", name)).read()
            assert "se_warp" not in text and "se_plane_warp" not in text, name
    assert "se_warp.hip" in _lib.SOURCES and "se_api_move.hip" in _lib.SOURCES and _lib.SOURCES[-1] == "se_api.hip"
    assert re.search(r"#define SE_WARP_MAX_COEF \(1 << 20\)", hdr) and re.search(r"#define SE_WARP_MAX_TRANSLATION \(1ll << 40\)", hdr)
    import ctypes
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    lib = ctypes.CDLL(_lib.LIB_PATH)                                    # the built library, as the other host tests load it
    for s in declared:
        getattr(lib, s)
    from sketchedit_amd import kernel_labels
    assert kernel_labels.label_of("void se::warp_drop_kernel(unsigned char*, int)") == "warp_drop"
    assert kernel_labels.label_of("warp_drop_kernel(unsigned char*, int)") == "warp_drop"
    assert kernel_labels.label_of("plane_warp_kernel(unsigned char*, long, long)") == "plane_warp"
    misc = open(os.path.join(_lib.CSRC, "se_misc.hip")).read()
    enum = open(os.path.join(_lib.CSRC, "se_kernels.h")).read()
    assert '"move_drop", "plane_shift", "warp_drop", "plane_warp"};' in misc and "PL_PLANE_SHIFT, PL_WARP_DROP, PL_PLANE_WARP, PL_COUNT" in enum
    for label in ("warp_drop", "plane_warp"):
        assert label in set(kernel_labels.KERNEL_LABELS.values())
    from sketchedit_amd.models.editline2_model import EditLine2Model
    for name in ("warp_drop_u8", "plane_warp_u8"):
        assert callable(getattr(_lib.Engine, name)) and callable(getattr(EditLine2Model, name))


def test_the_kernels_cross_compile_for_gfx950(tmp_path):
    import shutil
    import subprocess
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc on this machine")
    obj = str(tmp_path / "se_warp.o")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(_lib.CSRC, "se_warp.hip"), "-o", obj])
    assert os.path.getsize(obj) > 0


# ---- the kernels' arithmetic, lane by lane -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(16, 16), (37, 53), (65, 129)], ids=lambda hw: "%dx%d" % hw)
def test_tiled_arithmetic_is_the_statement(hw):
    """se_warp.hip's per-tile int64 base and int32 lane deltas, its early return, the bounded spans of S and of the slot row and
    the byte stores, on one flat byte array in which every access is checked against the span the kernel may touch"""
    Hi, Wi = hw
    rng = np.random.RandomState(Hi)
    frame = rng.randint(0, 256, (Hi, Wi, 3)).astype(np.uint8)
    before = rng.randint(0, 256, (Hi, Wi, 3)).astype(np.uint8)
    sel = np.where(rng.rand(Hi, Wi) < 0.7, rng.randint(1, 256, (Hi, Wi)), 0).astype(np.uint8)
    lock = np.where(rng.rand(Hi, Wi) < 0.2, 255, 0).astype(np.uint8)
    box = (1, 2, Hi - 3, Wi - 1)
    rect = M.move_rect(box, (0, 0), hw)
    slot = M.slot_of(before, rect)
    whole = (0, 0, Hi, Wi)
    far = (ID, 0, -(1 << 40), 0, ID, 1 << 40)
    cases = [(W.warp_matrix(box, 1.0, 0.0, (0, 0), 0), whole, False), (W.warp_matrix(box, 1.0, 0.0, (0.5, -1.5), 3), whole, True),
             (W.warp_matrix(box, 1.5, 30.0, (2, 1), 1), None, False), (W.warp_matrix(box, (0.125, 8.0), 200.0, (0, 0), 0), whole, True),
             (W.warp_matrix(box, 0.5, 90.0, (-Hi // 2, Wi // 3), 2), None, True),
             ((W.MAX_COEF, -W.MAX_COEF, (6 << 16) + 0x8000, W.MAX_COEF, W.MAX_COEF, 0x8000 - (153 << 16)), whole, False),     # (5, 5) <- (6.5, 7.5)
             ((70000, 9000, -200000, -12000, 50000, 300000), (Hi - 16, 0, 16, 16), True), (far, whole, False)]
    early_any = False
    for k, (m, R, locked) in enumerate(cases):
        R = R or W.warp_rect(box, m, hw)
        mem = M.Memory(16384 + 5 * Hi * Wi + slot.size)
        fa = mem.put(1024 + k % 4, frame)
        sa = mem.put(fa + 3 * Hi * Wi + 1031, sel)
        la = mem.put(sa + Hi * Wi + 1033, lock)
        pa = mem.put((la + Hi * Wi + 1024 + 15) // 16 * 16, slot)
        oa = pa + slot.size + 1024 + (k + 1) % 4
        clean = mem.mem.copy()
        tiles, early = W.tiled_drop(mem, fa, Hi, Wi, pa, rect, sa, la if locked else None, box, R, m)
        want = W.spec_drop(frame, slot, rect, sel, lock if locked else None, box, R, m)
        assert np.array_equal(mem.get(fa, frame.shape), want), (hw, m)
        changed = np.flatnonzero(mem.mem != clean)
        assert changed.size == 0 or (fa <= changed.min() and changed.max() < fa + 3 * Hi * Wi)
        assert tiles == -(-R[2] // 16) * -(-R[3] // 64) and (changed.size > 0) == (m != far) and (m != far or early == tiles)
        early_any |= 0 < early < tiles
        mem.mem[:] = clean
        W.tiled_warp(mem, sa, Hi, Wi, box, m, oa)
        assert np.array_equal(mem.get(oa, hw), W.spec_warp(sel, box, m)), (hw, m)
        changed = np.flatnonzero(mem.mem != clean)
        assert oa <= changed.min() and changed.max() < oa + Hi * Wi
    assert early_any or hw != (65, 129)                                  # some tiles return early while others of the launch work
