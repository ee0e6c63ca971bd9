"""GPU tests of moving and cloning a selection: the two kernels of se_move.hip against the statement of
tests/move_util.py on whole buffers between sentinels, at every alignment, and EditSession.move_selection / clone_selection
against a two-step route -- fill_selection of the grown selection on a twin session, then the statement's drop applied on the
host with the original pixels.  Every comparison is exact."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from sketchedit_amd import _lib, serve
import lasso_util as L
import move_util as M
import outline_util as O
import select_util as U
from test_gpu_lasso import FHW, GARBAGE, HOLE, RING, SENTINEL, _Buf, _blob_frame, _cuda, _lock_plane, _session, eng, model  # noqa: F401

pytestmark = pytest.mark.gpu

RADII = (0, 1, 3, 16)


def _values_disc(Hi, Wi):
    """a disc whose selected bytes take every non-zero value: non-zero = selected, not 255"""
    d = O.disc(Hi, Wi)
    yy, xx = np.mgrid[0:Hi, 0:Wi]
    return np.where(d != 0, ((yy * 7 + xx * 13) % 255 + 1).astype(np.uint8), 0).astype(np.uint8)


PATTERNS = {"noise": O.noise, "disc": _values_disc, "annulus": O.annulus, "full": O.full}


@functools.lru_cache(maxsize=None)
def _case(name, hw):
    """(frame, the frame as it was lifted, selection plane, lock plane, box, lift rectangle, slot): computed once, shared, read-only"""
    Hi, Wi = hw
    rng = np.random.RandomState(Hi * 1000 + Wi)
    frame, before = U._noise(hw, 3), U._noise(hw, 4)
    sel = np.ascontiguousarray(PATTERNS[name](Hi, Wi), np.uint8)
    lock = np.where(rng.rand(Hi, Wi) < 0.25, rng.randint(1, 256, hw), 0).astype(np.uint8)
    if name == "noise":                                                  # a box strictly inside the selected pixels: those outside stay
        box = (2, 3, Hi - 4, Wi - 2)
        rect = (0, 0, Hi, Wi)                                            # and a lift larger than the box
    else:
        box = M.box_of(sel)
        rect = M.move_rect(box, (0, 0), hw)
    slot = M.slot_of(before, rect)
    for a in (frame, before, sel, lock, slot):
        a.setflags(write=False)
    return frame, before, sel, lock, box, rect, slot


def _offsets(hw, box):
    """0, +-1, smaller than the object, over each of the four edges, and wholly out"""
    Hi, Wi = hw
    by0, bx0, by1, bx1 = box
    h, w = by1 - by0, bx1 - bx0
    return [(0, 0), (1, 0), (0, -1), (-1, 1), (h // 3, -(w // 4)), (-by0 - h // 2, 2), (Hi - by0 - h // 2, -1), (1, -bx0 - w // 2),
            (-2, Wi - bx0 - w // 2), (-by0 - 1, Wi - bx1 + 1), (Hi - by0, 0), (0, -bx1), (-M.MAX_OFFSET, M.MAX_OFFSET)]


class _Slot:
    """a lift on the device, 16-byte aligned between sentinel rows"""

    def __init__(self, slot):
        n = slot.size
        self.n = n
        self.buf = torch.full((4096 + n + 4096,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.lead = 4096 + (-self.buf.data_ptr()) % 16
        self.view = self.buf[self.lead:self.lead + n]
        self.view.copy_(_cuda(slot).reshape(-1))
        self.want = self.buf.cpu().numpy()

    def intact(self):
        return np.array_equal(self.buf.cpu().numpy(), self.want)


# ---- 1. the drop: every flip and radius at every size, offset and alignment ------------------------------------------------------------------
@pytest.mark.parametrize("hw", L.SIZES, ids=lambda hw: "%dx%d" % hw)
@pytest.mark.parametrize("flip", range(4))
@pytest.mark.parametrize("r", RADII)
def test_drop_follows_the_statement(eng, hw, flip, r):
    changed = 0
    dev = {}
    for k in range(13):
        name = sorted(PATTERNS)[k % len(PATTERNS)]                                 # every (flip, r) meets every pattern
        frame, _, sel, lock, box, rect, slot = _case(name, hw)
        if name not in dev:
            dev[name] = (_Buf(hw, 1, like=sel), _Buf(hw, 3, like=lock), _Slot(slot), sel, lock)       # planes at odd offsets
        sb, lb, pb = dev[name][:3]
        off = _offsets(hw, box)[k]
        for locked in (False, True):
            fb = _Buf(frame.shape, (k + locked) % 4, like=frame)                   # the frame at every byte offset mod 4
            eng.move_drop_u8(fb.view, pb.view, rect, sb.view, lb.view if locked else None, box, off, flip=flip, radius=r)
            got = fb.get()
            want = M.spec_drop(frame, slot, rect, sel, lock if locked else None, box, off, flip, r)
            assert np.array_equal(got, want), (name, hw, off, flip, r, locked, int((got != want).sum()))
            changed += int((got != frame).any())
    for sb, lb, pb, sel, lock in dev.values():
        assert np.array_equal(sb.get(), sel) and np.array_equal(lb.get(), lock) and pb.intact()
    assert changed >= 12                                                           # all but the offsets that are wholly out


def test_drop_known_answer_and_overlap(eng):
    # the header's known answer
    frame = np.full((16, 16, 3), 10, np.uint8)
    slot = M.slot_of(np.full((16, 16, 3), 200, np.uint8), (0, 0, 16, 16))
    sel = np.zeros((16, 16), np.uint8)
    sel[2:4, 2:5] = 1
    for r, corner, middle in ((0, 200, 200), (1, 94, 137)):
        fb, pb = _Buf(frame.shape, 2, like=frame), _Slot(slot)
        eng.move_drop_u8(fb.view, pb.view, (0, 0, 16, 16), _cuda(sel), None, (2, 2, 4, 5), (1, 3), radius=r)
        want = frame.copy()
        want[3:5, 5:8] = corner
        want[3:5, 6] = middle
        assert np.array_equal(fb.get(), want)
    # source and destination overlap: the object's pixels come from the lift, never from the frame it is written into
    f, _, sel, _, box, rect, _ = _case("full", (65, 129))
    fb, pb = _Buf(f.shape, 1, like=f), _Slot(M.slot_of(f, rect))
    eng.move_drop_u8(fb.view, pb.view, rect, _cuda(sel), None, box, (3, 5))
    want = f.copy()
    want[3:, 5:] = f[:-3, :-5]
    assert np.array_equal(fb.get(), want)


# ---- 2. the shift ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", L.SIZES, ids=lambda hw: "%dx%d" % hw)
@pytest.mark.parametrize("flip", range(4))
def test_shift_follows_the_statement(eng, hw, flip):
    name = sorted(PATTERNS)[flip]
    _, _, sel, _, box, _, _ = _case(name, hw)
    sb = _Buf(hw, 3, like=sel)
    for k, off in enumerate(_offsets(hw, box)):
        ob = _Buf(hw, k % 4, fill=GARBAGE)                                          # every byte must be written
        eng.plane_shift_u8(sb.view, box, off, flip=flip, out=ob.view)
        got, want = ob.get(), M.spec_shift(sel, box, off, flip)
        assert np.array_equal(got, want), (name, hw, off, flip, int((got != want).sum()))
    assert np.array_equal(sb.get(), sel)
    assert np.array_equal(eng.plane_shift_u8(_cuda(sel), box, (1, -2), flip=flip).cpu().numpy(), M.spec_shift(sel, box, (1, -2), flip))


# ---- 3. both again with every scratch byte poisoned ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(37, 53), (130, 70)], ids=lambda hw: "%dx%d" % hw)
def test_drop_and_shift_under_poison(eng, seopt, hw):
    seopt.set("SE_TEST_POISON", 0xFF)
    frame, _, sel, lock, box, rect, slot = _case("disc", hw)
    sb, lb, pb = _Buf(hw, 1, like=sel), _Buf(hw, 3, like=lock), _Slot(slot)
    for k, off in enumerate(_offsets(hw, box)[3:9]):
        flip, r = k % 4, RADII[(k + 1) % 4]
        fb, ob = _Buf(frame.shape, k % 4, like=frame), _Buf(hw, (k + 1) % 4, fill=GARBAGE)
        eng.move_drop_u8(fb.view, pb.view, rect, sb.view, lb.view, box, off, flip=flip, radius=r)
        eng.plane_shift_u8(sb.view, box, off, flip=flip, out=ob.view)
        assert np.array_equal(fb.get(), M.spec_drop(frame, slot, rect, sel, lock, box, off, flip, r)), (hw, off, flip, r)
        assert np.array_equal(ob.get(), M.spec_shift(sel, box, off, flip)), (hw, off, flip)
    assert np.array_equal(sb.get(), sel) and np.array_equal(lb.get(), lock) and pb.intact()


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(eng):
    Hi, Wi = 37, 53
    frame, _, sel, lock, box, rect, slot = _case("disc", (Hi, Wi))
    fb, sb, lb, pb, ob = (_Buf(frame.shape, 1, like=frame), _Buf((Hi, Wi), 1, like=sel), _Buf((Hi, Wi), 2, like=lock), _Slot(slot),
                          _Buf((Hi, Wi), 3, fill=GARBAGE))
    lib, h, st = eng.lib, eng.h, eng._stream()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else t)     # noqa: E731
    F, S, K, P, OUT = fb.view, sb.view, lb.view, pb.view, ob.view
    by0, bx0, by1, bx1 = box
    ly0, lx0, lh, lw = rect
    ok = dict(F=F, Hi=Hi, Wi=Wi, P=P, ly0=ly0, lx0=lx0, lh=lh, lw=lw, S=S, K=K, by0=by0, bx0=bx0, by1=by1, bx1=bx1, dy=2, dx=-3, flip=1, r=2)
    inside_frame = F.data_ptr() + 3 * Hi * Wi - 1                          # begins on the frame's last byte
    drops = [(dict(F=None), "frame_u8"), (dict(P=None), "lift"), (dict(S=None), "sel_u8"), (dict(Hi=15), "Hi"), (dict(Wi=15), "Wi"),
             (dict(lh=15), "lift rectangle"), (dict(lw=15), "lift rectangle"), (dict(ly0=-1), "lift rectangle"), (dict(lx0=Wi - lw + 1), "lift rectangle"),
             (dict(ly0=Hi - lh + 1), "lift rectangle"), (dict(P=P.data_ptr() + 8), "16-byte aligned"), (dict(by1=by0), "box"), (dict(bx1=bx0), "box"),
             (dict(by0=ly0 - 1), "lies outside the lift rectangle"), (dict(bx1=lx0 + lw + 1), "lies outside the lift rectangle"),
             (dict(by1=ly0 + lh + 1), "lies outside the lift rectangle"), (dict(dy=16385), "dy"), (dict(dy=-16385), "dy"), (dict(dx=16385), "dx"),
             (dict(dx=-16385), "dx"), (dict(flip=4), "flip"), (dict(flip=-1), "flip"), (dict(r=17), "radius"), (dict(r=-1), "radius"),
             (dict(S=inside_frame), "sel_u8 overlaps"), (dict(K=F.data_ptr() - Hi * Wi + 1), "lock_u8 overlaps"),
             (dict(P=(F.data_ptr() + 16) // 16 * 16), "lift overlaps")]
    for change, what in drops:
        a = dict(ok, **change)
        rc = lib.se_move_drop_u8(h, st, p(a["F"]), a["Hi"], a["Wi"], p(a["P"]), a["ly0"], a["lx0"], a["lh"], a["lw"], p(a["S"]), p(a["K"]),
                                 a["by0"], a["bx0"], a["by1"], a["bx1"], a["dy"], a["dx"], a["flip"], a["r"])
        assert rc != 0, (change, what)
        assert what in lib.se_last_error(h).decode(), (what, lib.se_last_error(h).decode())
    sok = dict(S=S, Hi=Hi, Wi=Wi, by0=by0, bx0=bx0, by1=by1, bx1=bx1, dy=2, dx=-3, flip=1, O=OUT)
    shifts = [(dict(S=None), "sel_u8"), (dict(O=None), "plane_out"), (dict(Hi=15), "Hi"), (dict(Wi=15), "Wi"), (dict(by1=by0), "box"),
              (dict(by0=-1), "lies outside the frame"), (dict(bx1=Wi + 1), "lies outside the frame"), (dict(dy=16385), "dy"), (dict(dx=-16385), "dx"),
              (dict(flip=4), "flip"), (dict(O=S), "plane_out overlaps"), (dict(O=S.data_ptr() + Hi * Wi - 1), "plane_out overlaps"),
              (dict(O=S.data_ptr() - Hi * Wi + 1), "plane_out overlaps")]
    for change, what in shifts:
        a = dict(sok, **change)
        rc = lib.se_plane_shift_u8(h, st, p(a["S"]), a["Hi"], a["Wi"], a["by0"], a["bx0"], a["by1"], a["bx1"], a["dy"], a["dx"], a["flip"], p(a["O"]))
        assert rc != 0, (change, what)
        assert what in lib.se_last_error(h).decode(), (what, lib.se_last_error(h).decode())
    # the bindings refuse planes and lifts of another shape or size
    for call in (lambda: eng.move_drop_u8(F.view(-1), P, rect, S, None, box, (0, 0)), lambda: eng.move_drop_u8(F, P, rect, S.view(Wi, Hi), None, box, (0, 0)),
                 lambda: eng.move_drop_u8(F, P, rect, S, K.view(Wi, Hi), box, (0, 0)), lambda: eng.move_drop_u8(F, P[:-1], rect, S, None, box, (0, 0)),
                 lambda: eng.plane_shift_u8(S, box, (0, 0), out=OUT.view(Wi, Hi)), lambda: eng.plane_shift_u8(S.view(-1), box, (0, 0))):
        with pytest.raises(_lib.SketchEditHipError):
            call()
    # valid, and nothing to do: the whole box lands outside the frame
    eng.move_drop_u8(F, P, rect, S, K, box, (Hi, 0), flip=3, radius=16)
    torch.cuda.synchronize()
    assert np.array_equal(fb.get(), frame) and np.array_equal(sb.get(), sel) and np.array_equal(lb.get(), lock) and pb.intact()
    assert (ob.get() == GARBAGE).all()
    eng.plane_shift_u8(S, box, (Hi, 0), out=OUT)
    assert not ob.get().any()


# ---- 5. sessions ------------------------------------------------------------------------------------------------------------------------------
SESSION_CASES = [dict(), dict(locked=True), dict(max_side=64), dict(feather=4, locked=True), dict(feather=3, flip="h", hole_grow=0),
                 dict(keep_source=True, flip="hv", feather=2, locked=True), dict(offset=(-40, 30), flip="v", max_side=64, feather=16, locked=True),
                 dict(window=(16, 8, 96, 88), hole_grow=5), dict(offset=(-50, -45), keep_source=True)]


@pytest.mark.parametrize("poison", [0, 0xFF])
@pytest.mark.parametrize("case", SESSION_CASES, ids=lambda c: "-".join("%s=%s" % kv for kv in sorted(c.items())) or "defaults")
def test_session_move_is_fill_then_the_statements_drop(model, seopt, case, poison):
    """a twin session fills the grown selection through the same window in the same mode, the statement drops the ORIGINAL pixels
    on the host: every byte of the frame, its sentinel margins included, is equal.  In every case but the far offsets the fill
    window holds the destination rectangle, so a journal that swapped in the wrong order would not restore the frame."""
    case = dict(case)
    f, _ = _blob_frame()
    lock = _lock_plane() if case.pop("locked", False) else None
    offset = case.pop("offset", (7, -9))                                 # smaller than the object: source and destination overlap
    flip, keep, hole_grow = case.get("flip"), case.get("keep_source", False), case.get("hole_grow", 2)
    if poison:
        seopt.set("SE_TEST_POISON", poison)
    a, abuf = _session(model, f, lock, history=2)
    b, bbuf = _session(model, f, lock, history=2)
    sel = a.select_lasso([RING, HOLE])
    plane = L.spec_select_lasso([RING, HOLE], FHW, 0)
    box = L.box_count(plane)[0]
    patches, positions, info = a.move_selection(sel, offset, low_latency=False, **case)
    dst = M.move_rect(box, offset, FHW)
    wins = info["windows"]
    assert wins[-1] == dst and len(wins) == (1 if keep else 2) and positions == [(w[1], w[0]) for w in wins]
    if not keep:
        grown = (max(box[0] - hole_grow, 0), max(box[1] - hole_grow, 0), min(box[2] + hole_grow, FHW[0]), min(box[3] + hole_grow, FHW[1]))
        assert wins[0] == (case["window"] if "window" in case else serve.choose_window(grown, FHW, margin=0.5))
        fill = {k: case[k] for k in ("max_side", "feather") if k in case}
        _, _, ib = b.fill_selection(b.select_lasso([RING, HOLE], grow=hole_grow), window=wins[0], low_latency=False, **fill)
        assert info.get("work") == ib.get("work")
    rect = M.move_rect(box, (0, 0), FHW)
    want = M.spec_drop(bbuf.get(), M.slot_of(f, rect), rect, plane, lock, box, offset, serve.MOVE_FLIPS[flip], case.get("feather") or 0)
    after = abuf.get()                                                   # (checks the margins)
    assert np.array_equal(after, want) and not np.array_equal(after, f)
    for pch, w in zip(patches, wins):
        assert np.array_equal(pch, after[w[0]:w[0] + w[2], w[1]:w[1] + w[3]])
    if lock is not None:
        assert np.array_equal(after[lock != 0], f[lock != 0]) and info["locked"] is True
    assert info["move"] is True and info["offset"] == offset and info["flip"] == flip and info["selected"] == sel.count and info["undoable"] is True
    # the moved selection: the statement's shift in plane, box and count; the one passed in stays what it was
    moved = info["selection"]
    shifted = M.spec_shift(plane, box, offset, serve.MOVE_FLIPS[flip])
    assert np.array_equal(moved.plane.cpu().numpy(), shifted) and (moved.box, moved.count) == L.box_count(shifted)
    assert np.array_equal(sel.plane.cpu().numpy(), plane) and sel.box == box
    # one call is one undo step, byte for byte both ways
    a.undo()
    assert np.array_equal(abuf.get(), f) and not a.can_undo
    a.redo()
    assert np.array_equal(abuf.get(), after) and not a.can_redo


def test_session_moved_selection_round_trips_and_moves_again(model):
    f, _ = _blob_frame()
    s, fb = _session(model, f, None, history=4)
    sel = s.select_lasso([RING, HOLE])
    plane = sel.plane.cpu().numpy()
    _, _, info = s.move_selection(sel, (-45, 30), flip="h", low_latency=False)         # partly over the top and right edges
    moved = info["selection"]
    shifted = M.spec_shift(plane, sel.box, (-45, 30), 1)
    assert 0 < moved.count < sel.count and np.array_equal(moved.plane.cpu().numpy(), shifted)
    again = s.select_lasso(moved.rings())                                # its rings re-make it
    assert np.array_equal(again.plane.cpu().numpy(), shifted) and (again.box, again.count) == (moved.box, moved.count)
    before = fb.get().copy()
    _, _, info2 = s.clone_selection(moved, (50, -40), feather=2)
    rect = M.move_rect(moved.box, (0, 0), FHW)
    want = M.spec_drop(before, M.slot_of(before, rect), rect, shifted, None, moved.box, (50, -40), 0, 2)
    assert np.array_equal(fb.get(), want) and info2["selection"].count == moved.count and info2["windows"] == [M.move_rect(moved.box, (50, -40), FHW)]
    assert len(s._undo) == 2
    s.undo()
    assert np.array_equal(fb.get(), before)
    s.undo()
    assert np.array_equal(fb.get(), f)
    with pytest.raises(ValueError, match="out of the frame"):
        s.move_selection(sel, (200, 0))
    assert np.array_equal(fb.get(), f) and not s.can_undo


def test_session_move_encode_forms(model):
    f, _ = _blob_frame()
    for encode, ref in (("png", lambda s, w: s.frame_png(w)), (("jpg", 90), lambda s, w: s.frame_jpg(w, quality=90)),
                        (("jpg", 75, "420", True), lambda s, w: s.frame_jpg(w, quality=75, subsampling="420", optimize=True))):
        s, fb = _session(model, f, _lock_plane(), history=1)
        sel = s.select_lasso([RING])
        patches, _, info = s.move_selection(sel, (6, 11), encode=encode, low_latency=False)
        assert len(patches) == 2 and all(isinstance(p, bytes) for p in patches)
        assert patches == [ref(s, w) for w in info["windows"]], encode
        s.undo()
        assert np.array_equal(fb.get(), f)
