"""GPU tests of the canvas of an editing session: the two kernels of se_canvas.hip against the statement of
tests/canvas_util.py on whole buffers between sentinels, at every alignment, every refusal of the entry, and EditSession.canvas,
its wrappers and the outpaint against twin sessions built from the statement's result.  Every comparison is exact."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from sketchedit_amd import _lib, serve
import canvas_util as C
import lasso_util as L
import select_util as U
from test_gpu_lasso import FHW, GARBAGE, HOLE, RING, SENTINEL, _Buf, _blob_frame, _cuda, _lock_plane, _session, eng, model  # noqa: F401

pytestmark = pytest.mark.gpu

RGB = {1: 0x5A, 3: 0x0A | 0xC8 << 8 | 0x1F << 16}


@functools.lru_cache(maxsize=None)
def _image(hw, ch):
    """computed once, shared, read-only"""
    a = U._noise(hw, 11) if ch == 3 else np.ascontiguousarray(U._noise(hw, 12)[:, :, 1])
    a.setflags(write=False)
    return a


# ---- 1. the entry: every orientation, pad mode and rectangle at every size and alignment ----------------------------------------------------
@pytest.mark.parametrize("hw", C.SIZES, ids=lambda hw: "%dx%d" % hw)
@pytest.mark.parametrize("ch", [1, 3])
def test_canvas_follows_the_statement(eng, hw, ch):
    img = _image(hw, ch)
    ib = _Buf(img.shape, 1 + 2 * (hw[0] % 2), like=img)                   # the input at odd offsets
    k = 0
    for o in range(8):
        oriented = (hw[1], hw[0]) if o & 4 else hw
        for (y0, x0, h, w) in C.rects(oriented):
            for mode in (C.EDGE, C.REFLECT, C.CONSTANT):
                shape = (h, w) if ch == 1 else (h, w, 3)
                ob = _Buf(shape, k % 4, fill=GARBAGE)                     # the output at every byte offset mod 4; an unwritten byte shows
                eng.canvas_u8(ib.view, (h, w), origin=(y0, x0), orient=o, pad=mode, pad_rgb=RGB[ch], out=ob.view)
                got = ob.get()                                            # (checks the margins)
                want = C.spec_canvas(img, hw, (h, w), (y0, x0), o, mode, RGB[ch])
                assert np.array_equal(got, want), (hw, ch, o, (y0, x0, h, w), mode, k % 4, int((got != want).sum()))
                k += 1
    assert np.array_equal(ib.get(), img)                                  # the input and its margins are what they were
    if hw in ((130, 70), (200, 150)):                                     # both routes of the turn ran
        seen = set()
        for r in C.rects((hw[1], hw[0])):
            seen |= set(C.turn_routes(hw, r[2:], r[:2], 6).reshape(-1).tolist())
        assert seen == {True, False}


def test_canvas_known_answers_new_planes_and_the_null_input(eng):
    img = np.array([[1, 2, 3], [4, 5, 6]], np.uint8)
    for out_hw, origin, o, mode, rgb, want in (((3, 2), (0, 0), 6, C.EDGE, 0, [[4, 1], [5, 2], [6, 3]]), ((3, 2), (0, 0), 5, C.EDGE, 0, [[3, 6], [2, 5], [1, 4]]),
                                               ((2, 5), (0, -1), 1, C.EDGE, 0, [[3, 3, 2, 1, 1], [6, 6, 5, 4, 4]]),
                                               ((1, 9), (1, -4), 0, C.REFLECT, 0, [[4, 5, 6, 5, 4, 5, 6, 5, 4]]),
                                               ((3, 4), (-1, 1), 0, C.CONSTANT, 9, [[9, 9, 9, 9], [2, 3, 9, 9], [5, 6, 9, 9]])):
        got = eng.canvas_u8(_cuda(img), out_hw, origin=origin, orient=o, pad=mode, pad_rgb=rgb)
        assert np.array_equal(got.cpu().numpy(), np.array(want, np.uint8)), (o, mode)
    # the NULL input: the plane of the new area, through both kernels, at every alignment
    for k, (hw, out_hw, origin, o) in enumerate((((2, 3), (3, 4), (-1, 1), 0), ((120, 104), (131, 150), (-7, -3), 0), ((120, 104), (130, 140), (-20, 5), 6),
                                                 ((65, 129), (140, 70), (3, -2), 5), ((37, 53), (37, 53), (0, 0), 3))):
        ob = _Buf(out_hw, k % 4, fill=GARBAGE)
        eng.canvas_u8(None, out_hw, origin=origin, orient=o, pad=C.CONSTANT, pad_rgb=255, src_hw=hw, out=ob.view)
        want = C.spec_canvas(None, hw, out_hw, origin, o, C.CONSTANT, 255)
        assert np.array_equal(ob.get(), want) and set(np.unique(want)) <= {0, 255}
    fresh = eng.canvas_u8(None, (20, 24), origin=(-4, 0), pad=C.CONSTANT, pad_rgb=255, src_hw=(16, 24))
    assert fresh.shape == (20, 24) and (fresh[:4] == 255).all() and not fresh[4:].any()
    # inverse orientations give the input back
    f = _image((65, 129), 3)
    for o, inv in ((5, 6), (6, 5), (4, 4), (7, 7), (1, 1), (3, 3)):
        turned = eng.canvas_u8(_cuda(f), (129, 65) if o & 4 else (65, 129), orient=o)
        assert np.array_equal(eng.canvas_u8(turned, (65, 129), orient=inv).cpu().numpy(), f)


def test_refusals_enqueue_nothing(eng):
    Hi, Wi, Hn, Wn = 37, 53, 41, 60
    img = _image((Hi, Wi), 3)
    ib, ob = _Buf(img.shape, 1, like=img), _Buf((Hn, Wn, 3), 3, fill=GARBAGE)
    lib, h, st = eng.lib, eng.h, eng._stream()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else t)     # noqa: E731
    I, O = ib.view, ob.view
    ok = dict(I=I, Hi=Hi, Wi=Wi, C=3, O=O, Hn=Hn, Wn=Wn, oy=-2, ox=-3, o=6, pad=1, rgb=0)
    cases = [(dict(O=None), "out"), (dict(I=None), "in"), (dict(C=2), "C"), (dict(C=0), "C"), (dict(C=4), "C"), (dict(o=8), "orient"), (dict(o=-1), "orient"),
             (dict(pad=3), "pad_mode"), (dict(pad=-1), "pad_mode"), (dict(Hi=0), "Hi"), (dict(Wi=0), "Wi"), (dict(Hi=32769), "Hi"), (dict(Wi=32769), "Wi"),
             (dict(Hi=32768, Wi=32768), "Hi"), (dict(Hn=0), "Hn"), (dict(Wn=0), "Wn"), (dict(Hn=32769), "Hn"), (dict(Wn=-5), "Wn"),
             (dict(Hn=32768, Wn=32768), "Hn"), (dict(oy=(1 << 20) + 1), "oy"), (dict(oy=-(1 << 20) - 1), "oy"), (dict(ox=(1 << 20) + 1), "ox"),
             (dict(ox=-(1 << 20) - 1), "ox"), (dict(O=I), "overlaps"), (dict(O=I.data_ptr() + 3 * Hi * Wi - 1), "overlaps"),
             (dict(O=I.data_ptr() - 3 * Hn * Wn + 1), "overlaps")]
    for change, what in cases:
        a = dict(ok, **change)
        rc = lib.se_canvas_u8(h, st, p(a["I"]), a["Hi"], a["Wi"], a["C"], p(a["O"]), a["Hn"], a["Wn"], a["oy"], a["ox"], a["o"], a["pad"], a["rgb"])
        assert rc != 0, (change, what)
        assert what in lib.se_last_error(h).decode(), (what, lib.se_last_error(h).decode())
    # the binding refuses arrays of another shape
    for call in (lambda: eng.canvas_u8(I.view(-1), (Hn, Wn)), lambda: eng.canvas_u8(I, (Hn, Wn), out=O.view(Wn, Hn, 3)),
                 lambda: eng.canvas_u8(I, (Hn, Wn), out=O[:, :, 0]), lambda: eng.canvas_u8(None, (Hn, Wn)), lambda: eng.canvas_u8(I, (0, 5))):
        with pytest.raises(_lib.SketchEditHipError):
            call()
    torch.cuda.synchronize()
    assert np.array_equal(ib.get(), img) and (ob.get() == GARBAGE).all()
    # valid at the limits of the offsets: the rectangle lies wholly in the pad area
    eng.canvas_u8(I, (Hn, Wn), origin=(1 << 20, -(1 << 20)), orient=5, pad=C.REFLECT, out=O)
    assert np.array_equal(ob.get(), C.spec_canvas(img, (Hi, Wi), (Hn, Wn), (1 << 20, -(1 << 20)), 5, C.REFLECT))


# ---- 2. sessions --------------------------------------------------------------------------------------------------------------------------------
def _twin(model, frame, lock, **kw):
    return serve.EditSession(model, np.ascontiguousarray(frame), **kw) if lock is None else _session(model, np.ascontiguousarray(frame), lock, **kw)[0]


def _carried(t, plane):
    box, count = L.box_count(plane)
    return serve.Selection(t.backend, _cuda(plane), box, count, plane.shape)


WRAPPERS = [("orient_canvas", ("cw",), {}, 6, None, C.EDGE, 0), ("orient_canvas", ("ccw",), {}, 5, None, C.EDGE, 0),
            ("orient_canvas", ("180",), {}, 3, None, C.EDGE, 0), ("orient_canvas", ("h",), {}, 1, None, C.EDGE, 0),
            ("orient_canvas", ("v",), {}, 2, None, C.EDGE, 0), ("orient_canvas", ("transpose",), {}, 4, None, C.EDGE, 0),
            ("orient_canvas", ("transverse",), {}, 7, None, C.EDGE, 0), ("crop_canvas", ((13, 21, 83, 67),), {}, 0, (13, 21, 83, 67), C.EDGE, 0),
            ("extend_canvas", (), dict(top=5, right=31, pad="reflect"), 0, (-5, 0, 125, 135), C.REFLECT, 0),
            ("extend_canvas", (), dict(bottom=130, left=1, pad=(3, 200, 77)), 0, (0, -1, 250, 105), C.CONSTANT, 3 | 200 << 8 | 77 << 16),
            ("canvas", (), dict(orient="cw", rect=(-9, 30, 100, 97), pad="edge"), 6, (-9, 30, 100, 97), C.EDGE, 0)]


@pytest.mark.parametrize("case", WRAPPERS, ids=lambda c: "%s-%s" % (c[0], c[3] if c[4] is None else "x".join(str(v) for v in c[4])))
def test_session_wrappers_are_the_statement_and_carry_lock_and_selections(model, case):
    name, args, kw, o, rect, mode, rgb = case
    f, _ = _blob_frame()
    lock = _lock_plane()
    s, fb = _session(model, f, lock, history=3)
    sel, small = s.select_lasso([RING, HOLE]), s.select_lasso([[(2.0, 3.0), (14.5, 4.0), (6.0, 17.0)]])
    plane, small_plane = L.spec_select_lasso([RING, HOLE], FHW, 0), small.plane.cpu().numpy()
    oriented = (FHW[1], FHW[0]) if o & 4 else FHW
    y0, x0, h, w = rect if rect is not None else (0, 0) + oriented
    patch, pos, info = getattr(s, name)(*args, selections=[sel, small], **kw)
    want = C.spec_canvas(f, FHW, (h, w), (y0, x0), o, mode, rgb)
    want_lock = C.spec_canvas(lock, FHW, (h, w), (y0, x0), o, C.CONSTANT, 0)
    assert patch is None and pos == (0, 0) and s.frame_hw == (h, w) and info["canvas"] == (h, w) and info["previous"] == FHW
    assert np.array_equal(s.frame(), want) and np.array_equal(s.lock(), want_lock) and info["locked"] is True and info["undoable"] is True
    assert np.array_equal(fb.get(), f)                                     # out of place: the old frame and its margins are whole
    planes = []
    for old, new, old_plane in zip((sel, small), info["selections"], (plane, small_plane)):
        moved = C.spec_canvas(old_plane, FHW, (h, w), (y0, x0), o, C.CONSTANT, 0)
        assert new.frame_hw == (h, w) and np.array_equal(new.plane.cpu().numpy(), moved) and (new.box, new.count) == L.box_count(moved)
        assert np.array_equal(old.plane.cpu().numpy(), old_plane) and old.frame_hw == FHW
        planes.append(moved)
    # a hard clone and a filter of the carried selection, against the same operations on a twin built from the statement
    t = _twin(model, want, want_lock, history=2)
    new = info["selections"][0]
    assert new.box is not None
    tsel = _carried(t, planes[0])
    s.clone_selection(new, (3, -4))
    t.clone_selection(tsel, (3, -4))
    assert np.array_equal(s.frame(), t.frame()) and not np.array_equal(s.frame(), want)
    s.filter_selection(new, kind="blur", radius=3, feather=2)
    t.filter_selection(tsel, kind="blur", radius=3, feather=2)
    assert np.array_equal(s.frame(), t.frame())
    s.undo()
    s.undo()
    assert np.array_equal(s.frame(), want) and np.array_equal(s.lock(), want_lock)
    s.undo()                                                               # the canvas step itself
    assert s.frame_hw == FHW and np.array_equal(fb.get(), f) and np.array_equal(s.lock(), lock) and not s.can_undo


def test_session_undo_and_redo_across_edit_canvas_edit(model):
    f, _ = _blob_frame()
    lock = _lock_plane()
    s, fb = _session(model, f, lock, history=4)
    sk = np.zeros(FHW, np.uint8)
    sk[40:44, 20:80] = 255
    sk[30:90, 50:53] = 255
    s.edit(sk, max_grow=0, low_latency=False)
    f1 = s.frame()
    _, _, info = s.canvas(orient="ccw", rect=(-6, 8, 112, 100), pad="reflect")
    f2, l2 = s.frame(), s.lock()
    assert s.frame_hw == (112, 100) and np.array_equal(f2, C.spec_canvas(f1, FHW, (112, 100), (-6, 8), 5, C.REFLECT))
    mask = np.zeros((112, 100), np.uint8)
    mask[30:60, 20:70] = 255
    s.fill(mask, low_latency=False)
    f3 = s.frame()
    assert not np.array_equal(f1, f) and not np.array_equal(f3, f2)
    s.undo()
    assert np.array_equal(s.frame(), f2)
    assert s.undo() == (None, (0, 0), dict(canvas=FHW, undo_depth=1, redo_depth=2))
    assert s.frame_hw == FHW and np.array_equal(s.frame(), f1) and np.array_equal(s.lock(), lock) and np.array_equal(fb.get(), f1)
    s.undo()
    assert np.array_equal(fb.get(), f) and not s.can_undo
    s.redo()
    assert np.array_equal(fb.get(), f1)
    assert s.redo() == (None, (0, 0), dict(canvas=(112, 100), undo_depth=2, redo_depth=1))
    assert s.frame_hw == (112, 100) and np.array_equal(s.frame(), f2) and np.array_equal(s.lock(), l2)
    s.redo()
    assert np.array_equal(s.frame(), f3) and not s.can_redo


def test_session_encode_forms_after_a_crop(model):
    f, _ = _blob_frame()
    s, _ = _session(model, f, None)
    s.crop_canvas((7, 9, 96, 80))
    t = serve.EditSession(model, np.ascontiguousarray(f[7:103, 9:89]))
    assert np.array_equal(s.frame(), t.frame())
    assert s.frame_png() == t.frame_png() and s.frame_png((5, 3, 64, 48)) == t.frame_png((5, 3, 64, 48))
    assert s.frame_jpg(quality=90) == t.frame_jpg(quality=90)
    assert s.frame_jpg((8, 8, 32, 48), quality=75, subsampling="420", optimize=True) == t.frame_jpg((8, 8, 32, 48), quality=75, subsampling="420", optimize=True)
    mask = np.zeros((96, 80), np.uint8)
    mask[20:40, 10:50] = 255
    for encode in ("png", ("jpg", 80)):
        a, _, ia = s.fill(mask, low_latency=False, encode=encode)
        b, _, ib = t.fill(mask, low_latency=False, encode=encode)
        assert isinstance(a, bytes) and a == b and ia["window"] == ib["window"]


# ---- 3. the outpaint ----------------------------------------------------------------------------------------------------------------------------
def _edge_lock():
    lock = np.zeros(FHW, np.uint8)
    lock[40:80, 90:] = 255                                               # touches the old right edge
    lock[::11, ::5] = 255
    return lock


@pytest.mark.parametrize("case", [dict(), dict(max_side=64), dict(locked=True), dict(locked=True, feather=3, encode="png")],
                         ids=lambda c: "-".join("%s=%s" % kv for kv in sorted(c.items())) or "plain")
def test_outpaint_is_extend_then_fill_in_one_undo_step(model, case):
    case = dict(case)
    lock = _edge_lock() if case.pop("locked", False) else None
    encode = case.pop("encode", None)
    f, _ = _blob_frame()
    s, fb = _session(model, f, lock, history=2)
    t, _ = _session(model, f, lock, history=2)
    ext = dict(right=24, bottom=8, pad="reflect")
    patch, pos, info = s.extend_canvas(fill="network", low_latency=False, encode=encode, **ext, **case)
    new_hw = (FHW[0] + 8, FHW[1] + 24)
    t.extend_canvas(**ext)
    padded = t.frame()
    area = C.spec_canvas(None, FHW, new_hw, (0, 0), 0, C.CONSTANT, 255)
    tp, tpos, ti = t.fill(area, low_latency=False, encode=encode, **case)
    after = s.frame()
    assert s.frame_hw == new_hw == t.frame_hw and np.array_equal(after, t.frame()) and not np.array_equal(after, padded)
    assert np.array_equal(after[:FHW[0], :FHW[1]], f)                     # only the new area can change
    assert info["window"] == ti["window"] and pos == tpos and info["fill"] is True and info.get("work") == ti.get("work")
    assert (patch == tp) if encode else np.array_equal(patch, tp)
    assert info["canvas"] == new_hw and info["previous"] == FHW and info["undoable"] is True and info["locked"] == (lock is not None)
    if lock is not None:
        assert np.array_equal(s.lock(), C.spec_canvas(lock, FHW, new_hw, (0, 0), 0, C.CONSTANT, 0))
    assert len(s._undo) == 1 and len(t._undo) == 2                         # ONE undo step
    assert s.undo() == (None, (0, 0), dict(canvas=FHW, undo_depth=0, redo_depth=1))
    assert s.frame_hw == FHW and np.array_equal(fb.get(), f) and (lock is None or np.array_equal(s.lock(), lock))
    s.redo()
    assert s.frame_hw == new_hw and np.array_equal(s.frame(), after)
