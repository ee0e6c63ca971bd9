"""GPU tests of scaling and rotating a selection: the two kernels of se_warp.hip against the statement of
tests/warp_util.py on whole buffers between sentinels, at every alignment, and EditSession.transform_selection against a
two-step route -- fill_selection of the grown selection on a twin session, then the statement's drop applied on the host with
the original pixels.  Every comparison is exact."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from sketchedit_amd import _lib, serve
import lasso_util as L
import move_util as M
import warp_util as W
from test_gpu_lasso import FHW, GARBAGE, HOLE, RING, _Buf, _blob_frame, _cuda, _lock_plane, _session, eng, model  # noqa: F401
from test_gpu_move import PATTERNS, _Slot, _case

pytestmark = pytest.mark.gpu

ID = 65536
GROUPS = ("shifts", "flips_turns", "scales", "angles", "edges")
NAMES = sorted(PATTERNS)


def _limit_map(sel, box):
    """the coefficient limit itself (a 16-fold reduction with a turn): destination pixel (5, 5) takes the source position half a
    pixel past a selected pixel of the box in both axes"""
    by0, bx0, by1, bx1 = box
    ys, xs = np.nonzero(sel[by0:by1 - 1, bx0:bx1 - 1])
    qy, qx = int(ys[len(ys) // 2]) + by0, int(xs[len(xs) // 2]) + bx0
    return (W.MAX_COEF, -W.MAX_COEF, (qy << 16) + 0x8000, W.MAX_COEF, W.MAX_COEF, (qx << 16) + 0x8000 - 10 * W.MAX_COEF)


@functools.lru_cache(maxsize=None)
def _maps(group, name, hw):
    """the group's cases for a pattern and a size -> [(m, R, integer offset or None)]; R None: the frame (nothing lands in it)"""
    Hi, Wi = hw
    _, _, sel, _, box, _, _ = _case(name, hw)
    by0, bx0, by1, bx1 = box
    h, w = by1 - by0, bx1 - bx0
    wm = lambda *a: W.warp_matrix(box, *a)                                  # noqa: E731  (scale, angle, offset, flip bits)
    out = []
    if group == "shifts":
        for off in ((0, 0), (1, -1), (h // 3, -(w // 4)), (-by0 - h // 2, 2), (2, Wi - bx0 - w // 2)):
            out.append((wm(1.0, 0.0, off, 0), None, off))
        out += [(wm(1.0, 0.0, o, 0), None, None) for o in ((0.5, 0), (0, 0.5), (-0.5, 1.5))]
    elif group == "flips_turns":
        out += [(wm(1.0, 0.0, (1, 0.5), f), None, None) for f in range(4)]
        out += [(wm(1.0, float(a), (0, 0), 0), None, None) for a in (90, 180, 270)] + [(wm(1.0, 90.0, (0.5, 0.5), 1), None, None)]
    elif group == "scales":
        out += [(wm(s, 0.0, (0, 0), 0), None, None) for s in (0.125, 0.5, 1.5, 2.0, 8.0)]
        out.append((wm(0.5, 0.0, (0.5, 0.5), 0), None, None))              # a rim between the grid's steps, also of a full frame
    elif group == "angles":
        out += [(wm(1.0, 30.0, (0, 0), 0), None, None), (wm(1.0, 45.0, (1, -2), 2), None, None), (wm((0.75, 1.5), 20.0, (0.5, 0), 0), None, None),
                ((70000, 9000, (by0 << 16) - 200000, -12000, 50000, (bx0 << 16) + 300000), None, None),            # a raw sheared matrix
                (_limit_map(sel, box), None, None),
                (wm(1.5, 30.0, (0, 0), 0), (Hi - 16, 0, 16, 16), None)]                                            # an R that cuts the object
    else:
        for off in ((-by0 - h // 2, 0), (Hi - by0 - h // 2, 0.5), (0, -bx0 - w // 2), (0.5, Wi - bx0 - w // 2), (-by0 - h // 2, Wi - bx0 - w // 2)):
            out.append((wm(1.5, 30.0, off, 0), None, None))
        out.append(((ID, 0, 4 * Hi << 16, 0, ID, 0), None, None))                                                  # valid, and nothing lands
    return [(m, R or W.warp_rect(box, m, hw), off) for m, R, off in out]


def test_the_cases_are_not_vacuous():
    """conditions on the inputs, from the statement alone: in every group and at every size some case changes bytes and some
    case has a partly covered pixel; the last case of `edges` lands nothing"""
    for hw in L.SIZES:
        for g, group in enumerate(GROUPS):
            name = NAMES[(g + hw[0]) % 4]
            frame, _, sel, _, box, rect, slot = _case(name, hw)
            changes = partial = 0
            for m, R, _ in _maps(group, name, hw):
                a = W.coverage(sel, box, m)
                partial += int(((a > 0) & (a < ID)).any())
                if R is not None:
                    changes += int(not np.array_equal(W.spec_drop(frame, slot, rect, sel, None, box, R, m), frame))
            assert changes >= 3 and partial >= 1, (hw, group, changes, partial)
        assert _maps("edges", name, hw)[-1][1] is None
        m = _limit_map(sel, box)
        assert max(abs(v) for v in m[:2] + m[3:5]) == W.MAX_COEF and W.coverage(sel, box, m)[5, 5] > 0


# ---- 1. the drop and the warp: every group of maps at every size and alignment ---------------------------------------------------------------
@pytest.mark.parametrize("hw", L.SIZES, ids=lambda hw: "%dx%d" % hw)
@pytest.mark.parametrize("group", GROUPS)
def test_drop_and_warp_follow_the_statement(eng, hw, group):
    Hi, Wi = hw
    name = NAMES[(GROUPS.index(group) + Hi) % 4]
    frame, _, sel, lock, box, rect, slot = _case(name, hw)
    sb, lb, pb = _Buf(hw, 1, like=sel), _Buf(hw, 3, like=lock), _Slot(slot)                    # planes at odd offsets
    changed = 0
    for k, (m, R, off) in enumerate(_maps(group, name, hw)):
        R = R or (0, 0, Hi, Wi)
        for locked in (False, True):
            fb = _Buf(frame.shape, (k + locked) % 4, like=frame)                                # the frame at every byte offset mod 4
            eng.warp_drop_u8(fb.view, pb.view, rect, sb.view, lb.view if locked else None, box, R, m)
            got = fb.get()
            want = W.spec_drop(frame, slot, rect, sel, lock if locked else None, box, R, m)
            assert np.array_equal(got, want), (name, hw, m, R, locked, int((got != want).sum()))
            changed += int((got != frame).any())
            if off is not None:                                                                 # identity: ALSO the move's drop at r = 0
                tb = _Buf(frame.shape, (k + locked + 2) % 4, like=frame)
                eng.move_drop_u8(tb.view, pb.view, rect, sb.view, lb.view if locked else None, box, off, flip=0, radius=0)
                assert np.array_equal(tb.get(), got), (name, hw, off, locked)
        ob = _Buf(hw, k % 4, fill=GARBAGE)                                                      # every byte must be written
        eng.plane_warp_u8(sb.view, box, m, out=ob.view)
        got, want = ob.get(), W.spec_warp(sel, box, m)
        assert np.array_equal(got, want), (name, hw, m, int((got != want).sum()))
    assert np.array_equal(sb.get(), sel) and np.array_equal(lb.get(), lock) and pb.intact()
    assert changed >= 6


def test_known_answers_and_overlap(eng):
    frame = np.full((16, 16, 3), 10, np.uint8)
    slot = M.slot_of(np.full((16, 16, 3), 200, np.uint8), (0, 0, 16, 16))
    sel = np.zeros((16, 16), np.uint8)
    sel[2:4, 2:4] = 1
    for m, patch, plane_rows in (((ID, 0, 0, 0, ID, -32768), [[105, 200, 105]] * 2, [[1, 1, 1]] * 2),
                                 ((ID, 0, -32768, 0, ID, -32768), [[58, 105, 58], [105, 200, 105], [58, 105, 58]], [[0, 1, 0], [1, 1, 1], [0, 1, 0]])):
        fb, pb = _Buf(frame.shape, 2, like=frame), _Slot(slot)
        eng.warp_drop_u8(fb.view, pb.view, (0, 0, 16, 16), _cuda(sel), None, (2, 2, 4, 4), (0, 0, 16, 16), m)
        want = frame.copy()
        want[2:2 + len(patch), 2:5] = np.array(patch, np.uint8)[..., None]
        assert np.array_equal(fb.get(), want)
        plane = np.zeros((16, 16), np.uint8)
        plane[2:2 + len(patch), 2:5] = np.array(plane_rows, np.uint8) * 255
        assert np.array_equal(eng.plane_warp_u8(_cuda(sel), (2, 2, 4, 4), m).cpu().numpy(), plane)
    # source and destination overlap: the object's pixels come from the lift, never from the frame it is written into
    f, _, sel, _, box, rect, _ = _case("full", (65, 129))
    fb, pb = _Buf(f.shape, 1, like=f), _Slot(M.slot_of(f, rect))
    m = W.warp_matrix(box, 1.0, 0.0, (3, 5.5), 0)
    eng.warp_drop_u8(fb.view, pb.view, rect, _cuda(sel), None, box, (0, 0, 65, 129), m)
    assert np.array_equal(fb.get(), W.spec_drop(f, M.slot_of(f, rect), rect, sel, None, box, (0, 0, 65, 129), m))


# ---- 2. both again with every scratch byte poisoned ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(37, 53), (130, 70)], ids=lambda hw: "%dx%d" % hw)
def test_drop_and_warp_under_poison(eng, seopt, hw):
    seopt.set("SE_TEST_POISON", 0xFF)
    frame, _, sel, lock, box, rect, slot = _case("disc", hw)
    sb, lb, pb = _Buf(hw, 1, like=sel), _Buf(hw, 3, like=lock), _Slot(slot)
    cases = [_maps(g, "disc", hw)[i] for g, i in (("shifts", 5), ("flips_turns", 4), ("scales", 2), ("angles", 2), ("edges", 4), ("edges", 5))]
    for k, (m, R, _) in enumerate(cases):
        R = R or (0, 0) + hw
        fb, ob = _Buf(frame.shape, k % 4, like=frame), _Buf(hw, (k + 1) % 4, fill=GARBAGE)
        eng.warp_drop_u8(fb.view, pb.view, rect, sb.view, lb.view, box, R, m)
        eng.plane_warp_u8(sb.view, box, m, out=ob.view)
        assert np.array_equal(fb.get(), W.spec_drop(frame, slot, rect, sel, lock, box, R, m)), (hw, m)
        assert np.array_equal(ob.get(), W.spec_warp(sel, box, m)), (hw, m)
    assert np.array_equal(sb.get(), sel) and np.array_equal(lb.get(), lock) and pb.intact()


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(eng):
    Hi, Wi = 37, 53
    frame, _, sel, lock, box, rect, slot = _case("disc", (Hi, Wi))
    fb, sb, lb, pb, ob = (_Buf(frame.shape, 1, like=frame), _Buf((Hi, Wi), 1, like=sel), _Buf((Hi, Wi), 2, like=lock), _Slot(slot),
                          _Buf((Hi, Wi), 3, fill=GARBAGE))
    lib, h, st = eng.lib, eng.h, eng._stream()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else t)     # noqa: E731
    q = lambda m: None if m is None else (ctypes.c_longlong * 6)(*m)                                        # noqa: E731
    F, S, K, P, OUT = fb.view, sb.view, lb.view, pb.view, ob.view
    by0, bx0, by1, bx1 = box
    ly0, lx0, lh, lw = rect
    good = W.warp_matrix(box, 1.5, 30.0, (1, -2), 1)
    setm = lambda i, v: tuple(v if j == i else x for j, x in enumerate(good))                                # noqa: E731
    ok = dict(F=F, Hi=Hi, Wi=Wi, P=P, ly0=ly0, lx0=lx0, lh=lh, lw=lw, S=S, K=K, by0=by0, bx0=bx0, by1=by1, bx1=bx1, ry0=3, rx0=5, rh=20, rw=30, m=good)
    inside_frame = F.data_ptr() + 3 * Hi * Wi - 1                          # begins on the frame's last byte
    maps = [(dict(m=None), "null pointer argument: m"), (dict(m=setm(0, W.MAX_COEF + 1)), "ayy"), (dict(m=setm(1, -W.MAX_COEF - 1)), "ayx"),
            (dict(m=setm(3, W.MAX_COEF + 1)), "axy"), (dict(m=setm(4, -(1 << 62))), "axx"), (dict(m=setm(2, W.MAX_TRANSLATION + 1)), "ay0"),
            (dict(m=setm(5, -W.MAX_TRANSLATION - 1)), "ax0")]
    drops = [(dict(F=None), "frame_u8"), (dict(P=None), "lift"), (dict(S=None), "sel_u8"), (dict(Hi=15), "Hi"), (dict(Wi=15), "Wi"),
             (dict(lh=15), "lift rectangle"), (dict(lw=15), "lift rectangle"), (dict(ly0=-1), "lift rectangle"), (dict(lx0=Wi - lw + 1), "lift rectangle"),
             (dict(ly0=Hi - lh + 1), "lift rectangle"), (dict(P=P.data_ptr() + 8), "16-byte aligned"), (dict(by1=by0), "box"), (dict(bx1=bx0), "box"),
             (dict(by0=ly0 - 1), "lies outside the lift rectangle"), (dict(bx1=lx0 + lw + 1), "lies outside the lift rectangle"),
             (dict(by1=ly0 + lh + 1), "lies outside the lift rectangle"),
             (dict(rh=0), "destination rectangle"), (dict(rw=0), "destination rectangle"), (dict(rh=-4), "destination rectangle"),
             (dict(ry0=-1), "destination rectangle"), (dict(rx0=-1), "destination rectangle"), (dict(ry0=Hi - 19), "destination rectangle"),
             (dict(rx0=Wi - 29), "destination rectangle"), (dict(rh=Hi + 1, ry0=0), "destination rectangle"), (dict(rw=Wi + 1, rx0=0), "destination rectangle"),
             (dict(S=inside_frame), "sel_u8 overlaps"), (dict(K=F.data_ptr() - Hi * Wi + 1), "lock_u8 overlaps"),
             (dict(P=(F.data_ptr() + 16) // 16 * 16), "lift overlaps")] + maps
    for change, what in drops:
        a = dict(ok, **change)
        rc = lib.se_warp_drop_u8(h, st, p(a["F"]), a["Hi"], a["Wi"], p(a["P"]), a["ly0"], a["lx0"], a["lh"], a["lw"], p(a["S"]), p(a["K"]),
                                 a["by0"], a["bx0"], a["by1"], a["bx1"], a["ry0"], a["rx0"], a["rh"], a["rw"], q(a["m"]))
        assert rc != 0, (change, what)
        assert what in lib.se_last_error(h).decode(), (what, lib.se_last_error(h).decode())
    wok = dict(S=S, Hi=Hi, Wi=Wi, by0=by0, bx0=bx0, by1=by1, bx1=bx1, m=good, O=OUT)
    warps = [(dict(S=None), "sel_u8"), (dict(O=None), "plane_out"), (dict(Hi=15), "Hi"), (dict(Wi=15), "Wi"), (dict(by1=by0), "box"), (dict(bx1=bx0), "box"),
             (dict(by0=-1), "lies outside the frame"), (dict(bx1=Wi + 1), "lies outside the frame"), (dict(O=S), "plane_out overlaps"),
             (dict(O=S.data_ptr() + Hi * Wi - 1), "plane_out overlaps"), (dict(O=S.data_ptr() - Hi * Wi + 1), "plane_out overlaps")] + maps
    for change, what in warps:
        a = dict(wok, **change)
        rc = lib.se_plane_warp_u8(h, st, p(a["S"]), a["Hi"], a["Wi"], a["by0"], a["bx0"], a["by1"], a["bx1"], q(a["m"]), p(a["O"]))
        assert rc != 0, (change, what)
        assert what in lib.se_last_error(h).decode(), (what, lib.se_last_error(h).decode())
    # the bindings refuse planes and lifts of another shape or size, and maps that are not six ints
    R = (3, 5, 20, 30)
    for call in (lambda: eng.warp_drop_u8(F.view(-1), P, rect, S, None, box, R, good), lambda: eng.warp_drop_u8(F, P, rect, S.view(Wi, Hi), None, box, R, good),
                 lambda: eng.warp_drop_u8(F, P, rect, S, K.view(Wi, Hi), box, R, good), lambda: eng.warp_drop_u8(F, P[:-1], rect, S, None, box, R, good),
                 lambda: eng.warp_drop_u8(F, P, rect, S, None, box, R, good[:5]), lambda: eng.warp_drop_u8(F, P, rect, S, None, box, R, None),
                 lambda: eng.warp_drop_u8(F, P, rect, S, None, box, R, setm(2, 1 << 63)), lambda: eng.warp_drop_u8(F, P, rect, S, None, box, R, setm(0, W.MAX_COEF + 1)),
                 lambda: eng.plane_warp_u8(S, box, good, out=OUT.view(Wi, Hi)), lambda: eng.plane_warp_u8(S.view(-1), box, good),
                 lambda: eng.plane_warp_u8(S, box, good + (0,), out=OUT), lambda: eng.plane_warp_u8(S, box, setm(5, W.MAX_TRANSLATION + 1), out=OUT)):
        with pytest.raises(_lib.SketchEditHipError):
            call()
    # valid, and nothing to do: the map lands nothing in R
    eng.warp_drop_u8(F, P, rect, S, K, box, R, (ID, 0, 4 * Hi << 16, 0, ID, 0))
    torch.cuda.synchronize()
    assert np.array_equal(fb.get(), frame) and np.array_equal(sb.get(), sel) and np.array_equal(lb.get(), lock) and pb.intact()
    assert (ob.get() == GARBAGE).all()
    eng.plane_warp_u8(S, box, (ID, 0, 4 * Hi << 16, 0, ID, 0), out=OUT)
    assert not ob.get().any()


# ---- 4. sessions ------------------------------------------------------------------------------------------------------------------------------
SESSION_CASES = [dict(), dict(locked=True), dict(max_side=64), dict(keep_source=True, flip="hv", locked=True), dict(hole_grow=0, feather=3),
                 dict(hole_grow=5, angle=-45.0, locked=True), dict(window=(16, 8, 96, 88), scale=(0.75, 1.25), max_side=64, feather=4, locked=True),
                 dict(scale=3.0, angle=15.0, offset=(-20, 30.5)),                                # scaled up: clipped by the frame
                 dict(matrix=(70000, 9000, -1200000, -12000, 50000, 1500000), keep_source=True)]


@pytest.mark.parametrize("poison", [0, 0xFF])
@pytest.mark.parametrize("case", SESSION_CASES, ids=lambda c: "-".join("%s=%s" % (k, "m" if k == "matrix" else v) for k, v in sorted(c.items())) or "defaults")
def test_session_transform_is_fill_then_the_statements_drop(model, seopt, case, poison):
    """a twin session fills the grown selection through the same window in the same mode, the statement drops the ORIGINAL pixels
    on the host: every byte of the frame, its sentinel margins included, is equal; one undo restores every byte, one redo puts
    them back; the returned selection is the statement's plane, box and count, and its rings re-make it"""
    case = dict(case)
    f, _ = _blob_frame()
    lock = _lock_plane() if case.pop("locked", False) else None
    if "matrix" not in case:
        case.setdefault("scale", 1.5)
        case.setdefault("angle", 30.0)
        case.setdefault("offset", (7, -9.5))                              # the destination overlaps the source
    keep, hole_grow = case.get("keep_source", False), case.get("hole_grow", 2)
    if poison:
        seopt.set("SE_TEST_POISON", poison)
    a, abuf = _session(model, f, lock, history=2)
    b, bbuf = _session(model, f, lock, history=2)
    sel = a.select_lasso([RING, HOLE])
    plane = L.spec_select_lasso([RING, HOLE], FHW, 0)
    box = L.box_count(plane)[0]
    patches, positions, info = a.transform_selection(sel, low_latency=False, **case)
    m = case["matrix"] if "matrix" in case else W.warp_matrix(box, case["scale"], case["angle"], case["offset"], serve.MOVE_FLIPS[case.get("flip")])
    dst = W.warp_rect(box, m, FHW)
    wins = info["windows"]
    assert info["matrix"] == m and wins[-1] == dst and len(wins) == (1 if keep else 2) and positions == [(w[1], w[0]) for w in wins]
    if not keep:
        grown = (max(box[0] - hole_grow, 0), max(box[1] - hole_grow, 0), min(box[2] + hole_grow, FHW[0]), min(box[3] + hole_grow, FHW[1]))
        assert wins[0] == (case["window"] if "window" in case else serve.choose_window(grown, FHW, margin=0.5))
        fill = {k: case[k] for k in ("max_side", "feather") if k in case}
        _, _, ib = b.fill_selection(b.select_lasso([RING, HOLE], grow=hole_grow), window=wins[0], low_latency=False, **fill)
        assert info.get("work") == ib.get("work")
    rect = M.move_rect(box, (0, 0), FHW)
    want = W.spec_drop(bbuf.get(), M.slot_of(f, rect), rect, plane, lock, box, dst, m)
    after = abuf.get()                                                   # (checks the margins)
    assert np.array_equal(after, want) and not np.array_equal(after, f)
    assert np.array_equal(want, W.spec_drop(bbuf.get(), M.slot_of(f, rect), rect, plane, lock, box, (0, 0) + FHW, m))    # warp_rect lost nothing
    for pch, w in zip(patches, wins):
        assert np.array_equal(pch, after[w[0]:w[0] + w[2], w[1]:w[1] + w[3]])
    if lock is not None:
        assert np.array_equal(after[lock != 0], f[lock != 0]) and info["locked"] is True
    assert info["transform"] is True and info["selected"] == sel.count and info["undoable"] is True
    warped = info["selection"]
    spec = W.spec_warp(plane, box, m)
    assert np.array_equal(warped.plane.cpu().numpy(), spec) and (warped.box, warped.count) == L.box_count(spec) and warped.count > 0
    assert np.array_equal(sel.plane.cpu().numpy(), plane) and sel.box == box
    again = a.select_lasso(warped.rings())
    assert np.array_equal(again.plane.cpu().numpy(), spec) and (again.box, again.count) == (warped.box, warped.count)
    a.undo()
    assert np.array_equal(abuf.get(), f) and not a.can_undo
    a.redo()
    assert np.array_equal(abuf.get(), after) and not a.can_redo


def test_session_transform_encode_forms_and_refusal(model):
    f, _ = _blob_frame()
    for encode, ref in (("png", lambda s, w: s.frame_png(w)), (("jpg", 90), lambda s, w: s.frame_jpg(w, quality=90)),
                        (("jpg", 75, "420", True), lambda s, w: s.frame_jpg(w, quality=75, subsampling="420", optimize=True))):
        s, fb = _session(model, f, _lock_plane(), history=1)
        sel = s.select_lasso([RING])
        patches, _, info = s.transform_selection(sel, scale=0.75, angle=20.0, offset=(6, 11), encode=encode, low_latency=False)
        assert len(patches) == 2 and all(isinstance(p, bytes) for p in patches)
        assert patches == [ref(s, w) for w in info["windows"]], encode
        s.undo()
        assert np.array_equal(fb.get(), f)
    with pytest.raises(ValueError, match="puts nothing of the selection in the frame"):
        s.transform_selection(sel, offset=(300, 0))
    assert np.array_equal(fb.get(), f) and not s.can_undo
