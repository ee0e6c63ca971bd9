"""GPU tests of blurring, sharpening and pixelating a selection: the two kernels of se_filter.hip against the
statement of tests/filter_util.py on whole buffers between sentinels, at every alignment, and EditSession.filter_selection
against the statement applied on the host to the original frame.  Every comparison is exact."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from sketchedit_amd import _lib, serve
import filter_util as F
import lasso_util as L
import move_util as M
import select_util as U
from test_gpu_lasso import FHW, HOLE, RING, _Buf, _blob_frame, _cuda, _lock_plane, _session, eng, model  # noqa: F401
from test_gpu_move import PATTERNS, _Slot

pytestmark = pytest.mark.gpu

RADII = (1, 2, 7, 16, 32)
CELLS = (2, 3, 5, 16, 64)
AMOUNTS = (-128, 256, 1024)
FEATHERS = (1, 7, 16)
SHARPEN_R = 2


@functools.lru_cache(maxsize=None)
def _case(name, hw, R):
    """(frame, the frame as it was lifted, selection plane, lock plane, box, lift rectangle, slot) for a filter of radius R (0: the
    mosaic): computed once, shared, read-only"""
    Hi, Wi = hw
    rng = np.random.RandomState(Hi * 1000 + Wi)
    frame, before = U._noise(hw, 3), U._noise(hw, 4)
    sel = np.ascontiguousarray(PATTERNS[name](Hi, Wi), np.uint8)
    lock = np.where(rng.rand(Hi, Wi) < 0.25, rng.randint(1, 256, hw), 0).astype(np.uint8)
    if name == "noise":                                                  # a box strictly inside the selected pixels: those outside stay
        box = (2, 3, Hi - 4, Wi - 2)
        rect = (0, 0, Hi, Wi)                                            # and a lift larger than the filter needs
    else:
        box = M.box_of(sel)
        rect = F.filter_rect(box, R, hw)
    slot = M.slot_of(before, rect)
    for a in (frame, before, sel, lock, slot):
        a.setflags(write=False)
    return frame, before, sel, lock, box, rect, slot


class _Dev:
    """a case's planes at odd offsets and its slot, on the device once"""

    def __init__(self, case):
        _, _, sel, lock, _, _, slot = case
        self.sel, self.lock = sel, lock
        self.sb, self.lb, self.pb = _Buf(sel.shape, 1, like=sel), _Buf(sel.shape, 3, like=lock), _Slot(slot)

    def intact(self):
        return np.array_equal(self.sb.get(), self.sel) and np.array_equal(self.lb.get(), self.lock) and self.pb.intact()


def _run_blur(eng, case, dev, k, locked, t, a, f):
    frame, _, sel, lock, box, rect, slot = case
    fb = _Buf(frame.shape, k % 4, like=frame)                            # the frame at every byte offset mod 4
    eng.filter_blur_u8(fb.view, dev.pb.view, rect, dev.sb.view, dev.lb.view if locked else None, box, t, amount=a, feather=f)
    got = fb.get()                                                       # (checks the margins)
    want = F.spec_blur(frame, slot, rect, sel, lock if locked else None, box, t, a, f)
    assert np.array_equal(got, want), (frame.shape, box, len(t) - 1, a, f, locked, int((got != want).sum()))
    return int((got != frame).any())


def _run_mosaic(eng, case, dev, k, locked, cell, a, f):
    frame, _, sel, lock, box, rect, slot = case
    fb = _Buf(frame.shape, k % 4, like=frame)
    eng.filter_mosaic_u8(fb.view, dev.pb.view, rect, dev.sb.view, dev.lb.view if locked else None, box, cell, amount=a, feather=f)
    got = fb.get()
    want = F.spec_mosaic(frame, slot, rect, sel, lock if locked else None, box, cell, a, f)
    assert np.array_equal(got, want), (frame.shape, box, cell, a, f, locked, int((got != want).sum()))
    return int((got != frame).any())


# ---- 1. the four groups at every size, pattern and alignment ---------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", L.SIZES, ids=lambda hw: "%dx%d" % hw)
@pytest.mark.parametrize("R", RADII)
def test_blur_follows_the_statement(eng, hw, R):
    k = changed = 0
    for name in sorted(PATTERNS):
        case = _case(name, hw, R)
        dev = _Dev(case)
        for kind in ("gauss", "box"):
            for locked in (False, True):
                changed += _run_blur(eng, case, dev, k, locked, F.taps(kind, R), -256, 0)
                k += 1
        assert dev.intact()
    assert changed == k


@pytest.mark.parametrize("hw", L.SIZES, ids=lambda hw: "%dx%d" % hw)
@pytest.mark.parametrize("a", AMOUNTS)
def test_sharpen_follows_the_statement(eng, hw, a):
    k = changed = 0
    for name in sorted(PATTERNS):
        case = _case(name, hw, SHARPEN_R)
        dev = _Dev(case)
        for locked in (False, True):
            changed += _run_blur(eng, case, dev, k + 1, locked, F.taps("gauss", SHARPEN_R), a, 0)
            k += 1
        assert dev.intact()
    assert changed == k


@pytest.mark.parametrize("hw", L.SIZES, ids=lambda hw: "%dx%d" % hw)
@pytest.mark.parametrize("cell", CELLS)
def test_mosaic_follows_the_statement(eng, hw, cell):
    k = changed = 0
    for name in sorted(PATTERNS):
        case = _case(name, hw, 0)
        dev = _Dev(case)
        for locked in (False, True):
            changed += _run_mosaic(eng, case, dev, k + 2, locked, cell, (-256, 256)[k % 2], 0)
            k += 1
        assert dev.intact()
    assert changed == k


@pytest.mark.parametrize("hw", L.SIZES, ids=lambda hw: "%dx%d" % hw)
@pytest.mark.parametrize("f", FEATHERS)
def test_feather_follows_the_statement(eng, hw, f):
    k = changed = 0
    for name in sorted(PATTERNS):
        case, case0 = _case(name, hw, 7), _case(name, hw, 0)
        dev, dev0 = _Dev(case), _Dev(case0)
        for locked in (False, True):
            changed += _run_blur(eng, case, dev, k + 3, locked, F.taps("gauss", 7), -256, f)
            changed += _run_mosaic(eng, case0, dev0, k, locked, 5, -256, f)
            k += 1
        assert dev.intact() and dev0.intact()
    assert changed == 2 * k


@pytest.mark.parametrize("hw", L.SIZES, ids=lambda hw: "%dx%d" % hw)
def test_the_inputs_exercise_the_rule(hw):
    """of the inputs alone, from the CPU statement: every group changes bytes, the sharpen group clamps at 0 and at 255, the
    feather group has a pixel with 0 < c < n"""
    for name in sorted(PATTERNS):
        frame, before, sel, lock, box, rect, slot = _case(name, hw, SHARPEN_R)
        by0, bx0, by1, bx1 = box
        tg = np.zeros(hw, bool)
        tg[by0:by1, bx0:bx1] = sel[by0:by1, bx0:bx1] != 0
        assert tg.sum() >= 40
        for locked in (None, lock):
            for a in AMOUNTS:
                out = F.spec_blur(frame, slot, rect, sel, locked, box, F.taps("gauss", SHARPEN_R), a)
                t2 = tg if locked is None else tg & (lock == 0)
                assert (out != frame).any()
                if a > 0:
                    assert (out[t2] == 0).sum() >= 5 and (out[t2] == 255).sum() >= 5, (name, hw, a)
        for R in RADII:
            c = _case(name, hw, R)
            for kind in ("gauss", "box"):
                assert (F.spec_blur(c[0], c[6], c[5], sel, lock, box, F.taps(kind, R)) != frame).any()
        c0 = _case(name, hw, 0)
        for cell in CELLS:
            assert (F.spec_mosaic(frame, c0[6], c0[5], sel, lock, box, cell) != frame).any()
        for f in FEATHERS:
            cnt = F.counts(sel, box, f)[tg[by0:by1, bx0:bx1]]
            n = (2 * f + 1) ** 2
            assert cnt.min() >= 1 and (cnt < n).any(), (name, hw, f)


# ---- 2. further runs ----------------------------------------------------------------------------------------------------------------------
def test_the_all_255_frame_at_radius_32(eng):
    """255 * 2^24 + 2^23 in the vertical sum: a signed accumulator overflows"""
    for hw in ((37, 53), (100, 90)):
        P = np.full(hw + (3,), 255, np.uint8)
        rect = (0, 0) + hw
        sel = np.full(hw, 9, np.uint8)
        for k, t in enumerate((F.taps("box", 32), F.taps("gauss", 32), [0] * 32 + [2048])):
            fb, pb = _Buf(P.shape, k, fill=0), _Slot(M.slot_of(P, rect))
            eng.filter_blur_u8(fb.view, pb.view, rect, _cuda(sel), None, rect[:2] + hw, t)
            assert (fb.get() == 255).all(), (hw, k)
            fb = _Buf(P.shape, k + 1, fill=0)
            eng.filter_blur_u8(fb.view, pb.view, rect, _cuda(sel), None, rect[:2] + hw, t, amount=1024, feather=3)
            assert (fb.get() == 255).all(), (hw, k)


@pytest.mark.parametrize("box", [(20, 30, 40, 80), (0, 0, 20, 30), (45, 100, 65, 129), (0, 70, 65, 129)], ids=str)
def test_interior_and_edge_boxes(eng, box):
    """a box in the interior, whose taps read unselected lift pixels outside it, and boxes that touch two or three edges: the clamp"""
    hw = (65, 129)
    frame, before = U._noise(hw, 3), U._noise(hw, 4)
    sel = PATTERNS["noise"](*hw)
    lock = np.where(np.random.RandomState(5).rand(*hw) < 0.2, 255, 0).astype(np.uint8)
    sb, lb = _Buf(hw, 1, like=sel), _Buf(hw, 3, like=lock)
    k = 0
    for R in (3, 16, 32):
        rect = F.filter_rect(box, R, hw)
        slot = M.slot_of(before, rect)
        pb = _Slot(slot)
        for f in (0, 4):
            for locked in (False, True):
                fb = _Buf(frame.shape, k % 4, like=frame)
                t = F.taps(("gauss", "box")[k % 2], R)
                eng.filter_blur_u8(fb.view, pb.view, rect, sb.view, lb.view if locked else None, box, t, amount=(-256, 512)[k % 2], feather=f)
                want = F.spec_blur(frame, slot, rect, sel, lock if locked else None, box, t, (-256, 512)[k % 2], f)
                assert np.array_equal(fb.get(), want) and not np.array_equal(want, frame), (box, R, f, locked)
                k += 1
        assert pb.intact()
    rect = F.filter_rect(box, 0, hw)
    slot = M.slot_of(before, rect)
    pb = _Slot(slot)
    for cell in (3, 16):
        for f in (0, 4):
            fb = _Buf(frame.shape, k % 4, like=frame)
            eng.filter_mosaic_u8(fb.view, pb.view, rect, sb.view, lb.view, box, cell, feather=f)
            assert np.array_equal(fb.get(), F.spec_mosaic(frame, slot, rect, sel, lock, box, cell, -256, f)), (box, cell, f)
            k += 1
    assert np.array_equal(sb.get(), sel) and np.array_equal(lb.get(), lock) and pb.intact()


def test_known_answers_of_the_header(eng):
    P = np.full((16, 16, 3), 10, np.uint8)
    P[:, 8:] = 200
    whole = (0, 0, 16, 16)
    sel = np.full((16, 16), 255, np.uint8)
    pb = _Slot(M.slot_of(P, whole))
    for a, want in ((-256, (10, 58, 153, 200)), (-128, (10, 34, 177, 200)), (256, (10, 0, 247, 200)), (1024, (10, 0, 255, 200))):
        fb = _Buf(P.shape, 1, fill=99)
        eng.filter_blur_u8(fb.view, pb.view, whole, _cuda(sel), None, whole, (2048, 1024), amount=a)
        got = fb.get().reshape(16, 16, 3)
        assert all(tuple(got[row, 6:10, ch]) == want for row in (0, 9, 15) for ch in range(3)), a
    fb = _Buf(P.shape, 2, fill=99)
    eng.filter_mosaic_u8(fb.view, pb.view, whole, _cuda(sel), None, whole, 3)
    got = fb.get().reshape(16, 16, 3)
    assert (got[:, 6:9] == 73).all() and (got[:, 15] == 200).all()


@pytest.mark.parametrize("hw", [(37, 53), (130, 70)], ids=lambda hw: "%dx%d" % hw)
def test_the_runs_again_under_poison(eng, seopt, hw):
    seopt.set("SE_TEST_POISON", 0xFF)
    k = 0
    for name in ("disc", "noise"):
        for R in (2, 16, 32):
            case = _case(name, hw, R)
            dev = _Dev(case)
            _run_blur(eng, case, dev, k, bool(k & 1), F.taps("gauss", R), (-256, 256)[k % 2], (0, 7)[k % 2])
            k += 1
            assert dev.intact()
        case = _case(name, hw, 0)
        dev = _Dev(case)
        for cell in (2, 16):
            _run_mosaic(eng, case, dev, k, bool(k & 1), cell, -256, (0, 7)[k % 2])
            k += 1
        assert dev.intact()


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(eng):
    Hi, Wi = 37, 53
    R = 2
    frame, before, sel, lock = _case("noise", (Hi, Wi), R)[:4]
    box = (8, 12, 28, 40)                                                # in the interior: the lift is the box grown by R
    rect = F.filter_rect(box, R, (Hi, Wi))
    slot = M.slot_of(before, rect)
    fb, sb, lb, pb = _Buf(frame.shape, 1, like=frame), _Buf((Hi, Wi), 1, like=sel), _Buf((Hi, Wi), 2, like=lock), _Slot(slot)
    lib, h, st = eng.lib, eng.h, eng._stream()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else t)     # noqa: E731
    FR, S, K, P = fb.view, sb.view, lb.view, pb.view
    by0, bx0, by1, bx1 = box
    ly0, lx0, lh, lw = rect
    assert ly0 > 0 and lx0 > 0 and ly0 + lh < Hi and lx0 + lw < Wi and (ly0, lx0, lh, lw) == (6, 10, 24, 32)
    good = F.taps("gauss", R)
    ok = dict(F=FR, Hi=Hi, Wi=Wi, P=P, ly0=ly0, lx0=lx0, lh=lh, lw=lw, S=S, K=K, by0=by0, bx0=bx0, by1=by1, bx1=bx1, T=good, R=R, a=-256, f=2, cell=4)
    inside_frame = FR.data_ptr() + 3 * Hi * Wi - 1                         # begins on the frame's last byte
    common = [(dict(F=None), "frame_u8"), (dict(P=None), "lift"), (dict(S=None), "sel_u8"), (dict(Hi=15), "Hi"), (dict(Wi=15), "Wi"),
              (dict(lh=15), "lift rectangle"), (dict(lw=15), "lift rectangle"), (dict(ly0=-1), "lift rectangle"), (dict(lx0=Wi - lw + 1), "lift rectangle"),
              (dict(ly0=Hi - lh + 1), "lift rectangle"), (dict(P=P.data_ptr() + 8), "16-byte aligned"), (dict(by1=by0), "box"), (dict(bx1=bx0), "box"),
              (dict(by0=ly0 - 1), "lies outside the lift rectangle"), (dict(bx1=lx0 + lw + 1), "lies outside the lift rectangle"),
              (dict(by1=ly0 + lh + 1), "lies outside the lift rectangle"), (dict(a=-257), "amount"), (dict(a=1025), "amount"), (dict(f=-1), "feather"),
              (dict(f=17), "feather"), (dict(S=inside_frame), "sel_u8 overlaps"), (dict(K=FR.data_ptr() - Hi * Wi + 1), "lock_u8 overlaps"),
              (dict(P=(FR.data_ptr() + 16) // 16 * 16), "lift overlaps")]
    blurs = common + [(dict(T=None), "taps"), (dict(T=[good[0] + 2, good[1], -1]), "negative"), (dict(T=[good[0] + 1] + good[1:]), "not 4096"),
                      (dict(T=[4096, 1, 0]), "not 4096"), (dict(R=0), "radius"), (dict(R=33), "radius"), (dict(R=-1), "radius"),
                      (dict(ly0=ly0 + 1, lh=lh - 1), "does not contain the box"), (dict(lx0=lx0 + 1, lw=lw - 1), "does not contain the box"),
                      (dict(lh=lh - 1), "does not contain the box"), (dict(lw=lw - 1), "does not contain the box")]
    for change, what in blurs:
        a = dict(ok, **change)
        t = None if a["T"] is None else (ctypes.c_int * 33)(*(list(a["T"]) + [0] * (33 - len(a["T"]))))
        rc = lib.se_filter_blur_u8(h, st, p(a["F"]), a["Hi"], a["Wi"], p(a["P"]), a["ly0"], a["lx0"], a["lh"], a["lw"], p(a["S"]), p(a["K"]),
                                   a["by0"], a["bx0"], a["by1"], a["bx1"], t, a["R"], a["a"], a["f"])
        assert rc != 0, (change, what)
        assert what in lib.se_last_error(h).decode(), (what, lib.se_last_error(h).decode())
    mosaics = common + [(dict(cell=1), "cell"), (dict(cell=65), "cell"), (dict(cell=0), "cell")]
    for change, what in mosaics:
        a = dict(ok, **change)
        rc = lib.se_filter_mosaic_u8(h, st, p(a["F"]), a["Hi"], a["Wi"], p(a["P"]), a["ly0"], a["lx0"], a["lh"], a["lw"], p(a["S"]), p(a["K"]),
                                     a["by0"], a["bx0"], a["by1"], a["bx1"], a["cell"], a["a"], a["f"])
        assert rc != 0, (change, what)
        assert what in lib.se_last_error(h).decode(), (what, lib.se_last_error(h).decode())
    # the bindings refuse planes and lifts of another shape or size, and taps that are no list of 2 .. 33 ints
    for call in (lambda: eng.filter_blur_u8(FR.view(-1), P, rect, S, None, box, good), lambda: eng.filter_blur_u8(FR, P, rect, S.view(Wi, Hi), None, box, good),
                 lambda: eng.filter_blur_u8(FR, P, rect, S, K.view(Wi, Hi), box, good), lambda: eng.filter_blur_u8(FR, P[:-1], rect, S, None, box, good),
                 lambda: eng.filter_blur_u8(FR, P, rect, S, None, box, [4096]), lambda: eng.filter_blur_u8(FR, P, rect, S, None, box, [0] * 34),
                 lambda: eng.filter_blur_u8(FR, P, rect, S, None, box, 5), lambda: eng.filter_blur_u8(FR, P, rect, S, None, box, ["a", "b"]),
                 lambda: eng.filter_blur_u8(FR, P, rect, S, None, box, good, amount=2000), lambda: eng.filter_blur_u8(FR, P, rect, S, None, box, [4000, 48, 1]),
                 lambda: eng.filter_mosaic_u8(FR.view(-1), P, rect, S, None, box, 4), lambda: eng.filter_mosaic_u8(FR, P, rect, S.view(Wi, Hi), None, box, 4),
                 lambda: eng.filter_mosaic_u8(FR, P[:-1], rect, S, None, box, 4), lambda: eng.filter_mosaic_u8(FR, P, rect, S, None, box, 1),
                 lambda: eng.filter_mosaic_u8(FR, P, rect, S, None, box, 4, feather=17)):
        with pytest.raises(_lib.SketchEditHipError):
            call()
    torch.cuda.synchronize()
    assert np.array_equal(fb.get(), frame) and np.array_equal(sb.get(), sel) and np.array_equal(lb.get(), lock) and pb.intact()
    # valid: the largest of everything
    t = F.taps("box", 32)
    rect32 = F.filter_rect(box, 32, (Hi, Wi))
    slot32 = M.slot_of(before, rect32)
    eng.filter_blur_u8(FR, _Slot(slot32).view, rect32, S, K, box, t, amount=1024, feather=16)
    assert np.array_equal(fb.get(), F.spec_blur(frame, slot32, rect32, sel, lock, box, t, 1024, 16))


# ---- 4. sessions ------------------------------------------------------------------------------------------------------------------------------
SESSION_KINDS = [("blur", {}, 8, "gauss", -256), ("blur", dict(radius=32, sigma=12.5), 32, "gauss", -256), ("box", dict(radius=5), 5, "box", -256),
                 ("sharpen", dict(amount=1.5), 2, "gauss", 384), ("pixelate", {}, 0, None, -256), ("pixelate", dict(cell=7), 0, None, -256)]
VARIANTS = [dict(), dict(locked=True), dict(feather=5), dict(feather=16, locked=True)]


@pytest.mark.parametrize("poison", [0, 0xFF])
@pytest.mark.parametrize("variant", VARIANTS, ids=lambda c: "-".join("%s=%s" % kv for kv in sorted(c.items())) or "plain")
@pytest.mark.parametrize("kind", SESSION_KINDS, ids=lambda c: c[0] + "".join("-%s" % v for v in c[1].values()))
def test_session_filter_is_the_statement(model, seopt, kind, variant, poison):
    """the statement applied on the host to the original frame: every byte of the resident frame, its sentinel margins included,
    is equal; one undo restores every byte and redo repeats it; the selection stays what it was"""
    name, kw, R, tk, q8 = kind
    f, _ = _blob_frame()
    lock = _lock_plane() if variant.get("locked") else None
    feather = variant.get("feather")
    if poison:
        seopt.set("SE_TEST_POISON", poison)
    s, fb = _session(model, f, lock, history=2)
    sel = s.select_lasso([RING, HOLE])
    plane = L.spec_select_lasso([RING, HOLE], FHW, 0)
    box, count = L.box_count(plane)
    patches, positions, info = s.filter_selection(sel, name, feather=feather, **kw)
    rect = F.filter_rect(box, R, FHW)
    slot = M.slot_of(f, rect)
    if name == "pixelate":
        want = F.spec_mosaic(f, slot, rect, plane, lock, box, kw.get("cell", 16), q8, feather or 0)
    else:
        want = F.spec_blur(f, slot, rect, plane, lock, box, F.taps(tk, R, kw.get("sigma")), q8, feather or 0)
    after = fb.get()                                                     # (checks the margins)
    assert np.array_equal(after, want) and not np.array_equal(after, f)
    win = M.move_rect(box, (0, 0), FHW)
    assert info["windows"] == [win] and positions == [(win[1], win[0])] and len(patches) == 1
    assert np.array_equal(patches[0], after[win[0]:win[0] + win[2], win[1]:win[1] + win[3]])
    assert info["filter"] == name and info["selected"] == count and info["undoable"] is True and info.get("feather") == feather
    assert info["radius"] == (R or None) and info["cell"] == (kw.get("cell", 16) if name == "pixelate" else None)
    if lock is not None:
        assert np.array_equal(after[lock != 0], f[lock != 0]) and info["locked"] is True
    assert np.array_equal(sel.plane.cpu().numpy(), plane) and (sel.box, sel.count) == (box, count)
    assert len(s._undo) == 1
    s.undo()
    assert np.array_equal(fb.get(), f) and not s.can_undo
    s.redo()
    assert np.array_equal(fb.get(), after) and not s.can_redo


def test_session_filter_encode_forms(model):
    f, _ = _blob_frame()
    for encode, ref in (("png", lambda s, w: s.frame_png(w)), (("jpg", 90), lambda s, w: s.frame_jpg(w, quality=90)),
                        (("jpg", 75, "420", True), lambda s, w: s.frame_jpg(w, quality=75, subsampling="420", optimize=True))):
        s, fb = _session(model, f, _lock_plane(), history=1)
        sel = s.select_lasso([RING])
        patches, _, info = s.filter_selection(sel, "pixelate", cell=6, encode=encode)
        assert len(patches) == 1 and isinstance(patches[0], bytes)
        assert patches == [ref(s, w) for w in info["windows"]], encode
        s.undo()
        assert np.array_equal(fb.get(), f)
