"""GPU tests of adjusting a selection's tone and colour: the four kernels of se_adjust.hip against the statement of
tests/adjust_util.py on whole buffers between sentinels, at every alignment, and EditSession.adjust_selection / histogram against
the statement applied on the host to the original frame.  Every comparison is exact."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from sketchedit_amd import _lib, serve
import adjust_util as A
import lasso_util as L
import move_util as M
import select_util as U
from test_gpu_lasso import FHW, HOLE, RING, _Buf, _blob_frame, _cuda, _lock_plane, _session, eng, model  # noqa: F401
from test_gpu_move import PATTERNS, _Slot, _case

pytestmark = pytest.mark.gpu

AMOUNTS = (1, 128, 256)
FEATHERS = (1, 7, 16)
MIX = [3000, 1500, -404, -700, 5000, -204, 100, -900, 4896, 4096 * 9, -4096 * 14, 2000]
HOT = [8192, 0, 0, 0, 8192, 0, 0, 0, 8192, -100 * 4096, -100 * 4096, -100 * 4096]          # 2 x - 100: 0 up to 50, 255 from 178 (the noise is 0 .. 79, 177 .. 255)
# group -> the runs (table?, matrix, amount, feather) of one pattern
GROUPS = dict(table=[(True, None, 256, 0)], matrix=[(False, MIX, 256, 0), (False, HOT, 256, 0)],
              both=[(True, MIX, a, 0) for a in AMOUNTS], feather=[(True, HOT, 256, f) for f in FEATHERS])


@functools.lru_cache(maxsize=None)
def _table(seed=11):
    """a table without structure: random rows"""
    t = np.random.RandomState(seed).randint(0, 256, (3, 256)).astype(np.uint8)
    t.setflags(write=False)
    return t


class _Dev:
    """a case's planes and the table at odd offsets and its slot, on the device once"""

    def __init__(self, case):
        _, _, sel, lock, _, _, slot = case
        self.sel, self.lock = sel, lock
        self.sb, self.lb, self.pb, self.tb = _Buf(sel.shape, 1, like=sel), _Buf(sel.shape, 3, like=lock), _Slot(slot), _Buf((3, 256), 1, like=_table())

    def intact(self):
        return (np.array_equal(self.sb.get(), self.sel) and np.array_equal(self.lb.get(), self.lock) and self.pb.intact()
                and np.array_equal(self.tb.get(), _table()))


def _run(eng, case, dev, k, locked, with_lut, mx, a, f):
    frame, _, sel, lock, box, rect, slot = case
    fb = _Buf(frame.shape, k % 4, like=frame)                            # the frame at every byte offset mod 4
    eng.adjust_u8(fb.view, dev.pb.view, rect, dev.sb.view, dev.lb.view if locked else None, box, lut=dev.tb.view if with_lut else None,
                  matrix=mx, amount=a, feather=f)
    got = fb.get()                                                       # (checks the margins)
    want = A.spec_adjust(frame, slot, rect, sel, lock if locked else None, box, _table() if with_lut else None, mx, a, f)
    assert np.array_equal(got, want), (frame.shape, box, with_lut, mx, a, f, locked, int((got != want).sum()))
    return int((got != frame).any())


# ---- 1. the adjust kernel: the four groups at every size, pattern and alignment ---------------------------------------------------------------
@pytest.mark.parametrize("hw", L.SIZES, ids=lambda hw: "%dx%d" % hw)
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_adjust_follows_the_statement(eng, hw, group):
    k = changed = 0
    for name in sorted(PATTERNS):
        case = _case(name, hw)
        dev = _Dev(case)
        for with_lut, mx, a, f in GROUPS[group]:
            for locked in (False, True):
                changed += _run(eng, case, dev, k, locked, with_lut, mx, a, f)
                k += 1
        assert dev.intact()
    assert changed == k


@pytest.mark.parametrize("hw", L.SIZES, ids=lambda hw: "%dx%d" % hw)
def test_the_inputs_exercise_the_rule(hw):
    """of the inputs alone, from the CPU statement: every group changes bytes, both clamps occur, some pixel has 0 < c < n"""
    for name in sorted(PATTERNS):
        frame, before, sel, lock, box, rect, slot = _case(name, hw)
        by0, bx0, by1, bx1 = box
        tg = np.zeros(hw, bool)
        tg[by0:by1, bx0:bx1] = sel[by0:by1, bx0:bx1] != 0
        assert tg.sum() >= 40
        for group, runs in GROUPS.items():
            for with_lut, mx, a, f in runs:
                for locked in (None, lock):
                    out = A.spec_adjust(frame, slot, rect, sel, locked, box, _table() if with_lut else None, mx, a, f)
                    assert (out != frame).any(), (name, group)
        P = before[tg].astype(np.int64)
        Mh = A.adjusted(P, None, HOT, 256)
        assert (Mh == 0).sum() >= 5 and (Mh == 255).sum() >= 5 and ((Mh > 0) & (Mh < 255)).sum() >= 5, (name, hw)
        Mm = A.adjusted(A.adjusted(P, _table(), None, 256), None, MIX, 256)
        assert (Mm == 0).sum() >= 1 and (Mm == 255).sum() >= 1
        for f in FEATHERS:
            cnt = A.counts(sel, box, f)[tg[by0:by1, bx0:bx1]]
            n = (2 * f + 1) ** 2
            assert cnt.min() >= 1 and (cnt < n).any(), (name, hw, f)


def test_known_answers_of_the_header(eng):
    P = np.zeros((16, 16, 3), np.uint8)
    P[...] = (200, 100, 50)
    whole = (0, 0, 16, 16)
    sel = np.full((16, 16), 255, np.uint8)
    pb = _Slot(M.slot_of(P, whole))
    ident = _Buf((3, 256), 3, like=A.IDENTITY)
    for a, want in ((256, (124, 124, 124)), (128, (162, 112, 87)), (0, (200, 100, 50))):
        fb = _Buf(P.shape, 1, fill=99)
        eng.adjust_u8(fb.view, pb.view, whole, _cuda(sel), None, whole, lut=ident.view, matrix=A.GREY, amount=a)
        assert (fb.get().reshape(-1, 3) == want).all(), a
    assert A.luma(P[0, 0]) == 124


# ---- 2. the histogram ---------------------------------------------------------------------------------------------------------------------------
class _Rec:
    """a hist record on the device, 4-byte aligned between sentinel margins"""

    def __init__(self):
        self.buf = _Buf((4096,), 0, fill=0x77)
        assert self.buf.view.data_ptr() % 4 == 0
        self.view = self.buf.view.view(torch.int32)

    def get(self):
        return self.buf.get().view(np.uint32).reshape(4, 256)


def _hist(eng, frame, sel, box, k):
    fb = _Buf(frame.shape, k % 4, like=frame)
    sb = None if sel is None else _Buf(sel.shape, 1 + k % 3, like=sel)
    rec = _Rec()
    eng._workspace_bytes(256 * 4096).fill_(0x5A)                         # garbage: every word that is read is written first
    out = eng.adjust_hist_u8(fb.view, None if sb is None else sb.view, box, out=rec.view)
    assert out is rec.view
    got = rec.get()                                                      # all 1024 words, between sentinels
    assert np.array_equal(fb.get(), frame) and (sb is None or np.array_equal(sb.get(), sel))
    return got


@pytest.mark.parametrize("hw", L.SIZES + [(272, 1040)], ids=lambda hw: "%dx%d" % hw)
def test_hist_follows_the_statement(eng, hw):
    """noise and a flat frame, every pattern and S NULL, a box of one pixel; 272 x 1040 has 289 tiles, more than the 256 workgroups"""
    Hi, Wi = hw
    noise, flat = U._noise(hw, 3), np.zeros(hw + (3,), np.uint8)
    flat[...] = (200, 100, 50)
    k = 0
    for name in sorted(PATTERNS):
        sel = np.ascontiguousarray(PATTERNS[name](Hi, Wi), np.uint8)
        for frame in (noise, flat):
            for s in (sel, None):
                for box in ((0, 0, Hi, Wi), (2, 3, Hi - 4, Wi - 2), (Hi // 2, Wi // 2, Hi // 2 + 1, Wi // 2 + 1)):
                    if hw[0] > 200 and (k % 5 or box[2] - box[0] == 1):                    # the large frame: a few runs
                        k += 1
                        continue
                    got = _hist(eng, frame, s, box, k)
                    assert np.array_equal(got, A.spec_hist(frame, s, box)), (hw, name, s is None, box)
                    if frame is flat:
                        assert got[3, 124] == got.sum() // 4 and np.count_nonzero(got) in (0, 4)
                    k += 1
    if hw[0] > 200:
        assert -(-Hi // 16) * -(-Wi // 64) > _lib.ADJUST_HIST_GROUPS
        assert np.array_equal(_hist(eng, noise, None, (0, 0, Hi, Wi), 1), A.spec_hist(noise, None, (0, 0, Hi, Wi)))
        assert _hist(eng, flat, None, (0, 0, Hi, Wi), 2)[0, 200] == Hi * Wi


# ---- 3. the table builder -------------------------------------------------------------------------------------------------------------------------
def _lut(eng, src, ref, mode, which, clip, off):
    out = _Buf((3, 256), off, fill=0x33)
    eng.adjust_lut_u8(_cuda(src.view(np.int32)), None if ref is None else _cuda(ref.view(np.int32)), mode, which, clip=clip, out=out.view)
    return out.get()


@pytest.mark.parametrize("mode", [A.STRETCH, A.EQUALIZE, A.MATCH], ids=["stretch", "equalize", "match"])
@pytest.mark.parametrize("which", [A.PER_CHANNEL, A.LUMA], ids=["channels", "luma"])
def test_lut_follows_the_statement(eng, mode, which):
    """on histograms the device made (noise, a dark copy, a flat frame, an empty selection, one pixel) and on the known answers"""
    hw = (65, 129)
    noise = U._noise(hw, 3)
    dark, flat = (noise // 3 + 20).astype(np.uint8), np.full(hw + (3,), 90, np.uint8)
    disc = np.ascontiguousarray(PATTERNS["disc"](*hw), np.uint8)
    whole = (0, 0) + hw
    hists = dict(noise=_hist(eng, noise, disc, whole, 0), dark=_hist(eng, dark, None, whole, 1), flat=_hist(eng, flat, disc, whole, 2),
                 empty=_hist(eng, noise, np.zeros(hw, np.uint8), whole, 3), one=_hist(eng, noise, None, (7, 9, 8, 10), 0))
    assert hists["empty"].sum() == 0 and hists["one"].sum() == 4 and np.array_equal(hists["dark"], A.spec_hist(dark, None, whole))
    k = 0
    for name, h in hists.items():
        for rname, href in (hists.items() if mode == A.MATCH else [(None, None)]):
            for clip in ((0, 1, 25, 200) if mode == A.STRETCH else (0,)):
                got = _lut(eng, h, href, mode, which, clip, k % 4)
                assert np.array_equal(got, A.spec_lut(h, href, mode, which, clip)), (name, rname, clip)
                k += 1
    # the known answers of the header
    z = lambda: np.zeros((4, 256), np.uint32)       # noqa: E731
    h = z()
    if mode == A.STRETCH:
        h[:, 50] = h[:, 150] = 10
        got = _lut(eng, h, None, mode, which, 0, 1)
        assert [int(got[c][v]) for c in range(3) for v in (50, 100, 150, 200)] == [0, 128, 255, 255] * 3
    elif mode == A.EQUALIZE:
        h[:, 10], h[:, 20], h[:, 30] = 1, 1, 2
        got = _lut(eng, h, None, mode, which, 0, 2)
        assert [int(got[c][v]) for c in range(3) for v in (10, 15, 20, 30)] == [0, 0, 85, 255] * 3
    else:
        r = z()
        h[:, 10] = h[:, 20] = 2
        r[:, 100], r[:, 200] = 1, 3
        got = _lut(eng, h, r, mode, which, 0, 3)
        assert [int(got[c][v]) for c in range(3) for v in (5, 10, 20)] == [0, 200, 200] * 3
        n = 1 << 25                                                     # the products at 2^25 pixels: 2^50
        a, b = z(), z()
        a[:, 255] = n
        b[:, 0], b[:, 255] = n // 2, n // 2
        for src, ref in ((a, b), (b, a)):
            assert np.array_equal(_lut(eng, src, ref, mode, which, 0, 0), A.spec_lut(src, ref, mode, which))


# ---- 4. further runs ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(37, 53), (130, 70)], ids=lambda hw: "%dx%d" % hw)
def test_the_runs_again_under_poison(eng, seopt, hw):
    seopt.set("SE_TEST_POISON", 0xFF)
    k = 0
    for name in ("disc", "noise"):
        case = _case(name, hw)
        dev = _Dev(case)
        for group in sorted(GROUPS):
            with_lut, mx, a, f = GROUPS[group][-1]
            _run(eng, case, dev, k, bool(k & 1), with_lut, mx, a, f)
            k += 1
        assert dev.intact()
        frame, _, sel, _, box, _, _ = case
        h = _hist(eng, frame, sel, box, k)
        assert np.array_equal(h, A.spec_hist(frame, sel, box))
        ref = _hist(eng, frame, None, (0, 0) + hw, k + 1)
        for mode in (A.STRETCH, A.EQUALIZE, A.MATCH):
            got = _lut(eng, h, ref if mode == A.MATCH else None, mode, k % 2, 10 if mode == A.STRETCH else 0, k % 4)
            assert np.array_equal(got, A.spec_lut(h, ref if mode == A.MATCH else None, mode, k % 2, 10 if mode == A.STRETCH else 0))
            k += 1


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(eng):
    Hi, Wi = 37, 53
    frame, before, sel, lock = _case("noise", (Hi, Wi))[:4]
    box = (8, 12, 28, 40)
    rect = (6, 10, 24, 32)
    slot = M.slot_of(before, rect)
    fb, sb, lb, pb, tb = _Buf(frame.shape, 1, like=frame), _Buf((Hi, Wi), 1, like=sel), _Buf((Hi, Wi), 2, like=lock), _Slot(slot), _Buf((3, 256), 1, like=_table())
    rec, rec2, out = _Rec(), _Rec(), _Buf((3, 256), 2, fill=0x33)
    lib, h, st = eng.lib, eng.h, eng._stream()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else t)     # noqa: E731
    FR, S, K, P, T = fb.view, sb.view, lb.view, pb.view, tb.view
    by0, bx0, by1, bx1 = box
    ly0, lx0, lh, lw = rect
    need = lib.se_adjust_hist_u8_workspace_bytes(Hi, Wi)
    assert need == 3 * 4096
    ws = eng._workspace_bytes(need)
    ws.fill_(0x5A)
    ok = dict(F=FR, Hi=Hi, Wi=Wi, P=P, ly0=ly0, lx0=lx0, lh=lh, lw=lw, S=S, K=K, by0=by0, bx0=bx0, by1=by1, bx1=bx1, T=T, M=list(A.GREY), a=256, f=2)
    inside_frame = FR.data_ptr() + 3 * Hi * Wi - 1                         # begins on the frame's last byte
    mx = lambda k, v: [v if i == k else 0 for i in range(12)]           # noqa: E731
    adjusts = [(dict(F=None), "frame_u8"), (dict(P=None), "lift"), (dict(S=None), "sel_u8"), (dict(Hi=15), "Hi"), (dict(Wi=15), "Wi"),
               (dict(lh=15), "lift rectangle"), (dict(lw=15), "lift rectangle"), (dict(ly0=-1), "lift rectangle"), (dict(lx0=Wi - lw + 1), "lift rectangle"),
               (dict(ly0=Hi - lh + 1), "lift rectangle"), (dict(P=P.data_ptr() + 8), "16-byte aligned"), (dict(by1=by0), "box"), (dict(bx1=bx0), "box"),
               (dict(by0=ly0 - 1), "lies outside the lift rectangle"), (dict(bx1=lx0 + lw + 1), "lies outside the lift rectangle"),
               (dict(by1=ly0 + lh + 1), "lies outside the lift rectangle"), (dict(a=-1), "amount"), (dict(a=257), "amount"), (dict(f=-1), "feather"),
               (dict(f=17), "feather"), (dict(M=mx(0, 32769)), "matrix[0]"), (dict(M=mx(8, -32769)), "matrix[8]"), (dict(M=mx(9, (1 << 20) + 1)), "matrix[9]"),
               (dict(M=mx(11, -(1 << 20) - 1)), "matrix[11]"), (dict(S=inside_frame), "sel_u8 overlaps"), (dict(K=FR.data_ptr() - Hi * Wi + 1), "lock_u8 overlaps"),
               (dict(P=(FR.data_ptr() + 16) // 16 * 16), "lift overlaps"), (dict(T=inside_frame), "lut overlaps"), (dict(T=FR.data_ptr() - 767), "lut overlaps")]
    for change, what in adjusts:
        a = dict(ok, **change)
        m = None if a["M"] is None else (ctypes.c_int * 12)(*a["M"])
        rc = lib.se_adjust_u8(h, st, p(a["F"]), a["Hi"], a["Wi"], p(a["P"]), a["ly0"], a["lx0"], a["lh"], a["lw"], p(a["S"]), p(a["K"]),
                              a["by0"], a["bx0"], a["by1"], a["bx1"], p(a["T"]), m, a["a"], a["f"])
        assert rc != 0, (change, what)
        assert what in lib.se_last_error(h).decode(), (what, lib.se_last_error(h).decode())
    okh = dict(F=FR, Hi=Hi, Wi=Wi, S=S, by0=by0, bx0=bx0, by1=by1, bx1=bx1, H=rec.view, W=ws, n=need)
    hists = [(dict(F=None), "frame_u8"), (dict(H=None), "hist_dev"), (dict(W=None), "workspace"), (dict(Hi=15), "Hi"), (dict(Wi=15), "Wi"),
             (dict(by1=by0), "box"), (dict(bx1=bx0), "box"), (dict(by0=-1), "lies outside the frame"), (dict(bx1=Wi + 1), "lies outside the frame"),
             (dict(by1=Hi + 1), "lies outside the frame"), (dict(H=rec.view.data_ptr() + 2), "4-byte aligned"), (dict(n=need - 1), "workspace too small"),
             (dict(n=0), "workspace too small"), (dict(W=ws.data_ptr() + 128), "256-byte aligned"), (dict(H=FR.data_ptr() // 4 * 4 + 4), "hist_dev overlaps frame_u8"),
             (dict(W=(FR.data_ptr() + 256) // 256 * 256), "workspace overlaps frame_u8"), (dict(H=ws.data_ptr() + 4096), "hist_dev overlaps the workspace"),
             (dict(S=rec.view.data_ptr() + 8), "hist_dev overlaps sel_u8"), (dict(S=ws.data_ptr() + 100), "workspace overlaps sel_u8")]
    for change, what in hists:
        a = dict(okh, **change)
        rc = lib.se_adjust_hist_u8(h, st, p(a["F"]), a["Hi"], a["Wi"], p(a["S"]), a["by0"], a["bx0"], a["by1"], a["bx1"], p(a["H"]), p(a["W"]), a["n"])
        assert rc != 0, (change, what)
        assert what in lib.se_last_error(h).decode(), (what, lib.se_last_error(h).decode())
    assert lib.se_adjust_hist_u8_workspace_bytes(15, 100) == 0 and lib.se_adjust_hist_u8_workspace_bytes(100, 15) == 0
    okl = dict(A=rec.view, B=None, mode=0, which=1, clip=5, O=out.view)
    luts = [(dict(A=None), "hist_src_dev"), (dict(O=None), "lut_dev"), (dict(mode=3), "mode"), (dict(mode=-1), "mode"), (dict(which=2), "which"),
            (dict(which=-1), "which"), (dict(clip=201), "clip"), (dict(clip=-1), "clip"), (dict(mode=2), "hist_ref_dev"), (dict(B=rec2.view), "SE_ADJUST_MATCH only"),
            (dict(mode=1, B=rec2.view), "SE_ADJUST_MATCH only"), (dict(A=rec.view.data_ptr() + 1), "hist_src_dev must be 4-byte aligned"),
            (dict(mode=2, B=rec2.view.data_ptr() + 2), "hist_ref_dev must be 4-byte aligned"), (dict(O=rec.view.data_ptr() + 4095), "lut_dev overlaps hist_src_dev"),
            (dict(mode=2, B=rec2.view, O=rec2.view.data_ptr() - 767), "lut_dev overlaps hist_ref_dev")]
    for change, what in luts:
        a = dict(okl, **change)
        rc = lib.se_adjust_lut_u8(h, st, p(a["A"]), p(a["B"]), a["mode"], a["which"], a["clip"], p(a["O"]))
        assert rc != 0, (change, what)
        assert what in lib.se_last_error(h).decode(), (what, lib.se_last_error(h).decode())
    # the bindings refuse planes, lifts, tables and records of another shape, size or type
    H32 = rec.view
    for call in (lambda: eng.adjust_u8(FR.view(-1), P, rect, S, None, box, lut=T), lambda: eng.adjust_u8(FR, P, rect, S.view(Wi, Hi), None, box, lut=T),
                 lambda: eng.adjust_u8(FR, P, rect, S, K.view(Wi, Hi), box, lut=T), lambda: eng.adjust_u8(FR, P[:-1], rect, S, None, box, lut=T),
                 lambda: eng.adjust_u8(FR, P, rect, S, None, box, lut=T.view(-1)[:767]), lambda: eng.adjust_u8(FR, P, rect, S, None, box, lut=_table()),
                 lambda: eng.adjust_u8(FR, P, rect, S, None, box, matrix=[1] * 11), lambda: eng.adjust_u8(FR, P, rect, S, None, box, matrix="grey"),
                 lambda: eng.adjust_u8(FR, P, rect, S, None, box, matrix=[1 << 31] * 12), lambda: eng.adjust_u8(FR, P, rect, S, None, box, lut=T, amount=300),
                 lambda: eng.adjust_u8(FR, P, rect, S, None, box, lut=T, feather=17), lambda: eng.adjust_hist_u8(FR.view(-1), S, box),
                 lambda: eng.adjust_hist_u8(FR, S.view(Wi, Hi), box), lambda: eng.adjust_hist_u8(FR, S, box, out=T), lambda: eng.adjust_hist_u8(FR, S, box, out=H32[:1000]),
                 lambda: eng.adjust_hist_u8(FR, S, (0, 0, Hi + 1, Wi)), lambda: eng.adjust_lut_u8(T, None, 0, 0), lambda: eng.adjust_lut_u8(H32, T, 2, 0),
                 lambda: eng.adjust_lut_u8(H32, None, 2, 0), lambda: eng.adjust_lut_u8(H32, H32, 0, 0), lambda: eng.adjust_lut_u8(H32, None, 0, 0, clip=500),
                 lambda: eng.adjust_lut_u8(H32, None, 0, 0, out=H32), lambda: eng.adjust_lut_u8(H32, None, 0, 5)):
        with pytest.raises(_lib.SketchEditHipError):
            call()
    torch.cuda.synchronize()
    assert np.array_equal(fb.get(), frame) and np.array_equal(sb.get(), sel) and np.array_equal(lb.get(), lock) and pb.intact()
    assert np.array_equal(tb.get(), _table()) and (rec.buf.get() == 0x77).all() and (rec2.buf.get() == 0x77).all() and (out.get() == 0x33).all()
    assert (ws[:need].cpu().numpy() == 0x5A).all()
    # valid: the largest of everything
    eng.adjust_u8(FR, P, rect, S, K, box, lut=T, matrix=[32768] * 9 + [-(1 << 20)] * 3, amount=256, feather=16)
    assert np.array_equal(fb.get(), A.spec_adjust(frame, slot, rect, sel, lock, box, _table(), [32768] * 9 + [-(1 << 20)] * 3, 256, 16))


# ---- 6. sessions ------------------------------------------------------------------------------------------------------------------------------
SMALL = [(6.0, 5.0), (30.5, 8.0), (12.25, 28.0)]
SESSION_KINDS = [("lut", dict(lut="TABLE")), ("matrix", dict(matrix=MIX, amount=0.75)), ("levels", dict(auto="levels", clip=20)),
                 ("levels-channels", dict(auto="levels", which="channels", clip=100, matrix=A.GREY)), ("equalize", dict(auto="equalize", which="channels")),
                 ("match", dict(auto="match", reference="OTHER")), ("rim", dict(auto="match", reference=("rim", 8), which="channels", amount=0.5))]
VARIANTS = [dict(), dict(locked=True), dict(feather=5), dict(feather=16, locked=True)]


@pytest.mark.parametrize("poison", [0, 0xFF])
@pytest.mark.parametrize("variant", VARIANTS, ids=lambda c: "-".join("%s=%s" % kv for kv in sorted(c.items())) or "plain")
@pytest.mark.parametrize("kind", SESSION_KINDS, ids=lambda c: c[0])
def test_session_adjust_is_the_statement(model, seopt, kind, variant, poison):
    """the statement applied on the host to the original frame: every byte of the resident frame, its sentinel margins included,
    is equal; one undo restores every byte and redo repeats it; the selection stays what it was"""
    name, kw = kind
    kw = dict(kw)
    f, _ = _blob_frame()
    lock = _lock_plane() if variant.get("locked") else None
    feather = variant.get("feather")
    if poison:
        seopt.set("SE_TEST_POISON", poison)
    s, fb = _session(model, f, lock, history=2)
    sel = s.select_lasso([RING, HOLE])
    plane = L.spec_select_lasso([RING, HOLE], FHW, 0)
    box, count = L.box_count(plane)
    table = None
    if kw.get("lut") == "TABLE":
        table = kw["lut"] = np.array(_table())
    if kw.get("reference") == "OTHER":
        kw["reference"] = s.select_lasso([SMALL])
    auto, which = kw.get("auto"), A.LUMA if kw.get("which", "luma") == "luma" else A.PER_CHANNEL
    if auto:
        ref = None
        if name == "match":
            ref = A.spec_hist(f, L.spec_select_lasso([SMALL], FHW, 0), (0, 0) + FHW)
        elif name == "rim":
            ring = L.spec_combine(U.spec_grow(plane != 0, 8), plane, 1)
            assert 0 < np.count_nonzero(ring) < count
            ref = A.spec_hist(f, ring, (0, 0) + FHW)
        table = A.spec_lut(A.spec_hist(f, plane, box), ref, serve.ADJUST_AUTO[auto], which, kw.get("clip", 0))
        assert not np.array_equal(table, A.IDENTITY)
    patches, positions, info = s.adjust_selection(sel, feather=feather, **kw)
    win = M.move_rect(box, (0, 0), FHW)
    q8 = int(round(256 * kw.get("amount", 1.0)))
    want = A.spec_adjust(f, M.slot_of(f, win), win, plane, lock, box, table, kw.get("matrix"), q8, feather or 0)
    after = fb.get()                                                     # (checks the margins)
    assert np.array_equal(after, want) and not np.array_equal(after, f)
    assert info["windows"] == [win] and positions == [(win[1], win[0])] and len(patches) == 1
    assert np.array_equal(patches[0], after[win[0]:win[0] + win[2], win[1]:win[1] + win[3]])
    assert info["auto"] == auto and info["selected"] == count and info["undoable"] is True and info.get("feather") == feather
    assert info["adjust"] == "+".join(k for k in ("lut", "auto", "matrix") if k in kw) and info["amount"] == kw.get("amount", 1.0)
    if lock is not None:
        assert np.array_equal(after[lock != 0], f[lock != 0]) and info["locked"] is True
    assert np.array_equal(sel.plane.cpu().numpy(), plane) and (sel.box, sel.count) == (box, count)
    assert len(s._undo) == 1
    s.undo()
    assert np.array_equal(fb.get(), f) and not s.can_undo
    s.redo()
    assert np.array_equal(fb.get(), after) and not s.can_redo


def test_session_histogram_and_encode_forms(model):
    f, _ = _blob_frame()
    s, fb = _session(model, f, _lock_plane(), history=1)
    sel = s.select_lasso([RING, HOLE])
    plane = L.spec_select_lasso([RING, HOLE], FHW, 0)
    got = s.histogram(sel)
    assert got.dtype == np.uint32 and got.shape == (4, 256) and np.array_equal(got, A.spec_hist(f, plane, (0, 0) + FHW))
    assert np.array_equal(s.histogram(), A.spec_hist(f, None, (0, 0) + FHW)) and np.array_equal(fb.get(), f)
    assert s.histogram(s.combine(sel, sel, "subtract")).sum() == 0
    for encode, ref in (("png", lambda s, w: s.frame_png(w)), (("jpg", 90), lambda s, w: s.frame_jpg(w, quality=90)),
                        (("jpg", 75, "420", True), lambda s, w: s.frame_jpg(w, quality=75, subsampling="420", optimize=True))):
        s, fb = _session(model, f, _lock_plane(), history=1)
        sel = s.select_lasso([RING])
        patches, _, info = s.adjust_selection(sel, auto="equalize", matrix=serve.adjust_matrix(1.5, 30), encode=encode)
        assert len(patches) == 1 and isinstance(patches[0], bytes)
        assert patches == [ref(s, w) for w in info["windows"]], encode
        s.undo()
        assert np.array_equal(fb.get(), f)
