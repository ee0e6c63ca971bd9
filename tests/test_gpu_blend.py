"""GPU tests of the seamless move and clone: se_move_blend_u8 against the statement of tests/blend_util.py on whole
buffers between sentinels, at every alignment, and EditSession.move_selection / clone_selection with blend="seamless" against a
two-step route -- fill_selection of the grown selection on a twin session, then the statement applied on the host with the
original pixels.  Every comparison is exact; every case with a rim asserts that the expected bytes are neither the hard drop's
nor the untouched frame's."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from sketchedit_amd import _lib, serve
import blend_util as B
import lasso_util as L
import move_util as M
import outline_util as O
import select_util as U
from test_gpu_lasso import FHW, HOLE, RING, SENTINEL, _Buf, _blob_frame, _cuda, _lock_plane, _session, eng, model  # noqa: F401
from test_gpu_move import _Slot, _offsets, _values_disc

pytestmark = pytest.mark.gpu


def _line(Hi, Wi):
    """one pixel wide, from edge to edge but a pixel"""
    p = np.zeros((Hi, Wi), np.uint8)
    p[Hi // 2, 1:Wi - 1] = 3
    return p


PATTERNS = {"noise": O.noise, "disc": _values_disc, "annulus": O.annulus, "line": _line, "full": O.full}


def _grown_rect(box, hw):
    g = (max(box[0] - 1, 0), max(box[1] - 1, 0), min(box[2] + 1, hw[0]), min(box[3] + 1, hw[1]))
    return M.move_rect(g, (0, 0), hw)


@functools.lru_cache(maxsize=None)
def _case(name, hw):
    """(frame, selection plane, lock plane, box, lift rectangle, slot): computed once, shared, read-only"""
    Hi, Wi = hw
    rng = np.random.RandomState(Hi * 1000 + Wi + 1)
    frame, before = U._noise(hw, 3), U._noise(hw, 4)
    sel = np.ascontiguousarray(PATTERNS[name](Hi, Wi), np.uint8)
    lock = np.where(rng.rand(Hi, Wi) < 0.25, rng.randint(1, 256, hw), 0).astype(np.uint8)
    if name == "noise":                                                  # a box strictly inside the selected pixels, a lift larger than it
        box, rect = (2, 3, Hi - 4, Wi - 2), (0, 0, Hi, Wi)
    else:
        box = M.box_of(sel)
        rect = _grown_rect(box, hw)
    slot = M.slot_of(before, rect)
    for a in (frame, sel, lock, slot):
        a.setflags(write=False)
    return frame, sel, lock, box, rect, slot


class _Work:
    """a workspace on the device, 16-byte aligned between sentinel margins"""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((4096 + n + 4096,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.lead = 4096 + (-self.buf.data_ptr()) % 16
        self.ptr = self.buf.data_ptr() + self.lead

    def margins_intact(self):
        b = self.buf.cpu().numpy()
        return (b[:self.lead] == SENTINEL).all() and (b[self.lead + self.n:] == SENTINEL).all()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else t)


def _blend(eng, F, P, rect, S, K, box, off, flip, work):
    rc = eng.lib.se_move_blend_u8(eng.h, eng._stream(), _p(F), F.shape[0], F.shape[1], _p(P), rect[0], rect[1], rect[2], rect[3], _p(S), _p(K),
                                  box[0], box[1], box[2], box[3], off[0], off[1], flip, ctypes.c_void_p(work.ptr), work.n)
    assert rc == 0, eng.lib.se_last_error(eng.h).decode()


def _run_cases(eng, hw, flip):
    changed = rims = 0
    dev = {}
    names = sorted(PATTERNS)
    for k in range(13):
        name = names[(k + flip) % len(names)]                            # every flip meets every pattern
        frame, sel, lock, box, rect, slot = _case(name, hw)
        if name not in dev:
            dev[name] = (_Buf(hw, 1, like=sel), _Buf(hw, 3, like=lock), _Slot(slot), _Work(B.workspace_bytes(box[2] - box[0], box[3] - box[1])),
                         sel, lock)
        sb, lb, pb, wk = dev[name][:4]
        off = _offsets(hw, box)[k]
        for locked in (False, True):
            fb = _Buf(frame.shape, (k + locked) % 4, like=frame)          # the frame at every byte offset mod 4
            lk = lock if locked else None
            _blend(eng, fb.view, pb.view, rect, sb.view, lb.view if locked else None, box, off, flip, wk)
            got = fb.get()
            want = B.spec_blend(frame, slot, rect, sel, lk, box, off, flip)
            assert np.array_equal(got, want), (name, hw, off, flip, locked, int((got != want).sum()))
            l0 = B.level0(frame, slot, rect, sel, lk, box, off, flip)
            if l0 is not None and (l0[1] == B.KNOWN).any():               # a rim: the membrane is at work
                assert not np.array_equal(want, M.spec_drop(frame, slot, rect, sel, lk, box, off, flip, 0)) and not np.array_equal(want, frame)
                rims += 1
            changed += int((got != frame).any())
    for sb, lb, pb, wk, sel, lock in dev.values():
        assert np.array_equal(sb.get(), sel) and np.array_equal(lb.get(), lock) and pb.intact() and wk.margins_intact()
    return changed, rims


# ---- 1. the entry: every flip at every size, offset and alignment ------------------------------------------------------------------------
@pytest.mark.parametrize("hw", L.SIZES, ids=lambda hw: "%dx%d" % hw)
@pytest.mark.parametrize("flip", range(4))
def test_blend_follows_the_statement(eng, hw, flip):
    changed, rims = _run_cases(eng, hw, flip)
    assert changed >= 12 and rims >= 12                                  # all but the offsets that are wholly out


def test_blend_known_answers(eng):
    sel = np.zeros((16, 16), np.uint8)
    sel[2:4, 2:5] = 1
    wk = _Work(B.workspace_bytes(2, 3))
    for around, obj, want_v in ((180, 200, 30), (250, 100, 0)):
        frame = np.full((16, 16, 3), 10, np.uint8)
        before = np.full((16, 16, 3), around, np.uint8)
        before[2:4, 2:5] = obj
        fb, pb = _Buf(frame.shape, 2, like=frame), _Slot(M.slot_of(before, (0, 0, 16, 16)))
        _blend(eng, fb.view, pb.view, (0, 0, 16, 16), _cuda(sel), None, (2, 2, 4, 5), (1, 3), 0, wk)
        want = frame.copy()
        want[3:5, 5:8] = want_v
        assert np.array_equal(fb.get(), want)
    # the binding, with the engine's own workspace: source and destination overlap, the object's pixels come from the lift
    frame, sel, lock, box, rect, slot = _case("disc", (65, 129))
    fb, pb = _Buf(frame.shape, 1, like=frame), _Slot(slot)
    eng.move_blend_u8(fb.view, pb.view, rect, _cuda(sel), _cuda(lock), box, (3, 5), flip=2)
    assert np.array_equal(fb.get(), B.spec_blend(frame, slot, rect, sel, lock, box, (3, 5), 2)) and wk.margins_intact()


# ---- 2. everything again with every scratch byte poisoned ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(37, 53), (65, 129), (130, 70)], ids=lambda hw: "%dx%d" % hw)
def test_blend_under_poison(eng, seopt, hw):
    """every record the kernels read was written by them: 0xFF in a state or a value would change bytes"""
    seopt.set("SE_TEST_POISON", 0xFF)
    changed, rims = _run_cases(eng, hw, 1)
    assert changed >= 12 and rims >= 12


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(eng):
    Hi, Wi = 37, 53
    frame, sel, lock, box, rect, slot = _case("disc", (Hi, Wi))
    fb, sb, lb, pb = _Buf(frame.shape, 1, like=frame), _Buf((Hi, Wi), 1, like=sel), _Buf((Hi, Wi), 2, like=lock), _Slot(slot)
    need = B.workspace_bytes(box[2] - box[0], box[3] - box[1])
    wk = _Work(need)
    lib, h, st = eng.lib, eng.h, eng._stream()
    assert lib.se_move_blend_u8_workspace_bytes(box[2] - box[0], box[3] - box[1]) == need
    F, S, K, P = fb.view, sb.view, lb.view, pb.view
    by0, bx0, by1, bx1 = box
    ly0, lx0, lh, lw = rect
    ok = dict(F=F, Hi=Hi, Wi=Wi, P=P, ly0=ly0, lx0=lx0, lh=lh, lw=lw, S=S, K=K, by0=by0, bx0=bx0, by1=by1, bx1=bx1, dy=2, dx=-3, flip=1, W=wk.ptr, wn=need)
    inside_frame = F.data_ptr() + 3 * Hi * Wi - 1
    block = torch.zeros((1 << 20,), dtype=torch.uint8, device="cuda")
    mid = (block.data_ptr() + (1 << 19)) // 16 * 16
    cases = [(dict(F=None), "frame_u8"), (dict(P=None), "lift"), (dict(S=None), "sel_u8"), (dict(Hi=15), "Hi"), (dict(Wi=15), "Wi"),
             (dict(lh=15), "lift rectangle"), (dict(ly0=-1), "lift rectangle"), (dict(lx0=Wi - lw + 1), "lift rectangle"),
             (dict(P=P.data_ptr() + 8), "16-byte aligned"), (dict(by1=by0), "box"), (dict(bx1=bx0), "box"),
             (dict(by0=ly0 - 1), "lies outside the lift rectangle"), (dict(bx1=lx0 + lw + 1), "lies outside the lift rectangle"),
             (dict(dy=16385), "dy"), (dict(dx=-16385), "dx"), (dict(flip=4), "flip"), (dict(flip=-1), "flip"),
             (dict(S=inside_frame), "sel_u8 overlaps"), (dict(K=F.data_ptr() - Hi * Wi + 1), "lock_u8 overlaps"),
             (dict(P=(F.data_ptr() + 16) // 16 * 16), "lift overlaps"),
             (dict(W=None), "workspace"), (dict(wn=need - 1), "workspace too small"), (dict(wn=0), "workspace too small"),
             (dict(W=wk.ptr + 8), "16-byte aligned"),
             # an operand in the middle of a block of its own, the workspace beginning 64 bytes in front of it
             (dict(F=mid, W=mid - 64), "workspace overlaps frame_u8"), (dict(P=mid, W=mid - 64), "workspace overlaps lift"),
             (dict(S=mid, W=mid - 64), "workspace overlaps sel_u8"), (dict(K=mid, W=mid - 64), "workspace overlaps lock_u8"),
             (dict(K=mid, W=(mid + Hi * Wi - 1) // 16 * 16), "workspace overlaps lock_u8")]      # its last bytes
    for change, what in cases:
        a = dict(ok, **change)
        rc = lib.se_move_blend_u8(h, st, _p(a["F"]), a["Hi"], a["Wi"], _p(a["P"]), a["ly0"], a["lx0"], a["lh"], a["lw"], _p(a["S"]), _p(a["K"]),
                                  a["by0"], a["bx0"], a["by1"], a["bx1"], a["dy"], a["dx"], a["flip"], _p(a["W"]), a["wn"])
        assert rc != 0, (change, what)
        assert what in lib.se_last_error(h).decode(), (what, lib.se_last_error(h).decode())
    # a side of the box above the limit, in a frame wide enough to hold it
    wide = torch.zeros((16, 2064, 3), dtype=torch.uint8, device="cuda")
    wsel, wslot = torch.ones((16, 2064), dtype=torch.uint8, device="cuda"), torch.zeros((16 * 6192 + 16,), dtype=torch.uint8, device="cuda")
    wp = wslot[(-wslot.data_ptr()) % 16:]
    rc = lib.se_move_blend_u8(h, st, _p(wide), 16, 2064, _p(wp), 0, 0, 16, 2064, _p(wsel), None, 0, 0, 16, 2049, 0, 0, 0, ctypes.c_void_p(wk.ptr), 1 << 40)
    assert rc != 0 and "side above 2048" in lib.se_last_error(h).decode()
    assert lib.se_move_blend_u8_workspace_bytes(16, 2049) == 0 and lib.se_move_blend_u8_workspace_bytes(0, 5) == 0
    # the bindings refuse planes and lifts of another shape or size
    for call in (lambda: eng.move_blend_u8(F.view(-1), P, rect, S, None, box, (0, 0)), lambda: eng.move_blend_u8(F, P, rect, S.view(Wi, Hi), None, box, (0, 0)),
                 lambda: eng.move_blend_u8(F, P, rect, S, K.view(Wi, Hi), box, (0, 0)), lambda: eng.move_blend_u8(F, P[:-1], rect, S, None, box, (0, 0))):
        with pytest.raises(_lib.SketchEditHipError):
            call()
    # valid, and nothing to do: the whole box lands outside the frame
    _blend(eng, F, P, rect, S, K, box, (Hi, 0), 3, wk)
    torch.cuda.synchronize()
    assert np.array_equal(fb.get(), frame) and np.array_equal(sb.get(), sel) and np.array_equal(lb.get(), lock) and pb.intact()
    assert (wk.buf.cpu().numpy() == SENTINEL).all()                       # the workspace too


# ---- 4. sessions ---------------------------------------------------------------------------------------------------------------------------------
SESSION_CASES = [dict(), dict(locked=True), dict(max_side=64), dict(keep_source=True, flip="hv", locked=True), dict(offset=(-50, -45), flip="v"),
                 dict(feather=4, locked=True, flip="h")]


@pytest.mark.parametrize("case", SESSION_CASES, ids=lambda c: "-".join("%s=%s" % kv for kv in sorted(c.items())) or "defaults")
def test_session_seamless_move_is_fill_then_the_statement(model, case):
    """a twin session fills the grown selection through the same window in the same mode, the statement drops the ORIGINAL pixels
    on the host: every byte of the frame, its sentinel margins included, is equal"""
    case = dict(case)
    f, _ = _blob_frame()
    lock = _lock_plane() if case.pop("locked", False) else None
    offset = case.pop("offset", (7, -9))                                 # smaller than the object: source and destination overlap
    flip, keep = case.get("flip"), case.get("keep_source", False)
    a, abuf = _session(model, f, lock, history=2)
    b, bbuf = _session(model, f, lock, history=2)
    c, _ = _session(model, f, lock, history=2)
    sel = a.select_lasso([RING, HOLE])
    plane = L.spec_select_lasso([RING, HOLE], FHW, 0)
    box = L.box_count(plane)[0]
    patches, positions, info = a.move_selection(sel, offset, low_latency=False, blend="seamless", **case)
    dst = M.move_rect(box, offset, FHW)
    wins = info["windows"]
    assert wins[-1] == dst and len(wins) == (1 if keep else 2) and positions == [(w[1], w[0]) for w in wins]
    if not keep:
        fill = {k: case[k] for k in ("max_side", "feather") if k in case}
        _, _, ib = b.fill_selection(b.select_lasso([RING, HOLE], grow=2), window=wins[0], low_latency=False, **fill)
        assert info.get("work") == ib.get("work") and info.get("feather") == case.get("feather")
    else:
        assert "feather" not in info
    rect = _grown_rect(box, FHW)
    slot = M.slot_of(f, rect)
    want = B.spec_blend(bbuf.get(), slot, rect, plane, lock, box, offset, serve.MOVE_FLIPS[flip])
    after = abuf.get()                                                   # (checks the margins)
    assert np.array_equal(after, want) and not np.array_equal(after, f)
    assert not np.array_equal(want, M.spec_drop(bbuf.get(), slot, rect, plane, lock, box, offset, serve.MOVE_FLIPS[flip], 0))
    for pch, w in zip(patches, wins):
        assert np.array_equal(pch, after[w[0]:w[0] + w[2], w[1]:w[1] + w[3]])
    if lock is not None:
        assert np.array_equal(after[lock != 0], f[lock != 0]) and info["locked"] is True
    assert info["move"] is True and info["blend"] == "seamless" and info["offset"] == offset and info["flip"] == flip
    assert info["selected"] == sel.count and info["undoable"] is True
    # the moved selection is section 6r's
    moved = info["selection"]
    _, _, plain = c.move_selection(c.select_lasso([RING, HOLE]), offset, low_latency=False, **case)
    assert np.array_equal(moved.plane.cpu().numpy(), plain["selection"].plane.cpu().numpy())
    assert (moved.box, moved.count) == (plain["selection"].box, plain["selection"].count) and plain["windows"] == wins and "blend" not in plain
    assert np.array_equal(moved.plane.cpu().numpy(), M.spec_shift(plane, box, offset, serve.MOVE_FLIPS[flip]))
    # one call is one undo step, byte for byte both ways
    a.undo()
    assert np.array_equal(abuf.get(), f) and not a.can_undo
    a.redo()
    assert np.array_equal(abuf.get(), after) and not a.can_redo


def test_session_seamless_clone_encode_forms(model):
    f, _ = _blob_frame()
    for encode, ref in (("png", lambda s, w: s.frame_png(w)), (("jpg", 90), lambda s, w: s.frame_jpg(w, quality=90)),
                        (("jpg", 75, "420", True), lambda s, w: s.frame_jpg(w, quality=75, subsampling="420", optimize=True))):
        s, fb = _session(model, f, _lock_plane(), history=1)
        sel = s.select_lasso([RING])
        patches, _, info = s.clone_selection(sel, (6, 11), encode=encode, blend="seamless")
        assert len(patches) == 1 and all(isinstance(p, bytes) for p in patches)
        assert patches == [ref(s, w) for w in info["windows"]], encode
        s.undo()
        assert np.array_equal(fb.get(), f)
    with pytest.raises(ValueError, match="blend"):
        s.move_selection(sel, (6, 11), blend="mixed")
    assert np.array_equal(fb.get(), f) and not s.can_undo
