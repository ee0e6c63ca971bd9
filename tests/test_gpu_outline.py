"""GPU tests of the outline of a selection: se_outline_u8 against the statement of tests/outline_util.py, record
for record, with the plane at every alignment between sentinels, the records' buffer pre-filled and between sentinels at both
of the kernel's store alignments, and every capacity around the total; the records through se_lasso_fill_u8 re-make the plane;
the same under SE_TEST_POISON; every refusal; Selection.rings / EditSession.lock_rings against rings traced from the pixels.
Every comparison is exact."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from sketchedit_amd import _lib, serve
import lasso_util as L
import outline_util as O
import select_util as U
from test_gpu_lasso import _Buf, _blob_frame, _cuda, _session, model, eng, FHW, RING, HOLE, SMALL, STAR      # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

PATTERNS = {f.__name__: f for f in O.PATTERNS + O.MORE_PATTERNS}
SENT32, GARB32 = -1515870811, 1549556828                                # 0xA5A5A5A5, 0x5C5C5C5C


@functools.lru_cache(maxsize=None)
def _case(name, hw):
    """(plane, the statement's records): computed once, shared, never written"""
    plane = PATTERNS[name](*hw)
    rec = O.spec_outline(plane)
    plane.setflags(write=False)
    rec.setflags(write=False)
    return plane, rec


class _Words:
    """n int32 words on the device, pre-filled with garbage, `lead` sentinel words in front and 5 behind"""

    def __init__(self, n, lead):
        self.n, self.lead = n, lead
        self.host = np.full(lead + n + 5, SENT32, np.int32)
        self.host[lead:lead + n] = GARB32
        self.dev = _cuda(self.host)
        assert self.dev.data_ptr() % 256 == 0
        self.ptr = self.dev.data_ptr() + 4 * lead

    def get(self):
        """the n words back on the host; the margins must be what they were"""
        got = self.dev.cpu().numpy()
        assert (got[:self.lead] == SENT32).all() and (got[self.lead + self.n:] == SENT32).all()
        return got[self.lead:self.lead + self.n]


def _outline(eng, plane_view, Hi, Wi, cap, lead, null_edges=False):
    """one se_outline_u8 call through the C entry -> (info (2,), the cap records as they are afterwards (cap, 4))"""
    e, info = _Words(4 * cap, lead), _Words(2, 3)
    need = eng.lib.se_outline_u8_workspace_bytes(eng.h, Hi, Wi)
    assert need == ((Hi + 63) // 64) * ((Wi + 63) // 64) * 16 + 255 & ~255
    ws = eng._workspace_bytes(need)
    rc = eng.lib.se_outline_u8(eng.h, eng._stream(), ctypes.c_void_p(plane_view.data_ptr()), Hi, Wi, None if null_edges else ctypes.c_void_p(e.ptr),
                               cap, ctypes.c_void_p(info.ptr), ctypes.c_void_p(ws.data_ptr()), ws.numel())
    assert rc == 0, eng.lib.se_last_error(eng.h).decode()
    return info.get(), e.get().reshape(-1, 4), e


# ---- 1 - 3. the entry against the statement, the round trip through the lasso, and both again under poison -----------------------------
@pytest.mark.parametrize("poison", [0, 0xFF])
@pytest.mark.parametrize("hw", L.SIZES, ids=lambda hw: "%dx%d" % hw)
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_outline_follows_the_statement(eng, seopt, name, hw, poison):
    plane, want = _case(name, hw)
    total = len(want)
    if poison:
        seopt.set("SE_TEST_POISON", poison)
    sel = np.where(plane != 0, 255, 0).astype(np.uint8)
    for off in range(4):                                               # the plane's first byte at every offset mod 4
        pb = _Buf(hw, off, like=plane)
        for cap in sorted({0, max(total - 1, 0), total, total + 7}):
            # lead: the records' first byte at 16 k (one store of 16 bytes) and at 16 k + 4, 8, 12 (four stores of 4)
            info, got, e = _outline(eng, pb.view, hw[0], hw[1], cap, 4 + off)
            written = min(total, cap)
            assert info.tolist() == [total, written], (name, hw, off, cap)
            assert np.array_equal(got[:written], want[:written]), (name, hw, off, cap)
            assert (got[written:] == GARB32).all(), (name, hw, off, cap)     # the records at and beyond `written` are untouched
            if cap == total:                                           # the round trip on the device: the records as lasso edges
                back = eng.lasso_fill_u8(e.dev[e.lead:e.lead + 4 * total].view(-1, 4), hw[0], hw[1])
                assert np.array_equal(back.cpu().numpy(), sel), (name, hw, off)
        info, _, _ = _outline(eng, pb.view, hw[0], hw[1], 0, 4, null_edges=True)
        assert info.tolist() == [total, 0]
        assert np.array_equal(pb.get(), plane)                         # the plane and its margins are what they were
    print("%s %dx%d: %d records" % (name, hw[0], hw[1], total))


def test_known_answers_and_the_binding(eng):
    p = O.empty(37, 53)
    p[5, 9] = 1
    words = eng.outline_u8(_cuda(p), 6).cpu().numpy()
    assert words.shape == (2 + 4 * 6,) and words.dtype == np.int32
    assert words[:18].tolist() == [4, 4, 36, 20, 40, 20, 40, 24, 36, 24, 40, 20, 40, 24, 36, 24, 36, 20]
    for hw, n in (((64, 64), 4), ((100, 90), 8), ((65, 129), 10)):
        assert eng.outline_u8(_cuda(O.full(*hw)), 0).cpu().tolist() == [n, 0]
    assert eng.outline_u8(_cuda(O.checkerboard(64, 64)), 0).cpu().tolist() == [8192, 0]
    w = eng.outline_u8(_cuda(O.checkerboard(130, 70)), 18200).cpu().numpy()
    assert w[:2].tolist() == [18200, 18200] and np.array_equal(w[2:].reshape(-1, 4), _case("checkerboard", (130, 70))[1])


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(eng):
    Hi, Wi = 37, 53
    plane, want = _case("annulus", (Hi, Wi))
    cap = len(want)
    pb = _Buf((Hi, Wi), 1, like=plane)
    e, info = _Words(4 * cap, 4), _Words(2, 3)
    big = torch.full((16 * 8200,), 0x5C, dtype=torch.uint8, device="cuda")                 # room for a 16 x 8193 "plane"
    ws = torch.full((4096,), 0x5C, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0 and pb.buf.data_ptr() % 256 == 0
    lib, h, st = eng.lib, eng.h, eng._stream()
    need = lib.se_outline_u8_workspace_bytes(h, Hi, Wi)
    assert need == 256
    P, E, I, W = pb.view.data_ptr(), e.ptr, info.ptr, ws.data_ptr()
    B = big.data_ptr()
    in_plane = pb.buf.data_ptr() + 4096                                 # 256-byte aligned; its 256 bytes reach into the plane
    bad = [((None, Hi, Wi, E, cap, I, W, need), "plane"), ((P, Hi, Wi, None, cap, I, W, need), "edges_out"), ((P, Hi, Wi, E, cap, None, W, need), "info_out"),
           ((P, Hi, Wi, E, cap, I, None, need), "workspace"), ((P, 15, Wi, E, cap, I, W, need), "Hi"), ((P, Hi, 15, E, cap, I, W, need), "Wi"),
           ((B, 8193, 16, E, cap, I, W, 4096), "Hi"), ((B, 16, 8193, E, cap, I, W, 4096), "Wi"), ((P, Hi, Wi, E, -1, I, W, need), "cap"),
           ((P, Hi, Wi, E, (1 << 24) + 1, I, W, need), "cap"), ((P, Hi, Wi, E + 2, cap - 1, I, W, need), "edges_out must be 4-byte aligned"),
           ((P, Hi, Wi, E, cap, I + 1, W, need), "info_out must be 4-byte aligned"), ((P, Hi, Wi, E, cap, I, W, need - 1), "workspace too small"),
           ((P, Hi, Wi, E, cap, I, W, 0), "workspace too small"), ((P, Hi, Wi, E, cap, I, W + 128, need), "workspace must be 256-byte aligned"),
           ((E + 8, 16, 16, E, cap, I, W, need), "edges_out overlaps plane"), ((P, Hi, Wi, P + Hi * Wi - 1 & ~3, 1, I, W, need), "edges_out overlaps plane"),
           ((P, Hi, Wi, E, cap, P + 3 & ~3, W, need), "info_out overlaps plane"), ((P, Hi, Wi, E, cap, I, in_plane, need), "workspace overlaps plane"),
           ((P, Hi, Wi, E, cap, E + 16 * cap - 4, W, need), "edges_out overlaps info_out"), ((P, Hi, Wi, E, cap, E - 4, W, need), "edges_out overlaps info_out"),
           ((P, Hi, Wi, W + 252, 1, I, W, need), "edges_out overlaps the workspace"), ((P, Hi, Wi, E, cap, W + 248, W, need), "info_out overlaps the workspace")]
    vp = lambda v: None if v is None else ctypes.c_void_p(v)            # noqa: E731
    for (p, hi, wi, ed, c, inf, w, wb), what in bad:
        assert lib.se_outline_u8(h, st, vp(p), hi, wi, vp(ed), c, vp(inf), vp(w), wb) != 0, what
        assert what in lib.se_last_error(h).decode(), (what, lib.se_last_error(h).decode())
    for hi, wi in ((15, 53), (37, 15), (8193, 16), (16, 8193)):
        assert lib.se_outline_u8_workspace_bytes(h, hi, wi) == 0
    assert lib.se_outline_u8_workspace_bytes(h, 8192, 8192) == 128 * 128 * 16
    # cap == 0 takes a null edges_out, and an info_out just behind the plane is no overlap
    assert lib.se_outline_u8(h, st, vp(P), Hi, Wi, None, 0, vp(I), vp(W), need) == 0
    # the bindings refuse planes of another kind and capacities out of range
    A = pb.view
    for call in (lambda: eng.outline_u8(A.view(-1), 4), lambda: eng.outline_u8(A.float(), 4), lambda: eng.outline_u8(A.cpu(), 4),
                 lambda: eng.outline_u8(A, -1), lambda: eng.outline_u8(A, (1 << 24) + 1), lambda: eng.outline_u8(A, 2.0), lambda: eng.outline_u8(A, True),
                 lambda: eng.outline_u8(pb.buf[:15 * 53].view(15, 53), 4)):
        with pytest.raises(_lib.SketchEditHipError):
            call()
    torch.cuda.synchronize()
    assert info.get().tolist() == [cap, 0]                              # the one call that ran
    assert (e.get() == GARB32).all() and np.array_equal(pb.get(), plane) and (big.cpu().numpy() == 0x5C).all()
    assert (ws.cpu().numpy()[256:] == 0x5C).all()


# ---- 5. sessions --------------------------------------------------------------------------------------------------------------------------
def _check_rings(sel, want_plane, fb, f, **kw):
    assert np.array_equal(sel.plane.cpu().numpy(), want_plane)
    rings = sel.rings(**kw)
    assert rings == O.spec_rings(want_plane)
    assert np.array_equal(sel.edges(), O.spec_outline(want_plane))
    assert sum(O.ring_area(r) for r in rings) == sel.count
    assert np.array_equal(fb.get(), f)                                  # the frame is byte-equal after every outline call
    return rings


def test_session_rings_are_the_statement(model):
    f, seed = _blob_frame()
    s, fb = _session(model, f, None, history=1)
    three = [SMALL, HOLE, [(70.0, 90.0), (100.0, 92.5), (85.25, 115.0)]]
    n = 0
    for grow in (0, 3):
        wand = s.select_similar(seed, tolerance=3, grow=grow)
        _check_rings(wand, U.spec_select(f, seed, 3, True, grow), fb, f)
        for rings in ([RING], [RING, HOLE], three):
            sel = s.select_lasso(rings, grow=grow)
            got = _check_rings(sel, L.spec_select_lasso(rings, FHW, grow), fb, f)
            assert got == _check_rings(sel, L.spec_select_lasso(rings, FHW, grow), fb, f, first_cap=8)     # the second call happens
            n += 1
            # the round trip: the rings are a lasso that re-makes the selection
            back = s.select_lasso(got)
            assert np.array_equal(back.plane.cpu().numpy(), sel.plane.cpu().numpy()) and (back.box, back.count) == (sel.box, sel.count)
    assert n == 6
    assert len(s.select_lasso([RING, HOLE]).rings()) == 2 and len(s.select_lasso(three).rings()) == 3
    lasso, wand = s.select_lasso([RING]), s.select_similar(seed, tolerance=1, grow=1)
    minus = s.combine(lasso, wand, "subtract")                           # a lasso minus a wand selection
    want = L.spec_combine(lasso.plane.cpu().numpy(), wand.plane.cpu().numpy(), L.SUBTRACT)
    assert 0 < minus.count < lasso.count
    _check_rings(minus, want, fb, f)
    inv = s.invert(lasso)                                                # touches all four frame borders
    got = _check_rings(inv, L.spec_combine(lasso.plane.cpu().numpy(), None, L.INVERT), fb, f, first_cap=8)
    assert got[0] == [(0, 0), (FHW[1], 0), (FHW[1], FHW[0]), (0, FHW[0])] and len(got) == 2
    back = s.select_lasso(got)
    assert np.array_equal(back.plane.cpu().numpy(), inv.plane.cpu().numpy()) and (back.box, back.count) == (inv.box, inv.count)
    empty = s.combine(lasso, lasso, "subtract")
    assert empty.rings() == [] and empty.edges().shape == (0, 4)
    assert serve.rings_svg_path(lasso.rings()).startswith("M ") and not s.can_undo
    assert np.array_equal(fb.get(), f)


def test_session_lock_rings(model):
    f, _ = _blob_frame()
    s, fb = _session(model, f, None)
    assert s.lock_rings() == []
    sel = s.select_lasso([RING, HOLE], grow=1)
    s.set_lock(sel)
    assert s.lock_rings() == sel.rings() == O.spec_rings(L.spec_select_lasso([RING, HOLE], FHW, 1))
    lock = np.zeros(FHW, np.uint8)                                       # an uploaded lock
    lock[55:70, 30:60] = 1
    lock[::9, ::7] = 1
    s.set_lock(lock)
    assert s.lock_rings(first_cap=8) == O.spec_rings(lock)
    s.set_lock(None)
    assert s.lock_rings() == [] and np.array_equal(fb.get(), f)


# ---- 6. one larger plane: the scan crosses more than one wave's worth of tiles ------------------------------------------------------------------
def test_a_1080p_disc(eng):
    Hi, Wi = 1081, 1921
    yy, xx = np.mgrid[:Hi, :Wi]
    plane = np.where((yy - 540) ** 2 + (xx - 960) ** 2 <= 500 ** 2, 255, 0).astype(np.uint8)
    want = O.spec_outline(plane)
    assert ((Hi + 63) // 64) * ((Wi + 63) // 64) * 4 > 256 * 4          # more counts than the scan has threads, in chunks of 9
    dev = _cuda(plane)
    words = eng.outline_u8(dev, len(want) + 3).cpu().numpy()
    assert words[:2].tolist() == [len(want), len(want)]
    assert np.array_equal(words[2:2 + 4 * len(want)].reshape(-1, 4), want)
    words = eng.outline_u8(dev, 1000).cpu().numpy()
    assert words[:2].tolist() == [len(want), 1000] and np.array_equal(words[2:].reshape(-1, 4), want[:1000])
    rings = serve.outline_rings(want)
    assert len(rings) == 1 and O.ring_area(rings[0]) == int((plane != 0).sum())
    assert np.array_equal(eng.lasso_fill_u8(_cuda(want), Hi, Wi).cpu().numpy(), plane)
