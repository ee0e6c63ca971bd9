"""Host tests of the outline of a selection (no GPU): the statement of tests/outline_util.py on its known answers and
through the lasso's statement (the records re-make the plane), serve.outline_rings against rings traced straight from the pixels
and on its three properties, rings_svg_path, the kernels' mask arithmetic in Python integers against the statement, the sessions
against a scripted backend, and the two new symbols."""
import functools
import os
import re

import numpy as np
import pytest
from scipy import ndimage

from sketchedit_amd import _lib, serve
import lasso_util as L
import outline_util as O
import select_util as U
from test_fill_host import _OldStub, _Stub as _FillStub, _names
from test_lasso_host import _Stub as _LassoStub
from test_select_host import _Stub as _SelectStub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HW = (400, 600)
CASES = [(f, hw) for hw in L.SIZES for f in O.PATTERNS]
IDS = ["%s-%dx%d" % (f.__name__, hw[0], hw[1]) for f, hw in CASES]


@functools.lru_cache(maxsize=None)
def _case(f, hw):
    """(plane, the statement's records): computed once, shared, never written"""
    plane = f(*hw)
    rec = O.spec_outline(plane)
    plane.setflags(write=False)
    rec.setflags(write=False)
    return plane, rec


# ---- the statement ------------------------------------------------------------------------------------------------------------------------
def test_known_answers():
    for hw in ((16, 16), (65, 129)):
        for y, x in ((0, 0), (5, 9), (hw[0] - 1, hw[1] - 1)):
            p = O.empty(*hw)
            p[y, x] = 3
            assert O.spec_outline(p).tolist() == [[4 * x, 4 * y, 4 * x + 4, 4 * y], [4 * x + 4, 4 * y + 4, 4 * x, 4 * y + 4],
                                                  [4 * x + 4, 4 * y, 4 * x + 4, 4 * y + 4], [4 * x, 4 * y + 4, 4 * x, 4 * y]]
    assert O.spec_outline(O.full(64, 64)).tolist() == [[0, 0, 256, 0], [256, 256, 0, 256], [256, 0, 256, 256], [0, 256, 0, 0]]
    assert len(O.spec_outline(O.full(100, 90))) == 8
    assert len(O.spec_outline(O.full(65, 129))) == 10
    assert len(O.spec_outline(O.checkerboard(64, 64))) == 8192
    assert len(O.spec_outline(O.checkerboard(130, 70))) == 18200
    assert O.spec_outline(O.empty(37, 53)).shape == (0, 4)
    # the order: tiles row-major; N, S by (y, x), then E, W by (x, y).  Two pixels of one tile, then one of the next tile
    p = O.empty(16, 130)
    p[2, 5] = p[1, 7] = p[0, 64] = 255
    rec = O.spec_outline(p).tolist()
    assert rec[:8] == [[28, 4, 32, 4], [20, 8, 24, 8], [32, 8, 28, 8], [24, 12, 20, 12],          # N (1,7) (2,5); S (1,7) (2,5)
                       [24, 8, 24, 12], [32, 4, 32, 8], [20, 12, 20, 8], [28, 8, 28, 4]]          # E x=5, x=7; W x=5, x=7
    assert rec[8:] == [[256, 0, 260, 0], [260, 4, 256, 4], [260, 0, 260, 4], [256, 4, 256, 0]]
    # a run is split at a tile boundary and nowhere else
    p = O.empty(16, 130)
    p[3, 60:70] = 1
    rec = O.spec_outline(p).tolist()
    assert [240, 12, 256, 12] in rec and [256, 12, 280, 12] in rec and len(rec) == 6


@pytest.mark.parametrize("f,hw", CASES, ids=IDS)
def test_the_records_re_make_the_plane_through_the_lasso(f, hw):
    plane, rec = _case(f, hw)
    assert rec.dtype == np.int32 and rec.shape[1] == 4
    assert len(rec) <= L.LIM and (rec >= 0).all() and (rec[:, [0, 2]] <= 4 * hw[1]).all() and (rec[:, [1, 3]] <= 4 * hw[0]).all()
    want = np.where(plane != 0, 255, 0).astype(np.uint8)
    assert np.array_equal(L.spec_lasso(rec, *hw), want)
    vertical = rec[rec[:, 0] == rec[:, 2]]                              # horizontal edges never span a scanline
    assert np.array_equal(L.spec_lasso(vertical, *hw), want)
    # every boundary side once: the records' lengths add up to the sides of the set
    p = np.pad(plane != 0, 1)
    c = p[1:-1, 1:-1]
    sides = sum(int((c & ~n).sum()) for n in (p[:-2, 1:-1], p[2:, 1:-1], p[1:-1, 2:], p[1:-1, :-2]))
    assert int(np.abs(rec[:, 2] - rec[:, 0]).sum() + np.abs(rec[:, 3] - rec[:, 1]).sum()) == 4 * sides


def test_the_largest_record_count_of_the_test_planes():
    assert max(len(_case(f, hw)[1]) for f, hw in CASES) == 18200


# ---- the rings ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f,hw", CASES, ids=IDS)
def test_outline_rings_properties(f, hw):
    plane, rec = _case(f, hw)
    rings = serve.outline_rings(rec)
    assert rings == O.spec_rings(plane)                                  # traced from the pixels, no records and no tiles
    sel = plane != 0
    # the signed areas sum to the count
    assert sum(O.ring_area(r) for r in rings) == int(sel.sum())
    # 4-connected components of the set + 8-connected components of the zero-padded complement - 1 (the outside)
    n4 = ndimage.label(sel)[1]
    n8 = ndimage.label(~np.pad(sel, 1), structure=np.ones((3, 3), int))[1]
    assert len(rings) == n4 + n8 - 1
    assert sum(1 for r in rings if O.ring_area(r) > 0) == n4 and all(O.ring_area(r) != 0 for r in rings)
    # the round trip, through the front end's own conversion
    if rings:
        edges = L.spec_edges(rings, hw)
        assert len(edges) <= serve.LASSO_MAX_EDGES and np.array_equal(edges, serve.lasso_edges(rings, hw))
        assert np.array_equal(L.spec_lasso(edges, *hw), np.where(sel, 255, 0))
    else:
        assert not sel.any()
    # start vertices, order, no collinear point, integers
    starts = [(r[0][1], r[0][0]) for r in rings]
    assert starts == sorted(starts) and len(set(starts)) == len(starts)
    for r in rings:
        assert len(r) >= 4 and min(r, key=lambda q: (q[1], q[0])) == r[0]
        assert all(isinstance(v, int) for q in r for v in q)
        for a, b, c in zip(r, r[1:] + r[:1], r[2:] + r[:2]):
            assert (a[0] == b[0]) != (a[1] == b[1]) and (a[0] == b[0]) != (b[0] == c[0])      # axis parallel, and a turn at every point


def test_ring_orientation_start_and_tile_splits():
    p = O.empty(100, 90)
    p[10:80, 20:85] = 255                                                # spans four tiles
    p[30:40, 30:50] = 0                                                  # a hole
    rec = O.spec_outline(p)
    assert len(rec) == 8 + 4
    rings = serve.outline_rings(rec)
    assert rings == [[(20, 10), (85, 10), (85, 80), (20, 80)], [(30, 30), (30, 40), (50, 40), (50, 30)]]
    assert O.ring_area(rings[0]) == 70 * 65 and O.ring_area(rings[1]) == -200      # clockwise on the screen; the hole the other way
    # any order of the records gives the same rings
    perm = np.random.RandomState(3).permutation(len(rec))
    assert serve.outline_rings(rec[perm]) == rings
    assert serve.outline_rings(np.zeros((0, 4), np.int32)) == [] and serve.outline_rings([]) == []
    # records that are not a whole outline: a capped download
    for bad in (rec[:5], rec[1:], np.concatenate([rec, rec[:1]])):
        with pytest.raises(ValueError):
            serve.outline_rings(bad)
    with pytest.raises(ValueError):
        serve.outline_rings([[0, 0, 6, 0], [6, 0, 6, 4], [6, 4, 0, 4], [0, 4, 0, 0]])        # not on the corner lattice
    with pytest.raises(ValueError):
        serve.outline_rings([[0, 0, 4, 4], [4, 4, 0, 0]])                                      # not axis parallel


def test_diagonal_pixels_are_two_rings_that_touch():
    p = O.empty(16, 16)
    p[3, 4] = p[4, 5] = 255
    rings = serve.outline_rings(O.spec_outline(p))
    assert rings == [[(4, 3), (5, 3), (5, 4), (4, 4)], [(5, 4), (6, 4), (6, 5), (5, 5)]]      # 4-connected: two, touching at (5, 4)
    p = O.empty(16, 16)
    p[3, 5] = p[4, 4] = 255                                              # the other diagonal
    assert serve.outline_rings(O.spec_outline(p)) == [[(5, 3), (6, 3), (6, 4), (5, 4)], [(4, 4), (5, 4), (5, 5), (4, 5)]]
    # across a tile corner too
    p = O.empty(70, 70)
    p[63, 63] = p[64, 64] = 255
    assert serve.outline_rings(O.spec_outline(p)) == [[(63, 63), (64, 63), (64, 64), (63, 64)], [(64, 64), (65, 64), (65, 65), (64, 65)]]


def test_a_hole_whose_cells_touch_diagonally_is_one_ring():
    p = O.empty(16, 16)
    p[2:8, 2:8] = 255
    p[4, 4] = p[5, 5] = 0                                                # the background is 8-connected: one hole
    rings = serve.outline_rings(O.spec_outline(p))
    assert rings[0] == [(2, 2), (8, 2), (8, 8), (2, 8)] and len(rings) == 2
    assert rings[1] == [(4, 4), (4, 5), (5, 5), (5, 6), (6, 6), (6, 5), (5, 5), (5, 4)]       # through (5, 5) twice
    assert O.ring_area(rings[1]) == -2 and rings == O.spec_rings(p)
    assert np.array_equal(L.spec_lasso(L.spec_edges(rings, (16, 16)), 16, 16), p)


def test_rings_svg_path():
    assert serve.rings_svg_path([]) == ""
    assert serve.rings_svg_path([[(4, 3), (5, 3), (5, 4), (4, 4)]]) == "M 4 3 L 5 3 L 5 4 L 4 4 Z"
    assert (serve.rings_svg_path([[(0, 0), (2, 0), (2, 2), (0, 2)], [(5, 4), (6, 4), (6, 5), (5, 5)]])
            == "M 0 0 L 2 0 L 2 2 L 0 2 Z M 5 4 L 6 4 L 6 5 L 5 5 Z")
    d = serve.rings_svg_path(serve.outline_rings(_case(O.annulus, (37, 53))[1]))
    assert d.count("M") == d.count("Z") == 2 and "  " not in d and re.fullmatch(r"[MLZ0-9 ]+", d)


# ---- the kernels' arithmetic ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", L.SIZES, ids=lambda hw: "%dx%d" % hw)
def test_tiled_arithmetic_is_the_statement(hw):
    for f in O.PATTERNS + O.MORE_PATTERNS:
        plane = f(*hw)
        want = O.spec_outline(plane)
        info, rec = O.tiled_outline(plane)
        assert info == [len(want), len(want)] and np.array_equal(rec, want), (f.__name__, hw)
    plane, want = _case(O.noise, hw)
    for cap in (0, 1, len(want) // 2, len(want) - 1, len(want) + 7):
        info, rec = O.tiled_outline(plane, cap)
        assert info == [len(want), min(cap, len(want))] and np.array_equal(rec, want[:cap]), (hw, cap)


def test_mask_runs_at_the_ends_of_the_word():
    assert O._mask_runs(O.M64) == [(0, 64)] and O._mask_runs(0) == []
    assert O._mask_runs(1 | 1 << 63) == [(0, 1), (63, 64)]
    assert O._mask_runs(0b0110 | 0xF << 60) == [(1, 3), (60, 64)]
    assert O._mask_runs(int("01" * 32, 2)) == [(2 * k, 2 * k + 1) for k in range(32)]


def test_the_extra_planes_are_what_their_names_say():
    assert set(np.unique(O.values(37, 53))) == {0, 1, 7, 255}
    assert int((O.tile_corners(65, 129) != 0).sum()) == 4 and int((O.tile_corners(64, 64) != 0).sum()) == 1 and not O.tile_corners(37, 53).any()
    assert int((O.rect_60_70(130, 70) != 0).sum()) == 11 * 10 and len(O.spec_outline(O.rect_60_70(100, 90))) == 8
    n = O.noise(37, 53)
    assert 0.4 < (n != 0).mean() < 0.6 and len(np.unique(n)) > 200


# ---- the sessions against a scripted backend -------------------------------------------------------------------------------------------------
class _Stub(_LassoStub):
    """... with the one call of DESIGN.md 6q: the statement itself, on numpy planes"""

    def outline(self, plane, cap):
        self.calls.append(("outline", id(plane), cap))
        rec = O.spec_outline(plane)
        return len(rec), rec[:cap]


RING = [(300, 200), (340, 200), (340, 230), (300, 230)]
HOLE = [(310, 210), (310, 220), (330, 220), (330, 210)]                  # as rings() returns a hole: counter-clockwise


def _session(stub, **kw):
    s = serve.EditSession(None, U._noise(HW, 5), backend=stub, **kw)
    stub.calls.clear()
    return s


def test_rings_is_one_call_two_when_the_first_cap_is_small_none_when_empty():
    stub = _Stub()
    s = _session(stub, history=1)
    sel = s.select_lasso([RING, HOLE])
    stub.calls.clear()
    assert sel.rings() == [RING, HOLE]
    assert stub.calls == [("outline", id(sel.plane), 4096)]
    stub.calls.clear()
    total = len(O.spec_outline(sel.plane))
    assert total > 8
    assert sel.rings(first_cap=8) == [RING, HOLE]
    assert stub.calls == [("outline", id(sel.plane), 8), ("outline", id(sel.plane), total)]
    stub.calls.clear()
    assert sel.rings(first_cap=total) == [RING, HOLE] and len(stub.calls) == 1      # total == cap: no second call
    stub.calls.clear()
    e = sel.edges()
    assert stub.calls == [("outline", id(sel.plane), 4096)]
    assert isinstance(e, np.ndarray) and e.dtype == np.int32 and np.array_equal(e, O.spec_outline(sel.plane))
    stub.calls.clear()
    assert sel.rings(first_cap=0) == [RING, HOLE] and [c[2] for c in stub.calls] == [0, total]
    # an empty selection: no backend call
    empty = s.combine(sel, sel, "subtract")
    stub.calls.clear()
    assert empty.rings() == [] and empty.edges().shape == (0, 4) and stub.calls == []
    for bad in (-1, 1.5, True, (1 << 24) + 1):
        with pytest.raises(ValueError):
            sel.rings(first_cap=bad)
    assert stub.calls == [] and not s.can_undo


def test_rings_round_trip_through_select_lasso():
    stub = _Stub()
    s = _session(stub)
    f = np.zeros(HW, np.uint8)
    f[100:140, 200:260] = O.noise(40, 60)
    f[5, 7] = f[6, 8] = 255
    a = serve.Selection(stub, np.where(f != 0, 255, 0).astype(np.uint8), *L.box_count(f), HW)      # noise, and a diagonal pair
    rings = a.rings()
    b = s.select_lasso(rings)
    assert np.array_equal(b.plane, a.plane) and (b.box, b.count) == (a.box, a.count)
    assert "65 536" in serve.EditSession.select_lasso.__doc__ and "rings()" in serve.EditSession.select_lasso.__doc__


def test_lock_rings():
    stub = _Stub()
    s = _session(stub)
    assert s.lock_rings() == [] and stub.calls == []                     # no lock: nothing is asked
    sel = s.select_lasso([RING, HOLE])
    s.set_lock(sel)
    stub.calls.clear()
    assert s.lock_rings() == [RING, HOLE] == sel.rings()
    assert stub.calls[0] == ("outline", id(s._lock_plane), 4096) and _names(stub) == ["outline", "outline"]
    plane = np.zeros(HW, bool)                                           # an uploaded lock: any non-zero byte is locked
    plane[0:3, 0:2] = True
    plane[399, 599] = True
    s.set_lock(plane)
    assert s.lock_rings(first_cap=2) == [[(0, 0), (2, 0), (2, 3), (0, 3)], [(599, 399), (600, 399), (600, 400), (599, 400)]]
    s.set_lock(None)
    assert s.lock_rings() == []


def test_a_backend_without_outline_fails_in_rings_only():
    stub = _LassoStub()
    s = _session(stub)
    sel = s.select_lasso([RING])
    s.set_lock(sel)
    stub.calls.clear()
    for call in (sel.rings, sel.edges, s.lock_rings):
        with pytest.raises(NotImplementedError, match="cannot extract outlines"):
            call()
    assert stub.calls == []
    assert s.combine(sel, sel, "subtract").rings() == []                 # an empty selection needs no backend


def test_an_outline_of_more_runs_than_one_call_returns_is_refused_after_the_first_call():
    class _Huge(_Stub):
        def outline(self, plane, cap):
            self.calls.append(("outline", id(plane), cap))
            return (1 << 24) + 1, np.zeros((cap, 4), np.int32)

    stub = _Huge()
    s = _session(stub)
    sel = s.select_lasso([RING])
    stub.calls.clear()
    with pytest.raises(ValueError, match="more than one call returns"):
        sel.rings(first_cap=16)
    assert stub.calls == [("outline", id(sel.plane), 16)]


def test_existing_calls_issue_what_they_issued():
    """edit, fill, select_* and combine on a backend WITH outline never call it, and on the backends of before -- where it does
    not exist -- they run as they did"""
    sk = np.zeros(HW, np.uint8)
    sk[200:210, 300:330] = 255
    mask = np.zeros(HW, np.uint8)
    mask[200:230, 300:340] = 1
    f = U._noise(HW, 5)
    f[200:230, 300:340] = U.REGION
    seqs = {}
    for k, cls in enumerate((_LassoStub, _Stub)):
        for lock in (False, True):
            stub = cls()
            s = serve.EditSession(None, f, backend=stub, history=2)
            if lock:
                s.set_lock(mask)
            stub.calls.clear()
            s.edit(sk, max_grow=0)
            s.edit_strokes([([(30, 20), (60, 30)], 3)])
            s.fill(mask)
            s.fill_strokes([([(300.5, 200.0), (340.0, 230.25)], 12.0)])
            a = s.select_similar((210, 320))
            b = s.select_lasso([RING], grow=2)
            c = s.combine(a, b, "xor")
            s.invert(c)
            s.fill_selection(b)
            s.fill_similar((210, 320))
            s.fill_lasso([RING])
            s.set_lock(b)
            a.mask()
            s.undo()
            s.redo()
            seqs[k, lock] = _names(stub)
            assert stub.calls and "outline" not in _names(stub)
    assert seqs[0, False] == seqs[1, False] and seqs[0, True] == seqs[1, True]
    for old in (_OldStub, _FillStub, _SelectStub):                       # the backends of before: nothing new is asked of them
        stub = old()
        s = serve.EditSession(None, f, backend=stub, history=2)
        stub.calls.clear()
        s.edit(sk, max_grow=0)
        s.undo()
        assert stub.calls and "outline" not in _names(stub) and s.lock_rings() == []


def test_model_backend_outline_is_one_download():
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
            self.calls, self.out = [], []

        def outline_u8(self, plane, cap):
            self.calls.append(("outline_u8", cap))
            rec = O.spec_outline(plane)
            words = np.full(2 + 4 * cap, -7, np.int32)                   # behind the written records: whatever was there
            w = min(len(rec), cap)
            words[:2] = [len(rec), w]
            words[2:2 + 4 * w] = rec[:w].reshape(-1)
            self.out.append(_T(words))
            return self.out[-1]

    be = serve._ModelBackend.__new__(serve._ModelBackend)
    be.model = _Model()
    plane, want = _case(O.annulus, (37, 53))
    for cap in (0, 5, len(want), len(want) + 9):
        total, rec = be.outline(plane, cap)
        assert total == len(want) and rec.shape == (min(cap, len(want)), 4) and np.array_equal(rec, want[:cap])
    assert be.model.calls == [("outline_u8", c) for c in (0, 5, len(want), len(want) + 9)] and [t.n for t in be.model.out] == [1] * 4
    sel = serve.Selection(be, plane, *L.box_count(plane), (37, 53))
    assert sel.rings(first_cap=5) == O.spec_rings(plane) and be.model.calls[-2:] == [("outline_u8", 5), ("outline_u8", len(want))]


# ---- the C-ABI -------------------------------------------------------------------------------------------------------------
def test_abi_has_two_new_symbols_in_a_header_of_their_own():
    hdr = open(os.path.join(ROOT, "include", "sketchedit_outline.h")).read()
    declared = re.findall(r"^(?:int|size_t)\s+(se_\w+)\(", hdr, re.M)
    assert declared == _lib.abi_names("sketchedit_outline.h") == ["se_outline_u8_workspace_bytes", "se_outline_u8"]
    for name in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if name != "sketchedit_outline.h":
            assert "se_outline" not in open(os.path.join(ROOT, "include", name)).read(), name
    assert "se_outline.hip" in _lib.SOURCES and _lib.SOURCES[-1] == "se_api.hip"
    assert re.search(r"#define SE_OUTLINE_TILE 64\b", hdr) and re.search(r"#define SE_OUTLINE_MAX_CAP \(1 << 24\)", hdr)
    assert (_lib.OUTLINE_TILE, _lib.OUTLINE_MAX_CAP, serve.OUTLINE_MAX_CAP, O.TILE) == (64, 1 << 24, 1 << 24, 64)
    # the header's known answers are the statement's
    assert "8192 records at 64 x 64" in hdr and "18 200" in hdr
    import ctypes
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    lib = ctypes.CDLL(_lib.LIB_PATH)                                    # the built library, as the other host tests load it
    for s in declared:
        getattr(lib, s)
    from sketchedit_amd import kernel_labels
    args = "(unsigned char const*, int, int, int, int*, int*, int)"
    assert kernel_labels.label_of("void se::outline_tile_kernel<false>" + args) == "outline_count"
    assert kernel_labels.label_of("outline_tile_kernel<true>" + args) == "outline_emit"
    assert kernel_labels.label_of("outline_scan_kernel(int*, int, int, int*)") == "outline_scan"
    misc = open(os.path.join(_lib.CSRC, "se_misc.hip")).read()
    for label in ("outline_count", "outline_scan", "outline_emit"):
        assert '"%s"' % label in misc and label in set(kernel_labels.KERNEL_LABELS.values())


def test_the_kernels_cross_compile_for_gfx950(tmp_path):
    import shutil
    import subprocess
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc on this machine")
    obj = str(tmp_path / "se_outline.o")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(_lib.CSRC, "se_outline.hip"), "-o", obj])
    assert os.path.getsize(obj) > 0
