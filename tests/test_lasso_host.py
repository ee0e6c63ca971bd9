"""Host tests of lasso selections and the algebra of selections: the statement of tests/lasso_util.py against
independent formulations (exact rationals counting to the RIGHT, a direct paint of rectilinear rings, Pillow's polygon away
from the edges), the kernel's tile-by-tile algorithm in Python integers against the statement, serve.lasso_edges / lasso_box,
the host logic of EditSession.select_lasso / combine / invert / fill_lasso / set_lock(selection) against a scripted backend that
logs every call, and the new entries' place in the C-ABI.  CPU only."""
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from sketchedit_amd import _lib, serve
import lasso_util as L
import select_util as U
from test_fill_host import _OldStub, _Stub as _FillStub, _names
from test_select_host import _Stub as _SelectStub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HW = (400, 600)


# ---- the two known answers ---------------------------------------------------------------------------------------------------------
def test_known_answers():
    got = L.spec_lasso(L.ring_edges([(6, 6), (26, 6), (26, 18), (6, 18)]), 6, 8)
    want = np.zeros((6, 8), np.uint8)
    want[1:4, 2:7] = 255                       # top and right boundaries in, left and bottom out
    assert np.array_equal(got, want)
    for Hi, Wi in ((6, 8), (16, 16), (37, 53)):
        assert (L.spec_lasso(L.whole_frame(Hi, Wi), Hi, Wi) == 255).all()
    assert not L.spec_lasso(np.zeros((0, 4), np.int32), 16, 16).any()
    # the order and the direction of the edges play no part
    e = L.star(37, 53)
    want = L.spec_lasso(e, 37, 53)
    assert np.array_equal(L.spec_lasso(e[::-1], 37, 53), want) and np.array_equal(L.spec_lasso(e[:, [2, 3, 0, 1]], 37, 53), want)


# ---- the statement against exact rationals, counting to the right --------------------------------------------------------------------
def _right_parity(edges, Hi, Wi):
    """-> (plane of 0 / 255, on_edge): the parity of the crossings strictly to the RIGHT of every centre in exact rationals;
    on_edge marks the centres that lie on an edge (a horizontal one, or a vertex, included)"""
    plane, on_edge = np.zeros((Hi, Wi), np.uint8), np.zeros((Hi, Wi), bool)
    e = [tuple(int(v) for v in row) for row in edges]
    for y in range(Hi):
        py = 4 * y + 2
        for x in range(Wi):
            px, odd = 4 * x + 2, False
            for ax, ay, bx, by in e:
                if ay == by:
                    on_edge[y, x] |= py == ay and min(ax, bx) <= px <= max(ax, bx)
                    continue
                if not min(ay, by) <= py <= max(ay, by):
                    continue
                xc = ax + Fraction((py - ay) * (bx - ax), by - ay)
                on_edge[y, x] |= xc == px
                if min(ay, by) <= py < max(ay, by) and xc > px:
                    odd = not odd
            plane[y, x] = 255 if odd else 0
    return plane, on_edge


def _random_ring(rng, Hi, Wi, n):
    """a star-shaped ring of n vertices around a random centre, in quarter pixels, inside the frame's rectangle"""
    cx, cy = rng.uniform(0.3, 0.7) * 4 * Wi, rng.uniform(0.3, 0.7) * 4 * Hi
    ang = np.sort(rng.uniform(0, 2 * math.pi, n))
    rad = rng.uniform(0.1, 1.0, n)
    return [(int(np.clip(round(cx + r * 2 * Wi * math.cos(a)), 0, 4 * Wi)), int(np.clip(round(cy + r * 2 * Hi * math.sin(a)), 0, 4 * Hi)))
            for a, r in zip(ang, rad)]


def _statement_cases():
    rng = np.random.RandomState(11)
    for k, (Hi, Wi) in enumerate([(16, 16), (17, 31), (24, 40), (37, 53)]):
        for n in (3, 4, 7, 12):
            yield Hi, Wi, L.ring_edges(_random_ring(rng, Hi, Wi, n))
        yield Hi, Wi, L.ring_edges(_random_ring(rng, Hi, Wi, 5), _random_ring(rng, Hi, Wi, 9))       # two rings
        for pts in (5, 7, 9):                                                                          # self-crossing stars
            p = _random_ring(rng, Hi, Wi, pts)
            yield Hi, Wi, L.ring_edges([p[(2 * i) % pts] for i in range(pts)])
        for shape in (L.rect_on_centres, L.triangle_on_scanlines, L.star, L.ring_in_ring, L.horizontal_and_zero_length, L.sliver,
                      L.left_and_right, L.collinear):
            yield Hi, Wi, shape(Hi, Wi)


def test_statement_against_exact_rationals_to_the_right():
    n = centres = 0
    for Hi, Wi, edges in _statement_cases():
        want, on_edge = _right_parity(edges, Hi, Wi)
        got = L.spec_lasso(edges, Hi, Wi)
        assert np.array_equal(got[~on_edge], want[~on_edge]), (Hi, Wi, edges.tolist())
        n, centres = n + 1, centres + int((~on_edge).sum())
    assert n == 64 and centres > 40000


# ---- rectilinear rings on the pixel-corner lattice -------------------------------------------------------------------------------------
def test_rectilinear_rings_against_a_paint_of_their_cells():
    rng = np.random.RandomState(5)
    for Hi, Wi in ((16, 16), (37, 53), (65, 129)):
        for _ in range(6):
            # a histogram: column x holds the cells [base - h[x], base); its outline walks the baseline and the profile back
            x0 = rng.randint(0, Wi // 2)
            k = rng.randint(1, Wi - x0 + 1)
            base = rng.randint(Hi // 2, Hi + 1)
            h = rng.randint(1, base + 1, k)
            want = np.zeros((Hi, Wi), np.uint8)
            ring = [(4 * x0, 4 * base), (4 * (x0 + k), 4 * base)]
            for x in range(k - 1, -1, -1):
                want[base - h[x]:base, x0 + x] = 255
                ring += [(4 * (x0 + x + 1), 4 * (base - h[x])), (4 * (x0 + x), 4 * (base - h[x]))]
            edges = L.ring_edges(ring)
            assert np.array_equal(L.spec_lasso(edges, Hi, Wi), want)
            box = serve.lasso_box(edges, (Hi, Wi))
            assert box == L.box_count(want)[0]                           # on the corner lattice the bound is the tight box


# ---- Pillow's polygon, away from the edges -------------------------------------------------------------------------------------------------
def _far_from_edges(edges, Hi, Wi, dist):
    """centres more than `dist` pixels from every edge (float64; the margin swallows its rounding)"""
    py, px = np.mgrid[0:Hi, 0:Wi] + 0.5
    far = np.ones((Hi, Wi), bool)
    for ax, ay, bx, by in (np.asarray(edges, np.float64) / 4).tolist():
        dx, dy = bx - ax, by - ay
        dd = dx * dx + dy * dy
        t = np.clip(((px - ax) * dx + (py - ay) * dy) / dd, 0, 1) if dd > 0 else np.zeros((Hi, Wi))
        far &= np.hypot(px - ax - t * dx, py - ay - t * dy) > dist
    return far


def test_statement_against_pillow_polygon_away_from_the_edges():
    from PIL import Image, ImageDraw
    rng = np.random.RandomState(3)
    checked = inside = 0
    for Hi, Wi in ((37, 53), (65, 129), (100, 90)):
        rings = [_random_ring(rng, Hi, Wi, n) for n in (3, 6, 11, 24)] + [L._ellipse(Hi, Wi, 40)]
        for ring in rings:
            edges = L.ring_edges(ring)
            img = Image.new("L", (Wi, Hi), 0)
            ImageDraw.Draw(img).polygon([(x / 4, y / 4) for x, y in ring], fill=255)
            far = _far_from_edges(edges, Hi, Wi, 1.0)
            got = L.spec_lasso(edges, Hi, Wi)
            assert np.array_equal(got[far], np.asarray(img)[far])
            checked, inside = checked + int(far.sum()), inside + int((got[far] == 255).sum())
    assert checked > 30000 and 5000 < inside < checked - 5000


# ---- the kernel's algorithm in Python integers ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", L.SIZES, ids=lambda hw: "%dx%d" % hw)
def test_tiled_algorithm_is_the_statement(hw):
    """the cull predicate, the chunks of 256, the upward orientation -- and the optional left-parity fold, which the kernel does
    not use -- against the statement, on every shape the device tests run"""
    Hi, Wi = hw
    for shape in L.SHAPES:
        if shape in (L.polygon_300, L.polygon_600) and hw not in ((37, 53), (65, 129)):
            continue                                                     # (Python integers: the long polygons at two sizes)
        edges = shape(Hi, Wi)
        want = L.spec_lasso(edges, Hi, Wi)
        stats = []
        assert np.array_equal(L.tiled_lasso(edges, Hi, Wi, stats=stats), want), shape.__name__
        assert np.array_equal(L.tiled_lasso(edges, Hi, Wi, fold_left=True), want), shape.__name__
        tiles = ((Hi + 15) // 16) * ((Wi + 63) // 64)
        assert len(stats) == tiles * ((len(edges) + 255) // 256)          # 300 edges: two chunks, 600: three
        if shape is L.polygon_300 and hw == (65, 129):
            assert max(stats) < 150 and sum(stats) < len(edges) * tiles // 3          # the cull keeps a fraction


def test_shapes_are_what_their_names_say():
    for Hi, Wi in L.SIZES:
        assert not L.spec_lasso(L.collinear(Hi, Wi), Hi, Wi).any() and not L.spec_lasso(L.sliver(Hi, Wi), Hi, Wi).any()
        assert serve.lasso_box(L.sliver(Hi, Wi), (Hi, Wi)) is not None                  # a box, and no pixel in it
        rect = L.spec_lasso(L.rect_on_centres(Hi, Wi), Hi, Wi)
        assert L.box_count(rect) == ((1, 2, Hi - 2, Wi - 1), (Hi - 3) * (Wi - 3))
        st = L.spec_lasso(L.star(Hi, Wi), Hi, Wi)
        assert st[Hi // 2, Wi // 2] == 0 and st.any()                                   # the middle is a hole
        rr = L.spec_lasso(L.ring_in_ring(Hi, Wi), Hi, Wi)
        assert rr[Hi // 2, Wi // 2] == 0 and rr[Hi // 2, 3] == 255
        assert (L.polygon_300(Hi, Wi).shape[0], L.polygon_600(Hi, Wi).shape[0]) == (300, 600)
        oor = L.out_of_range(Hi, Wi).astype(np.int64)
        assert oor.min() == -2 ** 31 and oor.max() == 2 ** 31 - 1
        assert np.array_equal(L.spec_lasso(oor, Hi, Wi), L.spec_lasso(np.clip(oor, 0, L.LIM), Hi, Wi))


# ---- lasso_box and lasso_edges ----------------------------------------------------------------------------------------------------------------
def test_lasso_box_holds_every_selected_pixel():
    rng = np.random.RandomState(9)
    cases = [(Hi, Wi, shape(Hi, Wi)) for Hi, Wi in L.SIZES for shape in L.SHAPES if shape not in (L.no_edges, L.out_of_range)]
    for Hi, Wi in ((16, 16), (37, 53), (65, 129)):
        cases += [(Hi, Wi, L.ring_edges(_random_ring(rng, Hi, Wi, n))) for n in (3, 5, 8, 13) for _ in range(5)]
    empties = 0
    for Hi, Wi, edges in cases:
        plane = L.spec_lasso(edges, Hi, Wi)
        box = serve.lasso_box(edges, (Hi, Wi))
        if box is None:
            assert not plane.any()
            empties += 1
            continue
        y0, x0, y1, x1 = box
        assert 0 <= y0 < y1 <= Hi and 0 <= x0 < x1 <= Wi
        outside = plane.copy()
        outside[y0:y1, x0:x1] = 0
        assert not outside.any()
    assert serve.lasso_box(np.zeros((0, 4), np.int32), (16, 16)) is None
    # between two rows / two columns of centres: no centre can be selected, and the closed form says so
    assert serve.lasso_box(L.ring_edges([(3, 7), (60, 8), (30, 9)]), (16, 16)) is None
    assert serve.lasso_box(L.ring_edges([(7, 3), (9, 60), (8, 30)]), (16, 16)) is None
    assert serve.lasso_box(L.ring_edges([(6, 6), (26, 6), (26, 18), (6, 18)]), (6, 8)) == (1, 2, 4, 7)
    assert serve.lasso_box(L.whole_frame(37, 53), (37, 53)) == (0, 0, 37, 53)


def test_lasso_edges_rounds_clamps_and_closes():
    e = serve.lasso_edges([[(1.5, 1.5), (6.5, 1.5), (6.5, 4.5), (1.5, 4.5)]], (6, 8))
    assert e.dtype == np.int32 and e.tolist() == [[6, 6, 26, 6], [26, 6, 26, 18], [26, 18, 6, 18], [6, 18, 6, 6]]
    # floor(4 v + 0.5): half up, also below zero; a vertex outside the frame moves to its border
    e = serve.lasso_edges([[(0.125, 0.124), (-0.125, 3.0), (100.0, -7.5), (7.9, 6.1)]], (6, 8))
    assert e[:, :2].tolist() == [[1, 0], [0, 12], [32, 0], [32, 24]] and e[:, 2:].tolist() == [[0, 12], [32, 0], [32, 24], [1, 0]]
    two = serve.lasso_edges([[(1, 1), (5, 1), (3, 4)], np.array([(2.0, 2.0), (4.0, 2.0), (3.0, 3.0), (3.0, 2.5)])], (16, 16))
    assert two.shape == (7, 4) and two[2].tolist() == [12, 16, 4, 4] and two[6].tolist() == [12, 10, 8, 8]
    rings = [[(10.25, 20.5), (300.0, 31.0), (250.75, 390.0), (17.0, 200.0)], [(100, 100), (150, 100), (125, 160)]]
    assert np.array_equal(serve.lasso_edges(rings, HW), L.spec_edges(rings, HW))
    big = [(math.cos(k) * 50 + 60, math.sin(k) * 50 + 60) for k in range(65536)]
    assert serve.lasso_edges([big], (128, 128)).shape == (65536, 4)
    bad = [lambda: serve.lasso_edges([], HW), lambda: serve.lasso_edges([[(1, 1), (2, 2)]], HW),
           lambda: serve.lasso_edges([[(1, 1), (5, 1), (3, 4)], []], HW), lambda: serve.lasso_edges([[(1, 1), (5, float("nan")), (3, 4)]], HW),
           lambda: serve.lasso_edges([[(1, 1), (float("inf"), 1), (3, 4)]], HW), lambda: serve.lasso_edges([[(1, 1, 1), (5, 1, 1), (3, 4, 1)]], HW),
           lambda: serve.lasso_edges([big + [(1, 1)]], (128, 128)), lambda: serve.lasso_edges([big[:40000], big[:30000]], (128, 128)),
           lambda: serve.lasso_edges([[(1, 1), (5, 1), (3, 4)]], (8193, 64)), lambda: serve.lasso_edges([[(1, 1), (5, 1), (3, 4)]], (64, 8193))]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()


def test_combine_statement():
    a = np.array([[0, 1, 7, 255]] * 4, np.uint8)
    b = a.T.copy()
    assert L.spec_combine(a, b, L.ADD).tolist() == [[0, 255, 255, 255]] + [[255] * 4] * 3
    assert L.spec_combine(a, b, L.SUBTRACT).tolist() == [[0, 255, 255, 255]] + [[0] * 4] * 3
    assert L.spec_combine(a, b, L.INTERSECT).tolist() == [[0] * 4] + [[0, 255, 255, 255]] * 3
    assert L.spec_combine(a, b, L.XOR).tolist() == [[0, 255, 255, 255]] + [[255, 0, 0, 0]] * 3
    assert L.spec_combine(a, None, L.INVERT).tolist() == [[255, 0, 0, 0]] * 4
    assert (_lib.COMBINE_ADD, _lib.COMBINE_SUBTRACT, _lib.COMBINE_INTERSECT, _lib.COMBINE_XOR, _lib.COMBINE_INVERT) == (0, 1, 2, 3, 4)
    assert serve.COMBINE_OPS == dict(add=0, subtract=1, intersect=2, xor=3) and serve.COMBINE_INVERT == 4


# ---- the sessions against a scripted backend ----------------------------------------------------------------------------------------------------
class _Stub(_SelectStub):
    """... with the three calls of DESIGN.md 6p: the statements themselves, on numpy planes"""

    def select_lasso(self, edges, frame_hw, grow):
        self.calls.append(("select_lasso", tuple(edges.shape), edges.dtype.name, tuple(frame_hw), grow))
        plane = U.spec_grow(L.spec_lasso(edges, *frame_hw) == 255, grow)
        self.plane = plane
        return (plane,) + L.box_count(plane)

    def combine(self, a, b, op):
        self.calls.append(("combine", id(a), None if b is None else id(b), op))
        plane = L.spec_combine(a, b, op)
        self.plane = plane
        return (plane,) + L.box_count(plane)

    def copy(self, plane):
        self.calls.append(("copy", id(plane)))
        return plane.copy()


RING = [(300.0, 200.0), (340.0, 200.0), (340.0, 230.0), (300.0, 230.0)]           # on the corner lattice: rows 200 .. 229, columns 300 .. 339
BOX = (200, 300, 230, 340)
HOLE = [(310.0, 210.0), (330.0, 210.0), (330.0, 220.0), (310.0, 220.0)]
SLIVER = [(300.25, 200.0), (300.75, 200.0), (330.75, 230.0), (330.25, 230.0)]      # a diagonal strip between the centres: a box by the closed form, and no centre in it


def _session(stub, lock=False, **kw):
    s = serve.EditSession(None, U._noise(HW, 5), backend=stub, **kw)
    if lock:
        plane = np.zeros(HW, np.uint8)
        plane[0:8, 0:8] = 255
        s.set_lock(plane)
    stub.calls.clear()
    return s


def test_select_lasso_uploads_the_edges_and_makes_one_call():
    stub = _Stub()
    s = _session(stub, history=2)
    sel = s.select_lasso([RING])
    assert stub.calls == [("upload", (4, 4), "int32"), ("select_lasso", (4, 4), "int32", HW, 0)]
    assert isinstance(sel, serve.Selection) and sel.box == BOX and sel.count == 30 * 40 and sel.frame_hw == HW and sel.plane is stub.plane
    assert not s.can_undo                                            # not an edit
    stub.calls.clear()
    m = sel.mask()
    assert stub.calls == [("crop", (200, 300, 30, 40))] and m.shape == (30, 40) and (m == 255).all()
    stub.calls.clear()
    sel = s.select_lasso([RING, HOLE], grow=np.int64(3))
    assert stub.calls == [("upload", (8, 4), "int32"), ("select_lasso", (8, 4), "int32", HW, 3)]
    assert sel.box == (197, 297, 233, 343) and sel.count == 36 * 46 - 4 * 14
    assert np.array_equal(sel.plane, L.spec_select_lasso([RING, HOLE], HW, 3))


def test_combine_and_invert_are_one_call_and_leave_the_operands():
    stub = _Stub()
    s = _session(stub)
    a, b = s.select_lasso([RING]), s.select_lasso([HOLE])
    pa, pb = a.plane.copy(), b.plane.copy()
    for op, code, count in (("add", 0, 1200), ("subtract", 1, 1000), ("intersect", 2, 200), ("xor", 3, 1000)):
        box = (210, 310, 220, 330) if op == "intersect" else BOX
        stub.calls.clear()
        c = s.combine(a, b, op)
        assert stub.calls == [("combine", id(a.plane), id(b.plane), code)]
        assert isinstance(c, serve.Selection) and c is not a and c is not b and c.plane is not a.plane and c.plane is not b.plane
        assert c.count == count and c.frame_hw == HW and c.box == box and np.array_equal(c.plane, L.spec_combine(pa, pb, code))
    stub.calls.clear()
    inv = s.invert(b)
    assert stub.calls == [("combine", id(b.plane), None, 4)]
    assert inv.count == 400 * 600 - 200 and inv.box == (0, 0, 400, 600)
    assert np.array_equal(a.plane, pa) and np.array_equal(b.plane, pb) and (a.box, a.count, b.count) == (BOX, 1200, 200)
    # everything but b, confined to a: a minus b
    assert np.array_equal(s.combine(inv, a, "intersect").plane, s.combine(a, b, "subtract").plane)


def test_empty_selections_end_to_end():
    stub = _Stub()
    s = _session(stub, history=1)
    a, b = s.select_lasso([RING]), s.select_lasso([HOLE])
    stub.calls.clear()
    e = s.combine(b, a, "subtract")                                   # the hole lies inside the ring: nothing is left
    assert _names(stub) == ["combine"] and e.box is None and e.count == 0 and e.frame_hw == HW and not e.plane.any()
    stub.calls.clear()
    m = e.mask()
    assert m.shape == (0, 0) and m.dtype == np.uint8 and stub.calls == []                 # no backend call
    with pytest.raises(ValueError, match="empty selection: nothing to fill"):
        s.fill_selection(e)
    assert stub.calls == [] and not s.can_undo
    s.set_lock(e)                                                     # as None
    assert stub.calls == [] and not s.locked
    # an empty selection is an operand like any other
    assert s.combine(a, e, "add").count == 1200 and s.combine(a, e, "intersect").box is None
    assert s.invert(e).count == 400 * 600 and s.invert(s.invert(e)).box is None
    # a lasso around no pixel centre: select_lasso returns the empty selection
    stub.calls.clear()
    sl = s.select_lasso([SLIVER])
    assert _names(stub) == ["select_lasso"] and sl.box is None and sl.count == 0
    sl = s.select_lasso([[(1.0, 1.0), (30.0, 30.0), (15.5, 15.5)]])                      # collinear
    assert sl.box is None


@pytest.mark.parametrize("lock", [False, True])
@pytest.mark.parametrize("history", [0, 2])
@pytest.mark.parametrize("max_side", [None, 128])
@pytest.mark.parametrize("feather", [None, 4])
def test_fill_lasso_issues_upload_select_keep_run_save_one_paste_crop(lock, history, max_side, feather):
    stub = _Stub()
    s = _session(stub, lock, history=history)
    patch, (x0, y0), info = s.fill_lasso([RING], max_side=max_side, feather=feather, low_latency=True)
    grown = (198, 298, 232, 342)                                     # grow = 2 is fill_lasso's default
    win = serve.choose_window(grown, HW, margin=0.5)
    assert info["window"] == win == (y0, x0) + win[2:] and patch.shape == win[2:] + (3,)
    work = serve.choose_working_size(win[2:], max_side) if max_side else None
    paste = "paste_feather" if feather else "paste_locked"
    assert _names(stub) == ["select_lasso", "fill_keep", "run_fill"] + (["save"] if history else []) + [paste, "crop"]
    assert [c for c in stub.calls if c[0] == "upload"] == [("upload", (4, 4), "int32")] and stub.calls[0][0] == "upload"     # only the edges go up
    calls = {c[0]: c for c in stub.calls}
    assert calls["select_lasso"] == ("select_lasso", (4, 4), "int32", HW, 2)
    assert stub.holes[0] is stub.plane                               # the plane the selection made, as it is
    assert calls["fill_keep"] == ("fill_keep", [win[:2]], [HW], 1 if lock else None, win[2:])
    assert calls["run_fill"] == ("run_fill", [win[:2]], [None], 1 if lock else None, win[2:], work, True)
    out_hw = work or win[2:]
    assert calls[paste][:3] == (paste, [id(stub.keeps[0])], win[2:]) and calls[paste][-2:] == ((1,) + out_hw + (3,), (1,) + out_hw)
    want = dict(window=win, fill=True, selected=34 * 44)
    if lock:
        want["locked"] = True
    if work:
        want["work"] = work
    if history:
        want["undoable"] = True
    if feather:
        want["feather"] = 4
    assert info == want                                              # fill_selection's keys, no other
    if history:
        assert s.can_undo and len(s._undo) == 1                      # one call is one undo step
        s.undo()
        assert _names(stub)[-2:] == ["swap", "crop"] and s.can_redo and not s.can_undo


@pytest.mark.parametrize("history", [0, 1])
def test_fill_lasso_and_fill_selection_window_sketch_and_encode(history):
    stub = _Stub()
    s = _session(stub, history=history)
    sel = s.combine(s.select_lasso([RING], grow=1), s.select_lasso([HOLE]), "subtract")
    stub.calls.clear()
    _, _, info = s.fill_selection(sel, feather=3)
    assert _names(stub) == ["fill_keep", "run_fill"] + (["save"] if history else []) + ["paste_feather", "crop"]
    assert info["window"] == serve.choose_window((199, 299, 231, 341), HW, margin=0.5) and info["selected"] == 32 * 42 - 200
    assert stub.holes[0] is sel.plane
    sk = np.zeros(HW, np.uint8)
    sk[100:110, 500:520] = 255
    stub.calls.clear()
    _, _, info = s.fill_lasso([RING], grow=0, sketch=sk, margin=0.25)
    win = serve.choose_window((100, 300, 230, 520), HW, margin=0.25)
    assert info["window"] == win
    assert [c for c in stub.calls if c[0] == "upload"] == [("upload", (4, 4), "int32"), ("upload", win[2:], "uint8")]
    stub.calls.clear()
    _, (px, py), info = s.fill_lasso([RING], window=(180, 280, 96, 128))
    assert info["window"] == (180, 280, 96, 128) and (px, py) == (280, 180)
    _, _, info = s.fill_lasso([RING], window=(180, 280, 99, 131), max_side=64)
    assert info["window"] == (180, 280, 99, 131) and info["work"] == serve.choose_working_size((99, 131), 64)
    stub.calls.clear()
    patch, _, info = s.fill_lasso([RING, HOLE], encode="png")
    assert patch == b"png" and _names(stub)[-2:] == ["paste_locked", "crop_png"] and stub.calls[-1] == ("crop_png", [info["window"]])
    assert info["selected"] == 34 * 44 - 6 * 16
    patch, _, info = s.fill_lasso([RING], encode=("jpg", 80))
    assert patch == b"jpg" and stub.calls[-1][:3] == ("crop_jpg", [info["window"]], 80)


def test_set_lock_takes_a_selection_as_a_device_copy():
    stub = _Stub()
    s = _session(stub)
    sel = s.select_lasso([RING])
    stub.calls.clear()
    s.set_lock(sel)
    assert stub.calls == [("copy", id(sel.plane))]                    # nothing is uploaded
    assert s.locked and s._lock_plane is not sel.plane and np.array_equal(s.lock(), sel.plane)
    sel.plane[:] = 0                                                  # whatever happens to the selection's plane later
    assert int((s.lock() == 255).sum()) == 1200
    stub.calls.clear()
    _, _, info = s.fill_lasso([RING])
    assert info["locked"] is True and {c[0]: c for c in stub.calls}["fill_keep"][3] == 1
    # arrays and None as before
    plane = np.zeros(HW, bool)
    plane[5, 5] = True
    stub.calls.clear()
    s.set_lock(plane)
    assert stub.calls == [("upload", HW, "uint8")] and int(s.lock().sum()) == 255
    s.set_lock(None)
    assert not s.locked
    other = serve.EditSession(None, np.zeros((64, 64, 3), np.uint8), backend=_Stub())
    with pytest.raises(ValueError):
        other.set_lock(sel)


def test_refusals_make_no_backend_call():
    stub = _Stub()
    s = _session(stub, history=1)
    sel = s.select_lasso([RING])
    other = serve.EditSession(None, np.zeros((64, 64, 3), np.uint8), backend=_Stub()).select_lasso([[(1, 1), (30, 1), (15, 30)]])
    stub.calls.clear()
    nan = float("nan")
    bad = [lambda: s.select_lasso([]),
           lambda: s.select_lasso([RING[:2]]),
           lambda: s.select_lasso([RING, []]),
           lambda: s.select_lasso([[(1, 1), (nan, 5), (9, 9)]]),
           lambda: s.select_lasso([RING], grow=-1),
           lambda: s.select_lasso([RING], grow=17),
           lambda: s.select_lasso([RING], grow=2.0),
           lambda: s.select_lasso([RING], grow=True),
           lambda: s.combine(sel, sel, "or"),
           lambda: s.combine(sel, sel, 0),
           lambda: s.combine(sel, sel, "invert"),
           lambda: s.combine(sel, sel.plane, "add"),
           lambda: s.combine(None, sel, "add"),
           lambda: s.combine(sel, other, "add"),
           lambda: s.combine(other, sel, "add"),
           lambda: s.invert(other),
           lambda: s.invert(sel.plane),
           lambda: s.fill_selection(other),
           lambda: s.fill_lasso([]),
           lambda: s.fill_lasso([RING[:2]]),
           lambda: s.fill_lasso([[(1, 1), (5, float("inf")), (9, 9)]]),
           lambda: s.fill_lasso([RING], grow=17),
           lambda: s.fill_lasso([RING], grow=1.5),
           lambda: s.fill_lasso([RING], encode="gif"),
           lambda: s.fill_lasso([RING], feather=17),
           lambda: s.fill_lasso([RING], margin=-1.0),
           lambda: s.fill_lasso([RING], max_side=8),
           lambda: s.fill_lasso([RING], window=(0, 0, 100, 128)),                        # sides not multiples of 8 without max_side
           lambda: s.fill_lasso([RING], window=(350, 0, 64, 64)),                        # outside the frame
           lambda: s.fill_lasso([RING], window=(0, 0, 8, 64), max_side=64),              # under 16
           lambda: s.fill_lasso([RING], sketch=np.zeros((10, 10), np.uint8)),
           lambda: s.fill_lasso([[(3.6, 7.0), (3.7, 90.0), (3.65, 40.0)]])]              # between two columns of centres: no box
    for k, call in enumerate(bad):
        with pytest.raises((ValueError, TypeError)):
            call()
        assert stub.calls == [] and not s.can_undo, k
    # the one documented exception: a box by the closed form, and no centre in it -- known after the selection was made
    with pytest.raises(ValueError, match="the lasso covers no pixel centre"):
        s.fill_lasso([SLIVER], grow=0)
    assert _names(stub) == ["select_lasso"] and not s.can_undo       # nothing was changed
    assert "covers no pixel centre" in serve.EditSession.fill_lasso.__doc__


def test_a_session_that_never_uses_them_makes_no_new_call():
    """edit, fill and fill_similar on the backends of before: select_lasso, combine and copy do not exist there"""
    sk = np.zeros(HW, np.uint8)
    sk[200:210, 300:330] = 255
    mask = np.zeros(HW, np.uint8)
    mask[200:230, 300:340] = 1
    new = {"select_lasso", "combine", "copy"}
    for lock in (False, True):
        stub = _OldStub()
        s = _session(stub, lock, history=2)
        s.edit(sk, max_grow=0)
        s.edit_strokes([([(30, 20), (60, 30)], 3)])
        s.undo()
        s.redo()
        assert stub.calls and not new & set(_names(stub))
        with pytest.raises(AttributeError):
            s.select_lasso([RING])
        stub = _FillStub()
        s = _session(stub, lock, history=2)
        s.fill(mask)
        s.fill_strokes([([(300.5, 200.0), (340.0, 230.25)], 12.0)])
        s.undo()
        assert stub.calls and not new & set(_names(stub))
        with pytest.raises(AttributeError):
            s.fill_lasso([RING])
        stub = _SelectStub()
        f = U._noise(HW, 5)
        f[200:230, 300:340] = U.REGION
        s = serve.EditSession(None, f, backend=stub, history=2)
        if lock:
            s.set_lock(mask)
        stub.calls.clear()
        sel = s.select_similar((210, 320))
        s.fill_similar((210, 320))
        s.fill_selection(sel)
        s.undo()
        assert stub.calls and not new & set(_names(stub))
        with pytest.raises(AttributeError):
            s.combine(sel, sel, "add")
        with pytest.raises(AttributeError):
            s.set_lock(sel)


def test_model_backend_select_lasso_and_combine():
    """_ModelBackend.select_lasso / combine on a scripted model: the fill, the grow only when grow > 0, the tile records"""
    from sketch_tiles_util import sketch_tiles as spec_tiles

    class _T:                                                        # what the backend asks of a tensor
        def __init__(self, a):
            self.a, self.shape = a, a.shape

        def cpu(self):
            return self

        def numpy(self):
            return self.a

    class _Model:
        def __init__(self):
            self.calls = []

        def lasso_fill_u8(self, edges, Hi, Wi):
            self.calls.append(("lasso_fill", Hi, Wi))
            return _T(L.spec_lasso(edges.a, Hi, Wi))

        def select_grow_u8(self, state, grow):
            self.calls.append(("grow", grow))
            return _T(U.spec_grow(state.a == 255, grow))

        def plane_combine_u8(self, a, b, op):
            self.calls.append(("combine", op, b is None))
            return _T(L.spec_combine(a.a, None if b is None else b.a, op))

        def sketch_tiles_u8(self, plane, tile):
            self.calls.append(("tiles", tile))
            return _T(spec_tiles(plane.a, tile))

    hw = (120, 104)
    edges = L.star(*hw)
    for grow in (0, 2):
        be = serve._ModelBackend.__new__(serve._ModelBackend)
        be.model = _Model()
        plane, box, count = be.select_lasso(_T(edges), hw, grow)
        assert be.model.calls == [("lasso_fill", 120, 104)] + ([("grow", 2)] if grow else []) + [("tiles", 32)]
        want = U.spec_grow(L.spec_lasso(edges, *hw) == 255, grow)
        assert np.array_equal(plane.a, want) and (box, count) == L.box_count(want)
    be.model.calls.clear()
    a, b = _T(L.spec_lasso(edges, *hw)), _T(L.spec_lasso(L.ring_in_ring(*hw), *hw))
    plane, box, count = be.combine(a, b, L.SUBTRACT)
    assert be.model.calls == [("combine", 1, False), ("tiles", 32)] and (box, count) == L.box_count(L.spec_combine(a.a, b.a, L.SUBTRACT))
    be.model.calls.clear()
    plane, box, count = be.combine(a, a, L.XOR)
    assert (box, count) == (None, 0) and be.model.calls == [("combine", 3, False), ("tiles", 32)]
    plane, box, count = be.combine(a, None, L.INVERT)
    assert be.model.calls[-2:] == [("combine", 4, True), ("tiles", 32)] and count == 120 * 104 - int((a.a > 0).sum())


# ---- the C-ABI -------------------------------------------------------------------------------------------------------------
def test_abi_has_two_new_symbols_in_a_header_of_their_own():
    hdr = open(os.path.join(ROOT, "include", "sketchedit_lasso.h")).read()
    declared = re.findall(r"^(?:int|size_t) (se_\w+)\(", hdr, re.M)
    assert declared == _lib.abi_names("sketchedit_lasso.h") == ["se_lasso_fill_u8", "se_plane_combine_u8"]
    for name in ("sketchedit_hip.h", "sketchedit_fill.h", "sketchedit_feather.h", "sketchedit_select.h"):
        text = open(os.path.join(ROOT, "include", name)).read()
        assert "se_lasso" not in text and "se_plane_combine" not in text
    assert "se_lasso.hip" in _lib.SOURCES
    defines = {k: int(v) for k, v in re.findall(r"#define (SE_\w+) (\d+)", hdr)}
    assert defines == dict(SE_LASSO_MAX_EDGES=65536, SE_LASSO_MAX_EXTENT=8192, SE_COMBINE_ADD=0, SE_COMBINE_SUBTRACT=1, SE_COMBINE_INTERSECT=2,
                           SE_COMBINE_XOR=3, SE_COMBINE_INVERT=4)
    assert (_lib.LASSO_MAX_EDGES, _lib.LASSO_MAX_EXTENT, serve.LASSO_MAX_EDGES, serve.STROKE_MAX_EXTENT) == (65536, 8192, 65536, 8192)
    import ctypes
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    lib = ctypes.CDLL(_lib.LIB_PATH)                                    # the built library, as the other host tests load it
    for s in declared:
        getattr(lib, s)
    from sketchedit_amd import kernel_labels
    assert kernel_labels.label_of("lasso_fill_kernel(int const*, int, int, int, unsigned char*)") == "lasso_fill"
    assert kernel_labels.label_of("plane_combine_kernel(unsigned char const*, unsigned char const*, unsigned char*, long, int, long)") == "plane_combine"


def test_the_kernels_cross_compile_for_gfx950(tmp_path):
    import shutil
    import subprocess
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc on this machine")
    obj = str(tmp_path / "se_lasso.o")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(_lib.CSRC, "se_lasso.hip"), "-o", obj])
    assert os.path.getsize(obj) > 0
