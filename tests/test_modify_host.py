"""Host tests of the modification of a selection's shape: the statement of tests/modify_util.py against independent
formulations (scipy's Euclidean distance transform and its binary morphology, where scipy is present), its known answers and
identities, the kernels' tile-by-tile algorithm in Python integers against the statement, the host logic of
EditSession.modify_selection against a scripted backend that logs every call, and the new entry's place in the C-ABI.  CPU only."""
import os
import re

import numpy as np
import pytest

from sketchedit_amd import _lib, serve
import abi_util
import lasso_util as L
import modify_util as M
import select_util as U
from test_fill_host import _names
from test_lasso_host import _Stub as _LassoStub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HW = (120, 104)


# ---- the statement against independent ones --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [1, 5, 32])
def test_statement_against_scipy(r):
    ndi = pytest.importorskip("scipy.ndimage")
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    disc = yy * yy + xx * xx <= r * r
    assert int(disc.sum()) == len(M.disc(r))
    for density, seed in ((0.01, 1), (0.5, 2), (0.99, 3)):
        plane = M.random_plane(93, 131, density, seed, values=(1, 128, 255))
        sel = plane != 0
        want = M.spec_expand(plane, r) == 255
        d2 = np.rint(ndi.distance_transform_edt(~sel) ** 2).astype(np.int64)        # squared distances are integers: exact after rint
        assert np.array_equal(want, d2 <= r * r)
        assert np.array_equal(want, ndi.binary_dilation(sel, structure=disc))
        assert np.array_equal(M.spec_contract(plane, r) == 255, ndi.binary_erosion(sel, structure=disc, border_value=1))
        c = ndi.convolve(sel.astype(np.int32), disc.astype(np.int32), mode="constant", cval=0)
        n = ndi.convolve(np.ones(sel.shape, np.int32), disc.astype(np.int32), mode="constant", cval=0)
        assert np.array_equal(M.spec_smooth(plane, r) == 255, (2 * c > n) | ((2 * c == n) & sel))


def test_known_disc_counts():
    hdr = open(os.path.join(ROOT, "include", "sketchedit_modify.h")).read()
    assert "5, 13, 29, 49, 81, 197, 797, 3001 and 3209 offsets for r = 1, 2, 3, 4, 5, 8, 16, 31 and 32" in hdr
    for r, count in M.DISC_COUNTS.items():
        assert len(M.disc(r)) == count
        if r <= 16:                                                   # a single pixel far from the border
            got = M.spec_expand(M.points(40, 40, [(20, 20)]), r)
            assert int((got == 255).sum()) == count
    got = M.spec_expand(M.points(93, 131, [(46, 65)]), 32)
    assert int((got == 255).sum()) == 3209
    got = M.spec_expand(M.points(40, 40, [(20, 20)]), 5)
    assert got[23, 24] == 255 and got[24, 24] == 0 and got[25, 20] == 255 and got[25, 21] == 0
    assert int((M.spec_expand(M.points(40, 40, [(0, 0)]), 5) == 255).sum()) == 26        # a quarter disc with its two axes: outside adds nothing


def test_contract_is_the_inverted_expansion_and_a_full_plane_stays_full():
    inv = lambda p: L.spec_combine(p, None, L.INVERT)                # noqa: E731
    for hw in ((37, 53), (65, 129)):
        for plane in (M.blob(*hw), M.cross(*hw, half=9), M.random_plane(*hw, 0.9, 4), M.checkerboard(*hw)):
            assert plane[0].any() and plane[-1].any() and plane[:, 0].any() and plane[:, -1].any()      # it touches all four edges
            for r in (1, 3, 8):
                assert np.array_equal(M.spec_contract(plane, r), inv(M.spec_expand(inv(plane), r)))
        for r in (1, 16, 32):
            assert (M.spec_contract(np.full(hw, 255, np.uint8), r) == 255).all()
            assert not M.spec_expand(np.zeros(hw, np.uint8), r).any() and not M.spec_smooth(np.zeros(hw, np.uint8), r).any()
    c = M.spec_contract(M.cross(65, 129, half=9), 3)
    assert c[0].any() and c[-1].any() and c[:, 0].any() and c[:, -1].any()       # a selection at the frame's edge does not shrink away from it
    assert int((c[0] == 255).sum()) == 18 - 6


def test_expansions_compose_to_at_least_the_sum_less_one():
    plane = M.random_plane(60, 70, 0.004, 9)
    for a, b in ((1, 1), (2, 3), (5, 4), (8, 8)):
        twice = M.spec_expand(M.spec_expand(plane, a), b) == 255
        assert not ((M.spec_expand(plane, a + b - 1) == 255) & ~twice).any()
        assert not (twice & ~(M.spec_expand(plane, a + b) == 255)).any()     # and to at most the sum: discs do not compose exactly


def test_smooth_removes_a_speck_fills_a_pinhole_and_keeps_a_half_plane():
    for r in (1, 2, 7):
        assert not M.spec_smooth(M.points(40, 44, [(20, 20)]), r).any()
        assert (M.spec_smooth(M.points(40, 44, [(20, 20)], selected=False), r) == 255).all()
        for hw in ((40, 44), (16, 16)):
            assert np.array_equal(M.spec_smooth(M.half_plane(*hw), r), M.half_plane(*hw))
    # the tie: where the disc covers the whole frame every pixel sees 2c == n, and stays what it is
    p = M.half_plane(16, 16)
    assert (2 * M._count(p != 0, 22) == M._count(np.ones((16, 16), bool), 22)).all() and np.array_equal(M.spec_smooth(p, 22), p)
    # a corner is rounded
    sq = np.zeros((40, 44), np.uint8)
    sq[10:30, 10:30] = 255
    got = M.spec_smooth(sq, 3)
    assert got[10, 10] == 0 and got[11, 11] == 255 and got[10, 20] == 255 and got[9, 20] == 0


@pytest.mark.parametrize("hw,r", [((16, 16), 1), ((37, 53), 2), ((65, 129), 5), ((33, 131), 16), ((65, 70), 32)])
def test_the_kernels_algorithm_is_the_statement(hw, r):
    planes = [M.random_plane(*hw, 0.02, r), M.random_plane(*hw, 0.5, r + 1, values=(1, 128)), M.random_plane(*hw, 0.98, r + 2), M.half_plane(*hw),
              M.points(*hw, [(15, min(63, hw[1] - 1))]), np.zeros(hw, np.uint8), np.full(hw, 255, np.uint8)]
    for k, plane in enumerate(planes):
        for op in (M.EXPAND, M.CONTRACT, M.SMOOTH):
            assert np.array_equal(M.tiled_modify(plane, op, r, base=k % 4), M.spec_modify(plane, op, r)), (k, op)


# ---- the sessions against a scripted backend ----------------------------------------------------------------------------------------------
class _Stub(_LassoStub):
    """... with the call of DESIGN.md 6w: the statement itself, on numpy planes"""

    def modify(self, plane, op, radius, tiles=True):
        self.calls.append(("modify", id(plane), op, radius, tiles))
        out = M.spec_modify(plane, op, radius)
        self.plane = out
        return (out,) + (L.box_count(out) if tiles else (None, None))


RING = [(30.0, 20.0), (70.0, 20.0), (70.0, 50.0), (30.0, 50.0)]                   # rows 20 .. 49, columns 30 .. 69
TINY = [(80.0, 80.0), (83.0, 80.0), (83.0, 83.0), (80.0, 83.0)]                   # 3 x 3


def _session(stub, **kw):
    s = serve.EditSession(None, U._noise(HW, 5), backend=stub, **kw)
    stub.calls.clear()
    return s


def test_each_kind_and_side_makes_its_calls_and_leaves_the_operand():
    stub = _Stub()
    s = _session(stub, history=1)
    sel = s.select_lasso([RING])
    before = sel.plane.copy()
    pid = id(sel.plane)
    for kind, op in (("expand", 0), ("contract", 1), ("smooth", 2)):
        stub.calls.clear()
        got = s.modify_selection(sel, kind, np.int64(3))
        assert stub.calls == [("modify", pid, op, 3, True)]
        want = M.spec_modify(before, op, 3)
        assert isinstance(got, serve.Selection) and got is not sel and got.plane is not sel.plane and got.frame_hw == HW
        assert np.array_equal(got.plane, want) and (got.box, got.count) == L.box_count(want)
    assert s.modify_selection(sel, "expand", 3).box == (17, 27, 53, 73) and s.modify_selection(sel, "contract", 3).count == 24 * 34
    for side, ops in (("inside", [1]), ("outside", [0]), ("both", [0, 1])):
        stub.calls.clear()
        got = s.modify_selection(sel, "border", 2, side=side)
        assert [c[:1] + c[2:] for c in stub.calls[:-1]] == [("modify", o, 2, False) for o in ops] and all(c[1] == pid for c in stub.calls[:-1])
        assert stub.calls[-1][0] == "combine" and stub.calls[-1][3] == M.SUBTRACT and len(stub.calls) == len(ops) + 1
        if side != "both":                                            # the selection itself is one operand of the subtraction
            assert stub.calls[-1][1 if side == "inside" else 2] == pid
        want = M.spec_border(before, 2, side)
        assert np.array_equal(got.plane, want) and (got.box, got.count) == L.box_count(want) and got.count > 0
    assert s.modify_selection(sel, "border", 2).count == s.modify_selection(sel, "border", 2, side="both").count      # the default side
    assert np.array_equal(sel.plane, before) and (sel.box, sel.count) == ((20, 30, 50, 70), 1200)
    assert not s.can_undo                                            # not an edit
    # a result may be empty
    tiny = s.select_lasso([TINY])
    stub.calls.clear()
    e = s.modify_selection(tiny, "contract", 2)
    assert _names(stub) == ["modify"] and e.box is None and e.count == 0 and not e.plane.any()
    assert s.modify_selection(tiny, "border", 2, side="inside").count == 9


def test_an_empty_operand_makes_no_backend_call():
    stub = _Stub()
    s = _session(stub)
    a = s.select_lasso([RING])
    e = s.combine(a, a, "xor")
    assert e.box is None
    stub.calls.clear()
    for kind, kw in (("expand", {}), ("contract", {}), ("smooth", {}), ("border", {}), ("border", dict(side="inside")), ("border", dict(side="outside"))):
        got = s.modify_selection(e, kind, 5, **kw)
        assert isinstance(got, serve.Selection) and got is not e and got.box is None and got.count == 0 and got.frame_hw == HW
        assert not got.plane.any() and got.mask().shape == (0, 0)
    assert stub.calls == []


def test_refusals_come_before_any_backend_call():
    stub = _Stub()
    s = _session(stub, history=1)
    sel = s.select_lasso([RING])
    other = serve.EditSession(None, np.zeros((64, 64, 3), np.uint8), backend=_Stub()).select_lasso([[(1, 1), (30, 1), (15, 30)]])
    stub.calls.clear()
    bad = [(lambda: s.modify_selection(sel.plane, "expand", 2), TypeError, "modify_selection takes a Selection"),
           (lambda: s.modify_selection(None, "expand", 2), TypeError, "modify_selection takes a Selection"),
           (lambda: s.modify_selection(other, "expand", 2), ValueError, "was made on a 64x64 frame"),
           (lambda: s.modify_selection(sel, "grow", 2), ValueError, "kind is one of 'expand', 'contract', 'border', 'smooth'"),
           (lambda: s.modify_selection(sel, 0, 2), ValueError, "kind is one of"),
           (lambda: s.modify_selection(sel, None, 2), ValueError, "kind is one of"),
           (lambda: s.modify_selection(sel, "border", 2, side="left"), ValueError, "side is one of 'inside', 'outside', 'both'"),
           (lambda: s.modify_selection(sel, "border", 2, side=None), ValueError, "side is one of"),
           (lambda: s.modify_selection(sel, "expand", 2, side="inside"), ValueError, "side belongs to kind 'border' alone"),
           (lambda: s.modify_selection(sel, "smooth", 2, side="outside"), ValueError, "side belongs to kind 'border' alone"),
           (lambda: s.modify_selection(sel, "expand", 0), ValueError, r"radius is an int 1 \.\. 32"),
           (lambda: s.modify_selection(sel, "contract", 33), ValueError, r"radius is an int 1 \.\. 32"),
           (lambda: s.modify_selection(sel, "smooth", -1), ValueError, r"radius is an int 1 \.\. 32"),
           (lambda: s.modify_selection(sel, "border", 2.0), ValueError, r"radius is an int 1 \.\. 32"),
           (lambda: s.modify_selection(sel, "expand", True), ValueError, r"radius is an int 1 \.\. 32"),
           (lambda: s.modify_selection(sel, "expand", "2"), ValueError, r"radius is an int 1 \.\. 32"),
           (lambda: s.modify_selection(sel, "expand", None), ValueError, r"radius is an int 1 \.\. 32")]
    for k, (call, exc, msg) in enumerate(bad):
        with pytest.raises(exc, match=msg):
            call()
        assert stub.calls == [] and not s.can_undo, k
    # a backend from before: no `modify`
    old = _LassoStub()
    s2 = _session(old)
    sel2 = s2.select_lasso([RING])
    empty2 = s2.combine(sel2, sel2, "xor")
    old.calls.clear()
    for operand in (sel2, empty2):
        with pytest.raises(NotImplementedError, match="cannot modify selections: it has no `modify`"):
            s2.modify_selection(operand, "expand", 2)
    with pytest.raises(ValueError, match="radius"):                    # the arguments are judged first
        s2.modify_selection(sel2, "expand", 99)
    assert old.calls == []


def test_a_session_that_never_uses_it_makes_no_new_call():
    """every call of before on a backend of before: `modify` does not exist there and nobody asks for it"""
    stub = _LassoStub()
    s = _session(stub, history=2)
    a, b = s.select_lasso([RING], grow=2), s.select_lasso([TINY])
    s.combine(a, b, "add")
    s.invert(a)
    s.set_lock(b)
    s.fill_selection(a)
    s.fill_lasso([RING], grow=1)
    s.undo()
    s.redo()
    assert stub.calls and "modify" not in _names(stub) and not hasattr(stub, "modify")


def test_model_backend_modify():
    """_ModelBackend.modify on a scripted model: one launch, then the tile records -- or nothing, for a border's intermediate"""
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

        def plane_modify_u8(self, plane, op, radius):
            self.calls.append(("modify", op, radius))
            return _T(M.spec_modify(plane.a, op, radius))

        def sketch_tiles_u8(self, plane, tile):
            self.calls.append(("tiles", tile))
            return _T(spec_tiles(plane.a, tile))

    be = serve._ModelBackend.__new__(serve._ModelBackend)
    be.model = _Model()
    a = _T(L.spec_lasso(L.star(*HW), *HW))
    for op in (M.EXPAND, M.CONTRACT, M.SMOOTH):
        be.model.calls.clear()
        plane, box, count = be.modify(a, op, 4)
        want = M.spec_modify(a.a, op, 4)
        assert be.model.calls == [("modify", op, 4), ("tiles", 32)] and np.array_equal(plane.a, want) and (box, count) == L.box_count(want) and count > 0
    be.model.calls.clear()
    plane, box, count = be.modify(a, M.EXPAND, 4, tiles=False)
    assert be.model.calls == [("modify", 0, 4)] and (box, count) == (None, None) and np.array_equal(plane.a, M.spec_expand(a.a, 4))
    plane, box, count = be.modify(_T(M.points(*HW, [(5, 5)])), M.CONTRACT, 1)
    assert (box, count) == (None, 0)


# ---- the C-ABI -------------------------------------------------------------------------------------------------------------
def test_abi_has_one_new_symbol_in_a_header_of_its_own():
    hdr = open(os.path.join(ROOT, "include", "sketchedit_modify.h")).read()
    declared = re.findall(r"^(?:int|size_t)\s+(se_\w+)\(", hdr, re.M)
    assert declared == _lib.abi_names("sketchedit_modify.h") == ["se_plane_modify_u8"]
    others = [n for n in _lib.abi_names() if n not in declared]
    for name in others:                                               # the header refers to other families by DESIGN section
        assert name == "se_last_error" or not re.search(r"\b%s\b" % name, hdr), name      # (the conventions' error call apart)
    for name in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if name != "sketchedit_modify.h":
            assert "se_plane_modify" not in open(os.path.join(ROOT, "include", name)).read(), name
    assert "se_modify.hip" in _lib.SOURCES and "se_api_select.hip" in _lib.SOURCES and _lib.SOURCES[-1] == "se_api.hip"
    defines = {k: int(v) for k, v in re.findall(r"#define (SE_\w+) (\d+)", hdr)}
    assert defines == dict(SE_MODIFY_MAX_RADIUS=32, SE_MODIFY_EXPAND=0, SE_MODIFY_CONTRACT=1, SE_MODIFY_SMOOTH=2)
    assert _lib.MODIFY_MAX_RADIUS == defines["SE_MODIFY_MAX_RADIUS"] == serve.MODIFY_MAX_RADIUS == M.MAX_RADIUS
    assert (_lib.MODIFY_EXPAND, _lib.MODIFY_CONTRACT, _lib.MODIFY_SMOOTH) == (0, 1, 2) == (M.EXPAND, M.CONTRACT, M.SMOOTH)
    assert serve.MODIFY_OPS == dict(expand=0, contract=1, smooth=2) and serve.MODIFY_KINDS == ("expand", "contract", "border", "smooth")
    assert serve.MODIFY_SIDES == ("inside", "outside", "both") and serve.COMBINE_OPS["subtract"] == M.SUBTRACT
    # every kernel constant is derived from the one define
    src = open(os.path.join(_lib.CSRC, "se_modify.hip")).read()
    assert "MD_RMAX = SE_MODIFY_MAX_RADIUS;" in src and not re.search(r"\b(32|33|80|128)\b", re.sub(r"//.*", "", src.split("static_assert")[0]))
    import ctypes
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    lib = ctypes.CDLL(_lib.LIB_PATH)                                    # the built library, as the other host tests load it
    for s in declared:
        getattr(lib, s)
    from sketchedit_amd import kernel_labels
    for kernel, label in (("modify_disc_kernel", "modify_disc"), ("modify_vote_kernel", "modify_vote")):
        assert kernel_labels.label_of("void se::%s(unsigned char const*, unsigned char*, int, int, int, int)" % kernel) == label
        assert kernel_labels.label_of("%s(unsigned char const*, unsigned char*, int, int, int, int)" % kernel) == label
        assert label in set(kernel_labels.KERNEL_LABELS.values())
    names, labels = abi_util.prof_labels()
    assert len(names) == len(labels) - 1 and labels[-1] == "PL_COUNT"
    i = names.index("modify_disc")
    assert names[i - 1:i + 3] == ["select_grow", "modify_disc", "modify_vote", "lasso_fill"]           # behind the grow, not appended
    assert labels[i - 1:i + 3] == ["PL_SELECT_GROW", "PL_MODIFY_DISC", "PL_MODIFY_VOTE", "PL_LASSO_FILL"]      # one order in both
    for label in ("PL_MODIFY_DISC", "PL_MODIFY_VOTE"):
        assert label in src
    from sketchedit_amd.models.editline2_model import EditLine2Model
    assert callable(_lib.Engine.plane_modify_u8) and callable(EditLine2Model.plane_modify_u8)
    assert callable(serve._ModelBackend.modify) and callable(serve.EditSession.modify_selection)


def test_the_kernels_cross_compile_for_gfx950(tmp_path):
    import shutil
    import subprocess
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc on this machine")
    obj = str(tmp_path / "se_modify.o")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(_lib.CSRC, "se_modify.hip"), "-o", obj])
    assert os.path.getsize(obj) > 0
