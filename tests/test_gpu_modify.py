"""GPU tests of the modification of a selection's shape: the two kernels of se_modify.hip against the statement of
tests/modify_util.py on whole planes between sentinels, at every alignment of the input and of the output, plain and under
SE_TEST_POISON, the refusals, and EditSession.modify_selection against the statement.  Every comparison is byte for byte.

Which patterns must change: a pattern is compared at every op; where the definition makes the answer non-trivial -- a single
selected pixel under expand, a single unselected one under contract, while the disc around it does not cover the frame; noise of
density 0.5 under smooth -- the test also asserts that the expected plane differs from the input and is neither empty nor full.
The fixed points (empty, full, the half plane under smooth) are asserted to be fixed points."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from sketchedit_amd import _lib, serve, synth
import modify_util as M

pytestmark = pytest.mark.gpu

ARGV = ("--batchSize 1 --name celeb --joint_train_inp --dataset_mode testimage --image_dirs x --mask_dirs x "
        "--image_lists x --model editline2 --netG deepfillc2 --pool_type max --use_cam --output_dir {d} --gpu_ids 0")
SENTINEL, GARBAGE = 0xA5, 0x5C
LEAD, TAIL = 4096, 4099
FRAMES = [(16, 16), (64, 64), (65, 129), (93, 131), (120, 104)]
RADII = [1, 2, 15, 16, 31, 32]
OPS = {"expand": M.EXPAND, "contract": M.CONTRACT, "smooth": M.SMOOTH}


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    from sketchedit_amd import models
    from sketchedit_amd.options.test_options import TestOptions
    opt = TestOptions().parse(ARGV.format(d=tmp_path_factory.mktemp("out")).split(), quiet=True)
    opt.isSkip = True                      # no checkpoint on disk: procedural weights
    m = models.create_model(opt)
    m.netG.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict("G", 0).items()})
    m.netM.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict("M", 0).items()})
    return m.eval()


@pytest.fixture(scope="module")
def eng():
    return _lib.shared_engine(0)


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()                       # (a copy: the shared cases are read-only)


class _Buf:
    """an array's bytes on the device, `off` bytes past a 4-byte aligned address, between sentinel margins"""

    def __init__(self, shape, off, fill=None, like=None):
        n = int(np.prod(shape))
        self.lead, self.n = LEAD + off, n
        self.buf = torch.full((self.lead + n + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 4 == 0
        self.view = self.buf[self.lead:self.lead + n].view(shape)
        if like is not None:
            self.view.copy_(_cuda(like))
        else:
            self.view.fill_(fill)

    def get(self):
        """the array back on the host; the margins must be what they were"""
        got = self.buf.cpu().numpy()
        assert (got[:self.lead] == SENTINEL).all() and (got[self.lead + self.n:] == SENTINEL).all()
        return got[self.lead:self.lead + self.n].reshape(tuple(self.view.shape))


# ---- the patterns of a frame and a radius: name -> (plane, the ops under which it must change non-trivially) ----------------------------
def _far(hw, y, x, r):
    """the disc of r around (y, x) does not cover the frame: its farthest corner lies outside"""
    return max(y, hw[0] - 1 - y) ** 2 + max(x, hw[1] - 1 - x) ** 2 > r * r


@functools.lru_cache(maxsize=None)
def _patterns(hw, r):
    Hi, Wi = hw
    pats = {}

    def point(name, y, x):
        if 0 <= y < Hi and 0 <= x < Wi:
            strict = _far(hw, y, x, r)
            pats["on_" + name] = (M.points(Hi, Wi, [(y, x)]), {"expand"} if strict else set())
            pats["off_" + name] = (M.points(Hi, Wi, [(y, x)], selected=False), {"contract"} if strict else set())

    for k, (y, x) in enumerate(M.corners(Hi, Wi)):
        point("corner%d" % k, y, x)
    for k, (y, x) in enumerate(M.clamp_points(Hi, Wi, M.FOUR_TILES)):
        point("four_tiles%d" % k, y, x)
    # exactly r (inside the halo) and r + 1 (outside it) rows below the first band of tiles / columns right of the first tile
    point("halo_rows_in", 15 + r, min(20, Wi - 1))
    point("halo_rows_out", 16 + r, min(20, Wi - 1))
    point("halo_cols_in", 7, 63 + r)
    point("halo_cols_out", 7, 64 + r)
    # ... and above the second band / left of the second tile
    point("halo_rows_above_in", 16 - r, 9)
    point("halo_cols_left_in", 9, 64 - r)
    pats["empty"] = (np.zeros(hw, np.uint8), set())
    pats["full"] = (np.full(hw, 255, np.uint8), set())
    pats["full_of_ones"] = (np.full(hw, 1, np.uint8), set())
    pats["checkerboard"] = (M.checkerboard(Hi, Wi), set())
    pats["random_001"] = (M.random_plane(Hi, Wi, 0.01, Hi + r), set())
    pats["random_05"] = (M.random_plane(Hi, Wi, 0.5, Wi + r), {"smooth"} if r * r < min(Hi, Wi) ** 2 // 4 else set())
    pats["random_099"] = (M.random_plane(Hi, Wi, 0.99, Hi * Wi + r), set())
    pats["other_bytes"] = (M.random_plane(Hi, Wi, 0.4, 3 * r, values=(1, 128, 255)), set())
    pats["half_plane"] = (M.half_plane(Hi, Wi), set())
    pats["blob"] = (M.blob(Hi, Wi), set())
    for plane, _ in pats.values():
        plane.setflags(write=False)
    return pats


@functools.lru_cache(maxsize=None)
def _want(hw, r, name, op):
    """the statement's plane: computed once, shared by the plain and the poisoned run, never written"""
    want = M.spec_modify(_patterns(hw, r)[name][0], op, r)
    want.setflags(write=False)
    return want


def _check_not_vacuous(hw, r, name, opname, plane, want):
    sel = plane != 0
    if name in ("empty", "full", "full_of_ones") or (name == "half_plane" and opname == "smooth" and hw[1] % 2 == 0):
        assert np.array_equal(want != 0, sel), (name, opname)           # the stated fixed points
        return 0
    if opname not in _patterns(hw, r)[name][1]:
        return 0
    assert not np.array_equal(want != 0, sel), (hw, r, name, opname)
    assert (want != 0).any() and not (want != 0).all(), (hw, r, name, opname)
    return 1


# ---- 1. every op at every radius, frame, pattern and alignment ------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", [0, 0xFF])
@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("hw", FRAMES, ids=lambda hw: "%dx%d" % hw)
def test_modify_follows_the_statement(eng, seopt, hw, r, poison):
    if poison:
        seopt.set("SE_TEST_POISON", poison)
    strict, k = 0, 0
    for name, (plane, _) in _patterns(hw, r).items():
        for opname, op in OPS.items():
            want = _want(hw, r, name, op)
            strict += _check_not_vacuous(hw, r, name, opname, plane, want)
            offs = [(k % 4, (k // 4) % 4)] if name != "other_bytes" else [(o, (o + 1 + o // 2) % 4) for o in range(4)] + [(2, o) for o in range(4)]
            k += 1
            for ioff, ooff in offs:                                        # the planes' first bytes at offsets mod 4 of their own
                ib, ob = _Buf(hw, ioff, like=plane), _Buf(hw, ooff, fill=GARBAGE)
                eng.plane_modify_u8(ib.view, op, r, out=ob.view)
                got = ob.get()
                assert set(np.unique(got)) <= {0, 255}, (name, opname)
                assert np.array_equal(got, want), (hw, r, name, opname, ioff, ooff, int((got != want).sum()))
                assert np.array_equal(ib.get(), plane)
    assert k >= 16 * 3                                                 # every pair of offsets was used
    if r * r < (hw[0] - 1) ** 2 + (hw[1] - 1) ** 2:
        assert strict >= 8, (hw, r, strict)                             # the corners alone: four under expand, four under contract


def test_known_answers(eng):
    """a single pixel far from the border expands to exactly |D(r)| pixels; offsets on and off the disc's rim"""
    hw = (93, 131)
    for r, count in M.DISC_COUNTS.items():
        got = eng.plane_modify_u8(_cuda(M.points(93, 131, [(46, 65)])), M.EXPAND, r).cpu().numpy()
        assert int((got == 255).sum()) == count and np.array_equal(got, M.spec_expand(M.points(93, 131, [(46, 65)]), r)), r
    got = eng.plane_modify_u8(_cuda(M.points(*hw, [(40, 70)])), M.EXPAND, 5).cpu().numpy()
    assert got[43, 74] == 255 and got[44, 73] == 255 and got[45, 70] == 255 and got[40, 65] == 255      # (3, 4), (4, 3), (5, 0), (0, -5)
    assert got[44, 74] == 0 and got[46, 70] == 0 and got[45, 71] == 0                                    # (4, 4), (6, 0), (5, 1)
    # the halo is inclusive at r and exclusive at r + 1, across a tile boundary in rows and in columns
    for r in RADII:
        for (y, x), (py, px), hit in (((15 + r, 20), (15, 20), True), ((16 + r, 20), (15, 20), False), ((7, 63 + r), (7, 63), True),
                                      ((7, 64 + r), (7, 63), False)):
            got = eng.plane_modify_u8(_cuda(M.points(*hw, [(y, x)])), M.EXPAND, r).cpu().numpy()
            assert (got[py, px] == 255) == hit, (r, y, x)
            got = eng.plane_modify_u8(_cuda(M.points(*hw, [(y, x)], selected=False)), M.CONTRACT, r).cpu().numpy()
            assert (got[py, px] == 0) == hit, (r, y, x)


def test_contract_is_the_inverted_expansion_and_keeps_the_frame_edge(eng):
    for hw in ((65, 129), (93, 131)):
        for r, shape, bars in ((1, M.blob(*hw), 0), (5, M.blob(*hw), 0), (1, M.cross(*hw), 1), (5, M.cross(*hw), 1), (16, M.cross(*hw), 1)):
            assert shape[0].any() and shape[-1].any() and shape[:, 0].any() and shape[:, -1].any()       # it touches all four edges
            c = eng.plane_modify_u8(_cuda(shape), M.CONTRACT, r)
            inv = eng.plane_combine_u8(_cuda(shape), None, _lib.COMBINE_INVERT)
            e = eng.plane_combine_u8(eng.plane_modify_u8(inv, M.EXPAND, r), None, _lib.COMBINE_INVERT)
            got = c.cpu().numpy()
            assert torch.equal(c, e) and np.array_equal(got, M.spec_contract(shape, r))
            if bars:                                                   # 40 wide, head on: the frame's edges were not eaten
                assert got[0].any() and got[-1].any() and got[:, 0].any() and got[:, -1].any() and not np.array_equal(got, shape)
        full = torch.full(hw, 255, dtype=torch.uint8, device="cuda")
        assert bool((eng.plane_modify_u8(full, M.CONTRACT, 32) == 255).all())


def test_smooth_ties_keep_the_pixel(eng):
    """a vertical half plane on an even width is a fixed point.  A run of the disc has an odd length, so inside a wide frame the
    boundary columns see 2c = n +- 1; a tie needs the frame's clip: where the disc covers the whole 16 x 16 frame (r^2 >= 2 15^2)
    EVERY pixel sees 2c == n, and the answer is the input only because a tie keeps the pixel"""
    for hw in ((16, 16), (64, 64), (120, 104)):
        p = M.half_plane(*hw)
        for r in RADII:
            c, n = M._count(p != 0, r), M._count(np.ones(hw, bool), r)
            if hw == (16, 16) and r * r >= 2 * 15 * 15:
                assert (2 * c == n).all()
            else:
                assert hw == (16, 16) or not (2 * c == n).any()
            for off in range(4):
                ob = _Buf(hw, off, fill=GARBAGE)
                eng.plane_modify_u8(_cuda(p), M.SMOOTH, r, out=ob.view)
                assert np.array_equal(ob.get(), p), (hw, r, off)
    # a speck goes, a pinhole fills
    for r in (1, 2, 15):
        assert not eng.plane_modify_u8(_cuda(M.points(65, 129, [(16, 64)])), M.SMOOTH, r).cpu().numpy().any()
        assert (eng.plane_modify_u8(_cuda(M.points(65, 129, [(16, 64)], selected=False)), M.SMOOTH, r).cpu().numpy() == 255).all()


# ---- 2. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(eng):
    Hi, Wi = 37, 53
    a = M.random_plane(Hi, Wi, 0.3, 1)
    ab, ob = _Buf((Hi, Wi), 1, like=a), _Buf((Hi, Wi), 3, fill=GARBAGE)
    big = torch.full((16 * 8200,), GARBAGE, dtype=torch.uint8, device="cuda")              # room for a 16 x 8193 "plane"
    lib, h, st = eng.lib, eng.h, eng._stream()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else t)     # noqa: E731
    A, O = ab.view, ob.view
    shifted = ab.buf[ab.lead + 1:]                                     # overlaps the plane
    last = ab.buf[ab.lead + Hi * Wi - 1:]                              # shares its last byte
    first = ab.buf[ab.lead - Hi * Wi + 1:]                             # shares its first byte
    bad = [((None, Hi, Wi, 0, 3, O), "plane"), ((A, Hi, Wi, 0, 3, None), "out"), ((A, 15, Wi, 0, 3, O), "Hi"), ((A, Hi, 15, 0, 3, O), "Wi"),
           ((A, 8193, 16, 0, 3, big), "Hi"), ((A, 16, 8193, 0, 3, big), "Wi"), ((A, Hi, Wi, -1, 3, O), "op"), ((A, Hi, Wi, 3, 3, O), "op"),
           ((A, Hi, Wi, 0, 0, O), "radius"), ((A, Hi, Wi, 1, 33, O), "radius"), ((A, Hi, Wi, 2, -1, O), "radius"),
           ((A, Hi, Wi, 0, 3, A), "overlaps"), ((A, Hi, Wi, 1, 3, shifted), "overlaps"), ((A, Hi, Wi, 2, 3, last), "overlaps"),
           ((A, Hi, Wi, 0, 3, first), "overlaps")]
    for (x, hi, wi, op, r, o), what in bad:
        assert lib.se_plane_modify_u8(h, st, p(x), hi, wi, op, r, p(o)) != 0, what
        assert what in lib.se_last_error(h).decode(), (what, lib.se_last_error(h).decode())
    for call in (lambda: eng.plane_modify_u8(A, 0, 3, out=ob.buf[:Hi * Wi].view(Wi, Hi)), lambda: eng.plane_modify_u8(A.view(-1), 0, 3),
                 lambda: eng.plane_modify_u8(A.float(), 0, 3), lambda: eng.plane_modify_u8(A, 0, 3, out=A), lambda: eng.plane_modify_u8(A, 3, 3),
                 lambda: eng.plane_modify_u8(A, 0, 0), lambda: eng.plane_modify_u8(A, 0, 33)):
        with pytest.raises(_lib.SketchEditHipError):
            call()
    torch.cuda.synchronize()
    assert np.array_equal(ab.get(), a) and (ob.get() == GARBAGE).all() and (big.cpu().numpy() == GARBAGE).all()


# ---- 3. through a real session -------------------------------------------------------------------------------------------------------------
RINGS = {(93, 131): [[(20.3, 12.1), (100.0, 8.5), (124.6, 40.2), (90.25, 86.0), (30.5, 80.75), (6.0, 50.4)], [(50.0, 30.0), (80.5, 32.25), (76.0, 55.5), (48.75, 50.0)]],
         (120, 104): [[(20.3, 30.1), (52.0, 22.5), (84.6, 35.2), (90.25, 70.0), (60.5, 98.75), (25.0, 88.4), (14.2, 60.0)]]}
KINDS = [("expand", "both"), ("contract", "both"), ("smooth", "both"), ("border", "inside"), ("border", "outside"), ("border", "both")]


@pytest.mark.parametrize("hw", sorted(RINGS), ids=lambda hw: "%dx%d" % hw)
def test_session_modify_selection_is_the_statement(model, hw):
    f = np.random.RandomState(3).randint(0, 256, hw + (3,)).astype(np.uint8)
    s = serve.EditSession(model, f, history=1)
    sel = s.select_lasso(RINGS[hw], grow=1)
    plane = sel.plane.cpu().numpy()
    assert 0 < sel.count < hw[0] * hw[1]
    for r in (2, 5, 32):
        for kind, side in KINDS:
            want = M.spec_kind(plane, kind, r, side)
            got = s.modify_selection(sel, kind, r, **({"side": side} if kind == "border" else {}))
            box, count = M.box_count(want)
            assert isinstance(got, serve.Selection) and got is not sel and (got.box, got.count, got.frame_hw) == (box, count, hw), (kind, side, r)
            assert np.array_equal(got.plane.cpu().numpy(), want), (kind, side, r)
            assert (box is None) == (count == 0)
            assert np.array_equal(sel.plane.cpu().numpy(), plane)      # the operand's plane is what it was
        assert M.spec_kind(plane, "expand", r).any() and not np.array_equal(M.spec_kind(plane, "smooth", 5), plane)
        out = s.combine(s.modify_selection(sel, "expand", r), sel, "subtract")
        rim = s.modify_selection(sel, "border", r, side="outside")
        assert torch.equal(out.plane, rim.plane) and (out.box, out.count) == (rim.box, rim.count) and rim.count > 0
    inner = s.modify_selection(sel, "contract", 2)
    s.set_lock(inner)
    assert np.array_equal(s.lock(), M.spec_contract(plane, 2)) and s.locked and inner.count > 0
    small = s.select_lasso([[(6.0, 5.0), (30.5, 8.0), (12.25, 28.0)]])
    assert small.count > 0 and not M.spec_contract(small.plane.cpu().numpy(), 16).any()
    e = s.modify_selection(small, "contract", 16)                      # contracted away: the empty selection
    assert e.box is None and e.count == 0 and not e.plane.cpu().numpy().any()
    assert s.modify_selection(small, "border", 16, side="inside").count == small.count
    assert s.modify_selection(e, "expand", 3).box is None and s.modify_selection(e, "smooth", 3).count == 0
    assert not s.can_undo and np.array_equal(s.frame(), f)           # not an edit
