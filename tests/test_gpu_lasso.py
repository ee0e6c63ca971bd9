"""GPU tests of lasso selections and the algebra of selections: the two kernels of se_lasso.hip against the
statement of tests/lasso_util.py on whole planes between sentinels, at every alignment, and EditSession.select_lasso / combine /
invert / fill_lasso / set_lock(selection) against the statement and against `fill` of the statement's mask on a twin session.
Every comparison is exact."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from sketchedit_amd import _lib, serve, synth
import lasso_util as L
import select_util as U

pytestmark = pytest.mark.gpu

ARGV = ("--batchSize 1 --name celeb --joint_train_inp --dataset_mode testimage --image_dirs x --mask_dirs x "
        "--image_lists x --model editline2 --netG deepfillc2 --pool_type max --use_cam --output_dir {d} --gpu_ids 0")
SHAPES = {f.__name__: f for f in L.SHAPES}
SENTINEL, GARBAGE = 0xA5, 0x5C
LEAD, TAIL = 4096, 4099


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
def eng(model):
    return model.engine()


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()                       # (a copy: the shared cases are read-only)


@functools.lru_cache(maxsize=None)
def _case(name, hw):
    """(edges, the statement's plane): computed once, shared, never written"""
    edges = SHAPES[name](*hw)
    want = L.spec_lasso(edges, *hw)
    edges.setflags(write=False)
    want.setflags(write=False)
    return edges, want


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


def _edges_dev(edges):
    """the edges on the device between two sentinel rows -> (the (N,4) view, a check that buffer and rows are what they were)"""
    e = np.ascontiguousarray(edges, np.int32).reshape(-1, 4)
    full = np.concatenate([np.full((1, 4), -1515870811, np.int32), e, np.full((1, 4), -1515870811, np.int32)])
    t = _cuda(full)

    def intact():
        return np.array_equal(t.cpu().numpy(), full)
    return t[1:1 + e.shape[0]], intact


# ---- 1. the lasso: every shape at every size and alignment ------------------------------------------------------------------------
@pytest.mark.parametrize("hw", L.SIZES, ids=lambda hw: "%dx%d" % hw)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_lasso_follows_the_statement(eng, name, hw):
    edges, want = _case(name, hw)
    dev, intact = _edges_dev(edges)
    for off in range(4):                                               # the plane's first byte at every offset mod 4
        ob = _Buf(hw, off, fill=GARBAGE)
        eng.lasso_fill_u8(dev, hw[0], hw[1], out=ob.view)
        got = ob.get()
        assert set(np.unique(got)) <= {0, 255}
        assert np.array_equal(got, want), (name, hw, off, int((got != want).sum()))
    assert intact()
    print("%s %dx%d: %d edges, %d pixels" % (name, hw[0], hw[1], edges.shape[0], int((want == 255).sum())))
    if name in ("collinear", "sliver", "no_edges"):
        assert not want.any()
    if name == "whole_frame":
        assert (want == 255).all()


def test_lasso_known_answers_and_order(eng):
    # the header's ring, placed in a 16 x 16 frame: rows 1 .. 3, columns 2 .. 6
    dev, _ = _edges_dev(L.ring_edges([(6, 6), (26, 6), (26, 18), (6, 18)]))
    got = eng.lasso_fill_u8(dev, 16, 16).cpu().numpy()
    want = np.zeros((16, 16), np.uint8)
    want[1:4, 2:7] = 255
    assert np.array_equal(got, want)
    # neither the order of the edges nor their direction plays a part; N = 0 takes a null pointer
    edges, want = _case("polygon_600", (65, 129))
    perm = np.random.RandomState(0).permutation(600)
    flipped = np.ascontiguousarray(edges[perm][:, [2, 3, 0, 1]])
    assert np.array_equal(eng.lasso_fill_u8(_cuda(flipped), 65, 129).cpu().numpy(), want)
    ob = _Buf((37, 53), 1, fill=GARBAGE)
    eng.lasso_fill_u8(torch.zeros((0, 4), dtype=torch.int32, device="cuda"), 37, 53, out=ob.view)
    assert not ob.get().any()


# ---- 2. combine -------------------------------------------------------------------------------------------------------------------------
def _planes(hw, seed):
    rng = np.random.RandomState(seed)
    vals = np.array([0, 0, 1, 7, 255], np.uint8)
    return vals[rng.randint(0, 5, hw)], vals[rng.randint(0, 5, hw)]


@pytest.mark.parametrize("hw", [(16, 16), (37, 53)], ids=lambda hw: "%dx%d" % hw)
@pytest.mark.parametrize("op", range(5), ids=["add", "subtract", "intersect", "xor", "invert"])
def test_combine_follows_the_statement(eng, op, hw):
    a, b = _planes(hw, op)
    if op == L.INVERT:
        b = None
    want = L.spec_combine(a, b, op)
    assert set(np.unique(want)) == {0, 255}
    for k in range(4):                                                 # a, b and out each at an offset of its own
        ab = _Buf(hw, k, like=a)
        bb = None if b is None else _Buf(hw, (k + 1) % 4, like=b)
        ob = _Buf(hw, (k + 2 + k // 2) % 4, fill=GARBAGE)
        eng.plane_combine_u8(ab.view, None if bb is None else bb.view, op, out=ob.view)
        assert np.array_equal(ob.get(), want), (op, hw, k)
        assert np.array_equal(ab.get(), a) and (bb is None or np.array_equal(bb.get(), b))
        # in place on a
        eng.plane_combine_u8(ab.view, None if bb is None else bb.view, op, out=ab.view)
        assert np.array_equal(ab.get(), want), (op, hw, k, "in place on a")
        assert bb is None or np.array_equal(bb.get(), b)
        if bb is not None:                                             # in place on b
            ab = _Buf(hw, (k + 3) % 4, like=a)
            eng.plane_combine_u8(ab.view, bb.view, op, out=bb.view)
            assert np.array_equal(bb.get(), want), (op, hw, k, "in place on b")
            assert np.array_equal(ab.get(), a)
            # a and b the same plane, the output another: a op a
            eng.plane_combine_u8(ab.view, ab.view, op, out=ob.view)
            assert np.array_equal(ob.get(), L.spec_combine(a, a, op)) and np.array_equal(ab.get(), a)
    assert np.array_equal(eng.plane_combine_u8(_cuda(a), None if b is None else _cuda(b), op).cpu().numpy(), want)


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(eng):
    Hi, Wi = 37, 53
    edges, _ = _case("star", (Hi, Wi))
    a, b = _planes((Hi, Wi), 1)
    E, intact = _edges_dev(edges)
    ab, bb, ob = _Buf((Hi, Wi), 1, like=a), _Buf((Hi, Wi), 2, like=b), _Buf((Hi, Wi), 3, fill=GARBAGE)
    big = torch.full((16 * 8200,), GARBAGE, dtype=torch.uint8, device="cuda")              # room for a 16 x 8193 "plane"
    lib, h, st = eng.lib, eng.h, eng._stream()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else t)     # noqa: E731
    A, B, O, N = ab.view, bb.view, ob.view, edges.shape[0]
    inside = E.data_ptr() + 8                                          # a "plane" that begins inside the edges' bytes
    lasso = [((None, N, Hi, Wi, O), "edges"), ((E, N, Hi, Wi, None), "plane_out"), ((E, N, 15, Wi, O), "Hi"), ((E, N, Hi, 15, O), "Wi"),
             ((E, N, 8193, 16, big), "Hi"), ((E, N, 16, 8193, big), "Wi"), ((E, -1, Hi, Wi, O), "N"), ((E, 65537, Hi, Wi, O), "N"),
             ((E.data_ptr() + 2, N - 1, Hi, Wi, O), "aligned"), ((E.data_ptr() + 1, 0, Hi, Wi, O), "aligned"),
             ((E, N, 16, 16, inside), "overlaps"), ((E, N, 16, 16, E.data_ptr() - 16 * 16 + 1), "overlaps")]
    for (e, n, hi, wi, o), what in lasso:
        assert lib.se_lasso_fill_u8(h, st, p(e), n, hi, wi, p(o)) != 0, what
        assert what in lib.se_last_error(h).decode(), (what, lib.se_last_error(h).decode())
    shifted = ab.buf[ab.lead + 1:]                                     # overlaps a without being a
    last = bb.buf[bb.lead + Hi * Wi - 1:]                              # shares b's last byte
    combine = [((None, B, Hi, Wi, 0, O), "a"), ((A, None, Hi, Wi, 0, O), "b"), ((A, None, Hi, Wi, 3, O), "b"), ((A, B, Hi, Wi, 0, None), "out"),
               ((A, B, Hi, Wi, 4, O), "b must be NULL"), ((A, B, 15, Wi, 0, O), "Hi"), ((A, B, Hi, 15, 0, O), "Wi"),
               ((A, B, 8193, 16, 0, big), "Hi"), ((A, B, 16, 8193, 0, big), "Wi"), ((A, B, Hi, Wi, -1, O), "op"), ((A, B, Hi, Wi, 5, O), "op"),
               ((A, B, Hi, Wi, 0, shifted), "overlaps a"), ((A, B, Hi, Wi, 1, last), "overlaps b"), ((A, None, Hi, Wi, 4, shifted), "overlaps a"),
               ((A, B, Hi, Wi, 2, ab.buf[ab.lead - Hi * Wi + 1:]), "overlaps a")]
    for (x, y, hi, wi, op, o), what in combine:
        assert lib.se_plane_combine_u8(h, st, p(x), p(y), hi, wi, op, p(o)) != 0, what
        assert what in lib.se_last_error(h).decode(), (what, lib.se_last_error(h).decode())
    # the bindings refuse edges and planes of another shape or kind
    for call in (lambda: eng.lasso_fill_u8(E.view(-1, 2), Hi, Wi), lambda: eng.lasso_fill_u8(E.float(), Hi, Wi),
                 lambda: eng.lasso_fill_u8(E, Hi, Wi, out=ob.buf[:Hi * Wi].view(Wi, Hi)), lambda: eng.lasso_fill_u8(E, 0, Wi),
                 lambda: eng.plane_combine_u8(A, ob.buf[:Hi * Wi].view(Wi, Hi), 0), lambda: eng.plane_combine_u8(A, B, 0, out=ob.buf[:Hi * Wi].view(Wi, Hi)),
                 lambda: eng.plane_combine_u8(A, B, 4), lambda: eng.plane_combine_u8(A, None, 0), lambda: eng.plane_combine_u8(A, B, 9)):
        with pytest.raises(_lib.SketchEditHipError):
            call()
    torch.cuda.synchronize()
    assert intact() and np.array_equal(ab.get(), a) and np.array_equal(bb.get(), b) and (ob.get() == GARBAGE).all()
    assert (big.cpu().numpy() == GARBAGE).all()


# ---- 4. sessions --------------------------------------------------------------------------------------------------------------------------
FHW = (120, 104)
RING = [(20.3, 30.1), (52.0, 22.5), (84.6, 35.2), (90.25, 70.0), (60.5, 98.75), (25.0, 88.4), (14.2, 60.0)]
HOLE = [(45.0, 50.0), (70.5, 52.25), (66.0, 75.5), (40.75, 70.0)]
SMALL = [(6.0, 5.0), (30.5, 8.0), (12.25, 28.0)]
OUTSIDE = [(-20.0, 40.0), (50.0, -10.0), (130.0, 60.0), (50.0, 140.0)]        # vertices outside the frame move to its border
STAR = [(52.0, 10.0), (75.0, 105.0), (8.0, 45.0), (96.0, 45.0), (29.0, 105.0)]
SLIVER = [(10.25, 10.0), (10.75, 10.0), (60.75, 60.0), (60.25, 60.0)]        # a diagonal strip between the centres


def _blob_frame():
    """a flat blob with a +-3 ramp inside it, on noise: what select_similar takes at (60, 52)"""
    H, W = FHW
    f = U._noise(FHW, 7)
    yy, xx = np.mgrid[0:H, 0:W]
    blob = (yy - 60) ** 2 * 4 + (xx - 52) ** 2 <= 40 * 40
    ramp = (U.REGION + (xx % 7) - 3).astype(np.uint8)
    f[blob] = np.stack([ramp, ramp, np.full_like(ramp, U.REGION)], axis=2)[blob]
    return f, (60, 52)


def _lock_plane():
    lock = np.zeros(FHW, np.uint8)
    lock[55:70, 30:60] = 255                                            # cuts the ring
    lock[::9, ::7] = 255
    return lock


def _session(model, f, lock, **kw):
    """a session whose resident frame lies between sentinel margins -> (session, _Buf)"""
    s = serve.EditSession(model, f, **kw)
    fb = _Buf(f.shape, 3, like=f)
    s._frame = fb.view
    if lock is not None:
        s.set_lock(lock)
    return s, fb


def test_session_select_lasso_is_the_statement(model):
    f, _ = _blob_frame()
    s, fb = _session(model, f, _lock_plane(), history=1)
    n = 0
    for rings in ([RING], [RING, HOLE], [SMALL], [OUTSIDE], [STAR], [SMALL, STAR, HOLE]):
        for grow in (0, 1, 3, 16):
            want = L.spec_select_lasso(rings, FHW, grow)
            sel = s.select_lasso(rings, grow=grow)
            box, count = L.box_count(want)
            assert (sel.box, sel.count, sel.frame_hw) == (box, count, FHW), (rings, grow)
            assert np.array_equal(sel.plane.cpu().numpy(), want)
            assert np.array_equal(sel.mask(), want[box[0]:box[2], box[1]:box[3]])
            n += 1
    assert n == 24 and np.array_equal(fb.get(), f) and not s.can_undo    # not an edit; frame and lock play no part
    hole = L.spec_select_lasso([RING, HOLE], FHW, 0)
    assert hole[60, 55] == 0 and hole[40, 50] == 255                      # a ring inside a ring is a hole
    e = s.select_lasso([SLIVER])
    assert e.box is None and e.count == 0 and not e.plane.cpu().numpy().any() and e.mask().shape == (0, 0)
    with pytest.raises(ValueError, match="empty selection"):
        s.fill_selection(e)
    with pytest.raises(ValueError, match="covers no pixel centre"):
        s.fill_lasso([SLIVER], grow=0)
    assert np.array_equal(fb.get(), f) and not s.can_undo


def test_session_combine_and_invert_are_the_statement(model):
    f, seed = _blob_frame()
    s, fb = _session(model, f, None)
    lasso, hole, small = s.select_lasso([RING]), s.select_lasso([HOLE], grow=1), s.select_lasso([SMALL])
    wand = s.select_similar(seed, tolerance=1, grow=1)                   # the seed's stripes of the ramp
    planes = {k: v.plane.cpu().numpy() for k, v in dict(lasso=lasso, hole=hole, small=small, wand=wand).items()}
    assert np.array_equal(planes["wand"], U.spec_select(f, seed, 1, True, 1)) and np.array_equal(planes["lasso"], L.spec_select_lasso([RING], FHW, 0))

    def check(sel, want):
        box, count = L.box_count(want)
        assert (sel.box, sel.count, sel.frame_hw) == (box, count, FHW)
        assert np.array_equal(sel.plane.cpu().numpy(), want)
        assert np.array_equal(sel.mask(), want[box[0]:box[2], box[1]:box[3]] if box else np.zeros((0, 0), np.uint8))

    sels = dict(lasso=lasso, hole=hole, small=small, wand=wand)
    for x, y in (("lasso", "wand"), ("wand", "lasso"), ("lasso", "hole"), ("small", "hole"), ("lasso", "lasso")):
        for op, code in serve.COMBINE_OPS.items():
            check(s.combine(sels[x], sels[y], op), L.spec_combine(planes[x], planes[y], code))
    minus = s.combine(lasso, wand, "subtract")                           # a lasso minus the part the wand took
    assert 0 < minus.count < lasso.count and minus.count == lasso.count - s.combine(lasso, wand, "intersect").count
    for k in sels:
        check(s.invert(sels[k]), L.spec_combine(planes[k], None, L.INVERT))
        assert np.array_equal(sels[k].plane.cpu().numpy(), planes[k])     # the operands stay what they were
    empty = s.combine(small, hole, "intersect")                          # apart: nothing in common
    assert empty.box is None and empty.count == 0 and not empty.plane.cpu().numpy().any()
    assert s.combine(hole, lasso, "subtract").box is None                # the hole lies inside the ring
    check(s.combine(empty, lasso, "add"), planes["lasso"])
    everything = s.invert(empty)
    assert everything.box == (0, 0) + FHW and everything.count == FHW[0] * FHW[1]
    assert s.invert(everything).box is None
    assert np.array_equal(fb.get(), f)


SESSION_CASES = [dict(), dict(grow=0), dict(grow=1, locked=True), dict(grow=3, locked=True), dict(max_side=64, locked=True),
                 dict(feather=4, locked=True), dict(grow=3, feather=4, max_side=64), dict(grow=0, window=(24, 8, 88, 88), locked=True),
                 dict(hole=True), dict(hole=True, grow=1, feather=4, locked=True)]


@pytest.mark.parametrize("poison", [0, 0xFF])
@pytest.mark.parametrize("case", SESSION_CASES, ids=lambda c: "-".join("%s=%s" % kv for kv in sorted(c.items())) or "defaults")
def test_session_fill_lasso_is_fill_of_the_statement(model, seopt, case, poison):
    """a twin session fills the statement's mask through `fill`: every byte of the two frames is equal, one undo restores every
    byte and redo repeats it.  Under SE_TEST_POISON every scratch byte is a NaN pattern until somebody writes it."""
    case = dict(case)
    f, _ = _blob_frame()
    lock = _lock_plane() if case.pop("locked", False) else None
    rings = [RING, HOLE] if case.pop("hole", False) else [RING]
    grow = case.pop("grow", None)
    mask = L.spec_select_lasso(rings, FHW, 2 if grow is None else grow)
    if poison:
        seopt.set("SE_TEST_POISON", poison)
    a, abuf = _session(model, f, lock, history=2)
    b, bbuf = _session(model, f, lock, history=2)
    pa, posa, ia = a.fill_lasso(rings, low_latency=False, **({} if grow is None else dict(grow=grow)), **case)
    pb, posb, ib = b.fill(mask, low_latency=False, **case)
    after = abuf.get()
    assert np.array_equal(after, bbuf.get()) and not np.array_equal(after, f)
    assert ia.pop("selected") == int((mask > 0).sum()) and ia == ib and posa == posb and np.array_equal(pa, pb)
    changed = (after != f).any(axis=2)
    assert not (changed & (mask == 0)).any() and (lock is None or not (changed & (lock != 0)).any())
    a.undo()
    assert np.array_equal(abuf.get(), f)                                 # one call is one undo step
    assert not a.can_undo
    a.redo()
    assert np.array_equal(abuf.get(), after)


def test_session_fill_lasso_encode_and_fill_of_a_combination(model):
    f, seed = _blob_frame()
    for encode, ref in (("png", lambda s, w: s.frame_png(w)), (("jpg", 90), lambda s, w: s.frame_jpg(w, quality=90))):
        s, fb = _session(model, f, _lock_plane(), history=1)
        patch, _, info = s.fill_lasso([RING], encode=encode, low_latency=False)
        assert isinstance(patch, bytes) and patch == ref(s, info["window"]), encode
        s.undo()
        assert np.array_equal(fb.get(), f)
    # a combination fills as any selection does: the twin fills the statement's mask
    a, abuf = _session(model, f, None, history=1)
    b, bbuf = _session(model, f, None, history=1)
    sel = a.combine(a.select_lasso([RING], grow=1), a.select_similar(seed, tolerance=1, grow=1), "subtract")
    mask = L.spec_combine(L.spec_select_lasso([RING], FHW, 1), U.spec_select(f, seed, 1, True, 1), L.SUBTRACT)
    _, _, ia = a.fill_selection(sel, low_latency=False)
    _, _, ib = b.fill(mask, low_latency=False)
    assert ia.pop("selected") == sel.count == int((mask > 0).sum()) and ia == ib
    assert np.array_equal(abuf.get(), bbuf.get()) and not np.array_equal(abuf.get(), f)
    a.undo()
    assert np.array_equal(abuf.get(), f)


def test_session_set_lock_takes_a_selection(model):
    f, _ = _blob_frame()
    a, abuf = _session(model, f, None, history=1)
    b, bbuf = _session(model, f, None, history=1)
    sel = a.select_lasso([HOLE], grow=2)
    full = L.spec_select_lasso([HOLE], FHW, 2)
    a.set_lock(sel)
    b.set_lock(full)
    assert a.locked and np.array_equal(a.lock(), full) and a._lock_plane.data_ptr() != sel.plane.data_ptr()
    # combining further, in place on the selection's own plane even, does not reach the lock
    a.combine(sel, a.select_lasso([RING]), "add")
    a.model.plane_combine_u8(sel.plane, None, _lib.COMBINE_INVERT, out=sel.plane)
    assert np.array_equal(a.lock(), full)
    sk = np.zeros(FHW, np.uint8)
    sk[40:80, 50:54] = 255
    sk[58:62, 30:80] = 255
    for s in (a, b):
        s.edit(sk, max_grow=0, low_latency=False)
        s.fill_lasso([RING], low_latency=False)
    after = abuf.get()
    assert np.array_equal(after, bbuf.get()) and not np.array_equal(after, f)
    assert not ((after != f).any(axis=2) & (full != 0)).any()           # no locked pixel changed
    a.set_lock(a.select_lasso([SLIVER]))                                 # an empty selection frees the lock
    assert not a.locked and a.lock() is None
