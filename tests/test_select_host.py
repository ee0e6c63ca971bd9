"""Host tests of the selection by colour: the numpy statement of tests/select_util.py against two independent
routes (scipy's labelling and Pillow's flood fill), the host logic of EditSession.select_similar / fill_selection / fill_similar
against a scripted backend that logs every call, and the new entries' place in the C-ABI.  CPU only."""
import os
import re

import numpy as np
import pytest

from sketchedit_amd import _lib, serve
import select_util as U
from test_fill_host import _OldStub, _Stub as _FillStub, _names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HW = (400, 600)
SIZES = [(16, 16), (37, 53), (64, 64), (65, 129), (100, 90), (130, 70)]
PATTERNS = [U.serpentine, U.diagonal, U.two_components, U.border_region, U.blob_with_ramp]


def _random_frame(hw, seed, levels=4):
    """few colours, so that components of every shape exist at every tolerance"""
    rng = np.random.RandomState(seed)
    return (rng.randint(0, levels, tuple(hw) + (3,)) * 20).astype(np.uint8)


def _cases():
    for hw in SIZES:
        for pat in PATTERNS:
            yield pat(hw)
    for k, hw in enumerate([(16, 16), (37, 53), (65, 129)]):
        f = _random_frame(hw, k)
        for seed in ((0, 0), (hw[0] - 1, hw[1] - 1), (hw[0] // 2, hw[1] // 3)):
            yield f, seed


# ---- the statement against independent routes -------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [0, 3, 16, 20, 40, 255])
def test_statement_against_scipy_label(t):
    from scipy import ndimage
    for frame, seed in _cases():
        sim = U.spec_similar(frame, seed, t)
        assert sim[seed]
        labels, _ = ndimage.label(sim)                               # the default structure: 4-connected
        want = labels == labels[seed]
        state = U.spec_state(frame, seed, t, True)
        assert np.array_equal(state == 255, want) and np.array_equal(state > 0, sim)
        assert np.array_equal(U.spec_state(frame, seed, t, False) == 255, sim)
        first = U.spec_state(frame, seed, t, True, flooded=False)
        assert np.array_equal(first > 0, sim) and int((first == 255).sum()) == 1 and first[seed] == 255


def test_statement_against_pillow_floodfill_at_tolerance_0():
    from PIL import Image, ImageDraw
    for frame, seed in _cases():
        img = Image.fromarray(frame).copy()
        mark = (1, 2, 3)                                             # a colour no pattern holds: painted = reached
        assert not (frame == np.array(mark, np.uint8)).all(axis=2).any()
        ImageDraw.floodfill(img, (seed[1], seed[0]), mark, thresh=0)
        want = (np.asarray(img) == np.array(mark, np.uint8)).all(axis=2)
        assert np.array_equal(U.spec_state(frame, seed, 0, True) == 255, want)


def test_serpentine_reaches_every_similar_pixel():
    frame, seed = U.serpentine((100, 90))
    state = U.spec_state(frame, seed, 16, True)
    assert int((state == 255).sum()) == 4361 and not (state == 1).any()
    frame, seed = U.two_components((100, 90))
    state = U.spec_state(frame, seed, 16, True)
    assert (state == 1).sum() == 30 and (state == 255).sum() == 30
    frame, seed = U.diagonal((100, 90))
    assert (U.spec_state(frame, seed, 16, True) == 255).sum() == 25


@pytest.mark.parametrize("r", [0, 1, 2, 3, 7, 16])
def test_grow_against_scipy_maximum_filter(r):
    from scipy import ndimage
    planes = [U.spec_state(f, s, 16, True) == 255 for f, s in (U.serpentine((100, 90)), U.diagonal((37, 53)), U.border_region((65, 129)))]
    for hw in SIZES:
        for at in ((0, 0), (0, hw[1] - 1), (hw[0] - 1, 0), (hw[0] - 1, hw[1] - 1), (0, hw[1] // 2), (hw[0] // 2, 0)):
            p = np.zeros(hw, bool)
            p[at] = True
            planes.append(p)
        planes.append(np.ones(hw, bool))
        planes.append(np.random.RandomState(r).rand(*hw) < 0.01)
    for p in planes:
        want = ndimage.maximum_filter(p.astype(np.uint8) * 255, size=2 * r + 1, mode="constant", cval=0)
        assert np.array_equal(U.spec_grow(p, r), want)
    f, s = U.blob_with_ramp((120, 104))
    assert np.array_equal(U.spec_select(f, s, 16, True, r), U.spec_grow(U.spec_state(f, s, 16, True) == 255, r))


def test_tiles_box_is_the_box_and_count_of_the_plane():
    from sketch_tiles_util import sketch_tiles as spec_tiles
    for frame, seed in (U.blob_with_ramp((120, 104)), U.serpentine((100, 90)), U.two_components((65, 129))):
        plane = U.spec_select(frame, seed, 16, True, 2)
        assert serve.tiles_box(spec_tiles(plane, 32)) == U.spec_box_count(plane)
    assert serve.tiles_box(np.zeros((3, 4, 5), np.int32)) == (None, 0)


# ---- the sessions against a scripted backend ----------------------------------------------------------------------------------
class _Stub(_FillStub):
    """... with the one call a selection adds: the statement itself, on the numpy frame"""

    def select_similar(self, frame, seed, tolerance, contiguous, grow):
        self.calls.append(("select_similar", frame.shape, tuple(seed), tolerance, contiguous, grow))
        plane = U.spec_select(frame, seed, tolerance, contiguous, grow)
        self.plane = plane
        return (plane,) + U.spec_box_count(plane)


def _frame():
    f = U._noise(HW, 5)
    f[200:230, 300:340] = U.REGION
    f[100:110, 100:110] = U.REGION                                    # a second component
    return f


SEED, BOX = (210, 320), (200, 300, 230, 340)


def _session(stub, lock=False, **kw):
    s = serve.EditSession(None, _frame(), backend=stub, **kw)
    if lock:
        plane = np.zeros(HW, np.uint8)
        plane[0:8, 0:8] = 255
        s.set_lock(plane)
    stub.calls.clear()
    return s


def test_select_similar_is_one_backend_call():
    stub = _Stub()
    s = _session(stub, history=2)
    sel = s.select_similar(SEED)
    assert stub.calls == [("select_similar", HW + (3,), SEED, 16, True, 0)]
    assert isinstance(sel, serve.Selection) and sel.box == BOX and sel.count == 30 * 40 and sel.frame_hw == HW and sel.plane is stub.plane
    assert not s.can_undo                                            # not an edit
    stub.calls.clear()
    m = sel.mask()
    assert stub.calls == [("crop", (200, 300, 30, 40))] and m.shape == (30, 40) and (m == 255).all()
    stub.calls.clear()
    sel = s.select_similar((np.int64(210), np.int32(320)), tolerance=0, contiguous=False, grow=3)      # numpy ints are ints
    assert stub.calls == [("select_similar", HW + (3,), SEED, 0, False, 3)]
    assert sel.box == (97, 97, 233, 343) and sel.count == 36 * 46 + 16 * 16


@pytest.mark.parametrize("lock", [False, True])
@pytest.mark.parametrize("history", [0, 2])
@pytest.mark.parametrize("max_side", [None, 128])
@pytest.mark.parametrize("feather", [None, 4])
def test_fill_similar_issues_select_keep_run_save_one_paste_crop(lock, history, max_side, feather):
    stub = _Stub()
    s = _session(stub, lock, history=history)
    patch, (x0, y0), info = s.fill_similar(SEED, max_side=max_side, feather=feather, low_latency=True)
    grown = (198, 298, 232, 342)                                     # grow = 2 is fill_similar's default
    win = serve.choose_window(grown, HW, margin=0.5)
    assert info["window"] == win == (y0, x0) + win[2:] and patch.shape == win[2:] + (3,)
    work = serve.choose_working_size(win[2:], max_side) if max_side else None
    paste = "paste_feather" if feather else "paste_locked"
    assert _names(stub) == ["select_similar", "fill_keep", "run_fill"] + (["save"] if history else []) + [paste, "crop"]
    assert [c for c in stub.calls if c[0] == "upload"] == []           # nothing goes up: no mask, no sketch
    calls = {c[0]: c for c in stub.calls}
    assert calls["select_similar"] == ("select_similar", HW + (3,), SEED, 16, True, 2)
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
    assert info == want
    if history:
        assert s.can_undo and len(s._undo) == 1                      # one call is one undo step
        s.undo()
        assert _names(stub)[-2:] == ["swap", "crop"] and s.can_redo and not s.can_undo


@pytest.mark.parametrize("history", [0, 1])
@pytest.mark.parametrize("feather", [None, 3])
def test_fill_selection_window_choice_sketch_and_encode(history, feather):
    stub = _Stub()
    s = _session(stub, history=history)
    sel = s.select_similar(SEED, grow=1)
    stub.calls.clear()
    _, _, info = s.fill_selection(sel, feather=feather)
    paste = "paste_feather" if feather else "paste_locked"
    assert _names(stub) == ["fill_keep", "run_fill"] + (["save"] if history else []) + [paste, "crop"] and stub.calls[0][0] == "fill_keep"
    assert info["window"] == serve.choose_window((199, 299, 231, 341), HW, margin=0.5) and info["fill"] is True
    assert info["selected"] == 32 * 42 and stub.holes[0] is sel.plane
    # the window is choose_window of the box of selection and sketch TOGETHER, at the call's margin; the sketch goes up as its window
    sk = np.zeros(HW, np.uint8)
    sk[100:110, 500:520] = 255
    stub.calls.clear()
    _, _, info = s.fill_selection(sel, sketch=sk, margin=0.25)
    win = serve.choose_window((100, 299, 231, 520), HW, margin=0.25)
    assert info["window"] == win
    assert [c for c in stub.calls if c[0] == "upload"] == [("upload", win[2:], "uint8")]
    y0, x0, h, w = win
    assert np.array_equal(stub.sketches[0], sk[y0:y0 + h, x0:x0 + w])
    # a given window is taken as it is; a selection is used again and again
    stub.calls.clear()
    _, (px, py), info = s.fill_selection(sel, window=(180, 280, 96, 128))
    assert info["window"] == (180, 280, 96, 128) and (px, py) == (280, 180)
    _, _, info = s.fill_selection(sel, window=(180, 280, 99, 131), max_side=64)
    assert info["window"] == (180, 280, 99, 131) and info["work"] == serve.choose_working_size((99, 131), 64)
    stub.calls.clear()
    patch, _, info = s.fill_selection(sel, encode="png")
    assert patch == b"png" and _names(stub)[-2:] == ["paste_locked", "crop_png"] and stub.calls[-1] == ("crop_png", [info["window"]])
    patch, _, info = s.fill_similar(SEED, encode=("jpg", 80))
    assert patch == b"jpg" and stub.calls[-1][:3] == ("crop_jpg", [info["window"]], 80)
    # a session's selection on a session of another size
    other = serve.EditSession(None, np.zeros((64, 64, 3), np.uint8), backend=_Stub())
    with pytest.raises(ValueError):
        other.fill_selection(sel)


def test_refusals_make_no_backend_call():
    stub = _Stub()
    s = _session(stub, history=1)
    sel = s.select_similar(SEED)
    stub.calls.clear()
    bad = [lambda: s.select_similar((400, 0)),                                          # outside the frame
           lambda: s.select_similar((0, 600)),
           lambda: s.select_similar((-1, 5)),
           lambda: s.select_similar((10.0, 5)),                                         # not ints
           lambda: s.select_similar((True, 5)),
           lambda: s.select_similar(7),
           lambda: s.select_similar((1, 2, 3)),
           lambda: s.select_similar(SEED, tolerance=-1),
           lambda: s.select_similar(SEED, tolerance=256),
           lambda: s.select_similar(SEED, tolerance=1.5),
           lambda: s.select_similar(SEED, grow=-1),
           lambda: s.select_similar(SEED, grow=17),
           lambda: s.select_similar(SEED, grow=2.0),
           lambda: s.fill_similar((400, 0)),
           lambda: s.fill_similar((10.5, 5)),
           lambda: s.fill_similar(SEED, tolerance=300),
           lambda: s.fill_similar(SEED, grow=17),
           lambda: s.fill_similar(SEED, encode="gif"),
           lambda: s.fill_similar(SEED, feather=17),
           lambda: s.fill_similar(SEED, margin=-1.0),
           lambda: s.fill_similar(SEED, max_side=8),
           lambda: s.fill_similar(SEED, window=(0, 0, 100, 128)),                        # sides not multiples of 8 without max_side
           lambda: s.fill_similar(SEED, window=(350, 0, 64, 64)),                        # outside the frame
           lambda: s.fill_similar(SEED, window=(0, 0, 8, 64), max_side=64),              # under 16
           lambda: s.fill_similar(SEED, sketch=np.zeros((10, 10), np.uint8)),
           lambda: s.fill_selection(sel, encode="gif"),
           lambda: s.fill_selection(sel, feather=-1),
           lambda: s.fill_selection(sel, margin=-1.0),
           lambda: s.fill_selection(sel, max_side=8),
           lambda: s.fill_selection(sel, window=(0, 0, 100, 128)),
           lambda: s.fill_selection(sel, window=(350, 0, 64, 64)),
           lambda: s.fill_selection(sel, sketch=np.zeros((10, 10), np.uint8)),
           lambda: s.fill_selection(sel.plane)]                                          # not a Selection
    for k, call in enumerate(bad):
        with pytest.raises((ValueError, TypeError)):
            call()
        assert stub.calls == [] and not s.can_undo, k


def test_a_session_that_never_selects_makes_no_new_call():
    """edit and fill on the backends of before: select_similar does not exist there"""
    sk = np.zeros(HW, np.uint8)
    sk[200:210, 300:330] = 255
    mask = np.zeros(HW, np.uint8)
    mask[200:230, 300:340] = 1
    for lock in (False, True):
        stub = _OldStub()
        s = _session(stub, lock, history=2)
        s.edit(sk, max_grow=0)
        s.edit_strokes([([(30, 20), (60, 30)], 3)])
        s.undo()
        s.redo()
        assert stub.calls and "select_similar" not in _names(stub)
        with pytest.raises(AttributeError):
            s.select_similar(SEED)
        stub = _FillStub()
        s = _session(stub, lock, history=2)
        s.fill(mask)
        s.fill_strokes([([(300.5, 200.0), (340.0, 230.25)], 12.0)])
        s.undo()
        assert stub.calls and "select_similar" not in _names(stub)
        with pytest.raises(AttributeError):
            s.fill_similar(SEED)


def test_model_backend_loop_stops_at_the_first_idle_pass():
    """_ModelBackend.select_similar on a scripted model: flood calls of 8 passes until a call's words hold a 0, then the grow
    and the tile records; not contiguous: no flood call at all"""
    from sketch_tiles_util import sketch_tiles as spec_tiles

    class _T:                                                        # what the backend asks of a tensor
        def __init__(self, a):
            self.a, self.shape = a, a.shape

        def cpu(self):
            return self

        def tolist(self):
            return self.a.tolist()

        def numpy(self):
            return self.a

    class _Model:
        def __init__(self, idle_after):
            self.calls, self.left = [], idle_after

        def select_similar_u8(self, frame, seed, tolerance, contiguous):
            self.calls.append(("similar", seed, tolerance, contiguous))
            self.frame, self.args = frame.a, (seed, tolerance, contiguous)
            return "state"

        def select_flood_u8(self, state, passes):
            self.calls.append(("flood", state, passes))
            words = [1 if k < self.left else 0 for k in range(passes)]
            self.left = max(self.left - passes, 0)
            return _T(np.array(words, np.int32))

        def select_grow_u8(self, state, grow):
            self.calls.append(("grow", state, grow))
            return _T(U.spec_select(self.frame, *self.args, grow))

        def sketch_tiles_u8(self, plane, tile):
            self.calls.append(("tiles", tile))
            return _T(spec_tiles(plane.a, tile))

    frame, seed = U.blob_with_ramp((120, 104))
    want = U.spec_box_count(U.spec_select(frame, seed, 16, True, 2))
    for idle_after, nflood in ((0, 1), (7, 1), (8, 2), (20, 3)):
        be = serve._ModelBackend.__new__(serve._ModelBackend)
        be.model = _Model(idle_after)
        plane, box, count = be.select_similar(_T(frame), seed, 16, True, 2)
        assert [c[0] for c in be.model.calls] == ["similar"] + ["flood"] * nflood + ["grow", "tiles"]
        assert all(c == ("flood", "state", serve.SELECT_PASSES) for c in be.model.calls[1:1 + nflood]) and serve.SELECT_PASSES == 8
        assert (box, count) == want and be.model.calls[-1] == ("tiles", 32)
    be = serve._ModelBackend.__new__(serve._ModelBackend)
    be.model = _Model(5)
    be.select_similar(_T(frame), seed, 16, False, 0)
    assert [c[0] for c in be.model.calls] == ["similar", "grow", "tiles"]


# ---- the C-ABI -------------------------------------------------------------------------------------------------------------
def test_abi_has_three_new_symbols_in_a_header_of_their_own():
    hdr = open(os.path.join(ROOT, "include", "sketchedit_select.h")).read()
    declared = re.findall(r"^(?:int|size_t) (se_\w+)\(", hdr, re.M)
    assert declared == _lib.abi_names("sketchedit_select.h") == ["se_select_similar_u8", "se_select_flood_u8", "se_select_grow_u8"]
    for name in ("sketchedit_hip.h", "sketchedit_fill.h", "sketchedit_feather.h"):
        assert "se_select" not in open(os.path.join(ROOT, "include", name)).read()
    assert "se_select.hip" in _lib.SOURCES
    assert (int(re.search(r"#define SE_SELECT_MAX_GROW (\d+)", hdr).group(1)), int(re.search(r"#define SE_SELECT_MAX_PASSES (\d+)", hdr).group(1))) \
        == (_lib.SELECT_MAX_GROW, _lib.SELECT_MAX_PASSES) == (serve.SELECT_MAX_GROW, 64)
    import ctypes
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    lib = ctypes.CDLL(_lib.LIB_PATH)                                    # the built library, as the other host tests load it
    for s in declared:
        getattr(lib, s)
    from sketchedit_amd import kernel_labels
    assert kernel_labels.label_of("select_similar_kernel(unsigned char const*, unsigned char*, long, long, int, int, long)") == "select_similar"
    assert kernel_labels.label_of("select_flood_kernel(unsigned char*, int, int, int, unsigned int*)") == "select_flood"
    assert kernel_labels.label_of("select_grow_kernel(unsigned char const*, unsigned char*, int, int, int, int)") == "select_grow"
