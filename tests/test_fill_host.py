"""Host tests of fills: the host logic of EditSession.fill / fill_strokes against a scripted backend that logs
every call, and the new entries' place in the C-ABI.  CPU only."""
import os
import re

import numpy as np
import pytest

from sketchedit_amd import _lib, serve
from strokes_util import spec_raster

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HW = (400, 600)


class _OldStub:
    """A scripted device as the sessions knew it before fills: frames and planes are numpy arrays, every backend call is
    logged; run_fill and fill_keep do not exist."""

    def __init__(self):
        self.calls = []

    def upload(self, a):
        self.calls.append(("upload", tuple(np.shape(a)), np.asarray(a).dtype.name))
        return np.array(a)

    def _ret(self, n, h, w):
        return np.zeros((n, h, w, 3), np.uint8), np.full((n, h, w), 255, np.uint8)

    def run(self, frames, origins, sketches, h, w, commit, low_latency):
        self.calls.append(("run", len(frames), (h, w), bool(commit)))
        return self._ret(len(frames), h, w) + ([[0, 0, 0, 0] for _ in frames],)

    def run_locked(self, frames, origins, sketches, locks, window_hw, work_hw, commit, low_latency):
        self.calls.append(("run_locked", len(frames), tuple(window_hw), work_hw, bool(commit)))
        return self._ret(len(frames), *(work_hw or window_hw)) + ([[0, 0, 0, 0] for _ in frames],)

    def paste_locked(self, frames, origins, locks, window_hw, rgb, m8):
        self.calls.append(("paste_locked", [id(t) for t in locks], tuple(window_hw), tuple(rgb.shape), tuple(m8.shape)))

    def paste_feather(self, frames, origins, locks, window_hw, radius, rgb, m8):
        self.calls.append(("paste_feather", [id(t) for t in locks], tuple(window_hw), radius, tuple(rgb.shape), tuple(m8.shape)))

    def save(self, frames, origins, window_hw):
        self.calls.append(("save", len(frames), tuple(window_hw)))
        return [np.zeros(1, np.uint8) for _ in frames]

    def swap(self, frames, origins, window_hw, slots):
        self.calls.append(("swap", len(frames)))

    def strokes(self, segs, frame_hw, windows):
        self.calls.append(("strokes", tuple(frame_hw), [tuple(w) for w in windows]))
        return [spec_raster(segs, frame_hw, w) for w in windows]

    def window_of(self, plane, y0, x0, h, w):
        self.calls.append(("window_of", (y0, x0, h, w)))
        return plane[y0:y0 + h, x0:x0 + w].copy()

    def crop(self, frame, y0, x0, h, w):
        self.calls.append(("crop", (y0, x0, h, w)))
        return frame[y0:y0 + h, x0:x0 + w].copy()

    def crop_png(self, frames, windows):
        self.calls.append(("crop_png", [tuple(w) for w in windows]))
        return [b"png"] * len(windows)

    def crop_jpg(self, frames, windows, quality, **kw):
        self.calls.append(("crop_jpg", [tuple(w) for w in windows], quality, kw))
        return [b"jpg"] * len(windows)

    def download(self, frame):
        return frame.copy()


class _Stub(_OldStub):
    """... with the two calls a fill adds"""

    def fill_keep(self, frames, origins, holes, locks, window_hw):
        self.calls.append(("fill_keep", list(origins), [h.shape for h in holes], None if locks is None else len(locks), tuple(window_hw)))
        self.holes = holes
        self.keeps = [np.zeros(h.shape, np.uint8) for h in holes]
        return self.keeps

    def run_fill(self, frames, origins, sketches, holes, locks, window_hw, work_hw, low_latency):
        self.calls.append(("run_fill", list(origins), [None if s is None else s.shape for s in sketches], None if locks is None else len(locks),
                           tuple(window_hw), work_hw, low_latency))
        assert all(a is b for a, b in zip(holes, self.holes))              # the plane the keep was made of
        self.sketches = sketches
        return self._ret(len(frames), *(work_hw or window_hw))


def _names(stub, skip=("upload", "window_of")):
    return [c[0] for c in stub.calls if c[0] not in skip]


def _mask():
    m = np.zeros(HW, np.uint8)
    m[200:230, 300:340] = 1
    return m


def _session(stub, lock=False, **kw):
    s = serve.EditSession(None, np.zeros(HW + (3,), np.uint8), backend=stub, **kw)
    if lock:
        plane = np.zeros(HW, np.uint8)
        plane[0:8, 0:8] = 255
        s.set_lock(plane)
    stub.calls.clear()
    return s


@pytest.mark.parametrize("lock", [False, True])
@pytest.mark.parametrize("history", [0, 2])
@pytest.mark.parametrize("max_side", [None, 128])
@pytest.mark.parametrize("feather", [None, 4])
def test_fill_issues_keep_run_save_one_paste_crop(lock, history, max_side, feather):
    stub = _Stub()
    s = _session(stub, lock, history=history)
    patch, (x0, y0), info = s.fill(_mask(), max_side=max_side, feather=feather, low_latency=True)
    win = serve.choose_window((200, 300, 230, 340), HW, margin=0.5)
    assert info["window"] == win == (y0, x0) + win[2:] and info["fill"] is True and patch.shape == win[2:] + (3,)
    work = serve.choose_working_size(win[2:], max_side) if max_side else None
    paste = "paste_feather" if feather else "paste_locked"
    assert _names(stub) == ["fill_keep", "run_fill"] + (["save"] if history else []) + [paste, "crop"]
    # the one upload: the mask as 0 / 255
    assert [c for c in stub.calls if c[0] == "upload"] == [("upload", HW, "uint8")]
    assert set(np.unique(stub.holes[0])) == {0, 255} and np.array_equal(stub.holes[0] > 0, _mask() > 0)
    calls = {c[0]: c for c in stub.calls}
    assert calls["fill_keep"] == ("fill_keep", [win[:2]], [HW], 1 if lock else None, win[2:])
    assert calls["run_fill"] == ("run_fill", [win[:2]], [None], 1 if lock else None, win[2:], work, True)
    out_hw = work or win[2:]
    if feather:
        assert calls[paste] == (paste, [id(stub.keeps[0])], win[2:], 4, (1,) + out_hw + (3,), (1,) + out_hw)
    else:
        assert calls[paste] == (paste, [id(stub.keeps[0])], win[2:], (1,) + out_hw + (3,), (1,) + out_hw)
    want = dict(window=win, fill=True)
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


def test_fill_window_choice_sketch_and_encode():
    # the window is choose_window of the box of mask and sketch TOGETHER, at the call's margin; the sketch goes up as its window
    sk = np.zeros(HW, np.uint8)
    sk[100:110, 500:520] = 255
    stub = _Stub()
    _, _, info = _session(stub).fill(_mask(), sketch=sk, margin=0.25)
    win = serve.choose_window((100, 300, 230, 520), HW, margin=0.25)
    assert info["window"] == win
    ups = [c for c in stub.calls if c[0] == "upload"]
    assert ups == [("upload", HW, "uint8"), ("upload", win[2:], "uint8")]
    y0, x0, h, w = win
    assert np.array_equal(stub.sketches[0], sk[y0:y0 + h, x0:x0 + w])   # as given: not masked by the hole
    # bool masks and PIL images; a given window is taken as it is (any sides >= 16 with max_side)
    from PIL import Image
    for m in (_mask() > 0, Image.fromarray(_mask() * 255)):
        stub = _Stub()
        _, (px, py), info = _session(stub).fill(m, window=(180, 280, 96, 128))
        assert info["window"] == (180, 280, 96, 128) and (px, py) == (280, 180) and np.array_equal(stub.holes[0] > 0, _mask() > 0)
    stub = _Stub()
    _, _, info = _session(stub).fill(_mask(), window=(180, 280, 99, 131), max_side=64)
    assert info["window"] == (180, 280, 99, 131) and info["work"] == serve.choose_working_size((99, 131), 64)
    # encode: the patch is made after the paste, by the encoder's call
    stub = _Stub()
    patch, _, info = _session(stub).fill(_mask(), encode="png")
    assert patch == b"png" and _names(stub) == ["fill_keep", "run_fill", "paste_locked", "crop_png"]
    assert stub.calls[-1] == ("crop_png", [info["window"]])
    stub = _Stub()
    patch, _, _ = _session(stub).fill(_mask(), encode=("jpg", 80))
    assert patch == b"jpg" and stub.calls[-1][:3] == ("crop_jpg", [info["window"]], 80)


def test_fill_refusals_make_no_backend_call():
    stub = _Stub()
    s = _session(stub, history=1)
    bad = [lambda: s.fill(np.zeros(HW, np.uint8)),                                     # all zero
           lambda: s.fill(np.zeros(HW, bool)),
           lambda: s.fill(np.ones((10, 10), np.uint8)),                                # another size
           lambda: s.fill(_mask().astype(np.float32)),                                 # another type
           lambda: s.fill(_mask(), sketch=np.zeros((10, 10), np.uint8)),
           lambda: s.fill(_mask(), window=(0, 0, 100, 128)),                           # sides not multiples of 8 without max_side
           lambda: s.fill(_mask(), window=(350, 0, 64, 64)),                           # outside the frame
           lambda: s.fill(_mask(), window=(0, 0, 8, 64), max_side=64),                 # under 16
           lambda: s.fill(_mask(), encode="gif"),
           lambda: s.fill(_mask(), feather=17),
           lambda: s.fill(_mask(), margin=-1.0),
           lambda: s.fill_strokes([]),
           lambda: s.fill_strokes([([(10, 10)], 0.1)]),                                # a width the rasteriser refuses
           lambda: s.fill_strokes([([(10, 10)], 4)], sketch_strokes=[([], 3)]),
           lambda: s.fill_strokes([([(10, 10)], 4)], window=(0, 0, 100, 128)),
           lambda: s.fill_strokes([([(10, 10)], 4)], feather=-1)]
    for call in bad:
        with pytest.raises((ValueError, TypeError)):
            call()
    assert stub.calls == [] and not s.can_undo
    from PIL import Image
    with pytest.raises(ValueError):
        s.fill(Image.fromarray(np.zeros(HW + (3,), np.uint8)))
    assert stub.calls == []


@pytest.mark.parametrize("lock", [False, True])
@pytest.mark.parametrize("history", [0, 1])
@pytest.mark.parametrize("feather", [None, 3])
@pytest.mark.parametrize("max_side", [None, 128])
def test_fill_strokes_uploads_segments_only(lock, history, feather, max_side):
    strokes = [([(300.5, 200.0), (340.0, 230.25)], 12.0)]
    guides = [([(310.0, 190.0), (320.0, 260.0)], 2.0)]
    for sketch_strokes in (None, guides):
        stub = _Stub()
        s = _session(stub, lock, history=history)
        _, _, info = s.fill_strokes(strokes, sketch_strokes=sketch_strokes, feather=feather, max_side=max_side)
        segs, _ = serve.stroke_segments(strokes, HW)
        all_segs = segs if sketch_strokes is None else np.concatenate([segs, serve.stroke_segments(guides, HW)[0]])
        win = serve.choose_window(serve.stroke_box(all_segs, HW), HW, margin=0.5)
        assert info["window"] == win and info["fill"] is True
        work = serve.choose_working_size(win[2:], max_side) if max_side else win[2:]
        assert work != win[2:] if max_side else "work" not in info
        assert info.get("work", win[2:]) == work
        n = 1 if sketch_strokes is None else 2
        # nothing but the segments goes up, and each set is rasterised with the whole frame as its one window
        assert [c[1:] for c in stub.calls if c[0] == "upload"] == [((len(segs), 5), "int32"), ((len(all_segs) - len(segs), 5), "int32")][:n]
        assert [c for c in stub.calls if c[0] == "strokes"] == [("strokes", HW, [(0, 0) + HW])] * n
        assert _names(stub) == ["strokes"] * n + ["fill_keep", "run_fill"] + (["save"] if history else []) + \
            ["paste_feather" if feather else "paste_locked", "crop"]
        assert np.array_equal(stub.holes[0], spec_raster(segs, HW))
        y0, x0, h, w = win
        if sketch_strokes is None:
            assert stub.sketches == [None]
        else:
            assert np.array_equal(stub.sketches[0], spec_raster(all_segs[len(segs):], HW)[y0:y0 + h, x0:x0 + w])


def test_a_session_that_only_edits_makes_no_new_call():
    """edit on the backend of before: neither run_fill nor fill_keep exists there"""
    sk = np.zeros(HW, np.uint8)
    sk[200:210, 300:330] = 255
    for lock in (False, True):
        stub = _OldStub()
        s = _session(stub, lock, history=2)
        s.edit(sk, max_grow=0)
        s.edit_strokes([([(30, 20), (60, 30)], 3)])
        s.undo()
        s.redo()
        assert stub.calls and not {"run_fill", "fill_keep"} & set(_names(stub))
        with pytest.raises(AttributeError):
            s.fill(_mask())


def test_a_fill_is_undone_like_an_edit():
    stub = _Stub()
    s = _session(stub, history=2)
    _, _, finfo = s.fill(_mask())
    win = finfo["window"]
    stub.calls.clear()
    patch, pos, uinfo = s.undo()
    assert stub.calls == [("swap", 1), ("crop", win)] and patch.shape == win[2:] + (3,) and pos == (win[1], win[0])
    assert uinfo == dict(window=win, undo_depth=0, redo_depth=1)
    stub.calls.clear()
    s.redo()
    assert stub.calls == [("swap", 1), ("crop", win)] and s.can_undo and not s.can_redo
    # a fill drops the redo entries, as an edit does
    s.undo()
    s.fill(_mask(), window=(100, 100, 64, 64))
    assert not s.can_redo and len(s._undo) == 1


def test_abi_has_four_new_symbols_in_a_header_of_their_own():
    hdr = open(os.path.join(ROOT, "include", "sketchedit_fill.h")).read()
    declared = set(re.findall(r"^(?:int|size_t) (se_\w+)\(", hdr, re.M))
    own = _lib.abi_names("sketchedit_fill.h")
    assert declared == set(own) and len(own) == 4
    main = open(os.path.join(ROOT, "include", "sketchedit_hip.h")).read()
    assert "se_fill" not in main and "se_fill.hip" in _lib.SOURCES
    import ctypes
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    lib = ctypes.CDLL(_lib.LIB_PATH)                                    # the built library, as the other host tests load it
    for s in own:
        getattr(lib, s)
    from sketchedit_amd import kernel_labels
    assert kernel_labels.label_of("fill_masks_kernel(unsigned char const*, long)") == "fill_masks"
    assert kernel_labels.label_of("fill_keep_kernel(se_window const*, int, int, int)") == "fill_keep"
