"""Host tests of the feathered paste: the host logic of `feather=` in EditSession.edit / edit_regions /
edit_strokes and BatchingServer(window=True, feather=...) against a scripted backend that logs every call, and the new entry's
place in the C-ABI.  CPU only."""
import os
import re

import numpy as np
import pytest

from sketchedit_amd import _lib, serve
from sketch_tiles_util import sketch_tiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HW = (400, 600)
POLICY = dict(min_side=64, bucket=8)


class _Stub:
    """A scripted device: frames and planes are numpy arrays, every backend call is logged.  `hits`: the border counts every run
    reports (non-zero: the window wants to grow)."""

    def __init__(self, hits=0):
        self.calls, self.hits = [], hits

    def upload(self, a):
        return np.array(a)

    def _ret(self, n, h, w):
        return np.zeros((n, h, w, 3), np.uint8), np.full((n, h, w), 255, np.uint8), [[self.hits, 0, 0, 0] for _ in range(n)]

    def run(self, frames, origins, sketches, h, w, commit, low_latency):
        self.calls.append(("run", len(frames), (h, w), bool(commit)))
        return self._ret(len(frames), h, w)

    def run_scaled(self, frames, origins, sketches, window_hw, work_hw, commit, low_latency):
        self.calls.append(("run_scaled", len(frames), tuple(window_hw), tuple(work_hw), bool(commit)))
        return self._ret(len(frames), *work_hw)

    def run_locked(self, frames, origins, sketches, locks, window_hw, work_hw, commit, low_latency):
        self.calls.append(("run_locked", len(frames), tuple(window_hw), work_hw, bool(commit)))
        return self._ret(len(frames), *(work_hw or window_hw))

    def paste(self, frames, origins, rgb, m8):
        self.calls.append(("paste", len(frames)))

    def paste_scaled(self, frames, origins, window_hw, rgb, m8):
        self.calls.append(("paste_scaled", len(frames)))

    def paste_locked(self, frames, origins, locks, window_hw, rgb, m8):
        self.calls.append(("paste_locked", len(frames)))

    def paste_feather(self, frames, origins, locks, window_hw, radius, rgb, m8):
        self.calls.append(("paste_feather", len(frames), tuple(window_hw), radius, None if locks is None else len(locks),
                           tuple(rgb.shape), tuple(m8.shape)))

    def save(self, frames, origins, window_hw):
        self.calls.append(("save", len(frames), tuple(window_hw)))
        return [np.zeros(1, np.uint8) for _ in frames]

    def swap(self, frames, origins, window_hw, slots):
        self.calls.append(("swap", len(frames)))

    def tiles(self, sketch, tile):
        self.calls.append(("tiles", tile))
        return sketch_tiles(sketch, tile)

    def window_of(self, plane, y0, x0, h, w):
        return plane[y0:y0 + h, x0:x0 + w].copy()

    def strokes(self, segs, frame_hw, windows):
        self.calls.append(("strokes", len(windows)))
        return [np.zeros(w[2:], np.uint8) for w in windows]

    def select(self, t, idx):
        return t[list(idx)]

    def crop(self, frame, y0, x0, h, w):
        return frame[y0:y0 + h, x0:x0 + w].copy()

    def crop_png(self, frames, windows):
        self.calls.append(("crop_png", len(windows)))
        return [b"png"] * len(windows)

    def download(self, frame):
        return frame.copy()


class _NoFeatherStub(_Stub):
    """the backend of the sessions before the feathered paste: the call does not exist"""
    paste_feather = None


def _sketch():
    sk = np.zeros(HW, np.uint8)
    sk[200:210, 300:330] = 255
    return sk


def _two():
    sk = np.zeros(HW, np.uint8)
    sk[20:30, 30:60] = 255               # a small stroke, top left
    sk[300:310, 400:520] = 255           # a longer one, bottom right: a window of another size
    return sk


def _session(stub, lock=False, **kw):
    s = serve.EditSession(None, np.zeros(HW + (3,), np.uint8), backend=stub, **kw)
    if lock:
        plane = np.zeros(HW, np.uint8)
        plane[0:8, 0:8] = 255
        s.set_lock(plane)
    return s


EDITS = [dict(max_grow=0), dict(max_grow=2), dict(max_grow=0, max_side=32), dict(max_grow=1, max_side=32), dict(max_grow=0, encode="png")]


@pytest.mark.parametrize("hits", [0, 1])
@pytest.mark.parametrize("lock", [False, True])
@pytest.mark.parametrize("history", [0, 2])
def test_feather_none_and_0_issue_todays_calls(hits, lock, history):
    """the expected lists come from the calls without the keyword, on a backend that has no paste_feather at all"""
    for kw in EDITS:
        want = _NoFeatherStub(hits)
        out = _session(want, lock, history=history).edit(_sketch(), **kw)
        assert want.calls
        for f in (None, 0):
            got = _Stub(hits)
            out_f = _session(got, lock, history=history).edit(_sketch(), feather=f, **kw)
            assert got.calls == want.calls and out_f[2] == out[2] and "feather" not in out_f[2]
    for method, arg, kw in (("edit_regions", _two(), dict(tile=16, **POLICY)), ("edit_strokes", [([(30, 20), (60, 30)], 3), ([(400, 300), (520, 310)], 3)], POLICY)):
        want = _NoFeatherStub(hits)
        out = getattr(_session(want, lock, history=history), method)(arg, **kw)
        assert len(out[2]["windows"]) == 2 and want.calls
        for f in (None, 0):
            got = _Stub(hits)
            out_f = getattr(_session(got, lock, history=history), method)(arg, feather=f, **kw)
            assert got.calls == want.calls and out_f[2] == out[2] and "feather" not in out_f[2]


def _names(stub):
    return [c[0] for c in stub.calls]


@pytest.mark.parametrize("lock", [False, True])
def test_feather_never_commits_and_saves_before_the_paste(lock):
    run = "run_locked" if lock else "run"
    stub = _Stub()
    s = _session(stub, lock, history=2)
    patch, (x0, y0), info = s.edit(_sketch(), max_grow=0, feather=5)
    h, w = info["window"][2:]
    assert info["feather"] == 5 and info["undoable"] is True and patch.shape == (h, w, 3)
    assert _names(stub) == [run, "save", "paste_feather"] and stub.calls[0][-1] is False
    assert stub.calls[2] == ("paste_feather", 1, (h, w), 5, 1 if lock else None, (1, h, w, 3), (1, h, w))
    # a grow loop: every run uncommitted, one save and one paste for the final window only
    stub = _Stub(hits=1)
    _, _, info = _session(stub, lock, history=2).edit(_sketch(), max_grow=2, feather=16)
    assert info["reruns"] == 2 and info["feather"] == 16
    assert _names(stub) == [run, run, run, "save", "paste_feather"] and not any(c[-1] for c in stub.calls[:3])
    assert stub.calls[4][2] == tuple(info["window"][2:])
    # no journal: no save
    stub = _Stub()
    _, _, info = _session(stub, lock).edit(_sketch(), max_grow=0, feather=1)
    assert _names(stub) == [run, "paste_feather"] and "undoable" not in info
    # at a working size: the scaled run, its results handed to the paste as they are
    stub = _Stub()
    _, _, info = _session(stub, lock, history=1).edit(_sketch(), max_grow=0, max_side=32, feather=3)
    assert _names(stub) == ["run_locked" if lock else "run_scaled", "save", "paste_feather"] and stub.calls[0][-1] is False
    assert stub.calls[2][5] == (1,) + tuple(info["work"]) + (3,) and stub.calls[2][2] == tuple(info["window"][2:])
    # encode: the patch is made after the paste
    stub = _Stub()
    patch, _, _ = _session(stub, lock).edit(_sketch(), max_grow=0, feather=3, encode="png")
    assert _names(stub) == [run, "paste_feather", "crop_png"] and patch == b"png"


def test_undo_is_one_step():
    stub = _Stub()
    s = _session(stub, history=2)
    s.edit(_sketch(), max_grow=0, feather=4)
    assert s.can_undo and len(s._undo) == 1
    s.undo()
    assert _names(stub)[-1] == "swap" and s.can_redo and not s.can_undo


@pytest.mark.parametrize("method,arg,kw", [("edit_regions", _two(), dict(tile=16, **POLICY)),
                                           ("edit_strokes", [([(30, 20), (60, 30)], 3), ([(400, 300), (520, 310)], 3)], POLICY)])
def test_region_edits_paste_once_per_size_group(method, arg, kw):
    stub = _Stub()
    s = _session(stub, history=1)
    _, _, info = getattr(s, method)(arg, feather=6, **kw)
    sizes = [w[2:] for w in info["windows"]]
    assert len(set(sizes)) == 2 and info["groups"] == 2 and info["feather"] == 6 and info["undoable"] is True
    per_group = [c for c in stub.calls if c[0] in ("run", "save", "paste_feather")]
    assert [c[0] for c in per_group] == ["run", "save", "paste_feather"] * 2
    assert not any(c[-1] for c in per_group if c[0] == "run")
    assert [c[2] for c in per_group if c[0] == "paste_feather"] == sizes and len(s._undo) == 1
    # two windows of one size: one group, one paste with B = 2
    sk = np.zeros(HW, np.uint8)
    sk[20:30, 30:60] = 255
    sk[300:310, 400:430] = 255
    stub = _Stub()
    _, _, info = _session(stub).edit_regions(sk, feather=2, tile=16, **POLICY)
    assert info["groups"] == 1 and [c[:2] for c in stub.calls if c[0] != "tiles"] == [("run", 2), ("paste_feather", 2)]


@pytest.mark.parametrize("bad", [-1, 17, True, 2.5, "3"])
def test_bad_feather_is_refused_before_any_backend_call(bad):
    stub = _Stub()
    s = _session(stub)
    for call in (lambda: s.edit(_sketch(), feather=bad), lambda: s.edit_regions(_two(), feather=bad),
                 lambda: s.edit_strokes([([(30, 20), (60, 30)], 3)], feather=bad)):
        with pytest.raises(ValueError):
            call()
    assert stub.calls == []
    with pytest.raises(ValueError):
        serve.BatchingServer(model=object(), window=True, feather=bad)
    with pytest.raises(ValueError):
        serve.BatchingServer(model=object(), feather=3)                # feather needs window=True


def test_server_runs_uncommitted_saves_then_pastes_once():
    model = object()
    stub = _Stub()
    a = serve.EditSession(model, np.zeros(HW + (3,), np.uint8), backend=stub, history=1)
    b = serve.EditSession(model, np.zeros((300, 500, 3), np.uint8), backend=stub)
    sk_b = np.zeros((300, 500), np.uint8)
    sk_b[100:110, 200:230] = 255
    srv = serve.BatchingServer(model=model, window=True, max_batch=2, max_wait_s=5.0, max_grow=0, feather=7)
    try:
        import threading
        outs = {}
        ts = [threading.Thread(target=lambda k=k, s=s, sk=sk: outs.__setitem__(k, srv.submit(s, sk)))
              for k, (s, sk) in enumerate([(a, _sketch()), (b, sk_b)])]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
    finally:
        srv.close()
    assert srv.batches == [2]
    assert outs[0][2]["feather"] == 7 and outs[1][2]["feather"] == 7 and outs[0][2]["undoable"] is True
    names = _names(stub)
    assert names == ["run", "save", "paste_feather"] and stub.calls[0][1] == 2 and stub.calls[0][-1] is False
    assert stub.calls[1][1] == 1 and stub.calls[2][1] == 2 and stub.calls[2][3] == 7
    # the same server without the keyword commits in the run
    stub2 = _NoFeatherStub()
    c = serve.EditSession(model, np.zeros(HW + (3,), np.uint8), backend=stub2)
    srv = serve.BatchingServer(model=model, window=True, max_batch=1, max_grow=0)
    try:
        _, _, info = srv.submit(c, _sketch())
    finally:
        srv.close()
    assert "feather" not in info and _names(stub2) == ["run"] and stub2.calls[0][-1] is True


def test_abi_has_one_new_symbol_in_a_header_of_its_own():
    hdr = open(os.path.join(ROOT, "include", "sketchedit_feather.h")).read()
    declared = set(re.findall(r"^(?:int|size_t) (se_\w+)\(", hdr, re.M))
    own = _lib.abi_names("sketchedit_feather.h")
    assert declared == set(own) and len(own) == 1
    assert re.search(r"int se_window_paste_feather_u8\(se_ctx\* ctx, void\* stream, const se_window\* wins, const unsigned char\* const\* locks, "
                     r"int B, int hs, int ws,\s+int radius, const unsigned char\* rgb, const unsigned char\* mask_u8\);", hdr)
    main = open(os.path.join(ROOT, "include", "sketchedit_hip.h")).read()
    assert "se_window_paste_feather_u8" not in main and "se_feather.hip" in _lib.SOURCES
    assert _lib.FEATHER_MAX_RADIUS == serve.FEATHER_MAX_RADIUS == int(re.search(r"#define SE_FEATHER_MAX_RADIUS (\d+)", hdr).group(1))
    if os.path.exists(_lib.LIB_PATH):
        import ctypes
        import torch  # noqa: F401  (before the library: one HIP runtime per process)
        lib = ctypes.CDLL(_lib.LIB_PATH)
        for s in own:
            getattr(lib, s)
    from sketchedit_amd import kernel_labels
    assert kernel_labels.label_of("window_paste_feather_kernel(se_window const*, int)") == "window_paste_feather"
