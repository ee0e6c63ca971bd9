"""Host-side logic of a session's undo journal, no GPU: stack semantics, the two caps and their eviction
order, the oversize-edit rule, what the grow loop journals, `history=0` as the session without a journal -- against a
numpy stand-in for the device side with `save` / `swap` -- and `se_window_saved_bytes` through the built library."""
import ctypes
import threading
import time

import numpy as np
import pytest

from sketchedit_amd import _lib, serve

HW = (1081, 1921)


class _Stub:
    """Frames are numpy arrays; an edit writes a new value (1, 2, 3, ...) over its whole window; a slot is the crop's copy."""

    def __init__(self, script=()):
        self.script = list(script)
        self.calls, self.value = [], 0

    def upload(self, a):
        return np.array(a)

    def _write(self, frames, origins, hw):
        for f, (y0, x0) in zip(frames, origins):
            self.value += 1
            f[y0:y0 + hw[0], x0:x0 + hw[1]] = self.value

    def run(self, frames, origins, sketches, h, w, commit, low_latency):
        self.calls.append(("run", [(y0, x0, h, w) for y0, x0 in origins], bool(commit)))
        n = len(frames)
        if commit:
            self._write(frames, origins, (h, w))
        counts = [list(self.script.pop(0) if self.script else [0, 0, 0, 0]) for _ in range(n)]
        return np.zeros((n, h, w, 3), np.uint8), np.full((n, h, w), 255, np.uint8), counts

    def paste(self, frames, origins, rgb, m8):
        self.calls.append(("paste", [(y0, x0) + tuple(rgb.shape[1:3]) for y0, x0 in origins]))
        self._write(frames, origins, rgb.shape[1:3])

    def save(self, frames, origins, window_hw):
        h, w = window_hw
        self.calls.append(("save", [(y0, x0, h, w) for y0, x0 in origins]))
        return [f[y0:y0 + h, x0:x0 + w].copy() for f, (y0, x0) in zip(frames, origins)]

    def swap(self, frames, origins, window_hw, slots):
        h, w = window_hw
        self.calls.append(("swap", [(y0, x0, h, w) for y0, x0 in origins]))
        for f, (y0, x0), s in zip(frames, origins, slots):
            old = f[y0:y0 + h, x0:x0 + w].copy()
            f[y0:y0 + h, x0:x0 + w] = s
            s[...] = old

    def select(self, t, idx):
        return t[list(idx)]

    def crop(self, frame, y0, x0, h, w):
        return frame[y0:y0 + h, x0:x0 + w].copy()

    def download(self, frame):
        return frame.copy()


def _sketch(box, hw=HW):
    sk = np.zeros(hw, np.uint8)
    sk[box[0]:box[2], box[1]:box[3]] = 255
    return sk


def _session(script=(), hw=HW, **kw):
    stub = _Stub(script)
    return serve.EditSession(None, np.zeros(hw + (3,), np.uint8), backend=stub, **kw), stub


WIN_A, WIN_B = (8, 16, 64, 32), (40, 24, 32, 64)           # overlapping, given windows (they never grow)


def test_stack_semantics():
    s, stub = _session(history=8)
    sk = _sketch((500, 900, 560, 1000))
    assert not s.can_undo and not s.can_redo
    for what in (s.undo, s.redo):
        with pytest.raises(IndexError):
            what()
    f0 = s.frame()
    _, _, info = s.edit(sk, window=WIN_A)
    assert info["undoable"] is True
    f1 = s.frame()
    s.edit(sk, window=WIN_B)
    f2 = s.frame()
    assert not np.array_equal(f1, f0) and not np.array_equal(f2, f1)
    patch, (x0, y0), info = s.undo()
    assert np.array_equal(s.frame(), f1) and info == dict(window=WIN_B, undo_depth=1, redo_depth=1) and (x0, y0) == (24, 40)
    assert np.array_equal(patch, f1[40:72, 24:88])
    patch, _, info = s.undo()
    assert np.array_equal(s.frame(), f0) and info == dict(window=WIN_A, undo_depth=0, redo_depth=2)
    assert np.array_equal(patch, f0[8:72, 16:48]) and s.can_redo and not s.can_undo
    with pytest.raises(IndexError):
        s.undo()
    patch, _, info = s.redo()
    assert np.array_equal(s.frame(), f1) and info == dict(window=WIN_A, undo_depth=1, redo_depth=1)
    assert np.array_equal(patch, f1[8:72, 16:48])
    s.redo()
    assert np.array_equal(s.frame(), f2) and not s.can_redo
    with pytest.raises(IndexError):
        s.redo()
    s.undo()
    s.undo()
    s.redo()                                                  # at f1, one entry on each side
    s.edit(sk, window=(100, 100, 16, 16))                     # a new edit drops the redo entries
    assert not s.can_redo and s.can_undo
    with pytest.raises(IndexError):
        s.redo()
    s.undo()
    assert np.array_equal(s.frame(), f1)
    # the save precedes the committing run, and there is one per edit
    kinds = [c[0] for c in stub.calls]
    assert kinds[:4] == ["save", "run", "save", "run"] and kinds.count("save") == 3


def test_history_count_evicts_the_oldest():
    s, stub = _session(history=2)
    sk = _sketch((500, 900, 560, 1000))
    frames = [s.frame()]
    for i in range(4):
        s.edit(sk, window=(8 * i, 16, 32, 32))
        frames.append(s.frame())
    assert s.history_bytes_used == 2 * serve.window_saved_bytes(32, 32)
    s.undo()
    assert np.array_equal(s.frame(), frames[3])
    s.undo()
    assert np.array_equal(s.frame(), frames[2])
    with pytest.raises(IndexError):                           # the entries of the first two edits were dropped, oldest first
        s.undo()
    assert s.history_bytes_used == 2 * serve.window_saved_bytes(32, 32)          # undo and redo slots count together


def test_history_bytes_cap_and_accounting():
    small, big = serve.window_saved_bytes(16, 16), serve.window_saved_bytes(32, 40)
    assert (small, big) == (16 * 48, 32 * 128)
    s, stub = _session(history=10, history_bytes=big + small)
    sk = _sketch((500, 900, 560, 1000))
    frames = [s.frame()]
    for win in [(0, 0, 16, 16), (0, 0, 32, 40), (8, 8, 16, 16)]:
        _, _, info = s.edit(sk, window=win)
        assert info["undoable"] is True
        frames.append(s.frame())
    # 768 + 4096 + 768 is over 4864: the oldest entry went
    assert s.history_bytes_used == big + small
    s.undo()
    s.undo()
    assert np.array_equal(s.frame(), frames[1]) and not s.can_undo and s.history_bytes_used == big + small
    s.redo()
    s.edit(sk, window=(0, 0, 16, 16))                         # drops one redo entry (small), adds one
    assert s.history_bytes_used == big + small and not s.can_redo


def test_oversize_edit_is_committed_unjournalled_and_clears_the_history():
    s, stub = _session(history=4, history_bytes=serve.window_saved_bytes(32, 32) + serve.window_saved_bytes(16, 16))
    sk = _sketch((500, 900, 560, 1000))
    s.edit(sk, window=(0, 0, 32, 32))
    s.edit(sk, window=(8, 8, 16, 16))
    s.undo()
    assert s.can_undo and s.can_redo
    n_saves = [c[0] for c in stub.calls].count("save")
    before = s.frame()
    _, _, info = s.edit(sk, window=(0, 0, 64, 64))
    assert info["undoable"] is False and not np.array_equal(s.frame(), before)          # committed all the same
    assert not s.can_undo and not s.can_redo and s.history_bytes_used == 0
    assert [c[0] for c in stub.calls].count("save") == n_saves                           # and nothing was saved for it
    with pytest.raises(ValueError):
        serve.EditSession(None, np.zeros(HW + (3,), np.uint8), backend=stub, history=-1)


def test_grow_loop_journals_the_committed_window_only():
    hit = [0, 3, 0, 0]
    box = (500, 900, 560, 1000)
    wins = [serve.choose_window(box, HW, margin=m) for m in (0.5, 1.0, 2.0)]
    # grows to the last allowed rerun, which commits in its run: the save is in front of that run
    s, stub = _session([hit] * 10, history=4)
    f0 = s.frame()
    _, _, info = s.edit(_sketch(box), max_grow=2)
    assert stub.calls == [("run", [wins[0]], False), ("run", [wins[1]], False), ("save", [wins[2]]), ("run", [wins[2]], True)]
    assert info["window"] == wins[2] and info["undoable"] is True
    assert s.undo()[2]["window"] == wins[2] and np.array_equal(s.frame(), f0)
    # the hits stop after one rerun: that run was not committed, the save is in front of the paste
    s, stub = _session([hit, [0, 0, 0, 0]], history=4)
    s.edit(_sketch(box), max_grow=5)
    assert stub.calls == [("run", [wins[0]], False), ("run", [wins[1]], False), ("save", [wins[1]]), ("paste", [wins[1]])]
    assert s.history_bytes_used == serve.window_saved_bytes(*wins[1][2:])
    s.undo()
    assert not s.frame().any()


def test_history_0_makes_no_journal_call():
    class _NoJournal(_Stub):
        save = swap = None                                    # calling either raises TypeError

    stub = _NoJournal([[0, 3, 0, 0], [0, 0, 0, 0]])
    s = serve.EditSession(None, np.zeros(HW + (3,), np.uint8), backend=stub)
    _, _, info = s.edit(_sketch((500, 900, 560, 1000)), max_grow=5)
    assert sorted(info) == ["counts", "margin", "reruns", "window"] and [c[0] for c in stub.calls] == ["run", "run", "paste"]
    assert s.history == 0 and not s.can_undo and s.history_bytes_used == 0
    with pytest.raises(IndexError):
        s.undo()


def test_server_orders_undo_like_an_edit_and_saves_once_per_group():
    stub = _Stub()
    srv = serve.BatchingServer(object(), max_batch=4, max_wait_s=0.05, window=True, max_grow=0)
    s = serve.EditSession(srv.model, np.zeros(HW + (3,), np.uint8), backend=stub, history=4)
    s2 = serve.EditSession(srv.model, np.zeros((601, 803, 3), np.uint8), backend=stub)       # no history: never saved
    sk1, sk2 = _sketch((500, 900, 560, 1000)), _sketch((100, 200, 160, 300))
    f0 = s.frame()
    outs = {}
    t = threading.Thread(target=lambda: outs.update(a=srv.submit(s, sk1)))
    t.start()
    while not srv._queue and not stub.calls:
        time.sleep(0.001)
    outs["b"] = srv.submit(s, sk2)                            # the first edit is queued (or running) before the second arrives
    t.join()
    f2 = s.frame()
    assert outs["a"][2]["undoable"] is True and outs["b"][2]["undoable"] is True
    patch, _, info = srv.undo(s)                              # after two edits: undoes the second
    assert info["window"] == outs["b"][2]["window"] and info["undo_depth"] == 1
    srv.undo(s)
    assert np.array_equal(s.frame(), f0)
    with pytest.raises(IndexError):
        srv.undo(s)
    srv.redo(s)
    srv.redo(s)
    assert np.array_equal(s.frame(), f2)
    # two sessions in one group, one journalled: ONE save, of that request only
    stub.calls.clear()
    sk_small = _sketch((300, 400, 360, 500), (601, 803))
    ts = [threading.Thread(target=srv.submit, args=(s, sk1)), threading.Thread(target=srv.submit, args=(s2, sk_small))]
    for x in ts:
        x.start()
    for x in ts:
        x.join()
    srv.close()
    saves = [c for c in stub.calls if c[0] == "save"]
    runs = [c for c in stub.calls if c[0] == "run"]
    assert sum(len(c[1]) for c in saves) == 1 and len(saves) == 1
    if len(runs) == 1:                                        # the two shared a group: the save precedes the committing run
        assert stub.calls.index(saves[0]) < stub.calls.index(runs[0])
    with pytest.raises(ValueError):
        serve.BatchingServer(object(), window=False).undo(s)


def test_saved_bytes_through_the_library():
    _lib.build_library()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.se_window_saved_bytes.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.se_window_saved_bytes.restype = ctypes.c_size_t
    for hs in (16, 17, 64, 1080, 4099):
        for ws in list(range(16, 48)) + [511, 512, 513, 1920, 1921]:          # ws = 0 ... 15 mod 16, twice over
            want = hs * -(-3 * ws // 16) * 16
            assert lib.se_window_saved_bytes(hs, ws) == want == serve.window_saved_bytes(hs, ws), (hs, ws)
    assert {(3 * ws) % 16 for ws in range(16, 48)} == set(range(16)) and {ws % 16 for ws in range(16, 48)} == set(range(16))
    for hs, ws in ((15, 64), (64, 15), (0, 0), (-1, 64), (64, -16), (15, 15)):
        assert lib.se_window_saved_bytes(hs, ws) == 0 == serve.window_saved_bytes(hs, ws), (hs, ws)
    assert lib.se_window_saved_bytes(1080, 1920) == 1080 * 5760          # the 6.2 MB slot of the whole 1080p window
