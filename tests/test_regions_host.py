"""Host-side logic of the region edits, no GPU: the numpy restatement of the tile records, the window policy
`serve.split_regions` (components, the merge rule, its literals), and `serve.EditSession.edit_regions` with its journal
against a scripted stand-in for the device side, in the style of tests/test_window_host.py."""
import os
import re

import numpy as np
import pytest

from sketchedit_amd import _lib, serve
from sketch_tiles_util import sketch_tiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HW = (80, 280)
POLICY = dict(min_side=64, bucket=8)
TWO = [(10, 20, 10, 20), (50, 60, 250, 260)]                  # strokes as (y0, y1, x0, x1)
THREE = TWO + [(30, 34, 90, 130)]
MERGE = [(10, 20, 10, 20), (10, 20, 70, 80)]


def _sketch(strokes, hw=HW):
    sk = np.zeros(hw, np.uint8)
    for y0, y1, x0, x1 in strokes:
        sk[y0:y1, x0:x1] = 255
    return sk


def _split(sk, tile=16, **kw):
    return serve.split_regions(sketch_tiles(sk, tile), tile, sk.shape, **(kw or POLICY))


# ---- the oracle itself ------------------------------------------------------------------------------------------------------
def test_tile_records_restated():
    sk = np.zeros((45, 67), np.uint8)
    assert not sketch_tiles(sk, 16).any() and sketch_tiles(sk, 16).shape == (3, 5, 5) and sketch_tiles(sk, 64).shape == (1, 2, 5)
    sk[15:17, 31:33] = 7                                      # one pixel in each of four tiles
    sk[44, 66] = 1                                            # the last pixel of the ragged last tile
    t = sketch_tiles(sk, 16)
    assert t.dtype == np.int32 and t[..., 0].sum() == 5
    assert t[0, 1].tolist() == [1, 15, 31, 16, 32] and t[0, 2].tolist() == [1, 15, 32, 16, 33]
    assert t[1, 1].tolist() == [1, 16, 31, 17, 32] and t[1, 2].tolist() == [1, 16, 32, 17, 33]
    assert t[2, 4].tolist() == [1, 44, 66, 45, 67]
    assert sketch_tiles(sk, 64)[0, 0].tolist() == [4, 15, 31, 17, 33] and sketch_tiles(sk, 64)[0, 1].tolist() == [1, 44, 66, 45, 67]
    full = np.full((45, 67), 255, np.uint8)
    assert sketch_tiles(full, 32)[1, 2].tolist() == [13 * 3, 32, 64, 45, 67]


# ---- split_regions ----------------------------------------------------------------------------------------------------------
def test_split_empty_and_single_blob():
    assert _split(np.zeros(HW, np.uint8)) == []
    assert serve.split_regions(np.zeros((34, 61, 5), np.int32), 32, (1081, 1921)) == []
    rng = np.random.RandomState(3)
    for hw in ((1081, 1921), (301, 333), HW):
        for tile in (16, 32, 64):
            y0, x0 = rng.randint(0, hw[0] - 40), rng.randint(0, hw[1] - 40)
            sk = np.zeros(hw, np.uint8)
            sk[y0:y0 + rng.randint(1, 40), x0:x0 + rng.randint(1, 40)] = 1      # one blob, across tile boundaries or not
            box = serve.sketch_bbox(sk)
            assert _split(sk, tile, margin=0.5, bucket=64, min_side=256) == [(box, serve.choose_window(box, hw))]
    with pytest.raises(ValueError):
        serve.split_regions(np.zeros((3, 3, 5), np.int32), 32, (1081, 1921))      # not this frame's grid


def test_split_literals():
    assert _split(_sketch(TWO)) == [((10, 10, 20, 20), (0, 0, 64, 64)), ((50, 250, 60, 260), (16, 216, 64, 64))]
    assert _split(_sketch(THREE)) == [((10, 10, 20, 20), (0, 0, 64, 64)), ((30, 90, 34, 130), (0, 70, 64, 80)),
                                      ((50, 250, 60, 260), (16, 216, 64, 64))]
    # the windows of the two strokes alone, (0, 0, 64, 64) and (0, 43, 64, 64), intersect: one component, the union's window
    sk = _sketch(MERGE)
    assert _split(sk) == [((10, 10, 20, 80), (0, 0, 80, 144))]
    assert _split(sk)[0][1] == serve.choose_window(serve.sketch_bbox(sk), HW, **POLICY)
    # the README's case: two 40-pixel strokes near opposite corners of a 1080p frame, the defaults
    sk = _sketch([(30, 70, 30, 70), (1000, 1040, 1850, 1890)], (1081, 1921))
    assert _split(sk, 32, margin=0.5, bucket=64, min_side=256) == [((30, 30, 70, 70), (0, 0, 256, 256)),
                                                                   ((1000, 1850, 1040, 1890), (825, 1665, 256, 256))]


def test_split_joins_diagonal_tiles():
    sk = np.zeros((1081, 1921), np.uint8)
    sk[31, 31] = sk[32, 32] = 1                               # tiles (0, 0) and (1, 1) at tile 32: 8-connected
    assert [b for b, _ in _split(sk, 32, margin=0.5, bucket=64, min_side=256)] == [(31, 31, 33, 33)]
    # components, not windows, are what connectivity decides: with windows too small to meet, two tiles apart stays two
    sk = np.zeros((200, 200), np.uint8)
    sk[15, 15] = sk[16, 16] = sk[60, 100] = 1
    assert [b for b, _ in _split(sk, 16, margin=0.0, bucket=8, min_side=16)] == [(15, 15, 17, 17), (60, 100, 61, 101)]
    sk[:] = 0
    sk[15, 15] = sk[16, 47] = 1                               # tiles (0, 0) and (1, 2): not neighbours
    assert len(_split(sk, 16, margin=0.0, bucket=8, min_side=16)) == 2


def test_merge_is_independent_of_the_order_of_its_input():
    rng = np.random.RandomState(11)
    merged_some = 0
    for _ in range(40):
        hw = (int(rng.randint(200, 1100)), int(rng.randint(200, 1950)))
        boxes = []
        for _ in range(rng.randint(2, 9)):
            y0, x0 = rng.randint(0, hw[0] - 30), rng.randint(0, hw[1] - 30)
            boxes.append((y0, x0, y0 + rng.randint(1, 30), x0 + rng.randint(1, 30)))
        want = serve.merge_regions(boxes, hw, min_side=128, bucket=64)
        merged_some += len(want) < len(boxes)
        for _ in range(5):
            assert serve.merge_regions([boxes[i] for i in rng.permutation(len(boxes))], hw, min_side=128, bucket=64) == want
        # the same through the grid: the sketch mirrored in y and x gives the mirrored boxes
        sk = np.zeros(hw, np.uint8)
        for y0, x0, y1, x1 in boxes:
            sk[y0:y1, x0:x1] = 1
        a = _split(sk, 32, min_side=128, bucket=64)
        assert a == _split(sk.copy(order="F"), 32, min_side=128, bucket=64)
    assert merged_some > 5


def test_windows_disjoint_and_inside_over_random_sparse_sketches():
    rng = np.random.RandomState(5)
    for k in range(60):
        hw = (int(rng.randint(64, 700)), int(rng.randint(64, 900)))
        tile = (16, 32, 64)[k % 3]
        sk = np.zeros(hw, np.uint8)
        for _ in range(rng.randint(1, 7)):
            y, x = rng.randint(0, hw[0]), rng.randint(0, hw[1])
            sk[y:y + rng.randint(1, 25), x:x + rng.randint(1, 25)] = rng.randint(1, 256)
        regions = _split(sk, tile, margin=0.5, bucket=(8, 64)[k % 2], min_side=(64, 256)[k % 2])
        wins = [w for _, w in regions]
        assert wins == sorted(wins, key=lambda w: w[:2]) and len(wins) >= 1
        covered = np.zeros(hw, bool)
        for (by0, bx0, by1, bx1), (y0, x0, h, w) in regions:
            assert 0 <= y0 and y0 + h <= hw[0] and 0 <= x0 and x0 + w <= hw[1] and h % 8 == 0 and w % 8 == 0
            assert not covered[y0:y0 + h, x0:x0 + w].any(), (hw, tile, wins)            # pairwise disjoint
            covered[y0:y0 + h, x0:x0 + w] = True
            assert (by0, bx0, by1, bx1) == tuple(np.add(serve.sketch_bbox(sk[by0:by1, bx0:bx1]), (by0, bx0, by0, bx0)))      # tight
        # the boxes hold every drawn pixel
        inside = np.zeros(hw, bool)
        for (by0, bx0, by1, bx1), _ in regions:
            inside[by0:by1, bx0:bx1] = True
        assert not (sk[~inside] > 0).any()


# ---- EditSession.edit_regions against a scripted backend -----------------------------------------------------------------
class _Stub:
    """Frames are numpy arrays; a committing run writes a new value (1, 2, 3, ...) over each of its windows; a slot is the
    crop's copy; the tiles call is the numpy oracle."""

    def __init__(self):
        self.calls, self.value, self.uploads = [], 0, []

    def upload(self, a):
        self.uploads.append(tuple(a.shape))
        return np.array(a)

    def tiles(self, sketch, tile):
        self.calls.append(("tiles", tuple(sketch.shape), tile))
        return sketch_tiles(sketch, tile)

    def window_of(self, plane, y0, x0, h, w):
        return plane[y0:y0 + h, x0:x0 + w].copy()

    def _run(self, name, frames, origins, sketches, hw, work, commit, low_latency, locks=None):
        h, w = hw
        assert len(frames) == len(origins) == len(sketches) and all(s.shape == (h, w) for s in sketches)
        self.calls.append((name, [(y0, x0, h, w) for y0, x0 in origins], bool(commit), low_latency, work))
        for f, (y0, x0), s in zip(frames, origins, sketches):
            self.value += 1
            sel = s > 0 if locks is None else (s > 0) & (locks[0][y0:y0 + h, x0:x0 + w] == 0)
            f[y0:y0 + h, x0:x0 + w][sel] = self.value
        n = len(frames)
        return np.zeros((n, h, w, 3), np.uint8), np.full((n, h, w), 255, np.uint8), [[k, 0, 0, y0] for k, (y0, _) in enumerate(origins)]

    def run(self, frames, origins, sketches, h, w, commit, low_latency):
        return self._run("run", frames, origins, sketches, (h, w), None, commit, low_latency)

    def run_scaled(self, frames, origins, sketches, window_hw, work_hw, commit, low_latency):
        return self._run("run_scaled", frames, origins, sketches, window_hw, work_hw, commit, low_latency)

    def run_locked(self, frames, origins, sketches, locks, window_hw, work_hw, commit, low_latency):
        assert len(locks) == len(frames) and all(t is locks[0] for t in locks)
        return self._run("run_locked", frames, origins, sketches, window_hw, work_hw, commit, low_latency, locks)

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

    def crop(self, frame, y0, x0, h, w):
        return frame[y0:y0 + h, x0:x0 + w].copy()

    def download(self, frame):
        return frame.copy()


def _session(**kw):
    stub = _Stub()
    return serve.EditSession(None, np.zeros(HW + (3,), np.uint8), backend=stub, **kw), stub


KW = dict(tile=16, **POLICY)
W1, W2, W3 = (0, 0, 64, 64), (16, 216, 64, 64), (0, 70, 64, 80)


def test_one_backend_call_per_size_group():
    s, stub = _session()
    patches, origins, info = s.edit_regions(_sketch(THREE), low_latency=False, **KW)
    assert stub.uploads == [HW + (3,), HW]                                   # the frame once, the full sketch once
    assert stub.calls == [("tiles", HW, 16), ("run", [W1, W2], True, False, None), ("run", [W3], True, False, None)]
    assert info == dict(windows=[W1, W3, W2], boxes=[(10, 10, 20, 20), (30, 90, 34, 130), (50, 250, 60, 260)],
                        counts=[[0, 0, 0, 0], [0, 0, 0, 0], [1, 0, 0, 16]], groups=2)
    assert origins == [(0, 0), (70, 0), (216, 16)] and [p.shape for p in patches] == [(64, 64, 3), (64, 80, 3), (64, 64, 3)]
    f = s.frame()
    assert all(np.array_equal(p, f[y0:y0 + p.shape[0], x0:x0 + p.shape[1]]) for p, (x0, y0) in zip(patches, origins))
    # each region's sketch was the full sketch cropped to its window: the frame changed exactly where the sketch is drawn
    assert np.array_equal(f[..., 0] > 0, _sketch(THREE) > 0) and f[15, 15, 0] == 1 and f[55, 255, 0] == 2 and f[32, 100, 0] == 3
    # two strokes: ONE call with B = 2; the merge case: one window
    s, stub = _session()
    _, _, info = s.edit_regions(_sketch(TWO), **KW)
    assert stub.calls[1:] == [("run", [W1, W2], True, None, None)] and info["groups"] == 1 and "undoable" not in info
    s, stub = _session()
    _, _, info = s.edit_regions(_sketch(MERGE), **KW)
    assert stub.calls[1:] == [("run", [(0, 0, 80, 144)], True, None, None)] and info["windows"] == [(0, 0, 80, 144)]


def test_a_neighbours_pixels_inside_a_window_are_part_of_its_sketch():
    # a frame so narrow that window 2, pushed inside it, holds the end of stroke 1: (0, 0, 64, 64) and (0, 64, 64, 64)
    hw = (64, 128)
    strokes = [(10, 20, 10, 20), (10, 20, 40, 70), (10, 20, 110, 120)]
    sk = _sketch(strokes[:1] + strokes[2:], hw)
    sk[30, 60:70] = 9                                         # drawn with stroke 1's component? no: a component of its own
    stub = _Stub()
    s = serve.EditSession(None, np.zeros(hw + (3,), np.uint8), backend=stub)
    _, _, info = s.edit_regions(sk, tile=16, margin=0.0, bucket=8, min_side=64)
    wins = info["windows"]
    assert all(not serve._windows_intersect(a, b) for i, a in enumerate(wins) for b in wins[i + 1:])
    # every drawn pixel lies in exactly one window and was part of that window's sketch, whichever component found it
    assert np.array_equal(s.frame()[..., 0] > 0, sk > 0)


def test_routing_to_the_scaled_and_locked_entries():
    s, stub = _session()
    _, _, info = s.edit_regions(_sketch(THREE), max_side=32, **KW)
    assert stub.calls[1:] == [("run_scaled", [W1, W2], True, None, (32, 32)), ("run_scaled", [W3], True, None, (24, 32))]
    assert info["work"] == [(32, 32), (24, 32), (32, 32)] and "locked" not in info
    lock = np.zeros(HW, np.uint8)
    lock[12:30, 0:15] = 1
    for max_side, work in ((None, [None, None]), (32, [(32, 32), (24, 32)])):
        s, stub = _session()
        s.set_lock(lock)
        _, _, info = s.edit_regions(_sketch(THREE), max_side=max_side, **KW)
        assert stub.calls[1:] == [("run_locked", [W1, W2], True, None, work[0]), ("run_locked", [W3], True, None, work[1])]
        assert info["locked"] is True and ("work" in info) == (max_side is not None)
        assert not s.frame()[12:30, 0:15].any() and s.frame()[10:12, 10:20].all()


def test_one_journal_entry_and_one_undo_step():
    s, stub = _session(history=4)
    f0 = s.frame()
    _, _, info = s.edit_regions(_sketch(THREE), **KW)
    assert info["undoable"] is True
    # every window's rectangle is saved in front of its group's commit
    assert [c[:2] for c in stub.calls[1:]] == [("save", [W1, W2]), ("run", [W1, W2]), ("save", [W3]), ("run", [W3])]
    f1 = s.frame()
    slot = lambda w: serve.window_saved_bytes(w[2], w[3])
    assert len(s._undo) == 1 and len(s._undo[0][1]) == 3 and s.history_bytes_used == slot(W1) + slot(W2) + slot(W3)
    del stub.calls[:]
    patches, origins, uinfo = s.undo()
    assert np.array_equal(s.frame(), f0) and not s.can_undo and s.can_redo
    assert stub.calls == [("swap", [W1, W2]), ("swap", [W3])]                # one exchange per window size, all of the entry
    assert uinfo == dict(windows=[W1, W3, W2], undo_depth=0, redo_depth=1) and origins == [(0, 0), (70, 0), (216, 16)]
    assert all(np.array_equal(p, f0[y0:y0 + p.shape[0], x0:x0 + p.shape[1]]) for p, (x0, y0) in zip(patches, origins))
    patches, _, rinfo = s.redo()
    assert np.array_equal(s.frame(), f1) and rinfo == dict(windows=[W1, W3, W2], undo_depth=1, redo_depth=0)
    assert np.array_equal(patches[2], f1[16:80, 216:280])
    # windows of one size: ONE swap call
    s, stub = _session(history=4)
    s.edit_regions(_sketch(TWO), **KW)
    del stub.calls[:]
    s.undo()
    assert stub.calls == [("swap", [W1, W2])]
    # `history` counts edits, single-window entries keep their shape beside region entries
    s, stub = _session(history=2)
    sk = _sketch(TWO)
    frames = [s.frame()]
    s.edit(sk, window=(8, 8, 32, 32))
    frames.append(s.frame())
    s.edit_regions(sk, **KW)
    frames.append(s.frame())
    s.edit_regions(_sketch(THREE), **KW)                      # the third edit: the oldest entry leaves
    assert len(s._undo) == 2
    s.undo()
    assert np.array_equal(s.frame(), frames[2])
    _, _, info = s.undo()
    assert np.array_equal(s.frame(), frames[1]) and "windows" in info and not s.can_undo
    s.redo()
    assert np.array_equal(s.frame(), frames[2])
    s, stub = _session(history=2)
    s.edit(sk, window=(8, 8, 32, 32))
    patch, (x0, y0), info = s.undo()                          # a single-window entry returns what it always did
    assert info == dict(window=(8, 8, 32, 32), undo_depth=0, redo_depth=1) and (x0, y0) == (8, 8) and patch.shape == (32, 32, 3)


def test_history_bytes_counts_all_slots_of_an_entry():
    one = serve.window_saved_bytes(64, 64)
    # the two slots together exceed the cap, each alone would not: unjournalled, and the history is cleared
    s, stub = _session(history=4, history_bytes=2 * one - 1)
    s.edit(_sketch(TWO), window=W1)
    assert s.can_undo
    _, _, info = s.edit_regions(_sketch(TWO), **KW)
    assert info["undoable"] is False and not s.can_undo and not s.can_redo and s.history_bytes_used == 0
    assert not any(c[0] == "save" for c in stub.calls[-2:]) and stub.calls[-1][0] == "run"
    # exactly at the cap: journalled; the older entry leaves to make room
    s, stub = _session(history=4, history_bytes=2 * one)
    s.edit(_sketch(TWO), window=W1)
    _, _, info = s.edit_regions(_sketch(TWO), **KW)
    assert info["undoable"] is True and len(s._undo) == 1 and s.history_bytes_used == 2 * one
    # history = 0: no journal, no save, no key
    s, stub = _session()
    _, _, info = s.edit_regions(_sketch(TWO), **KW)
    assert "undoable" not in info and not any(c[0] == "save" for c in stub.calls)
    with pytest.raises(IndexError):
        s.undo()


def test_server_undo_takes_a_region_entry_back():
    # region edits are not batched by the server, but a session that made one can still be undone through it
    stub = _Stub()
    srv = serve.BatchingServer(object(), max_batch=4, max_wait_s=0.01, window=True, max_grow=0)
    s = serve.EditSession(srv.model, np.zeros(HW + (3,), np.uint8), backend=stub, history=4)
    f0 = s.frame()
    s.edit_regions(_sketch(THREE), **KW)
    f1 = s.frame()
    patches, origins, info = srv.undo(s)
    assert np.array_equal(s.frame(), f0) and info == dict(windows=[W1, W3, W2], undo_depth=0, redo_depth=1) and len(patches) == 3
    srv.redo(s)
    srv.close()
    assert np.array_equal(s.frame(), f1)


def test_refusals():
    s, stub = _session(history=2)
    with pytest.raises(ValueError, match="empty"):
        s.edit_regions(np.zeros(HW, np.uint8), **KW)
    with pytest.raises(ValueError):
        s.edit_regions(np.zeros((80, 272), np.uint8), **KW)
    with pytest.raises(ValueError):
        s.edit_regions(np.zeros(HW, np.float32), **KW)
    with pytest.raises(ValueError):
        s.edit_regions(_sketch(TWO), tile=16, min_side=64, bucket=12)
    assert not any(c[0].startswith("run") or c[0] == "save" for c in stub.calls) and not s.frame().any() and not s.can_undo


# ---- ABI --------------------------------------------------------------------------------------------------------------------
def test_symbol_declared():
    hdr = open(os.path.join(ROOT, "include", "sketchedit_hip.h")).read()
    assert re.search(r"int se_sketch_tiles_u8\(se_ctx\* ctx, void\* stream, const unsigned char\* sketch_u8, int Hi, int Wi, int tile, "
                     r"int\* tiles_out\);", hdr)
    assert "se_sketch_tiles_u8" in _lib.abi_names("sketchedit_hip.h")       # (tests/test_host_cpu.py: they are the header's declarations)
