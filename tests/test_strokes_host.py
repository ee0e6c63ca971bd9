"""Host-side logic of the stroke edits, no GPU: the integer rule's numpy statement on literals, the host
functions `serve.stroke_segments` / `serve.stroke_box`, and `serve.EditSession.edit_strokes` with its journal against a
scripted stand-in for the device side, in the style of tests/test_regions_host.py."""
import os
import re

import numpy as np
import pytest

from sketchedit_amd import _lib, serve
from strokes_util import spec_cover, spec_raster

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HW = (80, 280)
POLICY = dict(min_side=64, bucket=8)


def _pixels(a):
    return sorted((int(y), int(x)) for y, x in zip(*np.nonzero(a)))


# ---- the rule itself, on literals ---------------------------------------------------------------------------------------------
def test_a_dot_at_a_frame_corner():
    # the corner point (0, 0) at r = 3: the centre of pixel (0, 0) is (2, 2), 8 <= 9; (0, 1) is (6, 2), 40 > 9
    assert _pixels(spec_raster([[0, 0, 0, 0, 3]], (8, 8))) == [(0, 0)]
    assert _pixels(spec_raster([[32, 32, 32, 32, 3]], (8, 8))) == [(7, 7)]          # the opposite corner (4 Wi, 4 Hi)
    assert _pixels(spec_raster([[0, 32, 0, 32, 3]], (8, 8))) == [(7, 0)]
    # r = 2 would miss every centre there (8 > 4): why 3 is the smallest radius
    assert not spec_raster([[0, 0, 0, 0, 2]], (8, 8)).any()


def test_the_smallest_radius_covers_a_centre_wherever_the_dot_is():
    for ax in range(0, 33):
        for ay in range(0, 33):
            assert spec_raster([[ax, ay, ax, ay, 3]], (8, 8)).any(), (ax, ay)
    # a dot on a pixel centre at r = 3: that pixel only (the next centre is 4 away)
    assert _pixels(spec_raster([[14, 10, 14, 10, 3]], (8, 8))) == [(2, 3)]
    # r = 4 reaches the four neighbours' centres exactly (16 <= 16), not the diagonal ones (32 > 16)
    assert _pixels(spec_raster([[14, 10, 14, 10, 4]], (8, 8))) == [(1, 3), (2, 2), (2, 3), (2, 4), (3, 3)]


def test_horizontal_vertical_and_diagonal_segments():
    # horizontal, along the centres of row 2 from pixel 1 to pixel 5, r = 3: the row's pixels 1..5 (pixel 0's centre is 4 in
    # front of A: 16 > 9) and nothing of rows 1 and 3 (their centres are 4 off the line)
    assert _pixels(spec_raster([[6, 10, 22, 10, 3]], (6, 8))) == [(2, x) for x in range(1, 6)]
    # the same at r = 4: rows 1 and 3 join (cr^2 = 16 dd), and the caps reach pixels 0 and 6 of row 2
    assert _pixels(spec_raster([[6, 10, 22, 10, 4]], (6, 8))) == sorted([(2, x) for x in range(0, 7)] + [(y, x) for y in (1, 3) for x in range(1, 6)])
    # vertical: the transpose
    assert _pixels(spec_raster([[10, 6, 10, 22, 3]], (8, 6))) == [(y, 2) for y in range(1, 6)]
    # 45 degrees through the centres of (1, 1) .. (4, 4), r = 3: the diagonal; (1, 2) is 2 sqrt 2 quarter pixels off the
    # line -- cr = 16 (ex = 4, ey = 0, d = (12, 12)), cr^2 = 256 <= 9 * 288 -- so the off-diagonal neighbours are covered too
    got = spec_raster([[6, 6, 18, 18, 3]], (6, 6))
    assert _pixels(got) == sorted([(i, i) for i in range(1, 5)] + [(i, i + 1) for i in range(1, 4)] + [(i + 1, i) for i in range(1, 4)])
    assert np.array_equal(got, got.T)
    # the direction of a segment does not matter
    assert np.array_equal(got, spec_raster([[18, 18, 6, 6, 3]], (6, 6)))


def test_the_three_cases_in_their_order():
    seg = [8, 8, 24, 8, 5]
    # behind A (t <= 0): the distance to A decides; (1, 0) has e = (-6, -2): 40 > 25, although it is within r of the LINE
    assert not spec_cover(seg, [1], [0])[0, 0] and spec_cover(seg, [1], [1])[0, 0]
    # past B (t >= dd): the distance to B; beside the segment: the distance to the line
    assert spec_cover(seg, [1], [6])[0, 0] and not spec_cover(seg, [1], [7])[0, 0]
    assert spec_cover(seg, [2], [3])[0, 0] and not spec_cover(seg, [3], [3])[0, 0]       # 2 and 6 off the line
    # a dot has dd = 0: t = 0 <= 0 for every pixel, the first case always
    assert spec_cover([8, 8, 8, 8, 5], [1], [1])[0, 0]


def test_the_largest_intermediates_fit_int64():
    # corner to corner of an 8192 x 8192 frame at r = 512: cr^2 at the far corners is the largest value of the rule
    seg = np.array([0, 0, 4 * 8192, 4 * 8192, 512], np.int64)
    ex, ey = np.int64(4 * 8191 + 2), np.int64(2)
    cr = ex * seg[3] - ey * seg[2]
    assert float(cr) ** 2 < 2.0 ** 62 and int(cr) ** 2 == int(cr * cr)              # no wrap in int64
    # beside the diagonal cr = 32768 * 4 (x - y) and dd = 2 * 32768^2, so the rule is 16 (x - y)^2 <= 2 * 512^2: |x - y| <= 181
    got = spec_raster([seg], (8192, 8192), (4000, 4173, 16, 16))
    want = np.abs(np.subtract.outer(np.arange(4000, 4016), np.arange(4173, 4189))) <= 181
    assert np.array_equal(got > 0, want) and got.any() and not got.all()
    assert not spec_raster([seg], (8192, 8192), (0, 8176, 16, 16)).any()              # the other corner: far from the diagonal


# ---- stroke_segments ----------------------------------------------------------------------------------------------------------
def test_segments_of_strokes():
    segs, ranges = serve.stroke_segments([([(1.5, 2.5), (5.5, 2.5), (5.5, 7.26)], 1.5), ([(10.1, 3.13)], 2.0)], HW)
    assert segs.dtype == np.int32 and segs.tolist() == [[6, 10, 22, 10, 3], [22, 10, 22, 29, 3], [40, 13, 40, 13, 4]]
    assert ranges == [(0, 2), (2, 1)]                                               # n points: n - 1 segments; one point: a dot
    # rounding is half up, at both signs of the fraction
    assert serve.stroke_segments([([(0.125, 0.375)], 2)], HW)[0].tolist() == [[1, 2, 1, 2, 4]]
    # r = round(2 width): 1.5 pixels is the thinnest brush, 256 the widest
    assert serve.stroke_segments([([(1, 1)], 256)], HW)[0][0, 4] == 512


def test_a_segment_is_clamped_at_the_frame_edge():
    segs, _ = serve.stroke_segments([([(-7.0, 10.0), (300.0, 90.0)], 2)], HW)
    assert segs.tolist() == [[0, 40, 4 * 280, 4 * 80, 4]]                           # [0, 4 Wi] x [0, 4 Hi], ends included
    segs, _ = serve.stroke_segments([([(279.9, -3.0), (279.9, 5.0)], 1.5)], HW)
    assert segs.tolist() == [[1120, 0, 1120, 20, 3]]
    # along the right edge at r = 3: the last column, rows 0 .. 5 (row 5's centre is 2 past B: 8 <= 9)
    assert _pixels(spec_raster(segs, HW)) == [(y, 279) for y in range(0, 6)]
    assert serve.stroke_box(segs, HW) == (0, 279, 6, 280)


def test_segment_refusals():
    ok = [([(5, 5), (9, 9)], 2)]
    serve.stroke_segments(ok, HW)
    for bad in ([], [([], 2)], [([(5, 5)], 1.2)], [([(5, 5)], 256.3)], [([(5, 5)], 0)], [([(5, 5)], -3)], [([(5, float("nan"))], 2)],
                [([(5, 5)], float("inf"))], [([(5, 5, 5)], 2)], [([5, 5], 2)]):
        with pytest.raises(ValueError):
            serve.stroke_segments(bad, HW)
    with pytest.raises(ValueError, match="8192"):
        serve.stroke_segments(ok, (8193, 64))
    serve.stroke_segments(ok, (8192, 8192))
    assert serve.stroke_segments([([(5, 5)], 1.25)], HW)[0][0, 4] == 3              # 2.5 rounds half up


# ---- stroke_box ---------------------------------------------------------------------------------------------------------------
def test_box_literals():
    assert serve.stroke_box([[0, 0, 0, 0, 3]], (8, 8)) == (0, 0, 1, 1)
    assert serve.stroke_box([[32, 32, 32, 32, 3]], (8, 8)) == (7, 7, 8, 8)
    assert serve.stroke_box([[6, 10, 22, 10, 3]], (6, 8)) == (2, 1, 3, 6)          # tight on the horizontal literal above
    assert serve.stroke_box([[6, 10, 22, 10, 4]], (6, 8)) == (1, 0, 4, 7)
    assert serve.stroke_box([[6, 10, 22, 10, 3], [22, 10, 22, 29, 3]], HW) == (2, 1, 8, 6)
    with pytest.raises(ValueError):
        serve.stroke_box(np.zeros((0, 5), np.int32), HW)


def test_box_contains_the_rule_s_pixels_over_random_segments():
    rng = np.random.RandomState(17)
    for k in range(300):
        hw = (int(rng.randint(16, 120)), int(rng.randint(16, 160)))
        n = rng.randint(1, 4)
        r = int(rng.choice([3, 4, 5, 9, 40, 512])) if k % 3 else int(rng.randint(3, 513))
        segs = np.stack([rng.randint(0, 4 * hw[1] + 1, n), rng.randint(0, 4 * hw[0] + 1, n), rng.randint(0, 4 * hw[1] + 1, n),
                         rng.randint(0, 4 * hw[0] + 1, n), np.full(n, r)], 1)
        if k % 5 == 0:
            segs[:, 2:4] = segs[:, 0:2]                                             # dots
        if k % 7 == 0:
            segs[0, :4] = [0, 0, 4 * hw[1], 4 * hw[0]][::(1 if k % 2 else -1)] if n else 0      # ends on the rectangle's corners
        y0, x0, y1, x1 = serve.stroke_box(segs, hw)
        assert 0 <= y0 < y1 <= hw[0] and 0 <= x0 < x1 <= hw[1]                      # never empty, inside the frame
        full = spec_raster(segs, hw)
        assert full[y0:y1, x0:x1].any()
        full[y0:y1, x0:x1] = 0
        assert not full.any(), (hw, segs.tolist())


# ---- EditSession.edit_strokes against a scripted backend --------------------------------------------------------------------
class _Stub:
    """Frames are numpy arrays; a committing run writes a new value (1, 2, 3, ...) over each of its windows where the
    window's sketch is drawn; a slot is the crop's copy; the rasteriser call is the numpy rule."""

    def __init__(self):
        self.calls, self.value, self.uploads = [], 0, []

    def upload(self, a):
        self.uploads.append(tuple(a.shape))
        return np.array(a)

    def strokes(self, segs, frame_hw, windows):
        assert segs.dtype == np.int32 and len({w[2:] for w in windows}) == 1
        self.calls.append(("strokes", len(segs), tuple(frame_hw), list(windows)))
        return [spec_raster(segs, frame_hw, w) for w in windows]

    def tiles(self, sketch, tile):
        raise AssertionError("a stroke edit runs no tile pass")

    def window_of(self, plane, y0, x0, h, w):
        raise AssertionError("a stroke edit has no full-size plane to crop")

    def _run(self, name, frames, origins, sketches, hw, work, commit, low_latency, locks=None):
        h, w = hw
        assert len(frames) == len(origins) == len(sketches) and all(s.shape == (h, w) and s.dtype == np.uint8 for s in sketches)
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


# the strokes of tests/test_regions_host.py's THREE, as polylines: a short diagonal near the top left, one near the bottom right,
# a long flat one between them; and two crossing strokes whose windows would intersect
S1 = ([(10.5, 10.5), (19.5, 19.5)], 2.0)
S2 = ([(250.5, 50.5), (259.5, 59.5)], 2.0)
S3 = ([(90.5, 32.5), (110.0, 31.0), (129.5, 32.5)], 1.5)
CROSS = [([(10.5, 10.5), (79.5, 19.5)], 2.0), ([(10.5, 19.5), (79.5, 10.5)], 2.0)]


WINS = [(0, 0, 64, 64), (0, 70, 64, 80), (16, 216, 64, 64)]       # serve.choose_window of the three boxes


def _windows(strokes):
    segs, ranges = serve.stroke_segments(strokes, HW)
    return serve.merge_regions([serve.stroke_box(segs[f:f + n], HW) for f, n in ranges], HW, **POLICY)


def test_one_rasteriser_call_and_one_backend_call_per_size_group():
    s, stub = _session()
    regions = _windows([S1, S2, S3])
    wins = [w for _, w in regions]
    assert [b for b, _ in regions] == [(9, 9, 21, 21), (30, 90, 33, 130), (49, 249, 61, 261)]
    assert wins == WINS
    patches, origins, info = s.edit_strokes([S1, S2, S3], low_latency=False, **POLICY)
    groups = serve._by_size(wins)
    assert stub.uploads == [HW + (3,), (4, 5)]                                      # the frame once; then the segments, nothing else
    want = []
    for hw, idx in groups.items():
        want += [("strokes", 4, HW, [wins[i] for i in idx]), ("run", [wins[i] for i in idx], True, False, None)]
    assert stub.calls == want and len(want) == 4
    assert info["windows"] == wins and info["boxes"] == [b for b, _ in regions] and info["groups"] == 2 and "undoable" not in info
    assert origins == [(w[1], w[0]) for w in wins] and [p.shape for p in patches] == [(w[2], w[3], 3) for w in wins]
    f = s.frame()
    assert all(np.array_equal(p, f[y0:y0 + p.shape[0], x0:x0 + p.shape[1]]) for p, (x0, y0) in zip(patches, origins))
    # the frame changed exactly where the rule draws the request's segments
    segs, _ = serve.stroke_segments([S1, S2, S3], HW)
    assert np.array_equal(f[..., 0] > 0, spec_raster(segs, HW) > 0) and f[15, 15, 0] > 0 and f[55, 255, 0] > 0 and f[31, 100, 0] > 0


def test_two_crossing_strokes_become_one_window():
    s, stub = _session()
    _, _, info = s.edit_strokes(CROSS, **POLICY)
    assert len(info["windows"]) == 1 and info["groups"] == 1 and info["boxes"] == [(9, 9, 21, 81)]
    assert info["windows"] == [serve.choose_window((9, 9, 21, 81), HW, **POLICY)]
    assert [c[0] for c in stub.calls] == ["strokes", "run"] and stub.calls[0][3] == info["windows"]
    # and two far strokes of one size: ONE rasteriser call and ONE run with B = 2
    s, stub = _session()
    _, _, info = s.edit_strokes([S1, S2], **POLICY)
    assert [c[0] for c in stub.calls] == ["strokes", "run"] and len(stub.calls[1][1]) == 2 and info["groups"] == 1


def test_routing_to_the_scaled_and_locked_entries():
    wins = [w for _, w in _windows([S1, S2, S3])]
    by = list(serve._by_size(wins).items())
    s, stub = _session()
    _, _, info = s.edit_strokes([S1, S2, S3], max_side=32, **POLICY)
    runs = [c for c in stub.calls if c[0] != "strokes"]
    assert runs == [("run_scaled", [wins[i] for i in idx], True, None, serve.choose_working_size(hw, 32)) for hw, idx in by]
    assert info["work"] == [serve.choose_working_size(w[2:], 32) for w in wins] and "locked" not in info
    lock = np.zeros(HW, np.uint8)
    lock[12:30, 0:15] = 1
    for max_side in (None, 32):
        s, stub = _session()
        s.set_lock(lock)
        _, _, info = s.edit_strokes([S1, S2, S3], max_side=max_side, **POLICY)
        runs = [c for c in stub.calls if c[0] != "strokes"]
        assert runs == [("run_locked", [wins[i] for i in idx], True, None, None if max_side is None else serve.choose_working_size(hw, 32))
                        for hw, idx in by]
        assert info["locked"] is True and ("work" in info) == (max_side is not None)
        assert not s.frame()[12:30, 0:15].any() and s.frame()[16, 16].all()


def test_one_journal_entry_per_call_and_one_undo_step():
    s, stub = _session(history=4)
    f0 = s.frame()
    wins = [w for _, w in _windows([S1, S2, S3])]
    _, _, info = s.edit_strokes([S1, S2, S3], **POLICY)
    assert info["undoable"] is True
    assert [c[0] for c in stub.calls] == ["strokes", "save", "run", "strokes", "save", "run"]      # a save in front of each commit
    f1 = s.frame()
    assert len(s._undo) == 1 and len(s._undo[0][1]) == 3
    assert s.history_bytes_used == sum(serve.window_saved_bytes(w[2], w[3]) for w in wins)
    patches, origins, uinfo = s.undo()
    assert np.array_equal(s.frame(), f0) and not s.can_undo and s.can_redo
    assert uinfo == dict(windows=wins, undo_depth=0, redo_depth=1) and len(patches) == 3
    s.redo()
    assert np.array_equal(s.frame(), f1)
    # the history_bytes rule of a region edit: all slots of the call together
    one = serve.window_saved_bytes(64, 64)
    s, stub = _session(history=4, history_bytes=2 * one - 1)
    _, _, info = s.edit_strokes([S1, S2], **POLICY)
    assert info["undoable"] is False and not s.can_undo and not any(c[0] == "save" for c in stub.calls)
    s, stub = _session(history=4, history_bytes=2 * one)
    _, _, info = s.edit_strokes([S1, S2], **POLICY)
    assert info["undoable"] is True and s.history_bytes_used == 2 * one


def test_edit_strokes_refusals():
    s, stub = _session(history=2)
    with pytest.raises(ValueError, match="no strokes"):
        s.edit_strokes([], **POLICY)
    with pytest.raises(ValueError):
        s.edit_strokes([([(5, 5)], 0.2)], **POLICY)
    with pytest.raises(ValueError):
        s.edit_strokes([S1], min_side=64, bucket=12)
    assert not stub.calls and stub.uploads == [HW + (3,)] and not s.frame().any() and not s.can_undo


def test_edit_regions_still_takes_its_own_path():
    # the shared helper left edit_regions' calls as they were: upload of the plane, the tile pass, crops of the plane
    from sketch_tiles_util import sketch_tiles

    class _Both(_Stub):
        def tiles(self, sketch, tile):
            self.calls.append(("tiles", tuple(sketch.shape), tile))
            return sketch_tiles(sketch, tile)

        def window_of(self, plane, y0, x0, h, w):
            return plane[y0:y0 + h, x0:x0 + w].copy()

    stub = _Both()
    s = serve.EditSession(None, np.zeros(HW + (3,), np.uint8), backend=stub)
    sk = np.zeros(HW, np.uint8)
    sk[10:20, 10:20] = sk[50:60, 250:260] = 255
    s.edit_regions(sk, tile=16, **POLICY)
    assert stub.uploads == [HW + (3,), HW]
    assert stub.calls == [("tiles", HW, 16), ("run", [(0, 0, 64, 64), (16, 216, 64, 64)], True, None, None)]


# ---- ABI --------------------------------------------------------------------------------------------------------------------
def test_symbol_declared():
    hdr = open(os.path.join(ROOT, "include", "sketchedit_hip.h")).read()
    assert re.search(r"int se_sketch_strokes_u8\(se_ctx\* ctx, void\* stream, const se_window\* wins, int B, int hs, int ws, "
                     r"const int\* segs, int N,\s+const int\* ranges, unsigned char\* sketch_out\);", hdr)
    assert "se_sketch_strokes_u8" in _lib.abi_names("sketchedit_hip.h")
