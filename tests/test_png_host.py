"""Host-side tests of the device PNG encoder, no GPU: the stream's statement (tests/png_stream_util.py) is a valid
zlib stream of the filtered rows and a PNG of the pixels, stays within the bound, and costs what 6j says against the host's fast
writer; the new header's symbols; and `encode=` of the session calls against a scripted stand-in for the device side."""
import ctypes
import glob
import io
import os
import re
import zlib

import numpy as np
import pytest
from PIL import Image

import png_cases
import png_stream_util as U
from sketchedit_amd import _lib, png_worker, serve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the statement's size over png_bytes_fast's, measured on the golden samples' composed crops, and the margin
RATIO_MEASURED = 0.9899
RATIO_MARGIN = 1.02


def _decode(png):
    return np.asarray(Image.open(io.BytesIO(png)).convert("RGB"))


def _check_stream(a):
    stream, filtered = U.png_stream(a)
    assert zlib.decompress(stream) == filtered
    assert len(stream) <= U.png_bound(*a.shape[:2])
    png = serve.png_from_zlib(stream, *a.shape[:2])
    got = Image.open(io.BytesIO(png))
    assert got.mode == "RGB" and np.array_equal(np.asarray(got), a)
    return stream


CASES = png_cases.cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0].split(":")[0] for c in CASES])
def test_the_statement_is_a_zlib_stream_and_a_png(case):
    _, frames, requests, hw = case
    for r in requests:
        _check_stream(png_cases.rectangle(frames, r, hw))


def test_two_hundred_random_small_rectangles():
    rng = np.random.RandomState(17)
    for i in range(200):
        h, w = rng.randint(16, 25, 2)
        kind = i % 4
        if kind == 0:
            a = rng.randint(0, 256, (h, w, 3))
        elif kind == 1:
            a = rng.randint(0, 2, (h, w, 3)) * 255                         # two values: many short runs
        elif kind == 2:
            a = np.repeat(rng.randint(0, 256, (h, 1, 3)), w, axis=1)        # flat rows: SUB
        else:
            a = np.repeat(rng.randint(0, 256, (1, w, 3)), h, axis=0) + np.arange(h)[:, None, None] * (i % 3)     # equal / stepped rows: UP
        _check_stream((a & 255).astype(np.uint8))


def test_what_each_case_is_there_for():
    by = {c[0].split(":")[0].split(",")[0]: c for c in CASES}
    flat = by["64x300 flat colour"][1][0]
    ml = png_cases.match_lengths(flat)
    assert len(ml) == 2 and all(m and min(m) >= 3 and max(m) == 258 for m in ml)
    f = U.filter_rows(flat)
    assert f[0, 0] == 1 and (f[1:, 0] == 2).all()                         # a flat colour: SUB wins a tie, UP the rows of zeros
    runs = png_cases.runs_image()
    f = U.filter_rows(runs)
    assert (f[:, 0] == 1).all()
    toks = [U.tokens(d) for d in U.stripes_of(f)]
    lens = {v for t in toks for k, v in t if k == "m"}
    assert {3, 257, 258}.issubset(lens)                                  # runs of 4, 258, and 259 .. 261 / 517: 258s, then literals
    # the run that ends ON the boundary: stripe 0 ends in a literal 1 and one match of 258; the one that STRADDLES it is cut:
    # stripe 1 starts with the type byte's literal 1 and a match of 100
    assert toks[0][-2:] == [("l", 1), ("m", 258)] and toks[1][:2] == [("l", 1), ("m", 100)]
    for n, want in ((3, []), (4, [3]), (258, [257]), (259, [258]), (260, [258]), (261, [258]), (262, [258, 3]), (517, [258, 258])):
        t = U.tokens(bytes([7]) * n + bytes([8]))
        assert [v for k, v in t if k == "m"] == want and sum(v if k == "m" else 1 for k, v in t) == n + 1
    ladder = png_cases.ladder_image()
    (d,) = U.stripes_of(U.filter_rows(ladder))
    cnt = U.counts_of(U.tokens(d))
    assert not png_cases.match_lengths(ladder)[0]
    assert max(U.tree_lengths(cnt)) == 16 and max(U.code_lengths(cnt)) <= 15   # the first tree is too deep, the halved one is not


def test_the_bound_on_uniform_random_bytes():
    rng = np.random.RandomState(23)
    for h, w in ((16, 16), (32, 40), (33, 64), (70, 30)):
        a = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        stream, filtered = U.png_stream(a)
        assert len(filtered) < len(stream) <= U.png_bound(h, w)           # noise does not compress, and still fits
    assert U.png_bound(16, 16) == 2 + U.stripe_bound(16 * 49) + 9 == 2 + 159 + 1470 + 9
    assert U.png_bound(33, 17) == 2 + U.stripe_bound(32 * 52) + U.stripe_bound(52) + 9
    assert U.HEADER_BITS == 1222


def test_size_against_the_fast_writer():
    """the statement's stream against zlib level 1 / Z_RLE on SUB rows (png_bytes_fast, the parent's writer), IDAT payloads, summed
    over the golden samples' composed crops quantised as test.py does"""
    ours = fast = n = 0
    for p in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "sample_*.npz"))):
        crops = np.load(p)["composed_crops"]
        for c in crops[:, 0]:
            a = np.ascontiguousarray(((c + 1) / 2 * 255).astype(np.uint8).transpose(1, 2, 0))
            ours += len(_check_stream(a))
            fast += len(png_worker.png_bytes_fast(a)) - (len(serve.png_from_zlib(b"", 64, 64)))
            n += 1
    ratio = ours / fast
    print("png size ratio over %d crops: %d / %d = %.4f" % (n, ours, fast, ratio))
    assert n == 28 and ratio <= RATIO_MEASURED * RATIO_MARGIN


def test_png_from_zlib_is_the_fast_writer_s_framing():
    a = np.random.RandomState(1).randint(0, 256, (16, 20, 3)).astype(np.uint8)
    fast = png_worker.png_bytes_fast(a)
    f = np.full((16, 61), 1, np.uint8)
    f[:, 1:4] = a.reshape(16, 60)[:, :3]
    f[:, 4:] = a.reshape(16, 60)[:, 3:] - a.reshape(16, 60)[:, :-3]
    z = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    assert serve.png_from_zlib(z.compress(f.tobytes()) + z.flush(), 16, 20) == fast


def test_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "sketchedit_png.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(se_[a-z_A-Z0-9]+)\s*\(", hdr))
    own = _lib.abi_names("sketchedit_png.h")
    assert declared == set(own) and len(own) == 3 and "se_png.hip" in _lib.SOURCES
    _lib.build_library()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in own:
        assert getattr(lib, s) is not None
    lib.se_png_bound.restype = ctypes.c_size_t
    for hw in ((16, 16), (33, 17), (64, 300), (512, 512), (8192, 8192), (1080, 1920)):
        assert lib.se_png_bound(*hw) == U.png_bound(*hw)
    assert [lib.se_png_bound(*hw) for hw in ((15, 16), (16, 15), (8193, 16), (16, 8193))] == [0] * 4


# ---- encode= of the session calls against a scripted backend ----------------------------------------------------------------------
HW = (80, 280)
POLICY = dict(min_side=64, bucket=8)
STROKES = [([(10.5, 10.5), (19.5, 19.5)], 2.0), ([(250.5, 50.5), (259.5, 59.5)], 2.0)]


class _Stub:
    """Frames are numpy arrays; a run paints its windows; every call is logged.  crop_png is the statement."""

    def __init__(self):
        self.calls, self.value = [], 0

    def upload(self, a):
        self.calls.append(("upload", tuple(a.shape)))
        return np.array(a)

    def strokes(self, segs, frame_hw, windows):
        self.calls.append(("strokes", list(windows)))
        return [np.full(w[2:], 255, np.uint8) for w in windows]

    def tiles(self, sketch, tile):
        self.calls.append(("tiles", tile))
        return _tiles(sketch, tile)

    def window_of(self, plane, y0, x0, h, w):
        self.calls.append(("window_of", (y0, x0, h, w)))
        return plane[y0:y0 + h, x0:x0 + w].copy()

    def _run(self, name, frames, origins, sketches, hw, work, commit, low_latency):
        h, w = hw
        self.calls.append((name, [(y0, x0, h, w) for y0, x0 in origins], bool(commit), low_latency, work))
        for f, (y0, x0), s in zip(frames, origins, sketches):
            self.value += 1
            f[y0:y0 + h, x0:x0 + w][s > 0] = self.value
        n = len(frames)
        return np.zeros((n, h, w, 3), np.uint8), np.full((n, h, w), 255, np.uint8), [[0, 0, 0, 0]] * n

    def run(self, frames, origins, sketches, h, w, commit, low_latency):
        return self._run("run", frames, origins, sketches, (h, w), None, commit, low_latency)

    def run_scaled(self, frames, origins, sketches, window_hw, work_hw, commit, low_latency):
        return self._run("run_scaled", frames, origins, sketches, window_hw, work_hw, commit, low_latency)

    def save(self, frames, origins, window_hw):
        h, w = window_hw
        self.calls.append(("save", [(y0, x0, h, w) for y0, x0 in origins]))
        return [f[y0:y0 + h, x0:x0 + w].copy() for f, (y0, x0) in zip(frames, origins)]

    def crop(self, frame, y0, x0, h, w):
        self.calls.append(("crop", (y0, x0, h, w)))
        return frame[y0:y0 + h, x0:x0 + w].copy()

    def crop_png(self, frames, windows):
        self.calls.append(("crop_png", list(windows)))
        return [serve.png_from_zlib(U.png_stream(np.ascontiguousarray(f[y0:y0 + h, x0:x0 + w]))[0], h, w)
                for f, (y0, x0, h, w) in zip(frames, windows)]

    def download(self, frame):
        self.calls.append(("download",))
        return frame.copy()


def _tiles(sketch, tile):
    """the tile records of se_sketch_tiles_u8, in numpy"""
    Hi, Wi = sketch.shape
    out = np.zeros((-(-Hi // tile), -(-Wi // tile), 5), np.int32)
    for ty in range(out.shape[0]):
        for tx in range(out.shape[1]):
            ys, xs = np.nonzero(sketch[ty * tile:(ty + 1) * tile, tx * tile:(tx + 1) * tile])
            if len(ys):
                out[ty, tx] = [len(ys), ty * tile + ys.min(), tx * tile + xs.min(), ty * tile + ys.max() + 1, tx * tile + xs.max() + 1]
    return out


def _session(**kw):
    stub = _Stub()
    return serve.EditSession(None, np.zeros(HW + (3,), np.uint8), backend=stub, **kw), stub


def _sketch():
    sk = np.zeros(HW, np.uint8)
    sk[10:20, 10:20] = 255
    sk[50:60, 250:260] = 255
    return sk


def _swap(calls):
    """the log of an encode=None call -> what encode="png" must log: the crops at the end become one crop_png"""
    k = next(i for i, c in enumerate(calls) if c[0] == "crop")
    assert all(c[0] == "crop" for c in calls[k:])
    return calls[:k] + [("crop_png", [c[1] for c in calls[k:]])]


@pytest.mark.parametrize("call", ["edit", "edit_window", "edit_scaled", "edit_regions", "edit_strokes"])
def test_encode_none_issues_what_it_issued_and_png_one_crop_png(call):
    def go(s, **kw):
        if call == "edit":
            return s.edit(_sketch(), low_latency=False, **kw)
        if call == "edit_window":
            return s.edit(_sketch(), window=(0, 0, 64, 64), low_latency=False, **kw)
        if call == "edit_scaled":
            return s.edit(_sketch(), window=(3, 5, 70, 90), max_side=32, low_latency=False, **kw)
        if call == "edit_regions":
            return s.edit_regions(_sketch(), low_latency=False, **POLICY, **kw)
        return s.edit_strokes(STROKES, low_latency=False, **POLICY, **kw)
    (s0, b0), (s1, b1), (s2, b2) = _session(history=2), _session(history=2), _session(history=2)
    r0 = go(s0)                                     # the call without the argument
    r1 = go(s1, encode=None)
    r2 = go(s2, encode="png")
    assert b0.calls == b1.calls and "crop_png" not in [c[0] for c in b1.calls]
    assert b2.calls == _swap(b1.calls) and [c[0] for c in b2.calls].count("crop_png") == 1
    assert r0[1:] == r1[1:] == r2[1:]               # positions and info
    many = isinstance(r1[0], list)
    for raw0, raw, png in zip(*[(r[0] if many else [r[0]]) for r in (r0, r1, r2)]):
        assert isinstance(raw, np.ndarray) and np.array_equal(raw0, raw)
        assert isinstance(png, bytes) and np.array_equal(_decode(png), raw) and raw.any()
    assert np.array_equal(s1._frame, s2._frame) and s1.can_undo and s2.can_undo


def test_frame_png_and_refusals():
    s, stub = _session()
    s.edit(_sketch(), low_latency=False)
    del stub.calls[:]
    assert np.array_equal(_decode(s.frame_png()), s._frame)
    assert np.array_equal(_decode(s.frame_png((3, 5, 17, 33))), s._frame[3:20, 5:38])
    assert stub.calls == [("crop_png", [(0, 0) + HW]), ("crop_png", [(3, 5, 17, 33)])]
    for rect in ((0, 0, 15, 16), (0, 0, 16, 15), (-1, 0, 16, 16), (70, 0, 16, 16), (0, 270, 16, 16)):
        with pytest.raises(ValueError, match="rectangle"):
            s.frame_png(rect)
    for fn in (lambda: s.edit(_sketch(), encode="jpeg"), lambda: s.edit_regions(_sketch(), encode="raw"),
               lambda: s.edit_strokes(STROKES, encode=True)):
        with pytest.raises(ValueError, match="encode"):
            fn()
    assert stub.calls[2:] == []                    # refused before anything was issued
