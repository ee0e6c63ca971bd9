"""Host-side tests of the device JPEG encoder, no GPU: the stream's statement (tests/jpg_stream_util.py) inside
serve.jpg_from_scan's headers is a JPEG Pillow opens, stays within the bound, uses Annex K's tables as Pillow writes them, keeps
the ranges 6k proves, and costs what 6k says against Pillow's own encoder; the new header's symbols; and `encode=` of the session
calls against a scripted stand-in for the device side."""
import ctypes
import glob
import io
import os
import re

import numpy as np
import pytest
from PIL import Image

import jpg_cases
import jpg_stream_util as U
from sketchedit_amd import _lib, serve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# measured on the CPU from the statement over the 28 composed crops of the golden samples, against Pillow's
# Image.save(format="JPEG", quality=Q, subsampling=0, optimize=False): file bytes summed, ours over Pillow's, per quality
RATIO_MEASURED = {50: 1.0220, 75: 1.0169, 90: 1.0088, 95: 1.0031}
RATIO_MARGIN = 1.02
# and the worst per-crop PSNR of our decoded file minus Pillow's, in dB, over the four qualities; the margin covers another libjpeg
PSNR_WORST_MEASURED = -0.0451
PSNR_MARGIN = 0.1

CASES = jpg_cases.cases()
IDS = [c[0].split(":")[0] for c in CASES]


def _open(jpg, hw):
    im = Image.open(io.BytesIO(jpg))
    im.load()
    assert im.format == "JPEG" and im.mode == "RGB" and im.size == (hw[1], hw[0])
    return np.asarray(im)


def _pillow(a, quality):
    f = io.BytesIO()
    Image.fromarray(a).save(f, format="JPEG", quality=quality, subsampling=0, optimize=False)
    return f.getvalue()


def _segments(jpg):
    """the marker segments in front of the scan: [(marker, payload)]"""
    assert jpg[:2] == b"\xff\xd8"
    i, out = 2, []
    while True:
        assert jpg[i] == 0xFF
        n = (jpg[i + 2] << 8) | jpg[i + 3]
        out.append((jpg[i + 1], jpg[i + 4:i + 2 + n]))
        i += 2 + n
        if out[-1][0] == 0xDA:
            return out


def _check(a, quality):
    scan = U.jpg_scan(a, quality)
    h, w = a.shape[:2]
    assert 0 < len(scan) <= U.jpg_bound(h, w)
    jpg = serve.jpg_from_scan(scan, h, w, quality)
    assert jpg == U.jpg_file(scan, h, w, quality)
    return scan, _open(jpg, (h, w))


@pytest.fixture(scope="module")
def scans():
    """the statement's segment of every request of every case, computed once"""
    return {name: [U.jpg_scan(jpg_cases.rectangle(frames, r, hw), q) for r in reqs] for name, frames, reqs, hw, q in CASES}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_statement_is_a_jpeg(case, scans):
    name, frames, requests, hw, quality = case
    assert len(requests) == len(scans[name])
    for scan in scans[name]:
        assert 0 < len(scan) <= U.jpg_bound(*hw)
        jpg = serve.jpg_from_scan(scan, hw[0], hw[1], quality)
        assert jpg == U.jpg_file(scan, hw[0], hw[1], quality)
        _open(jpg, hw)
    assert {c[4] for c in CASES} == {1, 50, 90, 100}


def test_two_hundred_random_small_rectangles():
    rng = np.random.RandomState(17)
    for i in range(200):
        h, w = rng.randint(16, 25, 2)
        kind = i % 4
        if kind == 0:
            a = rng.randint(0, 256, (h, w, 3))
        elif kind == 1:
            a = rng.randint(0, 2, (h, w, 3)) * 255
        elif kind == 2:
            a = np.repeat(rng.randint(0, 256, (h, 1, 3)), w, axis=1)
        else:
            a = np.repeat(rng.randint(0, 256, (1, w, 3)), h, axis=0) + np.arange(h)[:, None, None] * (i % 3)
        a = (a & 255).astype(np.uint8)
        q = (1, 35, 50, 75, 90, 100)[i % 6]
        _, got = _check(a, q)
        if q >= 90 and kind >= 2:                   # smooth and fine: the decoded picture is the picture, nearly
            assert np.abs(got.astype(np.int64) - a).mean() < 4


def test_the_tables_are_pillow_s():
    a = np.random.RandomState(1).randint(0, 256, (16, 24, 3)).astype(np.uint8)
    assert U.dct_table() == U.DCT_A
    assert sorted(U.ZIGZAG) == list(range(64))
    for q in (1, 50, 75, 90, 100):
        theirs = _segments(_pillow(a, q))
        ours = _segments(serve.jpg_from_scan(b"", 16, 24, q))
        dqt = [bytes(p) for m, p in theirs if m == 0xDB]
        assert dqt == [bytes([0] + U.quant_table(U.BASE_LUMA, q)), bytes([1] + U.quant_table(U.BASE_CHROMA, q))]
        assert dqt == [bytes(p) for m, p in ours if m == 0xDB]
        assert dqt == [bytes([0] + serve.jpg_quant_table(serve.JPG_BASE_LUMA, q)), bytes([1] + serve.jpg_quant_table(serve.JPG_BASE_CHROMA, q))]
        dht = [bytes(p) for m, p in theirs if m == 0xC4]
        assert dht == [bytes([t] + c + s) for t, (c, s) in ((0x00, U.DC_LUMA), (0x10, U.AC_LUMA), (0x01, U.DC_CHROMA), (0x11, U.AC_CHROMA))]
        assert dht == [bytes(p) for m, p in ours if m == 0xC4]
        for m in (0xE0, 0xC0, 0xDA):                # and the JFIF header, the frame header (4:4:4) and the scan header
            assert [p for k, p in theirs if k == m] == [p for k, p in ours if k == m]
        assert [p for k, p in ours if k == 0xDD] == [bytes([0, 3])] and [k for k, _ in ours][-2:] == [0xDD, 0xDA]
    for bad in (0, 101):
        with pytest.raises(ValueError, match="quality"):
            serve.jpg_from_scan(b"", 16, 16, bad)
    # the AC tables have sizes up to 10 only, the DC tables up to 11
    for t in (U.AC_LUMA, U.AC_CHROMA):
        assert max(s & 15 for s in t[1]) == 10 and len(t[1]) == 162 == sum(t[0]) and max(n for _, n in U.huff_codes(t).values()) == 16
    for t in (U.DC_LUMA, U.DC_CHROMA):
        assert t[1] == list(range(12)) and max(n for _, n in U.huff_codes(t).values()) <= 11
    assert U.huff_codes(U.AC_LUMA)[U.ZRL][1] == 11 and U.huff_codes(U.AC_LUMA)[0xEA][1] == 16


def test_the_ranges_on_the_sign_patterns():
    """|AC| <= 1021, -1024 <= DC <= 1016 at q = 1: the extreme of coefficient (v, u) over all blocks is taken at the sign pattern
    of its basis function (and its negative), DESIGN.md 6k"""
    ones = [1] * 64
    ac = dc_hi = dc_lo = 0
    for v in range(8):
        for u in range(8):
            sg = [[1 if U.DCT_A[v][y] * U.DCT_A[u][x] >= 0 else -1 for x in range(8)] for y in range(8)]
            for sign in (1, -1):
                block = [[255 if sign * sg[y][x] > 0 else 0 for x in range(8)] for y in range(8)]
                s = U.fdct(block)
                assert all(abs(e) < (1 << 27) for r in s for e in r)
                c = U.quantise(s, ones)[U.ZIGZAG.index(v * 8 + u)]
                if v == u == 0:
                    dc_hi, dc_lo = max(dc_hi, c), min(dc_lo, c)
                else:
                    ac = max(ac, abs(c))
    assert (ac, dc_hi, dc_lo) == (1020, 1016, -1024)
    assert ac <= 1021 < 1 << 10 and dc_hi - dc_lo == 2040 < 1 << 11
    # the row pass alone: |t1| <= 2896
    assert max(abs((sum(abs(a) for a in row) * 128 + 512) >> 10) for row in U.DCT_A) <= 2896


def test_what_each_case_is_there_for(scans):
    by = {c[0].split(":")[0]: c for c in CASES}
    blocks = lambda key: U.blocks_of(jpg_cases.rectangle(by[key][1], by[key][2][0], by[key][3]), by[key][4])      # noqa: E731
    # flat colour: every block is its DC and EOB, and every DC difference after a row's first is 0
    rows = blocks("16x16 flat colour")
    assert all(not any(b[1:]) for r in rows for m in r for b in m) and all(r[0] == r[1] for r in rows)
    assert len(scans[by["16x16 flat colour"][0]][0]) < 40
    # 33 x 17: 5 x 3 MCUs, and the pixels behind the edges are the rectangle's
    a = by["33x17 noise"][1][0]
    assert len(blocks("33x17 noise")) == 5 and len(blocks("33x17 noise")[0]) == 3
    padded = np.pad(a, ((0, 7), (0, 7), (0, 0)), mode="edge")
    assert U.jpg_scan(padded, 50)[:20] == scans[by["33x17 noise"][0]][0][:20]
    # ten rows: the markers are D0 .. D7, D0: row 8's marker is the index 8 (mod 8), nine in all
    scan = scans[by["80x16 noise"][0]][0]
    marks = [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF and scan[i + 1] != 0]
    assert marks == [0xD0 + i % 8 for i in range(9)] and len(blocks("80x16 noise")) == 10
    # extremes: DC differences of size 11, and the 59-bit token
    rows = blocks("16x32 extremes at quality 100")
    assert [m[0][0] for m in rows[0]] == [1016, -1024, 1016, -1024]
    assert U.magnitude(-2040)[0] == U.magnitude(2040)[0] == 11
    for mcu, want in ((rows[1][2], 520), (rows[1][3], -520)):
        assert mcu[0][63] == want and not any(mcu[0][:63]) and not any(mcu[1]) and not any(mcu[2])
        tok = U.block_tokens(mcu[0], 0, 0)
        assert tok[63][1] == 3 * 11 + 16 + 10 == 59 and sum(n for _, n in tok[1:63]) == 0
    # the wide case: more than one tile of the row kernel's walk
    assert len(blocks("16x100 noise at quality 100")[0]) * 3 > 2 * jpg_cases.ROW_TILE_BLOCKS
    # stuffing, and an FF completed by the padding directly in front of a marker
    key = "24x16 noise at quality 100"
    raws = [U.row_raw(r) for r in blocks(key)]
    assert any(0xFF in raw[:-1] for raw, _ in raws)
    assert any(pad > 0 and raw[-1] == 0xFF for raw, pad in raws[:-1])
    scan = scans[by[key][0]][0]
    assert b"\xff\x00\xff\xd0" in scan or b"\xff\x00\xff\xd1" in scan


def test_size_and_quality_against_pillow():
    """files summed over the golden samples' composed crops quantised as test.py does, ours over Pillow's; and per crop the PSNR
    of our decoded file minus that of Pillow's"""
    crops = []
    for p in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "sample_*.npz"))):
        for c in np.load(p)["composed_crops"][:, 0]:
            crops.append(np.ascontiguousarray(((c + 1) / 2 * 255).astype(np.uint8).transpose(1, 2, 0)))
    assert len(crops) == 28

    def psnr(jpg, a):
        d = np.asarray(Image.open(io.BytesIO(jpg))).astype(np.float64) - a
        return 10 * np.log10(255.0 ** 2 / np.mean(d ** 2))
    worst = 0.0
    for q, measured in sorted(RATIO_MEASURED.items()):
        ours = theirs = 0
        for a in crops:
            mine, ref = serve.jpg_from_scan(U.jpg_scan(a, q), 64, 64, q), _pillow(a, q)
            ours, theirs = ours + len(mine), theirs + len(ref)
            worst = min(worst, psnr(mine, a) - psnr(ref, a))
        print("jpg quality %d: %d / %d = %.4f" % (q, ours, theirs, ours / theirs))
        assert ours / theirs <= measured * RATIO_MARGIN
    print("worst PSNR difference %.4f dB" % worst)
    assert worst >= PSNR_WORST_MEASURED - PSNR_MARGIN


def test_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "sketchedit_jpg.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(se_[a-z_A-Z0-9]+)\s*\(", hdr))
    own = _lib.abi_names("sketchedit_jpg.h")
    assert declared == set(own) and len(own) == 3 and "se_jpg.hip" in _lib.SOURCES
    _lib.build_library()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in own:
        assert getattr(lib, s) is not None
    lib.se_jpg_bound.restype = ctypes.c_size_t
    for hw in ((16, 16), (33, 17), (80, 16), (16, 100), (512, 512), (8192, 8192), (1080, 1920)):
        assert lib.se_jpg_bound(*hw) == U.jpg_bound(*hw) > 0
    assert [lib.se_jpg_bound(*hw) for hw in ((15, 16), (16, 15), (8193, 16), (16, 8193))] == [0] * 4
    assert [U.jpg_bound(*hw) for hw in ((15, 16), (16, 15), (8193, 16), (16, 8193))] == [0] * 4
    assert U.jpg_bound(16, 16) == 2 * (2 * ((1660 * 6 + 7) // 8) + 2) and U.BLOCK_BITS == 1660


# ---- encode= of the session calls against a scripted backend ----------------------------------------------------------------------
HW = (80, 280)
POLICY = dict(min_side=64, bucket=8)
STROKES = [([(10.5, 10.5), (19.5, 19.5)], 2.0), ([(250.5, 50.5), (259.5, 59.5)], 2.0)]


class _Stub:
    """Frames are numpy arrays; a run paints its windows; every call is logged.  crop_jpg is the statement."""

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
            f[y0:y0 + h, x0:x0 + w][s > 0] = 60 * self.value
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
        return [b"png"] * len(windows)

    def crop_jpg(self, frames, windows, quality):
        self.calls.append(("crop_jpg", list(windows), quality))
        return [serve.jpg_from_scan(U.jpg_scan(np.ascontiguousarray(f[y0:y0 + h, x0:x0 + w]), quality), h, w, quality)
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


def _swap(calls, quality):
    """the log of an encode=None call -> what encode="jpg" must log: the crops at the end become ONE crop_jpg"""
    k = next(i for i, c in enumerate(calls) if c[0] == "crop")
    assert all(c[0] == "crop" for c in calls[k:])
    return calls[:k] + [("crop_jpg", [c[1] for c in calls[k:]], quality)]


@pytest.mark.parametrize("call", ["edit", "edit_window", "edit_scaled", "edit_regions", "edit_strokes"])
def test_encode_none_issues_what_it_issued_and_jpg_one_crop_jpg(call):
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
    sessions = [_session(history=2) for _ in range(5)]
    (s0, b0), (s1, b1), (s2, b2), (s3, b3), (s4, b4) = sessions
    r0 = go(s0)                                     # the call without the argument
    r1 = go(s1, encode=None)
    r2 = go(s2, encode="jpg")
    r3 = go(s3, encode=("jpg", 35))
    r4 = go(s4, encode="png")
    assert b0.calls == b1.calls and not {"crop_png", "crop_jpg"} & {c[0] for c in b1.calls}
    assert b2.calls == _swap(b1.calls, 90) and b3.calls == _swap(b1.calls, 35)
    assert [c[0] for c in b2.calls].count("crop_jpg") == 1 and "crop" not in [c[0] for c in b2.calls]
    assert [c[0] for c in b4.calls].count("crop_png") == 1 and "crop_jpg" not in [c[0] for c in b4.calls]
    assert r0[1:] == r1[1:] == r2[1:] == r3[1:] == r4[1:]            # positions and info
    many = isinstance(r1[0], list)
    for raw0, raw, jpg, jpg35 in zip(*[(r[0] if many else [r[0]]) for r in (r0, r1, r2, r3)]):
        assert isinstance(raw, np.ndarray) and np.array_equal(raw0, raw) and raw.any()
        for data, q in ((jpg, 90), (jpg35, 35)):
            assert isinstance(data, bytes) and data == serve.jpg_from_scan(U.jpg_scan(raw, q), raw.shape[0], raw.shape[1], q)
            _open(data, raw.shape[:2])
        assert len(jpg35) <= len(jpg)
    assert np.array_equal(s1._frame, s2._frame) and np.array_equal(s1._frame, s3._frame) and s1.can_undo and s2.can_undo


def test_frame_jpg_and_refusals():
    s, stub = _session()
    s.edit(_sketch(), low_latency=False)
    del stub.calls[:]
    assert s.frame_jpg() == serve.jpg_from_scan(U.jpg_scan(s._frame, 90), HW[0], HW[1], 90)
    part = s.frame_jpg((3, 5, 17, 33), quality=50)
    assert part == serve.jpg_from_scan(U.jpg_scan(np.ascontiguousarray(s._frame[3:20, 5:38]), 50), 17, 33, 50)
    _open(part, (17, 33))
    assert stub.calls == [("crop_jpg", [(0, 0) + HW], 90), ("crop_jpg", [(3, 5, 17, 33)], 50)]
    for rect in ((0, 0, 15, 16), (0, 0, 16, 15), (-1, 0, 16, 16), (70, 0, 16, 16), (0, 270, 16, 16)):
        with pytest.raises(ValueError, match="rectangle"):
            s.frame_jpg(rect)
    for q in (0, 101, -5):
        with pytest.raises(ValueError, match="quality"):
            s.frame_jpg(quality=q)
    for bad in ("jpeg", "raw", True, "JPG", ("jpg", 0), ("jpg", 101), ("jpg", 50.0), ("jpg", True), ("png", 50), ("jpg",), ["jpg", 50]):
        for fn in (lambda: s.edit(_sketch(), encode=bad), lambda: s.edit_regions(_sketch(), encode=bad),
                   lambda: s.edit_strokes(STROKES, encode=bad)):
            with pytest.raises(ValueError, match="encode"):
                fn()
    assert stub.calls[2:] == []                    # refused before anything was issued
    assert not hasattr(serve.BatchingServer, "jpg") and "encode" not in serve.EditSession.undo.__code__.co_varnames
