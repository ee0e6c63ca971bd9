"""Host-side tests of the device JPEG encoder with 4:2:0 sampling and per-image Huffman tables, no GPU: the stream's
statement (tests/jpg2_stream_util.py) inside serve.jpg_from_scan's headers is a JPEG Pillow opens; every case of tests/jpg2_cases.py
has the property it is there for; the table builder keeps its promises over random histograms; the bound holds; the files cost what
6l says against Pillow's own encoder with the same settings and against 6k's files; the new header's symbols; and the new `encode`
forms of the session calls against a scripted stand-in for the device side."""
import ctypes
import glob
import io
import os
import re

import numpy as np
import pytest
from PIL import Image

import jpg2_cases
import jpg2_stream_util as U2
import jpg_cases
import jpg_stream_util as U
import test_jpg_host as T1
from sketchedit_amd import _lib, serve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUB = {0: ("444", False), 1: ("420", False), 2: ("444", True), 3: ("420", True)}
# measured on the CPU from the statement over the 28 composed crops of the golden samples, against Pillow's
# Image.save(format="JPEG", quality=Q, subsampling=2 under flag 1 else 0, optimize=True under flag 2): file bytes summed, ours over
# Pillow's, per flags and quality
RATIO_MEASURED = {1: {50: 1.0133, 75: 1.0108, 90: 1.0059, 95: 1.0020}, 2: {50: 1.0343, 75: 1.0236, 90: 1.0100, 95: 1.0029},
                  3: {50: 1.0213, 75: 1.0154, 90: 1.0073, 95: 1.0019}}
RATIO_MARGIN = 1.02
# the worst per-crop PSNR of our decoded file minus Pillow's, in dB, over the flags and qualities; the margin covers another libjpeg
PSNR_WORST_MEASURED = -0.0739
PSNR_MARGIN = 0.1
# the same files' bytes over those of flags = 0 (6k's 4:4:4 / Annex K files), recorded; asserted only to be below 1
SAVING_MEASURED = {1: {50: 0.8973, 75: 0.8632, 90: 0.8087, 95: 0.7745}, 2: {50: 0.6559, 75: 0.7344, 90: 0.8192, 95: 0.8588},
                   3: {50: 0.5664, 75: 0.6060, 90: 0.6358, 95: 0.6428}}
# (on a 256 x 256 mosaic of sixteen of the crops: 0.786 / 0.761 / 0.726 / 0.712, 0.891 / 0.952 / 0.971 / 0.967 and 0.709 / 0.724 /
# 0.707 / 0.691; there the files are 0.993 .. 1.006 of Pillow's)

CASES = jpg2_cases.cases()
IDS = [c[0].split(":")[0] for c in CASES]
_DCT = {}


def scan_of(a, quality, flags, key=None):
    """jpg2_scan with the DCT of an image shared between its qualities and between the flags with the same sampling"""
    if key is None:
        return U2.jpg2_scan(a, quality, flags)
    k = (key, flags & 1)
    if k not in _DCT:
        _DCT[k] = U2.dct_of(a, flags)
    return U2.jpg2_code(U2.quantised(_DCT[k], quality, flags), flags)


def file_of(a, quality, flags, key=None):
    scan, rec = scan_of(a, quality, flags, key)
    return serve.jpg_from_scan(scan, a.shape[0], a.shape[1], quality, SUB[flags][0], rec)


def _pillow(a, quality, flags):
    f = io.BytesIO()
    Image.fromarray(a).save(f, format="JPEG", quality=quality, subsampling=2 if flags & 1 else 0, optimize=bool(flags & 2))
    return f.getvalue()


def _codes(rec):
    return [U.huff_codes(t) for t in U2.tables_of_record(rec)]


def _check_tables(rec, hist):
    """a record against the counts it was made from: rules 5b, 5c and 5e"""
    assert len(rec) == U2.RECORD_BYTES
    for t, (counts, symbols) in enumerate(U2.tables_of_record(rec)):
        part = rec[t * 272:(t + 1) * 272]
        assert len(symbols) == sum(counts) and not any(part[16 + len(symbols):]), "the padding is zero"
        assert sorted(symbols) == [s for s in range(256) if hist[t][s]], "exactly the symbols that occur are coded"
        codes = U.huff_codes((counts, symbols))
        assert all(n <= 16 and code != (1 << n) - 1 for code, n in codes.values()), "no code of 1-bits only"
        assert sum(2.0 ** -n for _, n in codes.values()) < 1.0
        if len(symbols) == 1:
            assert codes[symbols[0]] == (0, 1)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_statement_decodes_and_stays_within_the_bound(case):
    name, frames, reqs, hw, qualities = case
    for ri, r in enumerate(reqs):
        a = jpg2_cases.rectangle(frames, r, hw)
        for q in qualities:
            assert scan_of(a, q, 0, (name, ri)) == (U.jpg_scan(a, q), None)            # flags = 0 is 6k's stream
            pix = {}
            for flags in jpg2_cases.FLAGS:
                scan, rec = scan_of(a, q, flags, (name, ri))
                assert 0 < len(scan) <= U2.jpg2_bound(hw[0], hw[1], flags)
                assert (rec is None) == (not flags & 2)
                f = serve.jpg_from_scan(scan, hw[0], hw[1], q, SUB[flags][0], rec)
                assert f == U2.jpg2_file(scan, hw[0], hw[1], q, flags, rec)
                pix[flags] = T1._open(f, hw)
                if rec is not None:
                    _check_tables(rec, U2.histograms(U2.quantised(_DCT[((name, ri), flags & 1)], q, flags), flags))
            assert np.array_equal(pix[1], pix[3])                                     # the tables do not change a pixel
            assert np.array_equal(pix[2], T1._open(serve.jpg_from_scan(U.jpg_scan(a, q), hw[0], hw[1], q), hw))


def test_what_each_case_is_there_for():
    by = {c[0].split(":")[0]: c for c in CASES}
    # 16x16 flat: six blocks of EOB only under 420, every optimised table the single code 0
    name, frames, reqs, hw, qs = by["16x16 flat grey 128"]
    for q in qs:
        rows = U2.blocks_of(frames[0], q, 1)
        assert len(rows) == 1 and len(rows[0]) == 6 and not any(v for b in rows[0] for v in b)
        for flags in (2, 3):
            rec = U2.jpg2_scan(frames[0], q, flags)[1]
            for counts, symbols in U2.tables_of_record(rec):
                assert counts == [1] + [0] * 15 and len(symbols) == 1
    # 17x33: partial MCUs; the replicated column and row enter the averages
    name, frames, reqs, hw, qs = by["17x33 noise"]
    a = frames[0]
    assert len(U2.blocks_of(a, 90, 1)) == 2 and len(U2.blocks_of(a, 90, 1)[0]) == 18
    ext = a[np.minimum(np.arange(32), 16)][:, np.minimum(np.arange(48), 32)]
    assert U2.blocks_of(a, 90, 1) == U2.blocks_of(ext, 90, 1)
    cb = U.ycc(ext)[1]
    assert np.array_equal(U2.downsample(cb)[8, :16], (cb[16, 0:32:2] + cb[16, 1:32:2] + cb[17, 0:32:2] + cb[17, 1:32:2]
                                                      + 1 + (np.arange(16) & 1)) >> 2)
    behind = np.full((40, 60, 3), 255, np.uint8)                          # never from the frame behind the rectangle
    behind[:17, :33] = a
    assert U2.jpg2_scan(np.ascontiguousarray(behind[:17, :33]), 90, 3) == U2.jpg2_scan(a, 90, 3)
    # 144x16: nine rows under 420, the markers D0 .. D7, D0
    name, frames, reqs, hw, qs = by["144x16 noise"]
    scan = U2.jpg2_scan(frames[0], 50, 1)[0]
    marks = [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF and scan[i + 1] != 0]
    assert marks == [0xD0 + i % 8 for i in range(8)]
    assert len(U2.blocks_of(frames[0], 50, 2)) == 18
    scan = U2.jpg2_scan(by["160x16 noise"][1][0], 50, 3)[0]             # ten rows: the index wraps under 420 too
    assert [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF and scan[i + 1] != 0] == [0xD0 + i % 8 for i in range(9)]
    # 16x272: 102 blocks, seven tiles; MCU boundaries inside tiles; 3-back and 6-back predecessors across tile boundaries
    name, frames, reqs, hw, qs = by["16x272 noise at quality 100"]
    row = U2.blocks_of(frames[0], 100, 3)[0]
    T = jpg2_cases.ROW_TILE_BLOCKS
    assert len(row) == 102 and -(-102 // T) == 7 and any(t % 6 for t in range(T, 102, T))
    assert any(b % 6 == 0 and (b - 3) // T < b // T for b in range(6, 102))          # Y(0,0) against Y(1,1) of the tile before
    assert any(b % 6 >= 4 and (b - 6) // T < b // T for b in range(6, 102))          # Cb / Cr six back in the tile before
    # the bias: sums of every residue in even and odd chroma columns; a constant 2 or a start at 2 changes the stream
    name, frames, reqs, hw, qs = by["16x16 chroma sums of every residue mod 4 in even and odd columns"]
    cb = U.ycc(frames[0])[1]
    s = cb[0::2, 0::2] + cb[0::2, 1::2] + cb[1::2, 0::2] + cb[1::2, 1::2]
    for parity in (0, 1):
        assert {1, 2, 3} <= set((s[:, parity::2] % 4).ravel().tolist())
    good = U2.blocks_of(frames[0], 100, 1)                              # (quality 100: q = 1, no change is quantised away)
    assert U2.blocks_of(frames[0], 100, 1, bias_of=lambda x: 2) != good
    assert U2.blocks_of(frames[0], 100, 1, bias_of=lambda x: 2 - (x & 1)) != good
    assert U2.blocks_of(frames[0], 100, 1, bias_of=lambda x: 1 + (x & 1)) == good
    # stuffing: FF 00 inside a row, and an FF completed by the padding directly in front of a marker, under flags 2 and 3
    name, frames, reqs, hw, qs = by["32x16 noise at quality 100"]
    for flags in (2, 3):
        raws = U2.rows_raw(U2.blocks_of(frames[0], 100, flags), flags)[0]
        assert any(0xFF in raw[:-1] for raw, _ in raws)
        assert any(pad > 0 and raw[-1] == 0xFF for raw, pad in raws[:-1])
        assert re.search(b"\xff\x00\xff[\xd0-\xd7]", U2.jpg2_scan(frames[0], 100, flags)[0])
    # odd origins; B = 3 over two frames
    assert by["x0, y0 odd in a frame of width 53"][1][0].shape[1] == 53 and all(v % 2 for v in by["x0, y0 odd in a frame of width 53"][2][0][1:])
    assert len(by["B = 3, windows of two frames of different sizes"][2]) == 3 and len(by["B = 3, windows of two frames of different sizes"][1]) == 2


def _hist(plane, flags):
    return U2.histograms(plane[0].tolist(), flags)


def test_what_each_coefficient_plane_is_there_for():
    ac = [((r & 15) << 4) | s for r in range(16) for s in range(1, 11)] + [0x00, 0xF0]
    for flags in (2, 3):
        per = 6 if flags & 1 else 3
        # fibonacci: 17 symbols, 6763 in all; the first tree is 17 deep and the counts are halved once
        p = jpg2_cases.fibonacci(flags)
        h = _hist(p, flags)
        assert sorted(c for c in h[1] if c) == jpg2_cases.FIB and sum(h[1]) == 6763 and p.shape[2] % per == 0
        lifted, _ = U2.huff_lengths(h[1], limit=None)
        lengths, halvings = U2.huff_lengths(h[1])
        assert max(lifted.values()) == 17 and halvings == 1 and max(lengths.values()) <= 16
        plain = [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597]
        assert max(U2.huff_lengths(plain + [0] * 239, limit=None)[0].values()) <= 16   # (plain Fibonacci counts do not do it)
        # long_token: ZRL's code is at least 13 bits and the token of coefficient 63 is longer than 64 bits
        p = jpg2_cases.long_token(flags)
        rows = p[0].tolist()
        lengths, _ = U2.huff_lengths(_hist(p, flags)[1])
        assert lengths[0xF0] >= 13 and not any(rows[0][0][:63]) and rows[0][0][63] == 513
        codes = [U.huff_codes(t) for t in U2.rows_raw(rows, flags)[1]]
        tok = [t for t in U2.row_symbols(rows[0], flags) if t[1][:3] == [0xF0] * 3]
        assert len(tok) == 1 and tok[0][1] == [0xF0, 0xF0, 0xF0, 0xEA] and U2.token_bits(tok[0], codes)[1] > 64
        # all_symbols: the 162 AC symbols and the 12 DC sizes in both classes
        h = _hist(jpg2_cases.all_symbols(flags), flags)
        for t in (0, 2):
            assert [s for s in range(256) if h[t][s]] == list(range(12))
            assert [s for s in range(256) if h[t + 1][s]] == sorted(ac)
        # dc_extremes: -1024 next to 1016, differences of size 11
        p = jpg2_cases.dc_extremes(flags)
        assert {-1024, 1016} == set(p[..., 0].ravel().tolist()) - {0} and _hist(p, flags)[0][11] > 0 and _hist(p, flags)[2][11] > 0
        # ties: many symbols with equal counts
        h = _hist(jpg2_cases.ties(flags), flags)
        assert sum(1 for c in h[1] if c == 3) >= 40 and sum(1 for c in h[3] if c == 6) >= 40   # (Cb and Cr share a table)
        # out_of_range: the statement clamps; the segment is that of the clamped plane, and Pillow's decoder reads it
        p = jpg2_cases.out_of_range(flags)
        assert p.max() == 32767 and p.min() == -32768
        assert U2.jpg2_code(p[0].tolist(), flags) == U2.jpg2_code(jpg2_cases.clamped(p)[0].tolist(), flags)
        h = _hist(p, flags)
        assert h[0][11] + h[2][11] > 0 and not any(h[t][s] for t in (0, 2) for s in range(12, 256))
        assert not any(h[t][s] for t in (1, 3) for s in range(256) if (s & 15) > 10)
    for name, build in jpg2_cases.code_cases():
        for flags in jpg2_cases.code_flags(name):
            p = build(flags)
            scan, rec = U2.jpg2_code(p[0].tolist(), flags)
            assert len(scan) <= p.shape[1] * U2.row_bound(p.shape[2], flags)
            if rec is not None:
                _check_tables(rec, _hist(p, flags))
            mcu = 16 if flags & 1 else 8
            h, w = p.shape[1] * mcu, p.shape[2] // (6 if flags & 1 else 3) * mcu
            T1._open(serve.jpg_from_scan(scan, h, w, 100, SUB[flags][0], rec), (h, w))          # a decoder follows every code


def test_200_random_rectangles_decode():
    rng = np.random.RandomState(11)
    for i in range(200):
        h, w = (int(v) for v in rng.randint(16, 34, 2))
        a = (rng.randint(0, 256, (h, w, 3)) if i % 3 else np.clip(rng.randint(0, 40, (h, w, 3)) + 5 * np.arange(w)[None, :, None], 0, 255)).astype(np.uint8)
        q = int(rng.choice([1, 20, 50, 75, 90, 100]))
        pix = {}
        for flags in jpg2_cases.FLAGS:
            scan, rec = scan_of(a, q, flags, ("random", i))
            assert len(scan) <= U2.jpg2_bound(h, w, flags)
            pix[flags] = T1._open(serve.jpg_from_scan(scan, h, w, q, SUB[flags][0], rec), (h, w))
        assert np.array_equal(pix[1], pix[3])
    _DCT.clear()


def test_3000_random_histograms():
    rng = np.random.RandomState(12)
    halved = 0
    for i in range(3000):
        n = int(rng.randint(1, 257))
        counts = np.zeros(256, np.int64)
        where = rng.choice(256, n, replace=False)
        kind = i % 4
        if kind == 0:
            counts[where] = rng.randint(1, 1000, n)
        elif kind == 1:
            counts[where] = rng.randint(1, 4, n)                          # ties
        elif kind == 2:
            counts[where] = (1.7 ** np.minimum(np.arange(n), 38)).astype(np.int64) + rng.randint(0, 2, n)      # deep trees
        else:
            counts[where] = 2 ** rng.randint(0, 24, n)
        lengths, h = U2.huff_lengths(counts.tolist())
        halved += h > 0
        assert sorted(lengths) == sorted(where.tolist()) and 1 <= min(lengths.values()) and max(lengths.values()) <= 16
        table = U2.huff_table(counts.tolist(), lengths)
        codes = U.huff_codes(table)
        assert sorted(codes) == sorted(where.tolist()) and all(codes[s][1] == lengths[s] for s in codes)
        assert all(code != (1 << nb) - 1 for code, nb in codes.values())
        assert sum(2.0 ** -nb for _, nb in codes.values()) < 1.0
        rec = U2.table_record([table] * 4)
        assert len(rec) == 1088 and U2.tables_of_record(rec)[3] == (table[0], table[1])
    assert halved > 100                                                   # the limit was met often


def test_bound():
    assert U2.BLOCK_BITS_OPT == 1665 and U.BLOCK_BITS == 1660
    for hw in ((16, 16), (17, 33), (144, 16), (16, 272), (512, 512), (8192, 8192), (1081, 1921)):
        assert U2.jpg2_bound(hw[0], hw[1], 0) == U.jpg_bound(*hw)
        rows, n = -(-hw[0] // 16), 6 * -(-hw[1] // 16)
        assert U2.jpg2_bound(hw[0], hw[1], 3) == rows * (2 * ((1665 * n + 7) // 8) + 2)
        assert U2.jpg2_bound(hw[0], hw[1], 1) == rows * (2 * ((1660 * n + 7) // 8) + 2)
        assert U2.jpg2_bound(hw[0], hw[1], 2) == -(-hw[0] // 8) * (2 * ((1665 * 3 * -(-hw[1] // 8) + 7) // 8) + 2)
    for bad in ((15, 16, 0), (16, 15, 1), (8193, 16, 2), (16, 8193, 3), (16, 16, 4), (16, 16, -1)):
        assert U2.jpg2_bound(*bad) == 0
    # the worst block the clamp admits stays inside the block bound under tables whose codes are all 16 bits long
    assert 16 + 11 + 63 * (16 + 10) == 1665
    for r in range(63):
        assert 16 * (r >> 4) + 16 + 10 <= 26 * (r + 1)


def _segments(jpg):
    return T1._segments(jpg)


def test_headers_match_pillows():
    a = jpg2_cases.by_name("17x33 noise", CASES)[1][0]
    for flags in jpg2_cases.FLAGS:
        mine, ref = dict(_segments(file_of(a, 75, flags))), dict(_segments(_pillow(a, 75, flags)))
        assert mine[0xC0] == ref[0xC0] and mine[0xC0][6:] == bytes([1, 0x22 if flags & 1 else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
        assert mine[0xDA] == ref[0xDA]
        assert mine[0xDD] == (-(-33 // (16 if flags & 1 else 8))).to_bytes(2, "big")
    mine = _segments(file_of(a, 75, 3))
    dht = [p for m, p in mine if m == 0xC4]
    assert [p[0] for p in dht] == [0x00, 0x10, 0x01, 0x11] and all(len(p) == 17 + sum(p[1:17]) for p in dht)       # the true counts
    assert [m for m, _ in mine] == [m for m, _ in _segments(serve.jpg_from_scan(b"", 17, 33, 75))]
    with pytest.raises(ValueError):
        serve.jpg_from_scan(b"", 17, 33, 75, "422")
    with pytest.raises(ValueError):
        serve.jpg_from_scan(b"", 17, 33, 75, "420", b"\0" * 1087)
    scan = U.jpg_scan(a, 75)
    assert serve.jpg_from_scan(scan, 17, 33, 75) == serve.jpg_from_scan(scan, 17, 33, 75, "444", None) == U.jpg_file(scan, 17, 33, 75)


def test_size_and_quality_against_pillow():
    crops = []
    for p in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "sample_*.npz"))):
        for c in np.load(p)["composed_crops"][:, 0]:
            crops.append(np.ascontiguousarray(((c + 1) / 2 * 255).astype(np.uint8).transpose(1, 2, 0)))
    assert len(crops) == 28

    def psnr(jpg, a):
        d = np.asarray(Image.open(io.BytesIO(jpg))).astype(np.float64) - a
        return 10 * np.log10(255.0 ** 2 / np.mean(d ** 2))
    worst = 0.0
    for q in (50, 75, 90, 95):
        base = sum(len(file_of(a, q, 0, ("crop", i))) for i, a in enumerate(crops))
        for flags in jpg2_cases.FLAGS:
            ours = theirs = 0
            for i, a in enumerate(crops):
                mine, ref = file_of(a, q, flags, ("crop", i)), _pillow(a, q, flags)
                ours, theirs = ours + len(mine), theirs + len(ref)
                worst = min(worst, psnr(mine, a) - psnr(ref, a))
            print("jpg2 flags %d quality %d: %d / %d = %.4f of Pillow's, %.4f of flags 0" % (flags, q, ours, theirs, ours / theirs, ours / base))
            assert ours / theirs <= RATIO_MEASURED[flags][q] * RATIO_MARGIN
            assert ours / base < 1.0                                        # (SAVING_MEASURED records the figure)
    print("worst PSNR difference %.4f dB" % worst)
    assert worst >= PSNR_WORST_MEASURED - PSNR_MARGIN
    _DCT.clear()


def test_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "sketchedit_jpg2.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(se_[a-z_A-Z0-9]+)\s*\(", hdr))
    own = _lib.abi_names("sketchedit_jpg2.h")
    assert declared == set(own) and len(own) == 5 and "se_jpg2.hip" not in _lib.SOURCES and "se_jpg.hip" in _lib.SOURCES
    assert "#define SE_JPG_420 1" in hdr and "#define SE_JPG_OPTIMIZE 2" in hdr and (_lib.SE_JPG_420, _lib.SE_JPG_OPTIMIZE) == (1, 2)
    _lib.build_library()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in own + _lib.abi_names("sketchedit_jpg.h"):
        assert getattr(lib, s) is not None
    lib.se_jpg2_bound.restype = ctypes.c_size_t
    lib.se_jpg_bound.restype = ctypes.c_size_t
    for hw in ((16, 16), (17, 33), (144, 16), (16, 272), (512, 512), (8192, 8192), (1081, 1921)):
        for flags in range(4):
            assert lib.se_jpg2_bound(hw[0], hw[1], flags) == U2.jpg2_bound(hw[0], hw[1], flags) > 0
        assert lib.se_jpg2_bound(hw[0], hw[1], 0) == lib.se_jpg_bound(*hw)
    for bad in ((15, 16, 0), (16, 15, 1), (8193, 16, 2), (16, 8193, 3), (16, 16, 4), (16, 16, -1)):
        assert lib.se_jpg2_bound(*bad) == 0
    from sketchedit_amd import kernel_labels
    for k in ("jpg2_blocks420_kernel", "jpg2_hist_kernel", "jpg2_tables_kernel", "jpg2_rows_kernel"):
        assert kernel_labels.label_of("%s(short const*, int)" % k) == k[:-len("_kernel")]
    assert kernel_labels.label_of("jpg_rows_kernel(short const*, int)") == "jpg_rows"


# ---- the new encode forms of the session calls against a scripted backend ---------------------------------------------------------
class _Stub2(T1._Stub):
    """6k's stand-in with the new keywords: crop_jpg is the statement; a call with the defaults is logged as it always was"""

    def crop_jpg(self, frames, windows, quality, **kw):
        self.calls.append(("crop_jpg", list(windows), quality) + ((dict(kw),) if kw else ()))
        flags = (1 if kw.get("subsampling", "444") == "420" else 0) | (2 if kw.get("optimize", False) else 0)
        return [file_of(np.ascontiguousarray(f[y0:y0 + h, x0:x0 + w]), quality, flags) for f, (y0, x0, h, w) in zip(frames, windows)]


def _session(stub):
    return serve.EditSession(None, np.zeros(T1.HW + (3,), np.uint8), backend=stub, history=2)


FORMS = [(("jpg", 35, "420"), 1), (("jpg", 35, "444", True), 2), (("jpg", 35, "420", True), 3), (("jpg", 35, "420", False), 1)]


@pytest.mark.parametrize("call", ["edit", "edit_regions", "edit_strokes"])
def test_new_encode_forms_issue_one_crop_jpg_with_the_keywords(call):
    def go(s, **kw):
        if call == "edit":
            return s.edit(T1._sketch(), low_latency=False, **kw)
        if call == "edit_regions":
            return s.edit_regions(T1._sketch(), low_latency=False, **T1.POLICY, **kw)
        return s.edit_strokes(T1.STROKES, low_latency=False, **T1.POLICY, **kw)
    old, new = T1._Stub(), _Stub2()
    r_old, r_new = go(_session(old), encode=("jpg", 35)), go(_session(new), encode=("jpg", 35))
    assert old.calls == new.calls and r_old == r_new                      # the default form: today's three-argument call, today's bytes
    assert [c for c in new.calls if c[0] == "crop_jpg"][0][2:] == (35,)
    raw_stub = _Stub2()
    raw = go(_session(raw_stub))
    for form in (("jpg", 35, "444"), ("jpg", 35, "444", False)):          # the defaults spelled out are the default form
        b = T1._Stub()                                                    # (a backend without the keywords takes them)
        assert go(_session(b), encode=form) == r_old and b.calls == old.calls
    many = isinstance(raw[0], list)
    for form, flags in FORMS:
        b = _Stub2()
        r = go(_session(b), encode=form)
        assert r[1:] == raw[1:]
        want = T1._swap(raw_stub.calls, 35)
        want[-1] = want[-1] + (dict(subsampling=SUB[flags][0], optimize=SUB[flags][1]),)
        assert b.calls == want
        for patch, data in zip(raw[0] if many else [raw[0]], r[0] if many else [r[0]]):
            assert isinstance(data, bytes) and data == file_of(patch, 35, flags)
            T1._open(data, patch.shape[:2])


def test_frame_jpg_keywords_and_refusals():
    stub = _Stub2()
    s = _session(stub)
    s.edit(T1._sketch(), low_latency=False)
    del stub.calls[:]
    assert s.frame_jpg() == serve.jpg_from_scan(U.jpg_scan(s._frame, 90), T1.HW[0], T1.HW[1], 90)
    part = np.ascontiguousarray(s._frame[3:20, 5:38])
    assert s.frame_jpg((3, 5, 17, 33), quality=50, subsampling="420", optimize=True) == file_of(part, 50, 3)
    assert s.frame_jpg((3, 5, 17, 33), 50, "420") == file_of(part, 50, 1)
    assert s.frame_jpg((3, 5, 17, 33), 50, optimize=True) == file_of(part, 50, 2)
    assert s.frame_jpg((3, 5, 17, 33), 50, "444", False) == serve.jpg_from_scan(U.jpg_scan(part, 50), 17, 33, 50)
    assert stub.calls == [("crop_jpg", [(0, 0) + T1.HW], 90), ("crop_jpg", [(3, 5, 17, 33)], 50, dict(subsampling="420", optimize=True)),
                          ("crop_jpg", [(3, 5, 17, 33)], 50, dict(subsampling="420", optimize=False)),
                          ("crop_jpg", [(3, 5, 17, 33)], 50, dict(subsampling="444", optimize=True)), ("crop_jpg", [(3, 5, 17, 33)], 50)]
    for kw in (dict(subsampling="422"), dict(subsampling=420), dict(subsampling=None), dict(optimize=1), dict(optimize="yes"), dict(optimize=None)):
        with pytest.raises(ValueError, match="subsampling|optimize"):
            s.frame_jpg(**kw)
    bad_forms = [("jpg", 50, "422"), ("jpg", 50, 420), ("jpg", 50, "420", 1), ("jpg", 50, "420", None), ("jpg", 50, "420", True, 0),
                 ("jpg", 50, True), ("jpg", 0, "420"), ("jpg", 101, "420", True), ("jpg", 50.0, "420"), ("png", 50, "420"),
                 ["jpg", 50, "420"], ("jpg", 50, None, True)]
    bad_forms += ["jpeg", "raw", True, "JPG", ("jpg", 0), ("jpg", 101), ("jpg", 50.0), ("jpg", True), ("png", 50), ("jpg",), ["jpg", 50]]
    for bad in bad_forms:
        for fn in (lambda: s.edit(T1._sketch(), encode=bad), lambda: s.edit_regions(T1._sketch(), encode=bad),
                   lambda: s.edit_strokes(T1.STROKES, encode=bad)):
            with pytest.raises(ValueError, match="encode"):
                fn()
    assert stub.calls[5:] == []                     # refused before anything was issued
    assert not hasattr(serve.BatchingServer, "jpg") and "encode" not in serve.EditSession.undo.__code__.co_varnames
    import inspect
    assert list(inspect.signature(serve._ModelBackend.crop_jpg).parameters)[1:] == ["frames", "windows", "quality", "subsampling", "optimize"]
    assert list(inspect.signature(serve.EditSession.frame_jpg).parameters)[1:] == ["rect", "quality", "subsampling", "optimize"]
    assert list(inspect.signature(serve.jpg_from_scan).parameters) == ["scan", "h", "w", "quality", "subsampling", "tables"]
