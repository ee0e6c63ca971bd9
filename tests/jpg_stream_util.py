"""The entropy-coded segment of the device JPEG encoder (include/sketchedit_jpg.h) restated in plain Python ints,
with no Pillow and no libjpeg in the encoder: the yardstick of se_jpg_encode_u8, as tests/png_stream_util.py is of the PNG
encoder.  Slow and literal on purpose.

The source is an hs x ws RGB rectangle (16 <= hs, ws <= 8192) and a quality 1 .. 100.
 1. colour (JFIF, 16-bit fixed point): Y = (19595 R + 38470 G + 7471 B + 32768) >> 16,
    Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16, Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16.
    4:4:4, one MCU = one 8 x 8 block of each, in the order Y, Cb, Cr.
 2. edges: a side that is no multiple of 8 is extended by repeating the rectangle's last column and last row.
 3. DCT: A[u][x] = round(8192 * 1/2 * c(u) * cos((2 x + 1) u pi / 16)), c(0) = 1/sqrt 2, committed as 64 integers.  Rows:
    t = sum_x A[u][x] (p - 128), t1 = (t + 512) >> 10.  Columns: s = sum_y A[v][y] t1, 16 fraction bits.
 4. quantise: c = sign(s) ((|s| + (q << 15)) // (q << 16)); q = clamp((base scale + 50) // 100, 1, 255), scale = 5000 // Q for
    Q < 50, else 200 - 2 Q; base = Annex K's luminance table for Y, its chrominance table for Cb and Cr.
 5. entropy code: baseline Huffman with the four Annex K tables, bits MSB first.  The DC difference is against the previous block
    of the same component, 0 at the start of a restart interval.  AC: (run, size) and the magnitude bits, ZRL for every 16 zeros
    in front of a non-zero coefficient, EOB when the block ends in zeros.
 6. restart intervals: one interval = one row of MCUs.  At its end: pad with 1-bits to a byte; every FF byte of the interval's
    data (the padded byte included) is followed by 00; then FF D0+(row mod 8) after every row but the last.
 7. the segment is the rows and markers, no headers; jpg_file (= serve.jpg_from_scan) puts the file around it."""
import math

import numpy as np

SIDE_MIN, SIDE_MAX = 16, 8192
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
          49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
# Annex K's quantisation tables, in zigzag order (as a DQT segment carries them)
BASE_LUMA = [16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40, 26, 24, 22, 22, 24, 49, 35, 37, 29, 40, 58, 51, 61, 60,
             57, 51, 56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56, 80, 109, 81, 87, 95, 98, 103, 104, 103, 62, 77, 113, 121, 112,
             100, 120, 92, 101, 103, 99]
BASE_CHROMA = [17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66, 99] + [99] * 49
# Annex K's Huffman tables as a DHT segment carries them: the 16 counts of codes per length, then the symbols
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125],
           [1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240,
            36, 51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72,
            73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131,
            132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170,
            178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216,
            217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119],
             [0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240,
              21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70,
              71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121,
              122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167,
              168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213,
              214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250])
# rule 3's table, rows u, columns x
DCT_A = [[2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896],
         [4017, 3406, 2276, 799, -799, -2276, -3406, -4017],
         [3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784],
         [3406, -799, -4017, -2276, 2276, 4017, 799, -3406],
         [2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896],
         [2276, -4017, 799, 3406, -3406, -799, 4017, -2276],
         [1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567],
         [799, -2276, 3406, -4017, 4017, -3406, 2276, -799]]
BLOCK_BITS = 22 + 63 * 26                    # 1660: the most bits of one block
EOB, ZRL = 0x00, 0xF0


def dct_table():
    """rule 3's table from its formula (the committed integers are asserted against it)"""
    return [[int(round(8192 * 0.5 * (math.sqrt(0.5) if u == 0 else 1.0) * math.cos((2 * x + 1) * u * math.pi / 16))) for x in range(8)]
            for u in range(8)]


def huff_codes(table):
    """(counts, symbols) -> {symbol: (code, length)}, the canonical code of Annex C"""
    counts, symbols = table
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[symbols[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def quant_table(base, quality):
    """rule 4's table, in zigzag order"""
    q = int(quality)
    assert 1 <= q <= 100
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return [min(max((b * scale + 50) // 100, 1), 255) for b in base]


def ycc(a):
    """(h, w, 3) uint8 -> three (h, w) planes of ints 0 .. 255 by rule 1"""
    r, g, b = (np.asarray(a)[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def fdct(block):
    """8 x 8 ints 0 .. 255 (rows y, columns x) -> s[v][u] by rule 3, 16 fraction bits"""
    t1 = [[(sum(DCT_A[u][x] * (int(block[y][x]) - 128) for x in range(8)) + 512) >> 10 for u in range(8)] for y in range(8)]
    return [[sum(DCT_A[v][y] * t1[y][u] for y in range(8)) for u in range(8)] for v in range(8)]


def quantise(s, qt):
    """s[v][u], a zigzag table -> the 64 coefficients in zigzag order by rule 4"""
    out = []
    for k in range(64):
        v = s[ZIGZAG[k] >> 3][ZIGZAG[k] & 7]
        q = qt[k]
        c = (abs(v) + (q << 15)) // (q << 16)
        out.append(-c if v < 0 else c)
    return out


def blocks_of(a, quality):
    """-> [row][mcu][component] = 64 zigzag coefficients, rules 1 - 4"""
    a = np.asarray(a)
    assert a.ndim == 3 and a.shape[2] == 3 and a.dtype == np.uint8
    h, w = a.shape[:2]
    H, W = -(-h // 8) * 8, -(-w // 8) * 8
    a = a[np.minimum(np.arange(H), h - 1)][:, np.minimum(np.arange(W), w - 1)]       # rule 2
    planes = ycc(a)
    qts = [quant_table(BASE_LUMA, quality)] + [quant_table(BASE_CHROMA, quality)] * 2
    return [[[quantise(fdct(planes[c][y:y + 8, x:x + 8].tolist()), qts[c]) for c in range(3)] for x in range(0, W, 8)]
            for y in range(0, H, 8)]


class _Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, nbits):
        assert 0 <= value < (1 << nbits)
        self.acc = (self.acc << nbits) | value
        self.n += nbits


def magnitude(v):
    """a coefficient -> (size, its magnitude bits): v for v > 0, v - 1 in `size` bits for v < 0"""
    size = abs(v).bit_length()
    return size, (v if v >= 0 else v + (1 << size) - 1)


_CODES = None


def codes():
    global _CODES
    if _CODES is None:
        _CODES = [huff_codes(t) for t in (DC_LUMA, AC_LUMA, DC_CHROMA, AC_CHROMA)]
    return _CODES


def block_tokens(coef, pred, comp):
    """one block -> [(value, nbits)] per zigzag index: entry 0 the DC's token, entry k the token of coefficient k (its ZRLs, its
    code, its magnitude bits; empty for a zero), entry 63 also EOB if coefficient 63 is zero"""
    dc, ac = codes()[0 if comp == 0 else 2], codes()[1 if comp == 0 else 3]
    size, bits = magnitude(coef[0] - pred)
    assert size <= 11
    c, n = dc[size]
    out = [((c << size) | bits, n + size)]
    run = 0
    for k in range(1, 64):
        if coef[k] == 0:
            run += 1
            out.append((0, 0))
            continue
        value = nbits = 0
        for _ in range(run >> 4):
            c, n = ac[ZRL]
            value, nbits = (value << n) | c, nbits + n
        size, bits = magnitude(coef[k])
        assert size <= 10
        c, n = ac[((run & 15) << 4) | size]
        out.append(((((value << n) | c) << size) | bits, nbits + n + size))
        run = 0
    if coef[63] == 0:
        out[63] = ac[EOB]
    return out


def row_raw(row):
    """one row of MCUs (blocks_of's) -> (the bytes of its interval before stuffing, the number of 1-bits that pad the last)"""
    bits = _Bits()
    pred = [0, 0, 0]
    for mcu in row:
        for comp in range(3):
            for value, nbits in block_tokens(mcu[comp], pred[comp], comp):
                if nbits:
                    bits.put(value, nbits)
            pred[comp] = mcu[comp][0]
    pad = -bits.n % 8
    bits.put((1 << pad) - 1, pad)
    return bits.acc.to_bytes(bits.n // 8, "big"), pad


def row_bytes(row, index, last):
    """one row of MCUs -> the bytes of its restart interval by rules 5 and 6"""
    out = bytearray()
    for v in row_raw(row)[0]:
        out.append(v)
        if v == 0xFF:
            out.append(0)
    if not last:
        out += bytes([0xFF, 0xD0 + index % 8])
    return bytes(out)


def jpg_scan(a, quality=90):
    """(hs, ws, 3) uint8 -> the entropy-coded segment: what se_jpg_encode_u8 writes"""
    rows = blocks_of(a, quality)
    return b"".join(row_bytes(r, i, i == len(rows) - 1) for i, r in enumerate(rows))


def jpg_bound(hs, ws):
    """se_jpg_bound: rows x (2 ceil((1660 n + 7) / 8) + 2), n = 3 ceil(ws / 8) blocks a row; 0 for a side outside [16, 8192]"""
    if not (SIDE_MIN <= hs <= SIDE_MAX and SIDE_MIN <= ws <= SIDE_MAX):
        return 0
    n = 3 * -(-ws // 8)
    return -(-hs // 8) * (2 * ((BLOCK_BITS * n + 7) // 8) + 2)


def _segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def jpg_file(scan, h, w, quality):
    """rule 7: SOI, JFIF APP0, two DQT, SOF0, four DHT, DRI, SOS, the scan, EOI (restated; serve.jpg_from_scan is asserted against it)"""
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0")
    out += _segment(0xDB, [0] + quant_table(BASE_LUMA, quality)) + _segment(0xDB, [1] + quant_table(BASE_CHROMA, quality))
    out += _segment(0xC0, [8] + list(int(h).to_bytes(2, "big")) + list(int(w).to_bytes(2, "big")) + [3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
    for tc_th, (counts, symbols) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += _segment(0xC4, [tc_th] + counts + symbols)
    out += _segment(0xDD, (-(-int(w) // 8)).to_bytes(2, "big"))
    out += _segment(0xDA, [3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    return out + bytes(scan) + b"\xff\xd9"
