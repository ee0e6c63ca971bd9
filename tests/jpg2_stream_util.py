"""The stream of se_jpg2_encode_u8 / se_jpg2_code_i16 (include/sketchedit_jpg2.h) restated in plain Python ints: the
stream of tests/jpg_stream_util.py (rules 1 - 7, imported from there) with two independent options.  No Pillow and no libjpeg in
the encoder.  Slow and literal on purpose.

SE_JPG_420 (flag 1).  Sides are extended to a multiple of 16 by repeating the rectangle's last column and row (2'); Y stays at full
resolution, each Cb and Cr sample is (a + b + c + d + bias) >> 2 over its 2 x 2 pixels of the extended rectangle, bias = 1 + (x & 1)
with x the chroma sample's column (1''); one MCU is 16 x 16 pixels = Y(0,0), Y(0,1), Y(1,0), Y(1,1), Cb, Cr; the DC difference is
against the previous block of the same component in this order, 0 at the start of a restart interval; one restart interval is one
row of MCUs (6').
SE_JPG_OPTIMIZE (flag 2).  Four alphabets of 256 symbols (DC lum, AC lum, DC chr, AC chr), a symbol counted once for every time rule
5 emits its code over the whole image (5a); a 257th symbol of count 1; lengths by "remove the two smallest (weight, id)", a leaf's id
its symbol, internal nodes 257, 258, ...; while a length exceeds 16 every non-zero count c of the real symbols becomes (c + 1) >> 1
(5b); the real symbols with a non-zero count, sorted by (length, symbol), get Annex C's canonical codes (5c); the record of 4 x 272
bytes: per table the 16 counts of codes per length, then the symbols in code order, zero-padded to 256 (5e).
Clamp (the per-op entry takes any int16): an AC coefficient is clamped to -1023 .. 1023 and a DC DIFFERENCE to -2047 .. 2047 before
its size is taken; the predecessor of a DC is the neighbour's coefficient as it was given.  Neither does anything inside 6k's ranges."""
import heapq

import numpy as np

import jpg_stream_util as U

SE_JPG_420, SE_JPG_OPTIMIZE = 1, 2
TABLE_BYTES, RECORD_BYTES = 272, 4 * 272
BLOCK_BITS_OPT = 27 + 63 * 26                 # 1665: the most bits of one block under tables of 16-bit codes
AC_MAX, DC_DIFF_MAX = 1023, 2047


def mcu_side(flags):
    return 16 if flags & SE_JPG_420 else 8


def row_blocks(ws, flags):
    return 6 * -(-ws // 16) if flags & SE_JPG_420 else 3 * -(-ws // 8)


def block_bits(flags):
    return BLOCK_BITS_OPT if flags & SE_JPG_OPTIMIZE else U.BLOCK_BITS


def row_bound(nblk, flags):
    return 2 * ((block_bits(flags) * nblk + 7) // 8) + 2


def jpg2_bound(hs, ws, flags):
    """se_jpg2_bound; 0 for a side outside [16, 8192] or flags outside 0 .. 3"""
    if not (U.SIDE_MIN <= hs <= U.SIDE_MAX and U.SIDE_MIN <= ws <= U.SIDE_MAX) or flags not in (0, 1, 2, 3):
        return 0
    return -(-hs // mcu_side(flags)) * row_bound(row_blocks(ws, flags), flags)


def component(blk, flags):
    """the position of block `blk` of a row -> 0 for Y, 1 for Cb, 2 for Cr"""
    if flags & SE_JPG_420:
        return max(blk % 6 - 3, 0)
    return blk % 3


def downsample(plane, bias_of=lambda x: 1 + (x & 1)):
    """rule 1'': (H, W) -> (H / 2, W / 2); `bias_of` (chroma column -> bias) exists so that a test can show that the rule's matters"""
    p = np.asarray(plane, np.int64)
    s = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
    return (s + np.array([bias_of(x) for x in range(s.shape[1])], np.int64)[None, :]) >> 2


def dct_of(a, flags, **kw):
    """-> [row][blk] = s[v][u] of rule 3 in the order of the stream: rules 1 - 3 with 2' and 1'' (no quality enters yet)"""
    a = np.asarray(a)
    assert a.ndim == 3 and a.shape[2] == 3 and a.dtype == np.uint8
    h, w = a.shape[:2]
    m = mcu_side(flags)
    H, W = -(-h // m) * m, -(-w // m) * m
    a = a[np.minimum(np.arange(H), h - 1)][:, np.minimum(np.arange(W), w - 1)]       # rules 2 and 2'
    y, cb, cr = U.ycc(a)
    blk = lambda p, y0, x0: U.fdct(p[y0:y0 + 8, x0:x0 + 8].tolist())      # noqa: E731
    if not flags & SE_JPG_420:
        return [[blk(p, y0, x0) for x0 in range(0, W, 8) for p in (y, cb, cr)] for y0 in range(0, H, 8)]
    cb, cr = downsample(cb, **kw), downsample(cr, **kw)
    return [[b for mx in range(W // 16)
             for b in [blk(y, 16 * my + 8 * j, 16 * mx + 8 * i) for j in range(2) for i in range(2)] + [blk(cb, 8 * my, 8 * mx), blk(cr, 8 * my, 8 * mx)]]
            for my in range(H // 16)]


def quantised(dct, quality, flags):
    """dct_of's -> [row][blk] = 64 zigzag coefficients by rule 4"""
    qts = [U.quant_table(U.BASE_LUMA, quality), U.quant_table(U.BASE_CHROMA, quality)]
    return [[U.quantise(s, qts[1 if component(i, flags) else 0]) for i, s in enumerate(row)] for row in dct]


def blocks_of(a, quality, flags, **kw):
    """-> [row][blk] = 64 zigzag coefficients in the order of the stream, rules 1 - 4 with 2' and 1''"""
    return quantised(dct_of(a, flags, **kw), quality, flags)


def clamp(v, m):
    return min(max(int(v), -m), m)


def row_symbols(row, flags):
    """one row of blocks -> [(table 0 .. 3, [symbols], magnitude value, magnitude bits)] per emitted token, in stream order: the
    DC, then per non-zero AC coefficient its ZRLs and its (run, size), then EOB.  Tables: DC lum, AC lum, DC chr, AC chr."""
    out = []
    for i, coef in enumerate(row):
        comp = component(i, flags)
        tb = 0 if comp == 0 else 2
        if flags & SE_JPG_420:
            back = (3 if i % 6 == 0 else 1) if comp == 0 else 6
        else:
            back = 3
        pred = int(row[i - back][0]) if i - back >= 0 else 0
        size, bits = U.magnitude(clamp(int(coef[0]) - pred, DC_DIFF_MAX))
        out.append((tb, [size], bits, size))
        run = 0
        for k in range(1, 64):
            if coef[k] == 0:
                run += 1
                continue
            size, bits = U.magnitude(clamp(coef[k], AC_MAX))
            out.append((tb + 1, [U.ZRL] * (run >> 4) + [((run & 15) << 4) | size], bits, size))
            run = 0
        if coef[63] == 0:
            out.append((tb + 1, [U.EOB], 0, 0))
    return out


def histograms(rows, flags):
    """rule 5a: four lists of 256 counts"""
    h = [[0] * 256 for _ in range(4)]
    for row in rows:
        for tb, syms, _, _ in row_symbols(row, flags):
            for s in syms:
                h[tb][s] += 1
    return h


def tree_depths(counts):
    """257 counts (symbol 256 included) -> {symbol: depth} of the tree of "remove the two smallest (weight, id)"; no limit"""
    heap = [(c, s) for s, c in enumerate(counts) if c]
    heapq.heapify(heap)
    parent, nxt = {}, len(counts)
    if len(heap) == 1:
        return {heap[0][1]: 0}
    while len(heap) > 1:
        (w0, i0), (w1, i1) = heapq.heappop(heap), heapq.heappop(heap)
        parent[i0] = parent[i1] = nxt
        heapq.heappush(heap, (w0 + w1, nxt))
        nxt += 1
    out = {}
    for s, c in enumerate(counts):
        if c:
            d, n = 0, s
            while n in parent:
                n, d = parent[n], d + 1
            out[s] = d
    return out


def huff_lengths(counts, limit=16):
    """rule 5b: 256 counts -> ({symbol: length} of the real symbols with a non-zero count, the number of halvings)"""
    counts, halvings = [int(c) for c in counts], 0
    assert len(counts) == 256 and min(counts) >= 0 and any(counts)
    while True:
        d = tree_depths(counts + [1])
        if limit is None or max(d.values()) <= limit:
            d.pop(256)
            return d, halvings
        counts, halvings = [(c + 1) >> 1 if c else 0 for c in counts], halvings + 1


def huff_table(counts, lengths=None):
    """rules 5b and 5c: 256 counts -> (the 16 counts of codes per length, the symbols in code order), as a DHT segment carries them
    (`lengths`: huff_lengths(counts)[0] where the caller has it already)"""
    lengths = huff_lengths(counts)[0] if lengths is None else lengths
    symbols = sorted(lengths, key=lambda s: (lengths[s], s))
    return [sum(1 for s in symbols if lengths[s] == n) for n in range(1, 17)], symbols


def table_record(tables):
    """rule 5e: four (counts, symbols) -> 1088 bytes"""
    return b"".join(bytes(c) + bytes(s) + bytes(256 - len(s)) for c, s in tables)


def tables_of_record(record):
    """the inverse of table_record: the true symbol counts come from the 16 counts"""
    out = []
    for t in range(4):
        part = bytes(record[t * TABLE_BYTES:(t + 1) * TABLE_BYTES])
        counts = list(part[:16])
        out.append((counts, list(part[16:16 + sum(counts)])))
    return out


ANNEX_K = (U.DC_LUMA, U.AC_LUMA, U.DC_CHROMA, U.AC_CHROMA)


def token_bits(token, codes):
    """one entry of row_symbols -> (value, nbits)"""
    tb, syms, bits, size = token
    value = nbits = 0
    for s in syms:
        c, n = codes[tb][s]
        value, nbits = (value << n) | c, nbits + n
    return (value << size) | bits, nbits + size


def rows_raw(coef, flags):
    """coef[row][blk][64] -> ([(a row's bytes before stuffing, the number of 1-bits that pad its last)], the four tables)"""
    rows = [[[int(v) for v in blk] for blk in row] for row in coef]
    assert flags in (0, 1, 2, 3) and all(len(r) == len(rows[0]) and len(r) % (6 if flags & SE_JPG_420 else 3) == 0 for r in rows)
    tables = [huff_table(h) for h in histograms(rows, flags)] if flags & SE_JPG_OPTIMIZE else ANNEX_K
    codes = [U.huff_codes(t) for t in tables]
    out = []
    for row in rows:
        bits = U._Bits()
        for token in row_symbols(row, flags):
            bits.put(*token_bits(token, codes))
        pad = -bits.n % 8
        bits.put((1 << pad) - 1, pad)
        out.append((bits.acc.to_bytes(bits.n // 8, "big"), pad))
    return out, tables


def jpg2_code(coef, flags):
    """coef[row][blk][64] (ints, any int16; zigzag order) -> (the segment, the table record or None): se_jpg2_code_i16"""
    raws, tables = rows_raw(coef, flags)
    out = bytearray()
    for r, (raw, _) in enumerate(raws):
        for v in raw:
            out.append(v)
            if v == 0xFF:
                out.append(0)
        if r < len(raws) - 1:
            out += bytes([0xFF, 0xD0 + r % 8])
    return bytes(out), (table_record(tables) if flags & SE_JPG_OPTIMIZE else None)


def jpg2_scan(a, quality, flags):
    """(hs, ws, 3) uint8 -> (the segment, the table record or None): what se_jpg2_encode_u8 writes"""
    return jpg2_code(blocks_of(a, quality, flags), flags)


def jpg2_file(scan, h, w, quality, flags=0, tables=None):
    """rule 7': the file around a segment; `tables` is the record of 5e, None for Annex K's (restated; serve.jpg_from_scan is
    asserted against it)"""
    seg = U._segment
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0")
    out += seg(0xDB, [0] + U.quant_table(U.BASE_LUMA, quality)) + seg(0xDB, [1] + U.quant_table(U.BASE_CHROMA, quality))
    ysamp = 0x22 if flags & SE_JPG_420 else 0x11
    out += seg(0xC0, [8] + list(int(h).to_bytes(2, "big")) + list(int(w).to_bytes(2, "big")) + [3, 1, ysamp, 0, 2, 0x11, 1, 3, 0x11, 1])
    for tc_th, (counts, symbols) in zip((0x00, 0x10, 0x01, 0x11), tables_of_record(tables) if tables is not None else ANNEX_K):
        out += seg(0xC4, [tc_th] + list(counts) + list(symbols))
    out += seg(0xDD, (-(-int(w) // mcu_side(flags))).to_bytes(2, "big"))
    out += seg(0xDA, [3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    return out + bytes(scan) + b"\xff\xd9"
