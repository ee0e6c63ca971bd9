"""The zlib stream of the device PNG encoder restated in plain Python ints and numpy, with no zlib in the encoder:
the yardstick of se_png_encode_u8, as tests/strokes_util.py is of the rasteriser.  Slow and literal on purpose.

The source is an hs x ws RGB rectangle (16 <= hs, ws <= 8192).
 1. filter: a row becomes 1 + 3 ws bytes, the filter type and the residuals.  SUB (1) subtracts the byte 3 to the left (or 0), UP
    (2) the byte above (or 0 on the rectangle's first row); the row takes the one with the smaller sum of |residual as int8|, a
    tie goes to SUB.
 2. stripes: 32 filtered rows (the last may have fewer), compressed independently.
 3. tokens: each maximal run of n equal bytes of a stripe is a literal, then for the remaining r = n - 1: while r >= 3 a match of
    length min(r, 258) at distance 1; then r literals.  End-of-block after the last token.
 4. code: Huffman lengths of the 286 literal/length symbols by removing the two smallest (weight, id) nodes, internal nodes taking
    ids 286, 287, ...; deeper than 15: every non-zero count c becomes (c + 1) >> 1 and the tree is built again.  Canonical codes
    (RFC 1951 3.2.2).  One distance code, 0, of length 1.
 5. block: BFINAL 0, BTYPE 2, HLIT 29, HDIST 0, HCLEN 15; code-length code: symbols 0-15 length 4, 16-18 length 0; the 287 lengths
    at 4 bits each; after end-of-block an empty stored block, so that a stripe ends on a byte.
 6. stream: 78 01, the stripes, 01 00 00 FF FF, Adler-32 of all filtered bytes, big-endian."""
import heapq

import numpy as np

STRIPE_ROWS = 32
MAX_MATCH = 258
NSYM = 286
EOB = 256
HEADER_BITS = 17 + 19 * 3 + 287 * 4          # 1222: 152.75 bytes, "153 header bytes"
CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
# RFC 1951 3.2.5: the base length and the extra bits of symbols 257 .. 285
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]


def filter_rows(a):
    """(hs, ws, 3) uint8 -> (hs, 1 + 3 ws) uint8: the filtered rows by rule 1"""
    a = np.asarray(a)
    assert a.ndim == 3 and a.shape[2] == 3 and a.dtype == np.uint8
    h, w = a.shape[:2]
    raw = a.reshape(h, 3 * w).astype(np.int64)
    left = np.zeros_like(raw)
    left[:, 3:] = raw[:, :-3]
    up = np.zeros_like(raw)
    up[1:] = raw[:-1]
    out = np.empty((h, 1 + 3 * w), np.uint8)
    for y in range(h):
        sub, upr = (raw[y] - left[y]) & 255, (raw[y] - up[y]) & 255
        cost = lambda r: int(np.where(r >= 128, 256 - r, r).sum())      # noqa: E731  |r read as int8|
        t, r = (1, sub) if cost(sub) <= cost(upr) else (2, upr)
        out[y, 0] = t
        out[y, 1:] = r
    return out


def stripes_of(filtered):
    """the stripes' bytes, in order"""
    return [filtered[y:y + STRIPE_ROWS].tobytes() for y in range(0, filtered.shape[0], STRIPE_ROWS)]


def tokens(d):
    """bytes of one stripe -> [("l", byte) | ("m", length)] by rule 3 (without end-of-block)"""
    t, i, n = [], 0, len(d)
    while i < n:
        j = i + 1
        while j < n and d[j] == d[i]:
            j += 1
        t.append(("l", d[i]))
        r = j - i - 1
        while r >= 3:
            m = min(r, MAX_MATCH)
            t.append(("m", m))
            r -= m
        t += [("l", d[i])] * r
        i = j
    return t


def length_symbol(m):
    """match length 3 .. 258 -> (symbol, extra value, extra bits)"""
    for i in range(28, -1, -1):
        if m >= LEN_BASE[i]:
            return 257 + i, m - LEN_BASE[i], LEN_EXTRA[i]
    raise ValueError(m)


def counts_of(toks):
    cnt = [0] * NSYM
    cnt[EOB] = 1
    for k, v in toks:
        cnt[v if k == "l" else length_symbol(v)[0]] += 1
    return cnt


def tree_lengths(cnt):
    """ONE tree by rule 4, not limited: the leaves' depths (0 for a count of 0)"""
    heap = [(c, i) for i, c in enumerate(cnt) if c > 0]
    heapq.heapify(heap)
    parent, nid = {}, len(cnt)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        parent[a[1]] = parent[b[1]] = nid
        heapq.heappush(heap, (a[0] + b[0], nid))
        nid += 1
    out = [0] * len(cnt)
    for i, c in enumerate(cnt):
        if c > 0:
            n = i
            while n in parent:
                n = parent[n]
                out[i] += 1
    return out


def code_lengths(cnt):
    """rule 4 with the limit: halve the counts, rounding up, until no code is longer than 15"""
    cnt = list(cnt)
    while True:
        L = tree_lengths(cnt)
        if max(L) <= 15:
            return L
        cnt = [(c + 1) >> 1 if c > 0 else 0 for c in cnt]


def canonical_codes(L):
    """RFC 1951 3.2.2"""
    code, out = 0, [0] * len(L)
    for bits in range(1, 16):
        for i, l in enumerate(L):
            if l == bits:
                out[i] = code
                code += 1
        code <<= 1
    return out


class BitWriter:
    """RFC 1951 3.1.1: data elements from the least significant bit of a byte on, Huffman codes from their most significant"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, nbits):
        assert 0 <= value < (1 << nbits) or nbits == 0
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def huff(self, code, nbits):
        self.put(int(format(code, "0%db" % nbits)[::-1], 2), nbits)

    def align(self):
        if self.n:
            self.out.append(self.acc & 255)
            self.acc, self.n = 0, 0


def stripe_bytes(d):
    """one stripe's bytes -> its deflate blocks (rule 5): starts and ends on a byte boundary"""
    toks = tokens(d)
    L = code_lengths(counts_of(toks))
    C = canonical_codes(L)
    bw = BitWriter()
    bw.put(0, 1), bw.put(2, 2), bw.put(NSYM - 257, 5), bw.put(0, 5), bw.put(15, 4)
    for s in CLEN_ORDER:
        bw.put(0 if s >= 16 else 4, 3)
    for l in L + [1]:
        bw.huff(l, 4)
    assert len(bw.out) * 8 + bw.n == HEADER_BITS
    for k, v in toks:
        if k == "l":
            bw.huff(C[v], L[v])
        else:
            s, e, nb = length_symbol(v)
            bw.huff(C[s], L[s])
            bw.put(e, nb)
            bw.put(0, 1)
    bw.huff(C[EOB], L[EOB])
    bw.put(0, 3)
    bw.align()
    bw.out += b"\x00\x00\xff\xff"
    return bytes(bw.out)


def adler32(data):
    """RFC 1950 8.2, in 64-bit-safe pieces"""
    a, b = 1, 0
    d = np.frombuffer(bytes(data), np.uint8).astype(np.int64)
    for i in range(0, len(d), 4096):
        blk = d[i:i + 4096]
        n = len(blk)
        b = (b + n * a + int((blk * np.arange(n, 0, -1)).sum())) % 65521
        a = (a + int(blk.sum())) % 65521
    return (b << 16) | a


def png_stream(a):
    """(hs, ws, 3) uint8 -> (zlib stream, filtered bytes)"""
    f = filter_rows(a)
    out = bytearray(b"\x78\x01")
    for d in stripes_of(f):
        out += stripe_bytes(d)
    out += b"\x01\x00\x00\xff\xff"
    out += adler32(f.tobytes()).to_bytes(4, "big")
    return bytes(out), f.tobytes()


def stripe_bound(n):
    """bytes of a stripe of n filtered bytes, at most: 1222 header bits, at most 15 bits per filtered byte, at most
    15 for end-of-block, 3 for the stored block's header, the padding to a byte and the stored block's 4 length bytes --
    ceil((1222 + 15 n + 18) / 8) + 4 = 159 + ceil(15 n / 8)"""
    return 159 + (15 * n + 7) // 8


def png_bound(hs, ws):
    """bytes of the stream of an hs x ws rectangle, at most: 2 + the stripes' bounds + 5 + 4"""
    row = 1 + 3 * ws
    full, rest = divmod(hs, STRIPE_ROWS)
    return 2 + full * stripe_bound(STRIPE_ROWS * row) + (stripe_bound(rest * row) if rest else 0) + 9
