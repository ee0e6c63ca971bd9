"""The inputs the tests of the JPEG encoder with 4:2:0 sampling and per-image Huffman tables share, each with the
property it is there for.  tests/test_jpg2_host.py runs the statement (tests/jpg2_stream_util.py) over them and asserts each
property from the statement; tests/test_gpu_jpg2.py runs the kernels over the same.  These are the smallest inputs at which each
piece can still go wrong.

Through the encoder, cases() = (name, frames, requests, (hs, ws), qualities): frames = [(Hi,Wi,3) uint8], requests = [(frame index,
y0, x0)] of ONE rectangle size, run under flags 1, 2 and 3 at each of the qualities.

Through se_jpg2_code_i16, code_cases() = (name, build): build(flags) -> an int16 coefficient plane (1, R, nblk, 64) in the stream's
block order; each is run under flags 2 and 3 (the component pattern is blk % 3 and blk % 6), ALL_SYMBOLS also under 0 and 1 (every
code of Annex K's tables through the same entry).  A plane is made from three lists of blocks, one per component (plane())."""
import numpy as np

import jpg_cases
import jpg2_stream_util as U2

FLAGS = (1, 2, 3)
QUALITIES = (1, 50, 90, 100)
ROW_TILE_BLOCKS = 16
# the seeds of the stuffing case, by seed search on the CPU over 32 x 16 noise at quality 100: the first seed whose statement, under
# flags 2 AND under flags 3, has a stuffed FF 00 inside a row and a row that ends in an FF byte completed by the 1-padding (FF 00
# directly in front of a restart marker); tests/test_jpg2_host.py asserts that it does
PAD_SEED = 2


def bias_image():
    """16 x 16: one MCU under SE_JPG_420, 8 x 8 chroma samples.  R = G = 0 and B = 2 k gives Cb = 128 + k exactly, so the 2 x 2
    sum of Cb is 512 + the sum of four k.  Chroma sample (cy, cx) gets the four k = (j, 0, 0, 0), j = 1 + (cy % 3): sums of 1, 2
    and 3 mod 4 in every column, even and odd; rows 6 and 7 add 4 (cy + cx) to all four so that the plane is not periodic."""
    a = np.zeros((16, 16, 3), np.uint8)
    for cy in range(8):
        for cx in range(8):
            base = (cy + cx) if cy >= 6 else 0
            a[2 * cy:2 * cy + 2, 2 * cx:2 * cx + 2, 2] = 2 * base
            a[2 * cy, 2 * cx, 2] = 2 * (base + 1 + cy % 3)
    return a


def stuffing_image():
    return np.random.RandomState(PAD_SEED).randint(0, 256, (32, 16, 3)).astype(np.uint8)


def cases():
    rng = np.random.RandomState(5)
    noise = lambda h, w: rng.randint(0, 256, (h, w, 3)).astype(np.uint8)      # noqa: E731
    old = {c[0].split(":")[0]: c for c in jpg_cases.cases()}
    odd, many = old["x0, y0 odd in a frame of width 53"], old["B = 3, windows of two frames of different sizes"]
    return [
        ("16x16 flat grey 128: one MCU, DC 0 and EOB only, every optimised table the single code 0", [np.full((16, 16, 3), 128, np.uint8)],
         [(0, 0, 0)], (16, 16), QUALITIES),
        ("17x33 noise: partial MCUs on both axes, the replicated column and row enter the averages", [noise(17, 33)], [(0, 0, 0)], (17, 33),
         QUALITIES),
        ("144x16 noise: nine MCU rows under 420, all eight restart indices; 18 rows at 4:4:4, the index wraps twice", [noise(144, 16)],
         [(0, 0, 0)], (144, 16), QUALITIES),
        ("160x16 noise: ten MCU rows under 420, the marker after row 8 is D0 again", [noise(160, 16)], [(0, 0, 0)], (160, 16), (50,)),
        ("16x272 noise at quality 100: 102 blocks under 420, seven tiles, DC predecessors across tile boundaries", [noise(16, 272)],
         [(0, 0, 0)], (16, 272), (100,)),
        ("16x16 chroma sums of every residue mod 4 in even and odd columns: the bias", [bias_image()], [(0, 0, 0)], (16, 16), QUALITIES),
        ("32x16 noise at quality 100: stuffing and padding under optimised tables", [stuffing_image()], [(0, 0, 0)], (32, 16), (100,)),
        ("x0, y0 odd in a frame of width 53", odd[1], odd[2], odd[3], QUALITIES),
        ("B = 3, windows of two frames of different sizes", many[1], many[2], many[3], QUALITIES),
    ]


def rectangle(frames, request, hw):
    return jpg_cases.rectangle(frames, request, hw)


def by_name(prefix, which=None):
    (c,) = [c for c in (which or cases()) if c[0].startswith(prefix)]
    return c


# ---- coefficient planes for se_jpg2_code_i16 ---------------------------------------------------------------------------------------
def value_of(size, k=0):
    """a coefficient of `size` bits, its sign and low bits varying with k"""
    if size == 0:
        return 0
    v = (1 << (size - 1)) | (k * 37 & ((1 << (size - 1)) - 1))
    return -v if k & 1 else v


def block_of(dc, tokens):
    """dc and [(run, value)] -> 64 zigzag coefficients; the tokens must fit"""
    b, k = [0] * 64, 0
    b[0] = dc
    for run, value in tokens:
        k += run + 1
        assert k <= 63 and value != 0
        b[k] = value
    return b


def plane(ys, cbs, crs, flags, R=1):
    """three lists of blocks -> (1, R, nblk, 64) int16 in the stream's order, padded with zero blocks to whole MCUs and rows"""
    ny = 4 if flags & U2.SE_JPG_420 else 1
    m = max(-(-len(ys) // ny), len(cbs), len(crs), 1)
    m = -(-m // R) * R
    zero = [0] * 64
    ys, cbs, crs = (list(v) + [zero] * (n - len(v)) for v, n in ((ys, m * ny), (cbs, m), (crs, m)))
    out = []
    for i in range(m):
        out += ys[i * ny:(i + 1) * ny] + [cbs[i], crs[i]]
    return np.array(out, np.int16).reshape(1, R, -1, 64)


FIB = [1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584]           # 17 counts, 6763 in all
SKEW_BLOCKS = 144                                                                         # EOB's count: every block ends in one


def skew_blocks(counts, special):
    """SKEW_BLOCKS luminance blocks whose AC symbols have exactly the counts `counts` (a dict): every block ends in EOB, so
    counts[0x00] == SKEW_BLOCKS; with `special`, the first block's only non-zero AC coefficient is number 63 (three ZRL and the
    symbol (14, 10)), which accounts for ZRL's count 3 and (14, 10)'s count 1, and that block has no EOB."""
    counts = dict(counts)
    n_eob = SKEW_BLOCKS - (1 if special else 0)
    assert counts.pop(0x00) == n_eob
    first = []
    if special:
        assert counts.pop(0xF0) == 3 and counts.pop(0xEA) == 1
        first = [block_of(0, [(62, 513)])]
    flat = [s for s in sorted(counts, key=lambda s: (-counts[s], s)) for _ in range(counts[s])]
    blocks = []
    for i in range(n_eob):
        toks = [(s >> 4, value_of(s & 15, i + j)) for j, s in enumerate(flat[i::n_eob])]
        blocks.append(block_of(0, toks))
    return first + blocks


def fibonacci(flags):
    """luminance AC counts 1, 2, 3, 5, 8, ..., 2584 over 17 symbols: with the extra leaf of weight 1 the first tree is 17 deep, and
    the counts are halved.  (Plain Fibonacci counts 1, 1, 2, 3, ... do not do it: the extra leaf splits the chain.)  EOB has the
    count 144; the six smallest counts go to symbols of run 1, the others to run 0, so a block holds its share of the 6619 tokens."""
    small = [0x11, 0x12, 0x13, 0x14, 0x15, 0x16]
    large = [0x01, 0x02, 0x03, 0x04, 0x05, 0x06, 0x07, 0x08, 0x09, 0x0A]
    rest = [c for c in FIB if c != SKEW_BLOCKS]
    counts = dict(zip(small + large, rest))
    counts[0x00] = SKEW_BLOCKS
    return plane(skew_blocks(counts, False), [], [], flags, R=4)


def long_token(flags):
    """a block whose only non-zero AC coefficient is number 63, among blocks that make ZRL's code at least 13 bits: the lane's token
    (three ZRL, the code of (14, 10), 10 magnitude bits) is longer than 64 bits.  Counts: (14, 10) 1, ZRL 3, then 5, 8, ... as above
    with EOB at 143 (the special block has none)."""
    small = [0x11, 0x12, 0x13, 0x14]
    large = [0x01, 0x02, 0x03, 0x04, 0x05, 0x06, 0x07, 0x08, 0x09, 0x0A]
    rest = [c for c in FIB if c not in (1, 2, 3, SKEW_BLOCKS)]
    counts = dict(zip(small + large, rest))
    counts.update({0x00: SKEW_BLOCKS - 1, 0xF0: 3, 0xEA: 1})
    return plane(skew_blocks(counts, True), [], [], flags, R=4)


def dc_chain():
    """12 DC values whose differences (the first against 0) have the sizes 0 .. 11, all inside -1024 .. 1016"""
    out, dc = [], 0
    for size in range(12):
        dc += value_of(size, size)
        out.append(dc)
    assert min(out) >= -1024 and max(out) <= 1016
    return out


def all_symbol_blocks():
    """blocks that hold every AC symbol (run 0 .. 15) x (size 1 .. 10), ZRL and EOB, and the 12 DC sizes"""
    toks = [(r, value_of(s, r + s)) for r in range(16) for s in range(1, 11)]
    blocks, cur, used = [], [], 0
    for t in toks + [(33, 5)]:                                           # (and a run of 33: two ZRL)
        if used + t[0] + 1 > 62:                                         # (coefficient 63 stays zero: every block ends in EOB)
            blocks.append(cur)
            cur, used = [], 0
        cur.append(t)
        used += t[0] + 1
    blocks.append(cur)
    dcs = dc_chain()
    assert len(blocks) >= len(dcs)
    return [block_of(dcs[i] if i < len(dcs) else dcs[-1], b) for i, b in enumerate(blocks)]


def all_symbols(flags):
    """every one of the 162 AC symbols and the 12 DC sizes, in the luminance and in the chrominance tables; one row, so each
    component's DC chain is unbroken"""
    b = all_symbol_blocks()
    return plane(b, b, b[::-1], flags)


def dc_extremes(flags):
    """DC -1024 and 1016 in neighbouring blocks of every component: differences of +-2040, size 11, next to AC +-1021"""
    b = [block_of(-1024 if i & 1 else 1016, [(0, 1021), (5, -1021)]) for i in range(8)]
    return plane(b, b[:2], b[1:3], flags)


def ties(flags):
    """40 AC symbols with the count 3 each, in both classes: the tree is decided by the ids alone"""
    syms = [(r << 4) | s for r in range(4) for s in range(1, 11)]
    blocks = [block_of(7 * i, [(s >> 4, value_of(s & 15, i)) for s in syms[k:k + 10]]) for i in range(3) for k in range(0, 40, 10)]
    return plane(blocks, blocks, blocks, flags, R=2)


def out_of_range(flags):
    """what only the per-op entry can be given: AC 32767, -32768, 1024, -1024 (clamped to +-1023) and DC 32767 next to -32768
    (differences of +-65535, clamped to +-2047)"""
    b = [block_of(32767 if i & 1 else -32768, [(0, 32767), (1, -32768), (2, 1024), (3, -1024), (4, 1023)]) for i in range(6)]
    return plane(b, b, b, flags)


def clamped(p):
    """a plane with its AC coefficients clamped (the DC differences are the statement's business)"""
    q = np.clip(p, -U2.AC_MAX, U2.AC_MAX)
    q[..., 0] = p[..., 0]
    return q


def code_cases():
    return [("fibonacci", fibonacci), ("long_token", long_token), ("all_symbols", all_symbols), ("dc_extremes", dc_extremes), ("ties", ties),
            ("out_of_range", out_of_range)]


def code_flags(name):
    return (0, 1, 2, 3) if name == "all_symbols" else (2, 3)
