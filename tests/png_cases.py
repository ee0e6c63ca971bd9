"""The inputs the PNG encoder's tests share: each case is (name, frames, requests) with frames = [(Hi,Wi,3) uint8
arrays] and requests = [(frame index, y0, x0)] of ONE rectangle size (hs, ws).  tests/test_png_host.py runs the statement
(tests/png_stream_util.py) over them and checks what each is there for; tests/test_gpu_png.py runs the kernels over the same."""
import numpy as np

import png_stream_util as U


def _from_residuals(res):
    """(h, 3 w) SUB residuals -> the (h, w, 3) image they are the SUB filter of"""
    h, n = res.shape
    raw = np.cumsum(res.reshape(h, n // 3, 3).astype(np.int64), axis=1) & 255
    return raw.astype(np.uint8)


def runs_image():
    """40 x 300: two stripes.  SUB residuals: 40 bytes of noise (so that UP, against another row's noise, loses), then runs of
    exactly 3, 4, 258, 259, 260, 261 and 517 equal small bytes.  Row 31 ends in 259 ones -- a run that ends ON the stripe
    boundary -- and row 32 goes on with ones, its type byte among them: the run STRADDLES the boundary and is cut there."""
    rng = np.random.RandomState(5)
    lengths = [3, 4, 258, 259, 260, 261, 517]
    h, n = 40, 900
    res = np.zeros((h, n), np.uint8)
    for y in range(h):
        row, k, val = list(rng.randint(0, 256, 40)), y, 2
        while len(row) < n:
            L = lengths[k % len(lengths)]
            k += 1
            val = 2 + (val - 2 + 1 + y) % 5            # 2 .. 6, never the previous run's value
            row += [val] * L
            row.append(250 + len(row) % 5)             # a separator that is no neighbour's value
        res[y] = row[:n]
    res[31, n - 259:] = 1
    res[31, n - 260] = 9
    res[32, :100] = 1
    res[32, 100:140] = rng.randint(0, 256, 40)
    return _from_residuals(res)


# counts of a 17-symbol ladder whose tree is a chain, depth 16: end-of-block is the first 1, the rows' 32 type bytes and two
# residuals of value 1 are the 34
_LADDER = [1, 2, 3, 5, 8, 13, 21, 2, 55, 89, 144, 233, 377, 610, 987]
_LADDER_VALUES = [2, 254, 3, 253, 4, 252, 5, 1, 251, 6, 250, 7, 249, 8, 248]


def ladder_image():
    """32 x 64, ONE stripe whose symbol counts follow a Fibonacci ladder (1, 1, 2, 3, 5, ... 987, then the rest): SUB residuals,
    the most frequent value 0 between the others in runs of at most 3, so that no match exists and the counts are the bytes'"""
    others = [v for v, c in zip(_LADDER_VALUES, _LADDER) for _ in range(c)]
    rng = np.random.RandomState(11)
    rng.shuffle(others)
    n = 32 * 192
    zeros = n - len(others)
    assert len(others) <= zeros <= 3 * len(others)
    extra = zeros - len(others)                        # gaps that hold two zeros, not one
    seq = []
    for i, v in enumerate(others):
        seq += [v, 0, 0] if i < extra else [v, 0]
    assert len(seq) == n
    return _from_residuals(np.array(seq, np.uint8).reshape(32, 192))


def cases():
    rng = np.random.RandomState(3)
    noise = lambda h, w: rng.randint(0, 256, (h, w, 3)).astype(np.uint8)      # noqa: E731
    smooth = lambda h, w: ((np.arange(h)[:, None, None] * 3 + np.arange(w)[None, :, None] * 2 + np.arange(3)[None, None, :] * 40
                            + rng.randint(0, 3, (h, w, 3))) & 255).astype(np.uint8)      # noqa: E731
    a, b = smooth(40, 45), noise(64, 70)
    return [
        ("16x16: one short stripe", [smooth(16, 16)], [(0, 0, 0)], (16, 16)),
        ("33x17: two stripes, the second a single row", [smooth(33, 17)], [(0, 0, 0)], (33, 17)),
        ("64x300 flat colour: every run longer than 258", [np.full((64, 300, 3), (9, 130, 255), np.uint8)], [(0, 0, 0)], (64, 300)),
        ("runs of 3, 4, 258 .. 261, 517, on and across the stripe boundary", [runs_image()], [(0, 0, 0)], (40, 300)),
        ("a Fibonacci ladder: the first tree is deeper than 15", [ladder_image()], [(0, 0, 0)], (32, 64)),
        ("noise", [noise(40, 50)], [(0, 0, 0)], (40, 50)),
        ("x0, y0 odd, a frame width that is no multiple of 4", [smooth(47, 53)], [(0, 3, 5)], (33, 41)),
        ("B = 3, windows of two frames of different sizes", [a, b], [(0, 1, 3), (1, 30, 40), (0, 17, 19)], (20, 24)),
    ]


def rectangle(frames, request, hw):
    f, y0, x0 = request
    return np.ascontiguousarray(frames[f][y0:y0 + hw[0], x0:x0 + hw[1]])


def match_lengths(a):
    """the match lengths the statement emits for a rectangle, per stripe"""
    return [[v for k, v in U.tokens(d) if k == "m"] for d in U.stripes_of(U.filter_rows(a))]
