"""The inputs the JPEG encoder's tests share: each case is (name, frames, requests, (hs, ws), quality) with frames =
[(Hi,Wi,3) uint8 arrays] and requests = [(frame index, y0, x0)] of ONE rectangle size.  tests/test_jpg_host.py runs the statement
(tests/jpg_stream_util.py) over them and checks what each is there for; tests/test_gpu_jpg.py runs the kernels over the same.
Each is a few KB: the statement is plain Python.

The row kernel (se_jpg.hip, jpg_rows_kernel: the one row kernel of every form of the encoder) walks a row of MCUs in tiles of 16
blocks, a wave per block.  A row of ws pixels has 3 ceil(ws / 8)
blocks, so every ws > 40 spans more than one tile; the wide case is 100 pixels = 13 MCUs = 39 blocks = two tiles and 7 blocks of a
third, and no tile boundary but the first falls between two MCUs."""
import numpy as np

ROW_TILE_BLOCKS = 16
# 128 + 520 e(y, x), e = basis function (7, 7) = 1/4 cos((2y+1) 7 pi/16) cos((2x+1) 7 pi/16), rounded: at quality 100 (q = 1) its DC
# and AC coefficients 1 .. 62 are 0 and coefficient 63 is 520 (size 10) -- 62 zeros in front of a size-10 value: three ZRL, the
# 16-bit code of (14, 10) and 10 magnitude bits, the 59-bit token.  (Basis (7, 7)'s bare SIGN pattern does not do this: its
# projections on (1, 7), (7, 1), (3, 7) ... are not 0, fifteen other coefficients are non-zero at any amplitude.)
BASIS77 = np.array([[133, 114, 149, 103, 153, 107, 142, 123], [114, 168, 68, 199, 57, 188, 88, 142], [149, 68, 218, 22, 234, 38, 188, 107],
                    [103, 199, 22, 253, 3, 234, 58, 153], [153, 57, 234, 3, 253, 22, 199, 103], [107, 188, 38, 234, 22, 218, 68, 149],
                    [142, 88, 188, 58, 199, 68, 168, 114], [123, 142, 107, 153, 103, 149, 114, 133]], np.uint8)


def extremes_image():
    """16 x 32 grey (Cb = Cr = 128 exactly), for quality 100.  Row 0: white, black, white, black blocks: DC 1016, -1024, 1016,
    -1024, differences of 2040 in magnitude, size 11.  Row 1: black, white, then BASIS77 and its negative: coefficient 63 = 520
    and -520 behind 62 zeros."""
    g = np.zeros((16, 32), np.uint8)
    g[:8, 0:8] = g[:8, 16:24] = g[8:, 8:16] = 255
    g[8:, 16:24] = BASIS77
    g[8:, 24:32] = 256 - BASIS77.astype(np.int64)
    return np.repeat(g[:, :, None], 3, axis=2)


def cases():
    rng = np.random.RandomState(3)
    noise = lambda h, w: rng.randint(0, 256, (h, w, 3)).astype(np.uint8)      # noqa: E731
    smooth = lambda h, w: ((np.arange(h)[:, None, None] * 3 + np.arange(w)[None, :, None] * 2 + np.arange(3)[None, None, :] * 40
                            + rng.randint(0, 9, (h, w, 3))) & 255).astype(np.uint8)      # noqa: E731
    a, b = smooth(40, 45), noise(64, 70)
    return [
        ("16x16 flat colour: EOB only", [np.full((16, 16, 3), (9, 130, 255), np.uint8)], [(0, 0, 0)], (16, 16), 90),
        ("33x17 noise: partial blocks on both axes", [noise(33, 17)], [(0, 0, 0)], (33, 17), 50),
        ("80x16 noise: ten rows, the restart index wraps", [noise(80, 16)], [(0, 0, 0)], (80, 16), 1),
        ("16x32 extremes at quality 100: size-11 DC differences and the 59-bit token", [extremes_image()], [(0, 0, 0)], (16, 32), 100),
        ("16x100 noise at quality 100: a row of three tiles", [noise(16, 100)], [(0, 0, 0)], (16, 100), 100),
        ("24x16 noise at quality 100: stuffing and padding", [np.random.RandomState(PAD_SEED).randint(0, 256, (24, 16, 3)).astype(np.uint8)],
         [(0, 0, 0)], (24, 16), 100),
        ("x0, y0 odd in a frame of width 53", [smooth(47, 53)], [(0, 3, 5)], (33, 41), 90),
        ("B = 3, windows of two frames of different sizes", [a, b], [(0, 1, 3), (1, 30, 40), (0, 17, 19)], (20, 24), 50),
    ]


# the seed of the 24x16 case: the first whose statement has a row that ends in an FF byte completed by the 1-padding (so that
# FF 00 stands directly in front of a restart marker); tests/test_jpg_host.py asserts that it does
PAD_SEED = 4


def rectangle(frames, request, hw):
    f, y0, x0 = request
    return np.ascontiguousarray(frames[f][y0:y0 + hw[0], x0:x0 + hw[1]])


def by_name(prefix):
    (c,) = [c for c in cases() if c[0].startswith(prefix)]
    return c
