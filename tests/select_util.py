"""The selection by colour of DESIGN.md 6o (include/sketchedit_select.h) in plain numpy -- the statement the kernels of
se_select.hip and the sessions' select_similar / fill_similar are compared with, byte for byte -- and the test patterns."""
import numpy as np


def spec_similar(frame, seed, t):
    """similar[y, x] = max over c of |frame[y, x, c] - frame[seed, c]| <= t (bool)"""
    f = np.asarray(frame).astype(np.int32)
    return np.abs(f - f[seed[0], seed[1]]).max(axis=2) <= int(t)


def spec_flood(similar, seed):
    """the 4-connected component of `similar` that holds the seed: a masked 4-neighbour dilation repeated until nothing
    changes (diagonal neighbours do not connect; the border adds nothing)"""
    reached = np.zeros(similar.shape, bool)
    reached[seed[0], seed[1]] = True
    while True:
        near = reached.copy()
        near[1:] |= reached[:-1]
        near[:-1] |= reached[1:]
        near[:, 1:] |= reached[:, :-1]
        near[:, :-1] |= reached[:, 1:]
        near &= similar
        near[seed[0], seed[1]] = True
        if np.array_equal(near, reached):
            return reached
        reached = near


def spec_state(frame, seed, t, contiguous, flooded=True):
    """the state plane: 0 not similar, 1 similar and not reached, 255 reached.  flooded=False: as se_select_similar_u8 leaves
    it (the seed alone reached when `contiguous`)."""
    sim = spec_similar(frame, seed, t)
    sim[seed[0], seed[1]] = True
    if not contiguous:
        reached = sim
    elif flooded:
        reached = spec_flood(sim, seed)
    else:
        reached = np.zeros(sim.shape, bool)
        reached[seed[0], seed[1]] = True
    return np.where(reached, 255, np.where(sim, 1, 0)).astype(np.uint8)


def spec_grow(reached, r):
    """255 where a reached pixel lies within Chebyshev distance r inside the frame: 2r + 1 shifted ORs per axis"""
    reached = np.asarray(reached, bool)
    H, W = reached.shape
    rows = np.zeros((H, W), bool)
    for d in range(-r, r + 1):
        if abs(d) < W:
            rows[:, max(d, 0):W + min(d, 0)] |= reached[:, max(-d, 0):W + min(-d, 0)]
    out = np.zeros((H, W), bool)
    for d in range(-r, r + 1):
        if abs(d) < H:
            out[max(d, 0):H + min(d, 0)] |= rows[max(-d, 0):H + min(-d, 0)]
    return np.where(out, 255, 0).astype(np.uint8)


def spec_select(frame, seed, t, contiguous, grow):
    """the whole definition: frame (Hi,Wi,3) uint8, seed (y, x) -> the (Hi,Wi) uint8 fill plane of 0 / 255"""
    return spec_grow(spec_state(frame, seed, t, contiguous) == 255, grow)


def spec_box_count(plane):
    """(tight half-open box (y0, x0, y1, x1), count) of plane > 0"""
    ys, xs = np.nonzero(plane)
    return (int(ys.min()), int(xs.min()), int(ys.max()) + 1, int(xs.max()) + 1), int(ys.size)


# ---- patterns: each -> (frame (H,W,3) uint8, seed); the region is flat (128, 128, 128) on noise that is never within 40 of it ----
REGION = 128


def _noise(hw, seed=0):
    """noise whose every channel differs from REGION by more than 40 (values 0 .. 79 and 177 .. 255)"""
    rng = np.random.RandomState(seed)
    v = rng.randint(0, 159, tuple(hw) + (3,))
    return np.where(v < 80, v, v + 97).astype(np.uint8)


def serpentine(hw, seed=0):
    """A one-pixel corridor through noise: every other row is corridor from column 1 to W - 2, joined to the next corridor
    row by one pixel under it at alternating ends, so the path crosses every tile border once per corridor row.  The seed is the
    corridor's first pixel."""
    H, W = hw
    f = _noise(hw, seed)
    right = True
    for y in range(1, H - 1, 2):
        f[y, 1:W - 1] = REGION
        if y + 1 < H:
            f[y + 1, W - 2 if right else 1] = REGION
        right = not right
    return f, (1, 1)


def diagonal(hw, seed=0):
    """two blobs that touch only diagonally; the seed is in the first"""
    H, W = hw
    f = _noise(hw, seed)
    cy, cx = H // 2, W // 2
    f[cy - 5:cy, cx - 5:cx] = REGION
    f[cy:cy + 5, cx:cx + 5] = REGION
    return f, (cy - 3, cx - 3)


def two_components(hw, seed=0):
    """two similar blobs apart; the seed is in the first"""
    H, W = hw
    f = _noise(hw, seed)
    f[2:7, 2:8] = REGION
    f[H - 7:H - 2, W - 8:W - 2] = REGION
    return f, (4, 4)


def border_region(hw, seed=0):
    """a region that touches all four edges of the frame: a frame-wide ring and a cross; the seed is at the centre"""
    H, W = hw
    f = _noise(hw, seed)
    f[0], f[H - 1], f[:, 0], f[:, W - 1] = REGION, REGION, REGION, REGION
    f[H // 2], f[:, W // 2] = REGION, REGION
    return f, (H // 2, W // 2)


def blob_with_ramp(hw, seed=0):
    """a flat blob with a +-3 ramp inside it, on noise: the sessions' pattern; the seed is the blob's centre"""
    H, W = hw
    f = _noise(hw, seed)
    yy, xx = np.mgrid[0:H, 0:W]
    blob = (yy - H // 2) ** 2 * 4 + (xx - W // 2) ** 2 <= (min(H, W) // 3) ** 2 * 4
    ramp = (REGION + (xx % 7) - 3).astype(np.uint8)
    f[blob] = np.stack([ramp, ramp, np.full_like(ramp, REGION)], axis=2)[blob]
    return f, (H // 2, W // 2)
