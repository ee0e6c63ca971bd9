"""CPU self-test of tests/feather_util.py, the numpy statement of the feathered paste's rule: the consequences the
rule names, and its box count against plain loops over the definition."""
import numpy as np
import pytest

import feather_util as FU


def _case(seed, Hi, Wi, y0, x0, hs, ws, density=0.5, lock_density=0.0):
    rng = np.random.default_rng(seed)
    frame = rng.integers(0, 256, (Hi, Wi, 3), dtype=np.uint8)
    rgb = rng.integers(0, 256, (hs, ws, 3), dtype=np.uint8)
    mask = np.where(rng.random((hs, ws)) < density, rng.choice(np.array([1, 128, 255], np.uint8), (hs, ws)), np.uint8(0)).astype(np.uint8)
    lock = (rng.random((Hi, Wi)) < lock_density).astype(np.uint8) * 255 if lock_density else None
    return frame, (y0, x0), rgb, mask, lock


def _count_by_definition(sel, origin, frame_hw, r):
    """c by the rule's words: a loop over every sample of every box"""
    hs, ws = sel.shape
    (y0, x0), (Hi, Wi) = origin, frame_hw
    c = np.zeros((hs, ws), np.int64)
    for y in range(hs):
        for x in range(ws):
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    yy, xx = y + dy, x + dx
                    if (yy < 0 and y0 != 0) or (yy >= hs and y0 + hs != Hi) or (xx < 0 and x0 != 0) or (xx >= ws and x0 + ws != Wi):
                        continue
                    c[y, x] += sel[min(max(yy, 0), hs - 1), min(max(xx, 0), ws - 1)]
    return c


@pytest.mark.parametrize("origin,frame_hw", [((3, 5), (40, 40)), ((0, 0), (40, 40)), ((24, 20), (40, 40)), ((0, 20), (16, 40)), ((0, 0), (16, 20))])
@pytest.mark.parametrize("r", [1, 3, 16])
def test_count_is_the_definition(origin, frame_hw, r):
    sel = np.random.default_rng(r).random((16, 20)) < 0.6
    got = FU.box_count(FU.padded_selection(sel, origin, frame_hw, r), r)
    assert np.array_equal(got, _count_by_definition(sel, origin, frame_hw, r))


def test_radius_0_is_the_hard_paste():
    frame, origin, rgb, mask, lock = _case(1, 50, 61, 7, 9, 17, 23, lock_density=0.3)
    for lk in (None, lock):
        sel = FU.selection(mask, lk, origin, frame.shape[:2])
        want = frame.copy()
        want[7:24, 9:32] = np.where(sel[:, :, None], rgb, frame[7:24, 9:32])
        assert np.array_equal(FU.feather_paste(frame, origin, rgb, mask, 0, lock=lk), want)


@pytest.mark.parametrize("r", [1, 7, 16])
def test_all_selected_flush_with_all_edges_is_rgb(r):
    frame, origin, rgb, _, _ = _case(2, 16, 24, 0, 0, 16, 24)
    out = FU.feather_paste(frame, origin, rgb, np.full((16, 24), 255, np.uint8), r)
    assert np.array_equal(out, rgb)


@pytest.mark.parametrize("r", [1, 2, 16])
def test_single_pixel(r):
    frame, origin, rgb, _, _ = _case(3, 60, 60, 11, 13, 24, 32)
    mask = np.zeros((24, 32), np.uint8)
    mask[10, 17] = 1
    out = FU.feather_paste(frame, origin, rgb, mask, r)
    n = (2 * r + 1) ** 2
    want = frame.copy()
    want[21, 30] = (rgb[10, 17].astype(np.int64) + (n - 1) * frame[21, 30].astype(np.int64) + (n - 1) // 2) // n
    assert np.array_equal(out, want)


@pytest.mark.parametrize("r", [0, 2, 16])
def test_unselected_bytes_keep_their_values(r):
    frame, origin, rgb, mask, lock = _case(4, 48, 52, 5, 0, 33, 37, density=0.4, lock_density=0.3)
    out = FU.feather_paste(frame, origin, rgb, mask, r, lock=lock)
    sel = np.zeros(frame.shape[:2], bool)
    sel[5:38, 0:37] = FU.selection(mask, lock, origin, frame.shape[:2])
    assert sel.any() and np.array_equal(out[~sel], frame[~sel])
    assert np.array_equal(out[lock > 0], frame[lock > 0])
    assert not np.array_equal(out[sel], frame[sel])


def test_fades_towards_an_inner_side_and_not_towards_the_frames_edge():
    frame = np.zeros((40, 40, 3), np.uint8)
    rgb = np.full((16, 16, 3), 255, np.uint8)
    full = np.full((16, 16), 255, np.uint8)
    out = FU.feather_paste(frame, (0, 12), rgb, full, 2)          # the top side is the frame's edge, the others are not
    assert (out[0:8, 18:22] == 255).all()                         # no fade towards the top
    assert out[8, 12, 0] < out[8, 13, 0] < out[8, 14, 0] == 255   # fades towards the window's left side
    assert out[15, 20, 0] < out[14, 20, 0] < out[13, 20, 0] == 255
