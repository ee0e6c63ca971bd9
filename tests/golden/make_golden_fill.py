#!/usr/bin/env python3
"""Generate fill_64.npz: the REFERENCE's own netG run through the definition of a fill

    hole         = fill & ~lock
    coarse, fine = netG(image, image, hole, hole, sketch)
    composed     = fine * hole + image * (1 - hole)

on the inputs and weights of e2e_64.npz (synth.make_inputs(2, 64, 64, seed=1234), procedural weights) with
make_golden_lock.make_lock()'s plane as the lock.  netM never runs.  Runs only where the reference is present; it is imported at
run time exactly as make_golden.py imports it, and only the produced vectors are committed.

    python tests/golden/make_golden_fill.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402  (puts the repository and the reference on sys.path, stubs cv2)
import torch  # noqa: E402
from make_golden_lock import make_lock  # noqa: E402

from sketchedit_amd import synth  # noqa: E402


def make_fill(B=2, H=64, W=64, seed=8765):
    """(B,H,W) uint8, non-zero = fill: per image a rectangle, a brush-like blob (discs along a polyline) and ~1 % scattered
    pixels; image 1 has them elsewhere than image 0, and other non-zero values (any non-zero byte fills).  The rectangles
    overlap make_lock()'s, so the lock takes pixels out of the fill."""
    rng = np.random.RandomState(seed)
    fill = np.zeros((B, H, W), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]

    def brush(points, r):
        hit = np.zeros((H, W), bool)
        for (ax, ay), (bx, by) in zip(points[:-1], points[1:]):
            for t in np.linspace(0.0, 1.0, 33):
                hit |= (xx - (ax + t * (bx - ax))) ** 2 + (yy - (ay + t * (by - ay))) ** 2 <= r * r
        return hit

    fill[0, 14:40, 22:50] = 255
    fill[0][brush([(6, 50), (24, 58), (44, 47), (58, 56)], 4.5)] = 255
    fill[1, 30:52, 10:44] = 7
    fill[1][brush([(50, 8), (36, 20), (54, 30)], 5.5)] = 200
    fill[1][rng.rand(H, W) < 0.01] = 1
    fill[0][rng.rand(H, W) < 0.01] = 255
    return fill


def main():
    gain = synth.DEFAULT_GAIN
    m = make_golden.build_reference(gain)
    img, sk = synth.make_inputs(2, 64, 64, seed=1234)
    img, sk = torch.from_numpy(img), torch.from_numpy(sk)
    fill, lock = make_fill(), make_lock()
    hole_b = (fill > 0) & ~(lock > 0)
    hole = torch.from_numpy(hole_b.astype(np.float32))[:, None]
    with torch.no_grad():
        coarse, fine = m.netG(img, img, hole, hole, sk)
        composed = fine * hole + img * (1 - hole)
    assert torch.equal(composed, torch.where(hole > 0, fine, img)), "composed != where(hole, fine, image)"
    removed = int(((fill > 0) & (lock > 0)).sum())
    frac = float(hole_b.mean())
    print("fill %d px, of which the lock removes %d; hole fraction %.3f (per image %r)" % (
        int((fill > 0).sum()), removed, frac, [round(float(h.mean()), 3) for h in hole_b]))
    assert removed > 100, "degenerate fixture: the lock does not touch the fill"
    assert 0.1 < frac < 0.9, "degenerate fixture: hole fraction %.3f" % frac
    assert not np.array_equal(fill[0] > 0, fill[1] > 0)
    keep = dict(fill=fill, lock=lock, hole=hole_b.astype(np.uint8), coarse=coarse.numpy(), fine=fine.numpy(), composed=composed.numpy(),
                meta=np.array([gain, 0, 1234, 2, 64, 64], np.float64))
    path = os.path.join(HERE, "fill_64.npz")
    np.savez_compressed(path, **{k: (v if v.dtype in (np.uint8, np.float64) else v.astype(np.float32)) for k, v in keep.items()})
    print("fill_64.npz %.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
