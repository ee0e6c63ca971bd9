#!/usr/bin/env python3
"""Generate lock_64.npz: the REFERENCE's own netM and netG run through the definition of a locked forward

    mask, _      = netM(image, sketch)
    mask         = where(lock, 0, mask)
    hard         = (mask > 0.5)
    coarse, fine = netG(image, image, hard, hard, sketch)
    composed     = fine * mask + image * (1 - mask)

on the inputs and weights of e2e_64.npz (synth.make_inputs(2, 64, 64, seed=1234), procedural weights).  Runs only where the
reference is present; it is imported at run time exactly as make_golden.py imports it, and only the produced vectors are
committed.

    python tests/golden/make_golden_lock.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402  (puts the repository and the reference on sys.path, stubs cv2)
import torch  # noqa: E402

from sketchedit_amd import synth  # noqa: E402


def make_lock(B=2, H=64, W=64, seed=4321):
    """(B,H,W) uint8, non-zero = locked: a 20 x 24 rectangle, one full-height 1-pixel column and ~1 % scattered pixels per
    image; image 1 has them elsewhere than image 0, and other non-zero values (any non-zero byte locks)."""
    rng = np.random.RandomState(seed)
    lock = np.zeros((B, H, W), np.uint8)
    lock[0, 9:29, 30:54] = 255
    lock[0, :, 5] = 255
    lock[1, 37:57, 3:27] = 1
    lock[1, :, 58] = 128
    lock[rng.rand(B, H, W) < 0.01] = 255
    return lock


def main():
    gain = synth.DEFAULT_GAIN
    m = make_golden.build_reference(gain)
    img, sk = synth.make_inputs(2, 64, 64, seed=1234)
    img, sk = torch.from_numpy(img), torch.from_numpy(sk)
    lock = make_lock()
    lk = torch.from_numpy(lock > 0)[:, None]
    with torch.no_grad():
        soft, _ = m.netM(img, sk)
        mask = torch.where(lk, torch.zeros_like(soft), soft)
        hard = (mask > 0.5).float()
        coarse, fine = m.netG(img, img, hard, hard, sk)
        composed = fine * mask + img * (1 - mask)
    e2e = np.load(os.path.join(HERE, "e2e_64.npz"))
    # the unlocked values are e2e_64's (0 hard-mask flips there): locking only moves values to 0, away from the threshold
    assert np.array_equal(soft.numpy(), e2e["mask"]), "netM no longer reproduces e2e_64.npz"
    assert np.array_equal(hard.numpy(), e2e["hard_mask"] * (1 - lk.numpy())), "a lock moved a value across the threshold"
    assert torch.equal(composed[lk.expand(-1, 3, -1, -1)], img[lk.expand(-1, 3, -1, -1)]), "composed != image where locked"
    freed = int(((e2e["hard_mask"] > 0) & lk.numpy()).sum())
    print("locked %d px (%.1f %%), of which %d were inside the unlocked hard mask; hole fraction %.3f -> %.3f" % (
        int(lk.sum()), 100.0 * float(lk.float().mean()), freed, float(e2e["hard_mask"].mean()), float(hard.mean())))
    assert freed > 100, "degenerate fixture: the locks do not touch the hole"
    keep = dict(lock=lock, mask=mask.numpy(), hard_mask=hard.numpy(), composed=composed.numpy(), coarse=coarse.numpy(),
                fine=fine.numpy(), meta=np.array([gain, 0, 1234, 2, 64, 64], np.float64))
    path = os.path.join(HERE, "lock_64.npz")
    np.savez_compressed(path, **{k: (v if v.dtype in (np.uint8, np.float64) else v.astype(np.float32)) for k, v in keep.items()})
    print("lock_64.npz %.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
