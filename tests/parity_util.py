"""Shared by the GPU parity tests: the one-spacing rule of a bf16 layer (layer_close), and the composite the oracle gives FOR
THE HARD MASK THE GPU PIPELINE USED.

`mask_inpaint = (mask > 0.5)` (reference models/editline2_model.py:347) turns fp32 noise on a logit that sits on the
threshold into a different INPUT of netG.  Instead of skipping the composite comparison when a pixel flipped (a guard
that can pass vacuously), every test compares against this: the oracle's own composite when the hard masks agree,
otherwise the oracle's netG re-run on the GPU's hard mask and composited with the oracle's soft mask (:132)."""
import numpy as np
import torch


def _t(a):
    return a.detach().cpu().float() if hasattr(a, "detach") else torch.from_numpy(np.ascontiguousarray(a, np.float32))


def composed_for_hard_mask(O, WG, img, sk, ref_mask, ref_hard, ref_composed, gpu_hard, max_flips=2, **netg_kw):
    """-> (reference composite tensor, flips).  Fails when more than `max_flips` pixels thresholded differently."""
    gpu_hard, ref_hard = _t(gpu_hard), _t(ref_hard)
    flips = int((gpu_hard != ref_hard).sum())
    assert flips <= max_flips, "hard-mask flips: %d" % flips
    if flips == 0:
        return _t(ref_composed), 0
    img, sk, ref_mask = _t(img), _t(sk), _t(ref_mask)
    with torch.no_grad():
        _, fine = O.netG_forward(WG, img, img, gpu_hard, gpu_hard, sk, **netg_kw)
    return fine * ref_mask + img * (1 - ref_mask), flips


def layer_close(y, ref):
    """One bf16 layer (same bf16 inputs and weights, fp32 accumulation, ONE rounding of the result) against its reference: the
    two can differ by the accumulation order only, i.e. by at most one bf16 spacing of the result (2^-8 .. 2^-7 of |y|) where
    a value sits on a rounding boundary -- |d| <= 2^-7 |y| + 1e-6 on EVERY element -- and rarely: mean |d| < 2e-4
    (tests/test_gpu_bf16.py, "Tolerances")."""
    y = (y.detach().cpu().numpy() if hasattr(y, "detach") else np.asarray(y)).astype(np.float64)
    ref = (ref.detach().cpu().numpy() if hasattr(ref, "detach") else np.asarray(ref)).astype(np.float64)
    assert y.shape == ref.shape
    bad = np.abs(y - ref) > (2.0 ** -7) * np.abs(ref) + 1e-6
    assert not bad.any(), "%d of %d values off by more than one bf16 spacing, worst %.3e" % (
        bad.sum(), bad.size, np.abs(y - ref).max())
    # and the roundings are unbiased / rare: the mean difference is far below one spacing
    assert np.abs(y - ref).mean() < 2e-4 * max(1.0, np.abs(ref).mean())
