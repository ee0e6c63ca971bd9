"""The sampled-pixel attention reference (tests/att_sample_util.py) against the oracle's full contextual attention, on the
CPU: the large-image GPU tests (test_gpu_large_images.py) rest on it."""
import numpy as np
import pytest
import torch

from att_sample_util import gather_pixels, sample_pixels, sampled_attention
from oracle import sketchedit_oracle as O
from sketchedit_amd import synth


def _masks(B, h, w, kind):
    if kind == "all-invalid":
        return np.ones((B, 1, 4 * h, 4 * w), np.float32)
    full = (synth.uniform(3, "asu.m%dx%d" % (h, w), (B, 1, 4 * h, 4 * w), 0, 1) < 0.5).astype(np.float32)
    full[0, :, :, 2 * w:] = 1.0                                  # a hole: invalid keys next to valid ones
    return full


@pytest.mark.parametrize("regime", ["soft", "saturated"])
@pytest.mark.parametrize("mask", ["mixed", "all-invalid"])
@pytest.mark.parametrize("shape", [(2, 16, 16), (1, 24, 40), (1, 40, 72)], ids=lambda s: "%dx%dx%d" % s)
def test_sampled_reference_matches_oracle(shape, mask, regime):
    B, h, w = shape
    x = synth.uniform(2, "asu.x%dx%d" % (h, w), (B, 96, h, w), -1, 1)
    if regime == "soft":
        x = 0.004 * x
    full = _masks(B, h, w, mask)
    pix = sample_pixels(B, h, w, 200, seed=1)
    got = sampled_attention(x, full, pix)
    # the oracle's own arithmetic run in float64 (the helper sums in float64): the same function, to 1e-6 relative ...
    ref64, _ = O.contextual_attention(torch.from_numpy(x).double(), torch.from_numpy(full).double())
    want = gather_pixels(ref64.double(), pix)
    scale = float(want.abs().max())
    assert float((got.double() - want.double()).abs().max()) <= 1e-6 * scale
    # ... and the oracle as it runs (fp32), within its own rounding (measured up to 4e-6 relative in the saturated regime)
    ref, _ = O.contextual_attention(torch.from_numpy(x), torch.from_numpy(full))
    assert float((got - gather_pixels(ref, pix)).abs().max()) <= 1e-5 * scale


def test_sampled_reference_bf16_rounding():
    """With dt = bfloat16 the helper rounds where the oracle does (keys, P, the output)."""
    B, h, w = 1, 24, 40
    x = 0.004 * synth.uniform(2, "asu.xb", (B, 96, h, w), -1, 1)
    full = _masks(B, h, w, "mixed")
    xb = torch.from_numpy(x).to(torch.bfloat16).float()
    ref, _ = O.contextual_attention(xb, torch.from_numpy(full), torch.bfloat16)
    pix = sample_pixels(B, h, w, 100, seed=2)
    got = sampled_attention(xb, full, pix, dt=torch.bfloat16)
    want = gather_pixels(ref, pix)
    assert float((got - want).abs().max()) <= 2.0 ** -8 * float(want.abs().max())


def test_sample_pixels_cover_edges():
    pix = sample_pixels(2, 40, 72, 300, seed=0)
    assert len(pix) >= 300 and len(np.unique(pix, axis=0)) == len(pix)
    for b in (0, 1):
        p = pix[pix[:, 0] == b]
        assert {0, 39} <= set(p[:, 1].tolist()) and {0, 71} <= set(p[:, 2].tolist())


@pytest.mark.parametrize("regime", ["soft", "saturated"])
@pytest.mark.parametrize("shape,rows", [((2, 16, 16), 3), ((1, 24, 40), 8), ((1, 40, 72), 5)], ids=["16x16", "24x40", "40x72"])
def test_chunked_attention_matches_oracle(shape, rows, regime):
    """contextual_attention_chunked (the query-chunked restatement the 1080p end-to-end test runs inside the oracle) against
    the oracle's own contextual_attention, fp32: the same function up to summation order."""
    from att_sample_util import contextual_attention_chunked
    B, h, w = shape
    x = synth.uniform(2, "asc.x%dx%d" % (h, w), (B, 96, h, w), -1, 1)
    if regime == "soft":
        x = 0.004 * x
    full = _masks(B, h, w, "mixed")
    ref, _ = O.contextual_attention(torch.from_numpy(x), torch.from_numpy(full))
    got, sim = contextual_attention_chunked(torch.from_numpy(x), torch.from_numpy(full), rows=rows)
    assert sim is None and got.shape == ref.shape
    assert float((got - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
