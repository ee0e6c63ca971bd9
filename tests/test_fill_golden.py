"""Pin the fill fixture (tests/golden/fill_64.npz, made by tests/golden/make_golden_fill.py from the reference's own netG) to the
oracle: the definition of a fill is netG alone on hole = fill & ~lock.  CPU only."""
import os

import numpy as np
import pytest
import torch

from oracle import sketchedit_oracle as O
from sketchedit_amd import synth

TOL = 2e-6              # tests/test_oracle_golden.py's bound for netG at 64 x 64


@pytest.fixture(scope="module")
def fixture(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "fill_64.npz")))
    gain, _, iseed, B, H, W = g["meta"]
    img, sk = synth.make_inputs(int(B), int(H), int(W), seed=int(iseed))
    return g, img, sk, synth.make_state_dict("G", 0, float(gain))


def _maxdiff(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def test_fixture_is_the_definition_and_not_degenerate(fixture, golden_dir):
    g, img, _, _ = fixture
    hole = (g["fill"] > 0) & ~(g["lock"] > 0)
    assert np.array_equal(g["hole"], hole.astype(np.uint8))
    assert np.array_equal(g["lock"], np.load(os.path.join(golden_dir, "lock_64.npz"))["lock"])
    assert int(((g["fill"] > 0) & (g["lock"] > 0)).sum()) > 100          # the lock removes pixels from the fill
    assert 0.1 < hole.mean() < 0.9
    assert len(np.unique(g["fill"])) > 2 and not np.array_equal(g["fill"][0] > 0, g["fill"][1] > 0)
    # composed == where(hole, fine, image), exactly
    assert np.array_equal(g["composed"], np.where(hole[:, None], g["fine"], img))


def test_oracle_netG_reproduces_the_fixture(fixture):
    g, img, sk, WG = fixture
    hole = torch.from_numpy(g["hole"].astype(np.float32))[:, None]
    with torch.no_grad():
        coarse, fine = O.netG_forward(WG, img, img, hole, hole, sk)
    d = _maxdiff(coarse, g["coarse"]), _maxdiff(fine, g["fine"])
    print("oracle netG vs fill_64.npz: max |diff| coarse %.2e fine %.2e" % d)
    assert d[0] < TOL and d[1] < TOL
