"""The preconditions of the exact data sets (tests/exact_util.py), on the CPU, for every row of forms_util.FORMS at its last
shape: an amplitude exists (1), the share compared exactly (2), the pre-activations are integers / multiples of 2^-12 / of the
gate granule below 2^23 (3), bf16 operands survive the round trip (4).  The makers assert them; this runs every maker."""
import numpy as np
import pytest

import exact_util as EU
import forms_util as FU

ROWS = EU.rows()
IDS = [FU.row_id(r, s) for r, s in ROWS]


def test_family_norms():
    """The infinity norms of the transforms as written in se_pack.hip and the kernels' comments."""
    assert EU.norms("direct") == (1, 1, 1)
    assert EU.norms("f23xf23") == (1.5 * 1.5, 2 * 2, 3 * 3)
    g, bt, at = EU.norms("f23xf43")
    assert (bt, at) == (2 * 10, 3 * 19) and abs(g - 1.5) < 1e-12
    assert EU.norms("f23x") == (1.5, 2, 3)
    g, bt, at = EU.norms("f25x")
    assert (bt, at) == (10, 7) and abs(g - 31 / 24) < 1e-12
    assert EU.norms("subpixel") == (4, 4, 4)
    assert [EU.grid(f) for f in ("direct", "f23xf23", "f23xf43", "f23x", "f25x", "subpixel")] == [24, 6, 0.5, 12, 1, 24]


def test_every_form_has_a_family_and_an_amplitude():
    amps = {}
    for r in FU.FORMS:
        assert FU.family(r.form) in EU.FAMILIES
        amps.setdefault((r.form, r.cin, r.src2), EU.amplitude(r))
    # the two-source hybrid rows are the only ones that need A = 1; the one-source hybrid rows A = 2
    assert {k for k, a in amps.items() if a == 1} == {("wino24_2src", 192, "tensor")}
    assert {k[0] for k, a in amps.items() if a == 2} == {"wino24"}
    assert amps[("wino24_c48", 48, None)] == 4


def test_w_rows_are_the_direct_fp32_forms():
    w = [r for r in FU.FORMS if EU.W_ROW(r)]
    assert all(FU.family(r.form) == "direct" and "bf16" not in r.mode and "bf16" not in r.form for r in w)
    forms = {r.form for r in w}
    assert {"rtile", "rtile_up2", "rtile_dense5", "small_conv", "gconv_n192", "gconv_n192_small_2src"} <= forms
    assert not any(f.startswith(("wino", "rtilew", "rconv")) or f == "rtile_dense5w" for f in forms)


@pytest.mark.parametrize("case", ROWS, ids=IDS)
def test_preconditions(case):
    r, shape = case
    for kind in EU.sets_of(r):
        d = EU.MAKE[kind](r, shape)                 # asserts preconditions 1-4
        assert d.x.dtype == np.float32 and d.w.dtype == np.float32 and d.b.dtype == np.float32
        assert d.x.shape[0] == FU.BATCH and not np.array_equal(d.x[0], d.x[1])
        if kind != "G" and r.act is not None:
            pos, neg = EU.shares(r, d)
            assert 0.90 <= pos <= 0.99 and neg >= 0.01, (kind, pos, neg)
        if kind == "G":
            assert EU.teeth_ratio(d.granule) >= 100


def test_bf16_rne_is_torch_rounding_and_half_a_spacing_is_up_to_2_pow_minus_8():
    import torch
    v = np.concatenate([np.linspace(3e-4, 1, 20001), [257, 259, 0.5 + 2.0 ** -9, 0.5 + 3 * 2.0 ** -9]])
    mine = EU.bf16_rne(v)
    assert np.array_equal(mine, torch.from_numpy(v.astype(np.float32)).to(torch.bfloat16).double().numpy())     # (float32 grid: exact)
    assert EU.bf16_rne(257.0) == 256 and EU.bf16_rne(259.0) == 260                                              # ties to even
    rel = np.abs(mine - v) / v
    assert 2.0 ** -9 < rel.max() <= 2.0 ** -8       # why the bf16 G comparison is an interval of bf16 values, not 2^-9 sigmoid(g)
    lo, hi = EU.g_interval(np.array([-8.0, -0.3, 0.0, 2.5, 8.0]), True)
    assert (lo <= hi).all() and ((hi - lo) / hi <= 2.0 ** -7).all()
