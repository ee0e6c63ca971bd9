"""Every kernel form of a gated convolution on inputs where its arithmetic is exact (tests/exact_util.py): the
result must equal the float64 reference BIT FOR BIT wherever the feature pre-activation is positive -- no tolerance for a cut
transform constant, a narrowed operand, a dropped split term, a truncating bf16 store or an off weight at a ragged tile edge
to hide in --, and the live gate must sit within the rounding error of the hardware transcendentals.

Every row of forms_util.FORMS at its last shape (the ragged multi-tile one), under its own form name: the conv launches are
asserted first, as in test_gpu_forms, so that exactness is shown for the named form and not for a fallback.
  F, W: f > 0: got == want bit for bit (bf16 mode: the bf16-rounded values).  f <= 0: ReLU: got == 0; ELU: |got - (e^f - 1)|
        <= 3e-7 (one v_exp_f32 of a value <= 1, the argument rounding, one subtraction; se_device.h: ~1e-7 absolute per
        transcendental), in bf16 mode plus half a bf16 spacing, 2^-9 |want|.  act None: the whole output bit for bit.
  G:    |got - sigmoid(g)| <= (|g| + 8) 2^-24 sigmoid(g) (exact_util.g_bound); in bf16 mode got is the round-to-nearest-even
        bf16 value of a number within that bound (exact_util.g_interval): mostly one value is allowed.
"""
import numpy as np
import pytest

import exact_util as EU
import forms_util as FU

pytestmark = pytest.mark.gpu

ELU_NEG_TOL = 3e-7


@pytest.fixture(scope="module")
def eng():
    from sketchedit_amd._lib import Engine
    e = Engine(0)
    yield e
    e.close()


def _launch(eng, r, shape, d, seopt):
    for name, v in r.switches.items():
        seopt.set(name, v)
    y, launches = FU.run(eng, r, d.x, d.x1, d.w, d.b)
    assert FU.conv_launches(launches) == list(r.pre) + [r.form], (FU.row_id(r, shape), launches)
    got = y.detach().cpu().numpy()
    assert got.dtype == np.float32
    return got


def _ulps(a, b):
    """distance in units in the last place of float32 (bf16 values: of their float32 image)"""
    def key(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def _require_equal(rid, got, want, mask, what):
    """got == want bit for bit on `mask`; on failure the row, the count, the first few elements and the worst ulp distance."""
    want32 = want.astype(np.float32)
    assert (want32.astype(np.float64) == want)[mask].all(), rid       # the reference itself is a float32 value there
    if np.array_equal(got[mask], want32[mask]):
        return
    bad = np.argwhere(mask & (got != want32))
    u = _ulps(got, want32)[mask]
    lines = ["%s %s: %d of %d elements differ, worst %d ulp" % (rid, what, len(bad), int(mask.sum()), int(u.max()))]
    for b_, c, y, x in bad[:8]:
        lines.append("  (b %d, c %d, y %d, x %d) got %r want %r" % (b_, c, y, x, float(got[b_, c, y, x]), float(want32[b_, c, y, x])))
    pytest.fail("\n".join(lines))


def _require_within(rid, got, want, tol, mask, what):
    err = np.abs(got.astype(np.float64) - want)
    over = mask & (err > tol)
    if not over.any():
        return
    bad = np.argwhere(over)
    lines = ["%s %s: %d of %d elements outside the bound, worst excess over it %.3g" %
             (rid, what, len(bad), int(mask.sum()), float((err - tol)[mask].max()))]
    for b_, c, y, x in bad[:8]:
        lines.append("  (b %d, c %d, y %d, x %d) got %r want %r bound %.3g" %
                     (b_, c, y, x, float(got[b_, c, y, x]), float(want[b_, c, y, x]), float(tol[b_, c, y, x])))
    pytest.fail("\n".join(lines))


def _check_features(r, shape, d, got):
    rid = FU.row_id(r, shape) + " " + d.kind
    bf = r.mode.startswith("bf16")
    want = FU.reference(r, d.x, d.x1, d.w, d.b).numpy()
    assert got.shape == want.shape, (rid, got.shape, want.shape)
    if r.act is None:
        _require_equal(rid, got, want, np.ones(want.shape, bool), "raw output")
        return
    f = EU.preact(r, d.x, d.x1, d.w, d.b)[:, : r.cout // 2]
    pos = f > 0
    share = float(pos.mean())
    print("%s: A %d, %.1f %% of %d outputs compared bit for bit" % (rid, d.A, 100 * share, pos.size))
    assert share >= 0.90
    _require_equal(rid, got, want, pos, "f > 0")
    if r.act == "relu":
        _require_equal(rid, got, np.zeros_like(want), ~pos, "f <= 0 (relu)")
    else:
        neg = np.expm1(np.minimum(f, 0.0))
        tol = ELU_NEG_TOL + (2.0 ** -9 * np.abs(want) if bf else 0.0) + np.zeros_like(want)
        _require_within(rid, got, neg, tol, ~pos, "f <= 0 (elu)")


def _check_gates(r, shape, d, got):
    rid = FU.row_id(r, shape) + " G"
    bf = r.mode.startswith("bf16")
    g = EU.preact(r, d.x, d.x1, d.w, d.b)[:, r.cout // 2:]
    want = 1.0 / (1.0 + np.exp(-g))
    assert got.shape == want.shape, (rid, got.shape, want.shape)
    lo, hi = EU.g_interval(g, bf)
    # the distance to the allowed interval is compared with 0; the printed figure is the fp32 error over its bound (bf16: the
    # share of outputs at which two bf16 values are allowed)
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    if bf:
        print("%s: A %d, s %d, two bf16 values allowed at %.2f %% of the outputs" % (rid, d.A, d.s, 100 * float((hi > lo).mean())))
    else:
        print("%s: A %d, s %d, worst error / bound %.3f" % (rid, d.A, d.s, float((np.abs(got - want) / half).max())))
    _require_within(rid, got, mid, half, np.ones(want.shape, bool), "sigmoid(g)")


ROWS = EU.rows()
CASES = [(r, s, kind) for r, s in ROWS for kind in EU.sets_of(r)]


@pytest.mark.parametrize("case", CASES, ids=["%s-%s" % (FU.row_id(r, s), kind) for r, s, kind in CASES])
def test_form_is_exact(eng, case, seopt):
    r, shape, kind = case
    d = EU.MAKE[kind](r, shape)
    got = _launch(eng, r, shape, d, seopt)
    if kind == "G":
        _check_gates(r, shape, d, got)
    else:
        _check_features(r, shape, d, got)


BATCH_ROWS = [FU.row("wino24", 96, 192, [(10, 20)]), FU.row("rtile_bf16", 24, 24, [(33, 17)], mode="bf16")]


@pytest.mark.parametrize("r", BATCH_ROWS, ids=[FU.row_id(r) for r in BATCH_ROWS])
def test_batch_of_three_equals_three_single_images(eng, r, seopt):
    """The F result of B = 3 equals, bit for bit, the three B = 1 results (and the reference, as above)."""
    shape = r.shapes[-1]
    d = EU.make_F(r, shape, B=3)
    got = _launch(eng, r, shape, d, seopt)
    _check_features(r, shape, d, got)
    for i in range(3):
        one = _launch(eng, r, shape, d._replace(x=d.x[i:i + 1]), seopt)
        assert np.array_equal(one[0].view(np.int32), got[i].view(np.int32)), (FU.row_id(r, shape), i)
