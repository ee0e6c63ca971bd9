"""The polyphase F(2,2) form of the 48-channel stride-2 gated convs ("s2poly48", sketchedit_amd/csrc/se_s2poly.hip)
on the GPU, through Engine.gated_conv2d: 48 -> 96 and 48 -> 192 (two 96-row halves of one launch), at
    (4, 4), B = 8   one tile per image; every source of the first row and column is padding
    (8, 12)         2 x 3 tiles per image
    (12, 20), B = 3 45 tiles: one ragged 64-tile workgroup
    (36, 28), B = 2 126 tiles: two workgroups, the second ragged, tiles of one workgroup on both sides of the image seam
against the oracle's conv and against the gather-GEMM (SE_S2_POLY=0) at the per-op bound of the Winograd rows (1e-4), on the
exact sets of tests/exact_util.py bit for bit against the float64 reference (as tests/test_gpu_exact.py holds the other forms),
an image's bits against its own B = 1 run, and one whole forward with the switch on against off.

The exact sets are drawn for the direct row of the same call (forms_util knows no family for this form); the form's own
worst-case intermediate, |A^T| K |G g| |B^T d| + |b| with |G| = |B^T| = |A^T| = 2 per dimension and K = 48, is asserted below 2^23
for the amplitude they use.
"""
import numpy as np
import pytest
import torch

from sketchedit_amd import _lib, synth
import exact_util as EU
import forms_util as FU
import test_gpu_exact as TE
from parity_util import composed_for_hard_mask

pytestmark = pytest.mark.gpu

FORM = "s2poly48"
TOL_OP = FU.TOL_OP        # 1e-4: the bound of the existing Winograd rows
TOL_E2E = 1e-3            # tests/test_gpu_parity.py
FLAGS = 1 | 2 | 16
OLD = {96: "gconv_n96", 192: "gconv_n192"}
# (4, 4) at B = 8: the F set takes each channel's bias from the 5th percentile of its outputs, and 2 x 2 x 2 outputs per channel
# cannot leave 90 % of them positive (exact_util.check_FW); 32 can
SHAPES = [((4, 4), 8), ((8, 12), 2), ((12, 20), 3), ((36, 28), 2)]
CASES = [(cout, shape, B) for cout in (96, 192) for shape, B in SHAPES]
IDS = ["48to%d-%dx%d-B%d" % (c, s[0], s[1], B) for c, s, B in CASES]


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_w():
    e = _lib.Engine(0)
    e.load_state_dict("M", synth.make_state_dict("M", 0))
    e.load_state_dict("G", synth.make_state_dict("G", 0))
    assert e.weights_ready()
    yield e
    e.close()


def _row(cout, shape, act="elu"):
    """The call as a row of the form table: the direct form's name, which is what runs with the switch off."""
    return FU.row(OLD[cout], 48, cout, [shape], stride=2, act=act)


def _strided_forms(launches):
    return [f for f, _ in launches if f.startswith(FU.CONV_PREFIXES + ("s2poly",))]


def _run(eng, r, x, w, b, want_form):
    y, launches = FU.run(eng, r, x, None, w, b)
    assert _strided_forms(launches) == [want_form], launches
    # the launched form is the chooser's answer for the same call
    assert _lib.gconv_form(r.cin, r.cout, x.shape[2], x.shape[3], stride=2, act=r.act, B=x.shape[0]) == [want_form]
    return y


_REF = {}


def _case(cout, shape, B, act="elu"):
    """inputs and the two references of a case, computed once and shared"""
    key = (cout, shape, B, act)
    if key not in _REF:
        from oracle import sketchedit_oracle as O
        r = _row(cout, shape, act)
        x, _, w, b = FU.make_inputs(r, shape, B=B)
        ref64 = FU.reference(r, x, None, w, b)
        oracle = O.gated_conv(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b), 2, 1, act)
        _REF[key] = (r, x, w, b, ref64, oracle)
    return _REF[key]


def _md(a, b):
    a = a.detach().cpu().double() if hasattr(a, "detach") else torch.from_numpy(np.asarray(a)).double()
    b = b.detach().cpu().double() if hasattr(b, "detach") else torch.from_numpy(np.asarray(b)).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max())


@pytest.mark.parametrize("cout,shape,B", CASES, ids=IDS)
def test_values_vs_oracle_and_gather_form(eng, seopt, cout, shape, B):
    r, x, w, b, ref64, oracle = _case(cout, shape, B)
    y = _run(eng, r, x, w, b, FORM)
    assert tuple(y.shape) == (B, cout // 2, shape[0] // 2, shape[1] // 2)
    seopt.set("SE_S2_POLY", 0)
    yd = _run(eng, r, x, w, b, OLD[cout])
    d_or, d_64, d_g, d_go = _md(y, oracle), _md(y, ref64), _md(y, yd), _md(yd, oracle)
    print("48->%d %dx%d B %d: s2poly48 vs oracle %.3e, vs float64 %.3e, vs gather %.3e; gather vs oracle %.3e" % (cout, shape[0], shape[1], B, d_or, d_64, d_g, d_go))
    assert d_or < TOL_OP and d_64 < TOL_OP
    assert d_g < TOL_OP


@pytest.mark.parametrize("cout", [96, 192])
def test_relu_epilogue(eng, cout):
    r, x, w, b, ref64, oracle = _case(cout, (12, 20), 3, "relu")
    y = _run(eng, r, x, w, b, FORM)
    assert _md(y, oracle) < TOL_OP and _md(y, ref64) < TOL_OP


def _poly_bound(A):
    """exact_util.bound for the polyphase form on the F set, |A^T| K |G g| |B^T d| + |b|: per dimension |G| = 2 (w0 + w2),
    |B^T| = 2 (i1 - i3), |A^T| = 3 (each output folds three positions); K = 48 channels per position."""
    return 9 * 48 * (EU.WEIGHT_UNIT * 4) * (4 * A) + 48 * 9 * EU.WEIGHT_UNIT * A


@pytest.mark.parametrize("kind", ["F", "G"])
@pytest.mark.parametrize("cout,shape,B", CASES, ids=IDS)
def test_form_is_exact(eng, cout, shape, B, kind):
    """On representable inputs the result is the float64 reference bit for bit where the feature pre-activation is positive, and
    the live gate sits within the rounding of the hardware transcendentals: the checks of tests/test_gpu_exact.py."""
    r = _row(cout, shape)
    d = EU.MAKE[kind](r, shape, B=B)
    assert _poly_bound(d.A) + (2.0 ** (d.s + 1) if kind == "G" else 0.0) < EU.LIMIT
    y = _run(eng, r, d.x, d.w, d.b, FORM)
    got = y.detach().cpu().numpy()
    assert got.dtype == np.float32
    if kind == "G":
        TE._check_gates(r, shape, d, got)
    else:
        TE._check_features(r, shape, d, got)


@pytest.mark.parametrize("cout", [96, 192])
def test_batch_of_three_equals_three_single_images(eng, cout):
    """An image's result does not depend on its batch: B = 3 against three B = 1 runs, bit for bit (45 tiles in one workgroup
    against 15 tiles each; at (36, 28) an image's tiles sit in another workgroup and another lane than in its own run)."""
    for shape in [(12, 20), (36, 28)]:
        r = _row(cout, shape)
        x, _, w, b = FU.make_inputs(r, shape, B=3)
        y = _run(eng, r, x, w, b, FORM).cpu().numpy()
        for i in range(3):
            one = _run(eng, r, x[i:i + 1], w, b, FORM).cpu().numpy()
            assert np.array_equal(one[0].view(np.int32), y[i].view(np.int32)), (cout, shape, i)


def _forward(eng_w, ci, cs):
    with eng_w.launch_forms() as launches:
        r = eng_w.inference(ci, cs, FLAGS, visualize=True, low_latency=False)
    return r, [layer for form, layer in launches if form == FORM], [form for form, _ in launches]


def test_forward_64_switch_on_against_off(eng_w, seopt):
    """inference at 64x64, B = 3 (the five layers run at 32x32: 64 tiles per image, three workgroups per row half): the switch
    at 1 against 0.  Equal hard masks: the composites agree within the end-to-end tolerance; else each composite against the
    oracle's for the hard mask that run used."""
    img, sk = synth.make_inputs(3, 64, 64, seed=1234)
    ci, cs = torch.from_numpy(img).cuda(), torch.from_numpy(sk).cuda()
    on, layers_on, forms_on = _forward(eng_w, ci, cs)
    assert sorted(layers_on) == sorted(["conv4_downsample", "conv4_downsample", "wconv4_downsample", "xconv4_downsample", "pmconv4_downsample"]), layers_on
    seopt.set("SE_S2_POLY", 0)
    off, layers_off, forms_off = _forward(eng_w, ci, cs)
    assert layers_off == [] and len(forms_off) == len(forms_on)
    # launch for launch the same forms, but the gather-GEMM where the new form ran
    assert all(b == a or (a == FORM and b in OLD.values()) for a, b in zip(forms_on, forms_off)), (forms_on, forms_off)
    seopt.set("SE_S2_POLY", 2)
    g_only, layers_g, _ = _forward(eng_w, ci, cs)
    assert len(layers_g) == 4 and torch.equal(g_only["mask"], off["mask"])          # netM's layer stays on the gather form
    d_mask = _md(on["mask"], off["mask"])
    flips = int((on["hard"] != off["hard"]).sum())
    print("64x64 B 3: soft mask max-abs %.3e, hard-mask flips %d" % (d_mask, flips))
    assert d_mask < TOL_E2E
    if flips == 0:
        for k in ("composed", "coarse", "fine"):
            print("  %s max-abs %.3e" % (k, _md(on[k], off[k])))
            assert _md(on[k], off[k]) < TOL_E2E, k
    else:
        from oracle import sketchedit_oracle as O
        WM, WG = synth.make_state_dict("M", 0), synth.make_state_dict("G", 0)
        ref = O.inference(WM, WG, img, sk)
        for got in (on, off):
            want, _ = composed_for_hard_mask(O, WG, img, sk, ref["mask"], ref["hard_mask"], ref["composed"], got["hard"])
            assert _md(got["composed"], want) < TOL_E2E
