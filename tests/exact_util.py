"""Inputs on which a gated convolution is EXACT in fp32 (and in bf16 operands with fp32 accumulation), for every row of
forms_util.FORMS.  No GPU is needed here; tests/test_gpu_exact.py runs the rows, tests/test_exact_util.py checks
the preconditions below on the CPU.

Every kernel form is held to the float64 reference at TOL_OP = 1e-4, 16 to 40 times what the kernels deliver; a transform
constant cut at its sixth digit, an operand through a narrower type, a truncating bf16 store all fit inside.  On random real
data the bound cannot come down (the rigorous fp32 bound of an 864-term sum is above it).  On data whose every intermediate
value is representable the result is the same in any summation order and equals the reference bit for bit.  Three sets:

F  "features exact".  x (and the second source) integers in [-A, A]; feature weights 24 * {-1, 0, +1}; gate weights 0 and gate
   biases +64, so that the gate is exactly 1 (sigmoid_fast: 1 + e^-64 rounds to 1, v_rcp_f32(1) = 1); feature biases one
   integer per channel, minus the 5th percentile of the channel's bias-free pre-activations in the float64 reference, so that
   90 .. 99 % of the pre-activations are > 0 and pass ELU / ReLU unchanged.  Every Winograd-type weight transform of
   se_pack.hip is exact on multiples of 24 (its entries are multiples of 1/2 and 1/24), the input and output transforms have
   integer coefficients, and A is the largest of 4, 2, 1 for which the worst-case magnitude of any intermediate value stays
   below 2^23 in units of the coarsest grid the family's values lie on (1/2): see FAMILIES and bound().
G  "gates live" (rows with an activation).  Feature weights 0, feature biases 1 (act(1) = 1); gate weights
   24 * {-1, 0, +1} * 2^-s, gate biases j / 8.  The output is sigmoid(g) with g known exactly; s is the smallest for which
   |g| <= 8 everywhere and |g| <= 4 on 99 % of the outputs.  Where one granule of g would then move the result by less than
   100 times the bound of the comparison, the amplitude of x is halved (and s chosen again).
W  "wide mantissa", the direct fp32 forms only (W_ROW).  x = n * 2^-12, n in [-4096, 4096]: up to 13 significant bits, for
   four values in five not a bf16 value (a bf16 hi part plus a bf16 remainder does hold them); three non-zero feature taps
   +-2^k (k = 0, 1, 2) per output channel at drawn (cin, ky, kx); gates and biases as in F.  Products and partial sums are
   multiples of 2^-12 below 2^11 in any order.  W is NOT built for the Winograd-type forms: their inverse transforms form
   partial sums of transformed products, which on 13-bit inputs are wider than 24 bits (F(4,3): input transform x 10,
   inverse x 19 on top of the 2^-12 grid and a 1/2 weight grid).

References: forms_util.reference, unchanged; the pre-activations are the same function with act = None.
"""
import collections

import numpy as np
import torch

from sketchedit_amd import synth
import forms_util as FU

SEED = 83
LIMIT = float(2 ** 23)

# ---- the 1-D transforms, as written in se_pack.hip (G) and in the kernels' header comments (B^T, A^T) ----------------------------
T1 = collections.namedtuple("T1", "G BT AT wgrid")          # wgrid: the grid G's entries lie on
_ID = T1(np.eye(1), np.eye(1), np.eye(1), 1.0)
_BT6 = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                 [0, 4, 0, -5, 0, 1]], float)
_F23 = T1(np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]]),                                    # se_wino.hip
          np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], float),
          np.array([[1, 1, 1, 0], [0, 1, -1, -1]], float), 1 / 2)
_F43 = T1(np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6],   # se_wino24.hip
                    [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]]),
          _BT6, np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], float), 1 / 24)
_F25 = T1(np.array([[1 / 4, 0, 0, 0, 0], [-1 / 6] * 5, [-1 / 6, 1 / 6, -1 / 6, 1 / 6, -1 / 6],                   # se_rtile.hip
                    [1 / 24, 1 / 12, 1 / 6, 1 / 3, 2 / 3], [1 / 24, -1 / 12, 1 / 6, -1 / 3, 2 / 3], [0, 0, 0, 0, 1]]),
          _BT6, np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 1]], float), 1 / 24)
_F22 = T1(np.array([[1, 0], [1, 1], [0, 1]], float), np.array([[1, -1, 0], [0, 1, 0], [0, -1, 1]], float),    # se_wino_up.hip
          np.array([[1, 1, 0], [0, 1, 1]], float), 1.0)


def _norm(m):
    return float(np.abs(m).sum(1).max())


# Family: the transforms along y and x, the direct taps that remain per transformed position (ky of the 1-D forms, all k*k of
# the direct forms), and `presum`: how many checkpoint taps one operand of the transform sums (the sub-pixel classes: up to 4)
Family = collections.namedtuple("Family", "ty tx taps presum")
FAMILIES = {
    "direct": Family(_ID, _ID, lambda k: k * k, 1),
    "f23xf23": Family(_F23, _F23, lambda k: 1, 1),
    "f23xf43": Family(_F23, _F43, lambda k: 1, 1),
    "f23x": Family(_ID, _F23, lambda k: k, 1),
    "f25x": Family(_ID, _F25, lambda k: k, 1),
    "subpixel": Family(_F22, _F22, lambda k: 1, 4),
}
WEIGHT_UNIT = 24.0
AMPLITUDES = (4, 2, 1)


def norms(fam):
    """(|G|, |B^T|, |A^T|): the infinity norms of the family's transforms, y times x."""
    f = FAMILIES[fam]
    return tuple(_norm(getattr(f.ty, n)) * _norm(getattr(f.tx, n)) for n in ("G", "BT", "AT"))


def grid(fam):
    """The grid every transformed weight of the family lies on, for checkpoint weights that are multiples of 24."""
    f = FAMILIES[fam]
    return WEIGHT_UNIT * f.ty.wgrid * f.tx.wgrid


def bound(r, A):
    """Worst-case magnitude of any intermediate value of row r on the F set with amplitude A: |A^T| K |G g| |B^T d| + |b|, K the
    channels x taps summed per transformed position.  |b| <= cin k^2 24 A, the direct bound of the pre-activations the bias
    is a percentile of.  A folded vector source (vecbias) is a direct sum over its 96 channels on top of the form's own."""
    fam = FU.family(r.form)
    f = FAMILIES[fam]
    g, bt, at = norms(fam)
    cin = r.cin - (96 if "vecbias" in r.pre else 0)
    v = at * cin * f.taps(r.k) * (WEIGHT_UNIT * f.presum * g) * (bt * A)
    if "vecbias" in r.pre:
        v += 96 * r.k * r.k * WEIGHT_UNIT * A
    return v + r.cin * r.k * r.k * WEIGHT_UNIT * A


def amplitude(r):
    """The largest A of 4, 2, 1 whose bound() is below 2^23 -- in units of 1/2, the finest grid of any family: 24 bits."""
    assert grid(FU.family(r.form)) >= 0.5
    for A in AMPLITUDES:
        if bound(r, A) < LIMIT:
            return A
    raise AssertionError("no exact amplitude for " + FU.row_id(r))


def W_ROW(r):
    """The direct fp32 forms the W set is built for."""
    return r.mode in ("default", "lowlat") and (r.form.startswith("gconv_") or r.form in ("rtile", "rtile_up2", "rtile_dense5", "small_conv"))


# ---- keyed draws -----------------------------------------------------------------------------------------------------------------
def _ints(stream, shape, lo, hi):
    """integers uniform in [lo, hi], as float64"""
    u = synth.uniform01(SEED, stream, int(np.prod(shape)))
    return (np.floor(u * (hi - lo + 1)) + lo).reshape(shape)


def _key(r, shape, B):
    return "%s|%dx%d|%d" % (FU.row_id(r), shape[0], shape[1], B)


def _sources(r, shape, B, key, A, scale=1.0):
    H, W = shape
    c0 = r.cin - (96 if r.src2 else 0)
    x = _ints("exact.x" + key, (B, c0, H, W), -A, A) * scale
    x1 = None
    if r.src2 == "tensor":
        x1 = _ints("exact.y" + key, (B, 96, H, W), -A, A) * scale
    elif r.src2 == "vector":
        x1 = _ints("exact.v" + key, (B, 96), -A, A) * scale
    return x.astype(np.float32), None if x1 is None else x1.astype(np.float32)


def preact(r, x, x1, w, b):
    """The float64 pre-activations (B, cout, Ho, Wo) of row r: forms_util.reference without its epilogue."""
    return FU.reference(r._replace(act=None), x, x1, w, b).numpy()


def n_feat(r):
    return r.cout if r.act is None else r.cout // 2


def _feature_bias(r, x, x1, w):
    """One integer per feature channel: minus the 5th percentile of the channel's bias-free pre-activations."""
    nf = n_feat(r)
    p0 = preact(r, x, x1, w, np.zeros(r.cout, np.float32))[:, :nf]
    p5 = np.percentile(p0.transpose(1, 0, 2, 3).reshape(nf, -1), 5, axis=1)
    return -np.round(p5)


Data = collections.namedtuple("Data", "kind x x1 w b A s granule")


def _finish(kind, r, x, x1, w, A):
    b = np.zeros(r.cout)
    nf = n_feat(r)
    if r.act is not None:
        b[nf:] = 64.0
    b[:nf] = _feature_bias(r, x, x1, w)
    return Data(kind, x, x1, w.astype(np.float32), b.astype(np.float32), A, None, None)


def make_F(r, shape, B=FU.BATCH):
    key = _key(r, shape, B)
    A = amplitude(r)
    x, x1 = _sources(r, shape, B, key, A)
    w = np.zeros((r.cout, r.cin, r.k, r.k))
    nf = n_feat(r)
    w[:nf] = WEIGHT_UNIT * _ints("exact.w" + key, (nf, r.cin, r.k, r.k), -1, 1)
    d = _finish("F", r, x, x1, w, A)
    check_FW(r, d)
    return d


def make_W(r, shape, B=FU.BATCH):
    assert W_ROW(r)
    key = _key(r, shape, B)
    x, x1 = _sources(r, shape, B, key + "W", 4096, 2.0 ** -12)
    nf, T = n_feat(r), r.cin * r.k * r.k
    w = np.zeros((r.cout, T))
    # three distinct taps per channel: the three smallest of T keyed draws
    pos = np.argsort(synth.uniform01(SEED, "exact.wp" + key, nf * T).reshape(nf, T), axis=1)[:, :3]
    val = np.exp2(_ints("exact.wk" + key, (nf, 3), 0, 2)) * (2 * _ints("exact.ws" + key, (nf, 3), 0, 1) - 1)
    w[np.arange(nf)[:, None], pos] = val
    d = _finish("W", r, x, x1, w.reshape(r.cout, r.cin, r.k, r.k), 1)
    check_FW(r, d)
    return d


def make_G(r, shape, B=FU.BATCH):
    assert r.act is not None
    key = _key(r, shape, B)
    nf = r.cout // 2
    w0 = np.zeros((r.cout, r.cin, r.k, r.k))
    w0[nf:] = WEIGHT_UNIT * _ints("exact.gw" + key, (nf, r.cin, r.k, r.k), -1, 1)
    b = np.zeros(r.cout)
    b[:nf] = 1.0
    b[nf:] = _ints("exact.gb" + key, (nf,), -8, 8) / 8.0
    A = amplitude(r)
    while True:
        x, x1 = _sources(r, shape, B, key + "G%d" % A, A)
        g0 = preact(r, x, x1, w0.astype(np.float32), np.zeros(r.cout, np.float32))[:, nf:]
        for s in range(0, 24):
            g = np.abs(g0 * 2.0 ** -s + b[nf:][None, :, None, None])
            if g.max() <= 8 and (g <= 4).mean() >= 0.99:
                break
        else:
            raise AssertionError("no gate scale for " + FU.row_id(r, shape))
        granule = 2.0 ** min(3 - s, -3)
        if teeth_ratio(granule) >= 100 or A == 1:
            break
        A //= 2
    d = Data("G", x, x1, (w0 * 2.0 ** -s).astype(np.float32), b.astype(np.float32), A, s, granule)
    check_G(r, d)
    return d


def g_bound(g):
    """|y - sigmoid(g)| <= (|g| + 8) 2^-24 sigmoid(g) for the fp32 value y of the epilogue: the argument rounding of __expf is
    |g| 2^-24 relative, v_exp_f32 and v_rcp_f32 1-2 ulp each (se_device.h), the add half an ulp."""
    return (np.abs(g) + 8) * 2.0 ** -24 / (1.0 + np.exp(-g))


def bf16_rne(v):
    """float64 -> the nearest bf16 value (8 significant bits), ties to even, as float64; one rounding, in exact arithmetic."""
    v = np.asarray(v, np.float64)
    q = np.exp2(np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -120))) - 7)
    return np.round(v / q) * q


def g_interval(g, bf):
    """The values the output may take: [sigmoid(g) - g_bound, sigmoid(g) + g_bound]; in bf16 mode the bf16 roundings of that
    interval's ends -- the store is round-to-nearest-even of a value inside it, so mostly ONE bf16 value is allowed, two where
    a rounding boundary lies inside.  (Half a bf16 spacing is between 2^-9 and 2^-8 of the value: a flat 2^-9 sigmoid(g) on
    top of the fp32 bound is missed by the correctly rounded reference itself on a quarter of the outputs, by up to 1.99 x.)"""
    sg = 1.0 / (1.0 + np.exp(-g))
    t = g_bound(g)
    return (bf16_rne(sg - t), bf16_rne(sg + t)) if bf else (sg - t, sg + t)


def teeth_ratio(granule):
    """One granule of error in g moves sigmoid(g) by at least (1 - sigmoid(4)) granule relative where |g| <= 4 (d ln sigmoid / dg
    = 1 - sigmoid(g)); the ratio of that to the largest relative fp32 bound there, (4 + 8) 2^-24.
    (In bf16 mode that bound holds for the value in front of the store; an error of one granule then shows at the outputs it
    carries over a rounding boundary: all of them near g = 0, where it is a whole bf16 spacing, one in some fifty at g = 4.)"""
    return (1 - 1 / (1 + np.exp(-4.0))) * granule / (12 * 2.0 ** -24)


# ---- preconditions: conditions, not measurements ------------------------------------------------------------------------------------
def _bf16_exact(a):
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32))
    return bool(torch.equal(t.to(torch.bfloat16).float(), t))


def shares(r, d):
    """(share of feature pre-activations > 0, share <= 0) in the float64 reference."""
    f = preact(r, d.x, d.x1, d.w, d.b)[:, :n_feat(r)]
    return float((f > 0).mean()), float((f <= 0).mean())


def check_FW(r, d):
    rid = FU.row_id(r)
    nf = n_feat(r)
    unit = 1.0 if d.kind == "F" else 2.0 ** -12
    if d.kind == "F":
        assert bound(r, d.A) < LIMIT, rid                                                   # 1: representable in any order
        assert np.abs(d.b[:nf]).max() <= r.cin * r.k * r.k * WEIGHT_UNIT * d.A, rid          #    (the |b| bound() allowed for)
        assert np.isin(d.w[:nf], (-24, 0, 24)).all() and np.abs(d.x).max() <= d.A
    else:
        assert FU.family(r.form) == "direct" and (np.count_nonzero(d.w[:nf].reshape(nf, -1), axis=1) == 3).all(), rid
        assert np.isin(np.abs(d.w), (0, 1, 2, 4)).all() and np.abs(d.x).max() <= 1
        assert (3 * 4 * 1 + np.abs(d.b[:nf]).max()) / unit < LIMIT, rid
        # up to 13 significant bits: four in five values of x are no bf16 value (a 12-bit n IS the sum of two bf16 values, 8 + 4
        # bits: a two-term split is exact on this set and shows on no exact set at all -- it loses nothing)
        t = torch.from_numpy(d.x)
        assert float((t.to(torch.bfloat16).float() != t).float().mean()) > 0.75, rid
    assert (d.x == np.round(d.x / unit) * unit).all() and (d.b == np.round(d.b)).all(), rid
    if r.act is not None:
        assert not d.w[nf:].any() and (d.b[nf:] == 64).all(), rid
        pos, neg = shares(r, d)                                                             # 2: the share compared exactly
        assert pos >= 0.90 and neg >= 0.01, (rid, pos, neg)
    p = preact(r, d.x, d.x1, d.w, d.b)[:, :nf]                                              # 3: the data are what they claim
    assert (p == np.round(p / unit) * unit).all() and np.abs(p).max() / unit < LIMIT, rid
    if r.mode.startswith("bf16"):                                                           # 4: bf16 operands lose nothing
        assert _bf16_exact(d.x) and _bf16_exact(d.w) and (d.x1 is None or _bf16_exact(d.x1)), rid


def check_G(r, d):
    rid = FU.row_id(r)
    nf = r.cout // 2
    assert not d.w[:nf].any() and (d.b[:nf] == 1).all(), rid
    unit = WEIGHT_UNIT * 2.0 ** -d.s
    assert np.isin(d.w[nf:], (-unit, 0, unit)).all(), rid
    # 1: the F bound in units of the weights' scale, the gate bias (<= 1) on top, in units of half a transformed-weight grid step
    assert bound(r, d.A) + 2.0 ** (d.s + 1) < LIMIT, rid
    g = preact(r, d.x, d.x1, d.w, d.b)[:, nf:]
    assert (g == np.round(g / d.granule) * d.granule).all(), rid                            # 3: multiples of the granule
    assert np.abs(g).max() <= 8 and float((np.abs(g) <= 4).mean()) >= 0.99, rid
    assert teeth_ratio(d.granule) >= 100, (rid, d.s, teeth_ratio(d.granule))
    if r.mode.startswith("bf16"):
        assert _bf16_exact(d.x) and _bf16_exact(d.w) and (d.x1 is None or _bf16_exact(d.x1)), rid


def rows():
    """Every row of FORMS at its last shape: the ragged multi-tile one."""
    return [(r, r.shapes[-1]) for r in FU.FORMS]


def sets_of(r):
    return ["F"] + (["G"] if r.act is not None else []) + (["W"] if W_ROW(r) else [])


MAKE = {"F": make_F, "G": make_G, "W": make_W}
