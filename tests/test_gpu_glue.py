"""The kernels between the convolutions, each on its own: input packing, the column reduce (pooling, key norm) and the output
conv with its fused epilogue, through the per-op entry points se_pack_inputs / se_column_reduce / se_output_conv (the launchers
the forwards call) against plain numpy / torch float64 references written here.

The forwards reach these kernels too, but compare at 1e-3 (fp32) or 3e-2 (bf16): one pixel dropped from a mean over 4096 moves
the style vector by 2e-4, a wrong power of (1 - m) matters at soft-mask pixels only, a bf16 packing that truncates is inside the
bf16 bound.  So every assertion here is exact wherever the arithmetic allows it -- bit patterns for the packing, integer-valued
inputs for the reductions (every sum is exact in fp32 in any order), the uint8 outputs and the threshold against the GPU's own
floats of the same call -- and the float comparisons use the per-op bound TOL_OP = 1e-4.  Every test prints its measured worst
differences before it asserts (pytest -s shows them)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from sketchedit_amd import _lib
from test_gpu_parity import TOL_OP

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _bf16_bits(a):
    """fp32 array -> the uint16 bit patterns of torch's fp32 -> bf16 conversion (round to nearest even)"""
    t = torch.from_numpy(np.ascontiguousarray(a, F32)).to(torch.bfloat16)
    return t.view(torch.int16).numpy().view(np.uint16)


def _bf16_value(bits):
    """uint16 bf16 bit patterns -> fp32 values"""
    return (np.ascontiguousarray(bits).view(np.uint16).astype(np.uint32) << 16).view(F32)


def _bf16_round(a):
    return _bf16_value(_bf16_bits(a))


def _nhwc(a):
    return np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1)))


def _soft_mask(rng, shape):
    """values in (0,1) as well as exact 0 and 1"""
    m = rng.uniform(0.0, 1.0, shape).astype(F32)
    r = rng.uniform(size=shape)
    m[r < 0.25] = 0.0
    m[r > 0.75] = 1.0
    return m


# ---- input packing ------------------------------------------------------------------------------------------------------------
PACK_SIZES = [(5, 7), (24, 40), (64, 64)]          # B = 3: 105, 2880, 12288 pixels, none a multiple of the 256-thread block
# exactly half way between two bf16 neighbours: round-to-nearest-even takes the first of each pair DOWN (to the even
# neighbour, which truncation also gives) and the second UP (truncation does not); the sign does not change the rule
TIES = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 0.25 + 2.0 ** -10, 0.25 + 3 * 2.0 ** -10], F32)
MASK_TIES = np.array([0.5 + 2.0 ** -9, 0.5 + 3 * 2.0 ** -9], F32)


def _pack_case(H, W):
    rng = np.random.default_rng(100 * H + W)
    B = 3
    x = rng.uniform(-1, 1, (B, 3, H, W)).astype(F32)
    x2 = rng.uniform(-1, 1, (B, 3, H, W)).astype(F32)
    mask, mask2 = _soft_mask(rng, (B, 1, H, W)), _soft_mask(rng, (B, 1, H, W))
    guide = rng.uniform(0.1, 1, (B, 1, H, W)).astype(F32) * rng.choice(F32([-1, 1]), (B, 1, H, W))
    # the ties, where the packed value IS the planted one: x where mask == 0, x2 where mask2 == 1, the guide, the masks
    n = len(TIES)
    for c in range(3):
        x[0, c].reshape(-1)[:n] = np.roll(TIES, c)
        x2[0, c].reshape(-1)[:n] = np.roll(TIES, c + 1)
    mask[0, 0].reshape(-1)[:n] = 0.0
    mask2[0, 0].reshape(-1)[:n] = 1.0
    guide[1, 0].reshape(-1)[:n] = TIES
    mask[1, 0].reshape(-1)[:2] = MASK_TIES
    mask2[1, 0].reshape(-1)[2:4] = MASK_TIES
    assert ((mask > 0) & (mask < 1)).any() and (mask == 0).any() and (mask == 1).any() and (guide != 0).all()
    return x, x2, mask, mask2, guide


def _pack_g_reference(x, x2, mask, mask2, guide, joint, no_mask_cc):
    """editline_g.py:120-135 in numpy float32: one subtract, one multiply -- nothing a compiler could contract"""
    one, z = F32(1), np.zeros_like(mask)
    coarse = np.concatenate([x * (one - mask), guide, mask, z, z, z], 1)
    s = x2 if no_mask_cc else x2 * mask2
    style = np.concatenate([s, mask2] if joint else [s, guide, mask2, z, z, z], 1)
    return _nhwc(coarse), _nhwc(style)


def _pad8(a):
    """(B,H,W,C) -> (B,H,W,8), zero padded: the channels of one 16-byte bf16 granule"""
    return np.concatenate([a, np.zeros(a.shape[:3] + (8 - a.shape[3],), F32)], 3)


@pytest.mark.parametrize("no_mask_cc", [0, 1])
@pytest.mark.parametrize("joint", [0, 1])
@pytest.mark.parametrize("size", PACK_SIZES, ids=lambda s: "%dx%d" % s)
def test_pack_netG_fp32_is_bit_exact(eng, size, joint, no_mask_cc):
    x, x2, mask, mask2, guide = _pack_case(*size)
    flags = (_lib.FLAG_JOINT_TRAIN_INP if joint else 0) | (_lib.FLAG_NO_MASK_CC if no_mask_cc else 0)
    coarse, style = eng.pack_inputs("G", _cuda(x), _cuda(guide), _cuda(x2), _cuda(mask), _cuda(mask2), flags=flags)
    ref_c, ref_s = _pack_g_reference(x, x2, mask, mask2, guide, joint, no_mask_cc)
    coarse, style = _np(coarse), _np(style)
    assert coarse.shape == ref_c.shape == (3,) + size + (8,) and style.shape == ref_s.shape == (3,) + size + (4 if joint else 8,)
    assert np.array_equal(_bits(coarse), _bits(ref_c))
    assert np.array_equal(_bits(style), _bits(ref_s))
    assert (_bits(coarse[..., 5:]) == 0).all()                       # the padding channels: +0.0, bit for bit
    if joint:
        assert np.array_equal(_bits(style[..., 3]), _bits(mask2[:, 0]))      # the 4-channel style input carries m2 in slot 3
    else:
        assert (_bits(style[..., 5:]) == 0).all()
    assert not np.array_equal(x, x2) and not np.array_equal(mask, mask2)


@pytest.mark.parametrize("no_mask_cc", [0, 1])
@pytest.mark.parametrize("joint", [0, 1])
@pytest.mark.parametrize("size", PACK_SIZES, ids=lambda s: "%dx%d" % s)
def test_pack_netG_bf16_rounds_to_nearest_even(eng, size, joint, no_mask_cc):
    x, x2, mask, mask2, guide = _pack_case(*size)
    flags = (_lib.FLAG_JOINT_TRAIN_INP if joint else 0) | (_lib.FLAG_NO_MASK_CC if no_mask_cc else 0)
    coarse, style = eng.pack_inputs("G", _cuda(x), _cuda(guide), _cuda(x2), _cuda(mask), _cuda(mask2), flags=flags, bf16=True)
    ref_c, ref_s = _pack_g_reference(x, x2, mask, mask2, guide, joint, no_mask_cc)
    for got, ref in ((coarse, ref_c), (style, ref_s)):
        got = _np(got).view(np.uint16)
        want = _bf16_bits(_pad8(ref))
        assert got.shape == want.shape == (3,) + size + (8,)
        assert np.array_equal(got, want)
        assert (got[..., ref.shape[3]:] == 0).all()                  # the pad half-words
        # the comparison pins the rounding mode: the planted ties are there, and truncation would give other bits
        low = _bits(_pad8(ref)) & 0xFFFF
        assert (low == 0x8000).sum() >= len(TIES) and (want != (_bits(_pad8(ref)) >> 16)).any()


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("size", PACK_SIZES, ids=lambda s: "%dx%d" % s)
def test_pack_netM(eng, size, bf16):
    """editline2_g.py:62: [image, sketch]; the sketch is 0 / 1 in production, here it also carries the ties"""
    x, _, _, _, guide = _pack_case(*size)
    got = _np(eng.pack_inputs("M", _cuda(x), _cuda(guide), bf16=bf16))
    ref = _nhwc(np.concatenate([x, guide], 1))
    if bf16:
        got = got.view(np.uint16)
        assert got.shape == (3,) + size + (8,)
        assert np.array_equal(got, _bf16_bits(_pad8(ref))) and (got[..., 4:] == 0).all()
        assert (_bf16_bits(ref) != (_bits(ref) >> 16)).any()
    else:
        assert got.shape == ref.shape and np.array_equal(_bits(got), _bits(ref))


# ---- column reduce ------------------------------------------------------------------------------------------------------------
# HW: 1; 16 (most of the 128 splits empty); around one pixel per split; 180 (the 40 x 72 input); 1290; 4096; 8200 (more than
# 3 * groups pixels per split in both precisions: the four-loads-in-flight loop); 16384
POOL_HW = {1: (1, 1), 16: (4, 4), 127: (1, 127), 128: (8, 16), 129: (3, 43), 180: (10, 18), 1290: (30, 43), 4096: (64, 64),
           8200: (82, 100), 16384: (128, 128)}
# C: production; one granule; a granule count that does not divide the 256 threads (25 / 13); the most the launcher takes
POOL_C = {False: [96, 4, 100, 256], True: [96, 8, 104, 256]}
POOL_CASES = [(hw, bf, c) for hw in POOL_HW for bf in (False, True) for c in POOL_C[bf]]


def _pool_case(C, HW):
    """B = 3 integer-valued images in [-8, 8]: every sum of values (|.| <= 8 HW <= 2^17) and of squares (<= 64 HW = 2^20) is
    an integer below 2^24, exact in fp32 in any order, and every value is exact in bf16.  Each channel's maximum is unique
    and sits at a position drawn per (b, c) -- pixel 0 and pixel HW-1 among them --; image 1 is negative throughout."""
    rng = np.random.default_rng(7 * HW + C)
    B = 3
    x = rng.integers(-8, 8, (B, C, HW)).astype(F32)                  # -8 .. 7
    x[1] = rng.integers(-8, -1, (C, HW))                             # -8 .. -2
    pos = rng.integers(0, HW, (B, C))
    pos[:, 0], pos[:, 1], pos[:, C - 1], pos[:, C - 2] = 0, HW - 1, 0, HW - 1
    peak = F32([8, -1, 8])
    for b in range(B):
        x[b, np.arange(C), pos[b]] = peak[b]
    assert (pos == 0).any() and (pos == HW - 1).any() and (x[1] < 0).all()
    return x, pos


@pytest.mark.parametrize("case", POOL_CASES, ids=lambda c: "hw%d-%s-c%d" % (c[0], "bf16" if c[1] else "f32", c[2]))
def test_column_reduce_integer_inputs_are_exact(eng, case):
    HW, bf16, C = case
    H, W = POOL_HW[HW]
    x, pos = _pool_case(C, HW)
    xd = _cuda(x.reshape(3, C, H, W))
    xi = x.astype(np.int64)
    want = {"max": x.max(-1), "mean": xi.sum(-1).astype(F32) / F32(HW)}
    want_rsqrt = 1.0 / np.sqrt((xi * xi).sum(-1).astype(np.float64) + 1e-8)
    assert np.array_equal(want["max"], np.broadcast_to(F32([8, -1, 8])[:, None], (3, C)))
    for op in ("max", "mean", "rsqrt"):
        r = eng.column_reduce(xd, op, bf16=bf16)
        again = eng.column_reduce(xd, op, bf16=bf16)
        out, out16 = (r if bf16 else (r, None))
        out = _np(out)
        assert np.array_equal(_bits(out), _bits(_np(again[0] if bf16 else again))), "%s: two runs differ" % op
        if op == "rsqrt":      # sqrtf and the divide: a few ulp
            rel = np.abs(out.astype(np.float64) - want_rsqrt) / want_rsqrt
            print("column_reduce hw%d c%d %s rsqrt: worst relative difference %.2e (bound 1e-6)" % (HW, C, "bf16" if bf16 else "f32", rel.max()))
            assert rel.max() <= 1e-6
        else:
            bad = _bits(out) != _bits(want[op])
            assert not bad.any(), "%s: %d of %d differ, first at (b, c) = %s: got %r, want %r, maximum planted at pixel %d" % (
                op, bad.sum(), bad.size, tuple(np.argwhere(bad)[0]), out[bad][0], want[op][bad][0], pos[bad][0])
        if bf16:               # the bf16 copy: the fp32 result rounded to nearest even
            assert np.array_equal(_np(out16).view(np.uint16), _bf16_bits(out)), op


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_column_reduce_real_inputs(eng, bf16):
    """uniform [-1, 1], HW = 4096, C = 96: values that are not exact in bf16 (the widening of a rounded value), sums that
    round.  Against float64 of the values the kernel sums (bf16 mode: rounded first).  Bounds, with u = 2^-24: a sum of n fp32
    values in ANY order is within (n - 1) u sum|x| of the exact one, so the mean is within (HW - 1) u mean|x|; the squares
    enter through fmaf (no rounding of their own) and are non-negative, so their sum is within (HW - 1) u RELATIVE, which
    the inverse square root halves, plus the 1e-6 of the integer case for sqrtf and the divide.  The maximum is exact."""
    B, C, H, W = 3, 96, 64, 64
    HW = H * W
    rng = np.random.default_rng(4096 + bf16)
    x = rng.uniform(-1, 1, (B, C, HW)).astype(F32)
    xs = _bf16_round(x) if bf16 else x
    assert not bf16 or (xs != x).any()
    x64 = xs.astype(np.float64)
    xd = _cuda(x.reshape(B, C, H, W))
    get = lambda op: _np(eng.column_reduce(xd, op, bf16=bf16)[0] if bf16 else eng.column_reduce(xd, op))      # noqa: E731
    assert np.array_equal(_bits(get("max")), _bits(xs.max(-1)))
    u = 2.0 ** -24
    d_mean = np.abs(get("mean").astype(np.float64) - x64.mean(-1))
    b_mean = (HW - 1) * u * np.abs(x64).mean(-1)
    want = 1.0 / np.sqrt((x64 * x64).sum(-1) + 1e-8)
    d_rsq = np.abs(get("rsqrt").astype(np.float64) - want) / want
    b_rsq = 0.5 * (HW - 1) * u + 1e-6
    print("column_reduce real %s: mean worst %.2e (smallest bound %.2e), rsqrt worst relative %.2e (bound %.2e)" % (
        "bf16" if bf16 else "f32", d_mean.max(), b_mean.min(), d_rsq.max(), b_rsq))
    assert (d_mean <= b_mean).all() and d_rsq.max() <= b_rsq
    if bf16:
        r, r16 = eng.column_reduce(xd, "mean", bf16=True)
        assert np.array_equal(_np(r16).view(np.uint16), _bf16_bits(_np(r)))


@pytest.mark.parametrize("bf16,C", [(False, 260), (False, 6), (False, 98), (True, 12), (True, 100), (True, 264)])
def test_column_reduce_refuses_what_the_launcher_refuses(eng, bf16, C):
    x = torch.ones((2, C, 4, 4), dtype=torch.float32, device="cuda")
    with pytest.raises(_lib.SketchEditHipError, match="column reduce"):
        eng.column_reduce(x, "max", bf16=bf16)
    ok = eng.column_reduce(torch.ones((2, 8, 4, 4), dtype=torch.float32, device="cuda"), "mean", bf16=bf16)      # the ctx lives on
    assert bool(((ok[0] if bf16 else ok) == 1).all())


# ---- output conv ---------------------------------------------------------------------------------------------------------------
# (B, H, W).  launch_small_conv runs 2-row strips up to B ceil(H / 4) W = 65280 and 4-row strips above: the second group has
# ragged last strips of 2, 1, 3 and 2 rows, the last with B > 1
OC_SR2 = [(3, 5, 7), (2, 12, 16), (1, 2, 300), (2, 64, 64)]
OC_SR4 = [(1, 1022, 256), (1, 1037, 252), (1, 1023, 256), (3, 342, 256)]
assert all(B * ((H + 3) // 4) * W <= 65280 for B, H, W in OC_SR2) and all(B * ((H + 3) // 4) * W > 65280 for B, H, W in OC_SR4)
assert sorted(H % 4 for _, H, _ in OC_SR4) == [1, 2, 2, 3]
SENTINEL = 12345.0


def _oc_case(B, H, W, bf16):
    """Inputs and the float64 conv of one shape.  Weights uniform +-1.5 / sqrt(108); x uniform in [-4, 4], so the conv term
    has a standard deviation of 4 * 0.5 = 2, and the biases are spread over [-1, 1]: the pre-activations are wide and few
    lie near sigmoid's 0.5 crossing.  bf16 mode: the reference rounds x and w to bf16 first (the bias stays fp32)."""
    rng = np.random.default_rng(B * 1000003 + H * 1009 + W)
    a = 1.5 / np.sqrt(108.0)
    c = {"x": rng.uniform(-4, 4, (B, 12, H, W)).astype(F32),
         "w1": rng.uniform(-a, a, (1, 12, 3, 3)).astype(F32), "w3": rng.uniform(-a, a, (3, 12, 3, 3)).astype(F32),
         "b1": F32([0.3]), "b3": F32([-1.0, 0.1, 1.0]),
         "img": rng.uniform(-1, 1, (B, 3, H, W)).astype(F32), "mask": _soft_mask(rng, (B, 1, H, W)),
         "lock": rng.choice(np.array([0, 0, 0, 1, 255], np.uint8), (B, H, W))}
    rnd = _bf16_round if bf16 else (lambda v: v)
    xr = torch.from_numpy(rnd(c["x"])).double()
    for n in ("1", "3"):
        c["a" + n] = F.conv2d(xr, torch.from_numpy(rnd(c["w" + n])).double(), torch.from_numpy(c["b" + n]).double(), padding=1).numpy()
    assert set(np.unique(c["lock"])) == {0, 1, 255}
    return c


def _dev(shape, dtype=torch.float32, fill=SENTINEL):
    return torch.full(shape, fill, dtype=dtype, device="cuda")


def _worst(name, got, ref, tol, log):
    """|got - ref| <= tol everywhere (tol a number or an array); the worst difference goes to the log"""
    d = np.abs(np.asarray(got, np.float64) - ref)
    log.append("%s %.2e" % (name, d.max()))
    return bool((d <= tol).all())


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", OC_SR2 + OC_SR4, ids=lambda s: "%dx%dx%d" % s)
def test_output_conv_epilogues(eng, shape, bf16):
    """small_conv_kernel, modes 0-3, both cout, against the float64 3x3 zero-padded conv and the epilogues the kernel's comments
    cite: sigmoid + lock + threshold (editline2_g.py:94, editline2_model.py:346-347), tanh, the stage-2 input
    (editline_g.py:124,179-180), the composite (editline2_model.py:132) and the uint8 outputs (test.py:25-27)."""
    B, H, W = shape
    c = _oc_case(B, H, W, bf16)
    x, img, mask, lock = _cuda(c["x"]), _cuda(c["img"]), _cuda(c["mask"]), _cuda(c["lock"])
    m64, img64, locked = c["mask"].astype(np.float64), c["img"].astype(np.float64), c["lock"][:, None] != 0
    log, ok = [], True

    # ---- mode 0: sigmoid, lock, threshold.  The share of pixels too close to the threshold to be judged is a property of the
    # reference inputs alone (computed here on the CPU, before the GPU's result is looked at): at most 1 %
    sig = 1.0 / (1.0 + np.exp(-c["a1"]))
    ref_m = np.where(locked, 0.0, sig)
    judged = np.abs(ref_m - 0.5) > TOL_OP
    assert 1.0 - judged.mean() <= 0.01 and 1.0 - (np.abs(sig - 0.5) > TOL_OP).mean() <= 0.01
    out, hard = _dev((B, 1, H, W)), _dev((B, 1, H, W))
    eng.output_conv(x, c["w1"], c["b1"], 0, bf16=bf16, out=out, hard=hard, lock=lock)
    out0, hard0 = _np(out), _np(hard)
    ok &= _worst("mask", out0, ref_m, TOL_OP, log)
    assert np.array_equal(hard0, (out0 > F32(0.5)).astype(F32))                  # the threshold of the GPU's own mask
    assert (_bits(out0[locked]) == 0).all() and (_bits(hard0[locked]) == 0).all() and locked.any()
    assert np.array_equal(hard0[judged], (ref_m > 0.5).astype(F32)[judged])
    out_nl = _dev((B, 1, H, W))
    eng.output_conv(x, c["w1"], c["b1"], 0, bf16=bf16, out=out_nl)               # no lock, no hard mask
    ok &= _worst("mask-unlocked", _np(out_nl), sig, TOL_OP, log)
    assert np.array_equal(_np(out_nl)[~locked], out0[~locked])

    # ---- mode 1: tanh
    t64 = np.tanh(c["a3"])
    out = _dev((B, 3, H, W))
    eng.output_conv(x, c["w3"], c["b3"], 1, bf16=bf16, out=out)
    out1 = _np(out)
    ok &= _worst("tanh", out1, t64, TOL_OP, log)

    # ---- mode 2: tanh + the stage-2 input, with the soft mask that makes the (1 - m)^2 term visible
    for nmc in (0, 1):
        ref_x = t64 if nmc else t64 * m64 + (img64 * (1.0 - m64)) * (1.0 - m64)
        xnow = _dev((B, H, W, 8), torch.int16, 0x7777) if bf16 else _dev((B, H, W, 4))
        out = None if nmc else _dev((B, 3, H, W))                                # (out may be absent in modes 2 and 3)
        eng.output_conv(x, c["w3"], c["b3"], 2, bf16=bf16, no_mask_coarse=nmc, img=img, mask=mask, xnow=xnow,
                        **({} if out is None else {"out": out}))
        xn = _np(xnow)
        if bf16:
            xn = xn.view(np.uint16)
            assert (xn[..., 3:] == 0).all()                                      # the granule's padding channels
            tol = TOL_OP + 2.0 ** -8 * np.abs(_nhwc(ref_x))                      # one bf16 spacing on top of the per-op bound
            ok &= _worst("xnow%d" % nmc, _bf16_value(xn[..., :3]), _nhwc(ref_x), tol, log)
        else:
            assert (_bits(xn[..., 3]) == 0).all()
            ok &= _worst("xnow%d" % nmc, xn[..., :3], _nhwc(ref_x), TOL_OP, log)
        if out is not None:
            assert np.array_equal(_bits(_np(out)), _bits(out1))                  # the same tanh as mode 1

    # ---- mode 3: tanh + composite + uint8 outputs
    ref_c = t64 * m64 + img64 * (1.0 - m64)
    out, comp = _dev((B, 3, H, W)), _dev((B, 3, H, W))
    rgb8, m8 = _dev((B, H, W, 3), torch.uint8, 0x5A), _dev((B, H, W), torch.uint8, 0x5A)
    eng.output_conv(x, c["w3"], c["b3"], 3, bf16=bf16, out=out, img=img, mask=mask, composed=comp, rgb8=rgb8, m8=m8)
    comp3 = _np(comp)
    ok &= _worst("composed", comp3, ref_c, TOL_OP, log)
    assert np.array_equal(_bits(_np(out)), _bits(out1))
    # exact against the GPU's own composite: test.py:25-27 in numpy float32, same operation order, truncated
    q = ((comp3 + F32(1)) * F32(0.5)) * F32(255)
    assert q.dtype == F32
    assert np.array_equal(_np(rgb8), np.transpose(q.astype(np.int32).astype(np.uint8), (0, 2, 3, 1)))
    assert np.array_equal(_np(m8), (c["mask"][:, 0] * F32(255)).astype(np.int32).astype(np.uint8))
    rgb8b = _dev((B, H, W, 3), torch.uint8, 0x5A)
    eng.output_conv(x, c["w3"], c["b3"], 3, bf16=bf16, img=img, mask=mask, rgb8=rgb8b)      # the uint8 path: no fp32 output
    assert torch.equal(rgb8b, rgb8)

    # ---- packed strides: one (B,4,H,W) buffer between two guard bands, all sentinel.  Mode 0 writes plane 3 only, mode 3
    # reads the mask there and writes planes 0-2 only
    n, g = B * 4 * H * W, 1024
    flat = _dev((n + 2 * g,))
    packed = flat[g:g + n].view(B, 4, H, W)
    eng.output_conv(x, c["w1"], c["b1"], 0, bf16=bf16, packed=packed, hard=hard, lock=lock)
    pk = _np(packed)
    assert np.array_equal(_bits(pk[:, 3:]), _bits(out0)) and (pk[:, :3] == F32(SENTINEL)).all()
    eng.output_conv(x, c["w3"], c["b3"], 3, bf16=bf16, packed=packed, img=img)
    pk = _np(packed)
    assert np.array_equal(_bits(pk[:, 3:]), _bits(out0))
    ok &= _worst("packed", pk[:, :3], t64 * out0.astype(np.float64) + img64 * (1.0 - out0.astype(np.float64)), TOL_OP, log)
    fl = _np(flat)
    assert (fl[:g] == F32(SENTINEL)).all() and (fl[g + n:] == F32(SENTINEL)).all()

    print("output_conv %dx%dx%d %s: worst |difference| (bound %.0e): %s" % (B, H, W, "bf16" if bf16 else "f32", TOL_OP, ", ".join(log)))
    assert ok, log


def test_output_conv_refuses_bad_arguments(eng):
    x = torch.zeros((1, 12, 4, 4), dtype=torch.float32, device="cuda")
    w1, w3 = np.zeros((1, 12, 3, 3), F32), np.zeros((3, 12, 3, 3), F32)
    out = _dev((1, 3, 4, 4))
    for kw in (dict(w=w3, mode=0, out=out), dict(w=w1, mode=1, out=out), dict(w=w1, mode=0), dict(w=w3, mode=2, out=out),
               dict(w=w3, mode=3, composed=out), dict(w=w3, mode=4, out=out)):
        w = kw.pop("w")
        with pytest.raises(_lib.SketchEditHipError, match="output conv"):
            eng.output_conv(x, w, np.zeros(w.shape[0], F32), kw.pop("mode"), **kw)
    assert (_np(out) == F32(SENTINEL)).all()
