"""GPU parity tests of the bf16 path (BASELINE config 5: bf16 operands on v_mfma_f32_16x16x32_bf16, fp32 accumulate)
against the oracle's bf16 mode (oracle/sketchedit_oracle.py; pinned by tests/test_oracle_golden.py against the
reference run with the same roundings injected through module hooks, tests/golden/e2e_64_bf16.npz).

Tolerances.  The north star's 1e-3 bound is an fp32 statement; bf16 keeps 8 significant bits (relative spacing 2^-8).
  * one layer (same bf16 inputs and weights, fp32 accumulation, ONE rounding of the result): the GPU and the oracle can
    differ by the accumulation order only, i.e. by at most one bf16 spacing of the result (2^-8 .. 2^-7 of |y|) where a
    value sits on a rounding boundary: |d| <= 2^-7 |y| + 1e-6, and rarely: mean |d| < 2e-4.
  * a whole network: the roundings after every layer turn fp32-level differences into occasional one-spacing flips that
    propagate.  Two equally valid placements of the same roundings (fp64 vs fp32 accumulation, pre-summed sub-pixel
    weights vs the 3x3 on the upsampled grid) differ by 6e-3 .. 1.1e-2 on the soft mask and 3e-3 .. 6e-3 on the outputs at
    64x64 .. 128x128 (measured on the CPU).  Bound used here: 3e-2 max-abs, 3e-3 mean-abs at every size (no slack for
    large images); a handful of soft-mask pixels near 0.5 may threshold differently (<= 0.5 % of the pixels), so netG is
    compared on the oracle's hard mask.
  * what makes that bound a MEASURED one (test_bf16_error_triangle): on the same inputs and the same hard mask the HIP
    bf16 result must be no farther from the fp32 oracle than the bf16 oracle itself is -- max-abs and mean-abs of
    |HIP_bf16 - fp32 oracle| <= TRIANGLE x those of |bf16 oracle - fp32 oracle| -- i.e. the GPU path loses no more
    accuracy to bf16 than the reference-pinned CPU definition of the bf16 computation does.
"""
import os

import numpy as np
import pytest
import torch

from sketchedit_amd import synth
from forms_util import conv_as
from parity_util import layer_close as _layer_close

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
TOL_NET, TOL_NET_MEAN = 3e-2, 3e-3
TRIANGLE = 1.25
FLAGS = 1 | 2 | 16


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _np(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


@pytest.fixture(scope="module")
def eng():
    from sketchedit_amd._lib import Engine
    e = Engine(0)
    e.load_state_dict("M", synth.make_state_dict("M", 0))
    e.load_state_dict("G", synth.make_state_dict("G", 0))
    e.set_precision("bf16")
    yield e
    e.close()


SHAPES = [(96, 192, 1, 1, False, 3), (96, 192, 1, 16, False, 3), (96, 192, 1, 4, False, 3), (48, 192, 2, 1, False, 3),
          (48, 96, 1, 1, False, 3), (24, 96, 2, 1, False, 3), (96, 96, 1, 1, True, 3), (48, 48, 1, 1, True, 3),
          (24, 48, 2, 1, False, 3), (24, 24, 1, 1, False, 3), (4, 48, 1, 1, False, 5), (5, 48, 1, 1, False, 5),
          (3, 48, 1, 1, False, 5)]


@pytest.mark.parametrize("ll", [False, True], ids=["default", "lowlat"])
@pytest.mark.parametrize("shape", SHAPES, ids=["%d-%d-s%d-d%d-u%d-k%d" % s for s in SHAPES])
def test_op_gated_conv_bf16(eng, shape, ll):
    """Every layer shape of the network on the bf16 kernel, ragged sizes, both launch shapes."""
    from oracle import sketchedit_oracle as O
    cin, cout, s, r, up, k = shape
    H, W = (10, 14) if up else (22, 18)
    a = 1.5 / np.sqrt(cin * k * k)
    w = synth.uniform(31, "b16.w%s" % (shape,), (cout, cin, k, k), -a, a)
    b = synth.uniform(31, "b16.b%s" % (shape,), (cout,), -0.3, 0.3)
    x = synth.uniform(31, "b16.x%s" % (shape,), (3, cin, H, W), -1, 1)
    y = eng.gated_conv2d(_cuda(x), w, b, stride=s, rate=r, upsample=up, low_latency=ll, bf16=True)
    tw, tb, tx = torch.from_numpy(w), torch.from_numpy(b), torch.from_numpy(x)
    if up:
        # the kernel runs the sub-pixel form: its pre-summed weights are rounded once, the oracle rounds the 3x3 weights
        ref = O.gated_deconv(tx, tw, tb, BF)
        assert float(np.abs(_np(y) - _np(ref)).max()) < 2e-2
    else:
        _layer_close(y, O.gated_conv(tx, tw, tb, s, r, "elu", BF))


RCONV = [(1, 16, 16, "elu"), (1, 32, 48, "relu"), (1, 22, 18, "elu"), (2, 24, 32, "elu"), (4, 48, 64, "elu"), (2, 36, 28, "elu"),
         (1, 12, 12, "elu"), (8, 128, 96, "elu"),
         # sub-images 8 columns wide: two phases share an 8 x 16 tile (p.dual) -- full 8 x 8, ragged rows, dilation 16 at 128 x 128
         (4, 32, 32, "elu"), (8, 64, 64, "relu"), (8, 48, 64, "elu"), (16, 128, 128, "elu"), (2, 8, 16, "elu")]


@pytest.mark.parametrize("case", RCONV, ids=["d%d-%dx%d-%s" % c for c in RCONV])
def test_op_rconv16_raw_tile_bf16(eng, case):
    """96 -> 192 3x3 stride 1 in the raw-tile form (se_rconv16.hip): exact and ragged 8x16 tiles, the image borders (zero
    padding through the buffer range check), dilations through the polyphase sub-images."""
    from oracle import sketchedit_oracle as O
    d, H, W, act = case
    a = 1.5 / np.sqrt(96 * 9)
    w = synth.uniform(41, "rc.w%s" % (case,), (192, 96, 3, 3), -a, a)
    b = synth.uniform(41, "rc.b%s" % (case,), (192,), -0.3, 0.3)
    x = synth.uniform(41, "rc.x%s" % (case,), (2, 96, H, W), -1, 1)
    form = "rconv16" if H // d >= 12 and W // d >= 12 else "rconv16_dual"
    y = conv_as(eng, form, _cuda(x), w, b, stride=1, rate=d, act=act, bf16=True)
    _layer_close(y, O.gated_conv(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b), 1, d, act, BF))


RCONV96 = [(48, False, 16, 16, "elu"), (48, False, 22, 18, "elu"), (48, False, 40, 33, "relu"), (24, False, 22, 18, "elu"),
           (24, False, 32, 48, "elu"), (96, True, 16, 16, "elu"), (96, True, 22, 18, "elu"), (96, True, 12, 35, "elu")]


@pytest.mark.parametrize("case", RCONV96, ids=["c%d-u%d-%dx%d-%s" % c for c in RCONV96])
def test_op_rconv96_raw_tile_bf16(eng, case):
    """The 96-row stride-1 layers in the raw-tile form (se_rconv96.hip): 3x3 48 -> 96 (a 32-k step straddles two taps),
    24 -> 96 (padded pixel stride), gen_deconv 96 -> 96 (sub-pixel classes); exact and ragged 16x16 tiles, image borders."""
    from oracle import sketchedit_oracle as O
    cin, up, H, W, act = case
    a = 1.5 / np.sqrt(cin * 9)
    w = synth.uniform(43, "r96.w%s" % (case,), (96, cin, 3, 3), -a, a)
    b = synth.uniform(43, "r96.b%s" % (case,), (96,), -0.3, 0.3)
    x = synth.uniform(43, "r96.x%s" % (case,), (2, cin, H, W), -1, 1)
    form = "rconv96_up" if up else "rconv96" if cin == 48 else "rconv96_c24"
    y = conv_as(eng, form, _cuda(x), w, b, stride=1, rate=1, act=act, upsample=up, bf16=True)
    tw, tb, tx = torch.from_numpy(w), torch.from_numpy(b), torch.from_numpy(x)
    if up:
        ref = O.gated_deconv(tx, tw, tb, BF)       # pre-summed sub-pixel weights are rounded once (see above)
        assert float(np.abs(_np(y) - _np(ref)).max()) < 2e-2
    else:
        _layer_close(y, O.gated_conv(tx, tw, tb, 1, 1, act, BF))


@pytest.mark.parametrize("kind", ["tensor", "vector"])
def test_op_two_source_conv_bf16(eng, kind):
    """conv11 / allconv11 in bf16 mode at 14x18: the tensor source through the gather-GEMM's two-source gather, the vector
    source folded into a bias table (launch_vecbias with the vector rounded to bf16) in front of the raw-tile kernel on the
    first source alone (se_rconv16.hip; h, w >= 12)."""
    from oracle import sketchedit_oracle as O
    H, W = 14, 18
    a = 1.5 / np.sqrt(192 * 9)
    w = synth.uniform(37, "b16two.w" + kind, (192, 192, 3, 3), -a, a)
    b = synth.uniform(37, "b16two.b" + kind, (192,), -0.3, 0.3)
    x = synth.uniform(37, "b16two.x" + kind, (2, 96, H, W), -1, 1)
    if kind == "tensor":
        x1 = synth.uniform(37, "b16two.y", (2, 96, H, W), -1, 1)
        cat = np.concatenate([x, x1], 1)
    else:
        x1 = synth.uniform(37, "b16two.v", (2, 96), -1, 1)
        cat = np.concatenate([x, np.broadcast_to(x1[:, :, None, None], (2, 96, H, W))], 1)
    form = "gconv_n192_2src_bf16" if kind == "tensor" else ["vecbias", "rconv16"]
    y = conv_as(eng, form, _cuda(x), w, b, x1=_cuda(x1), bf16=True)
    _layer_close(y, O.gated_conv(torch.from_numpy(cat), torch.from_numpy(w), torch.from_numpy(b), 1, 1, "elu", BF))


@pytest.mark.parametrize("shape", [(2, 16, 12), (2, 16, 16), (1, 24, 40), (1, 132, 136)], ids=lambda s: "%dx%dx%d" % s)
def test_op_attention_bf16(eng, shape):
    """bf16 keys / probabilities / values, fp32 scores and softmax; soft (non-saturated) scores.  16x12: class grid 8x6
    (element-load box sum); 16x16 / 24x40: wc % 4 == 0 (vector box sum); 132x136: 4488 class-grid pixels, the softmax
    form for rows that do not fit in registers."""
    from oracle import sketchedit_oracle as O
    B, h, w = shape
    x = 0.004 * synth.uniform(5, "att96s.x%d" % h, (B, 96, h, w), -1, 1)
    full = (synth.uniform(5, "att96s.m%d" % h, (B, 1, 4 * h, 4 * w), 0, 1) < 0.5).astype(np.float32)
    full[0, :, :, 2 * w:] = 1.0
    out, sim = eng.attention(_cuda(x), _cuda(full), want_similar=True, bf16=True)
    xr = torch.from_numpy(x).to(BF).float()
    ro, rp = O.contextual_attention(xr, torch.from_numpy(full), BF)
    # P: fp32 softmax of fp32-accumulated bf16 products, stored rounded to bf16 (the oracle rounds it before the
    # reconstruction, attention_reconstruct): one bf16 step where the fp32 values differ in the last bits
    rp = _np(rp)
    assert bool((np.abs(_np(sim) - rp) <= 2.0 ** -8 * np.abs(rp) + 1e-6).all())
    # out: sums of <= 4L products of bf16 P (box-summed and rounded once more on the GPU) and bf16 values
    assert float(np.abs(_np(out) - _np(ro)).max()) < 2.0 ** -7 * float(ro.abs().max())


def test_netM_and_netG_64_bf16_golden(eng, golden_dir):
    """The reference itself with the bf16 roundings injected through hooks (tests/golden/make_golden.py)."""
    g = dict(np.load(os.path.join(golden_dir, "e2e_64_bf16.npz")))
    img, sk = synth.make_inputs(2, 64, 64, seed=1234)
    ci, cs = _cuda(img), _cuda(sk)
    mask, mim = eng.netM(ci, cs)
    for got, want in ((mask, g["mask"]), (mim, g["mask_image"])):
        d = np.abs(_np(got) - want)
        assert d.max() < TOL_NET and d.mean() < TOL_NET_MEAN
    hard = _cuda(g["hard_mask"])
    coarse, fine = eng.netG(ci, ci, hard, hard, cs, FLAGS)
    for got, want in ((coarse, g["coarse"]), (fine, g["fine"])):
        d = np.abs(_np(got) - want)
        assert d.max() < TOL_NET and d.mean() < TOL_NET_MEAN


def test_netG_taps_bf16_vs_oracle_bf16(eng):
    """se_netG_forward_taps in bf16 mode (the tapped tensors leave through the bf16 layout converters): the style vector (fp32 in
    both modes), the attention's input and the production attention's output against the oracle's bf16-mode taps."""
    from oracle import sketchedit_oracle as O
    img, sk = synth.make_inputs(2, 64, 64, seed=1234)
    g_hard = (synth.uniform(3, "taps16.hard", (2, 1, 64, 64), 0, 1) < 0.5).astype(np.float32)
    WG = synth.make_state_dict("G", 0)
    taps = {}
    with torch.no_grad():
        O.netG_forward(WG, img, img, g_hard, g_hard, sk, taps=taps, act_dtype=BF)
    ci, cs, ch = _cuda(img), _cuda(sk), _cuda(g_hard)
    r = eng.netG_taps(ci, ci, ch, ch, cs, FLAGS)
    assert set(r) >= {"pmconv6", "attn_out", "style_vec", "coarse", "fine"}
    for k, scale in (("style_vec", 1.0), ("pmconv6", 1.0), ("attn_out", 1.0)):
        want = taps[k]
        d = np.abs(_np(r[k]) - _np(want))
        assert d.max() < 4 * TOL_NET * max(1.0, float(want.abs().max())) and d.mean() < 4 * TOL_NET_MEAN * max(1.0, float(want.abs().mean())), k


@pytest.mark.parametrize("case", [(2, 64, 64, True), (1, 128, 128, False), (1, 40, 72, True), (1, 256, 256, False)],
                         ids=["2x64-lowlat", "1x128", "1x40x72-lowlat", "1x256"])
def test_inference_bf16_vs_oracle_bf16(eng, case):
    from oracle import sketchedit_oracle as O
    B, H, W, ll = case
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    img, sk = synth.make_inputs(B, H, W, seed=1234)
    WM, WG = synth.make_state_dict("M", 0), synth.make_state_dict("G", 0)
    ref = O.inference(WM, WG, img, sk, act_dtype=BF)
    ref32 = O.inference(WM, WG, img, sk)
    r = eng.inference(_cuda(img), _cuda(sk), FLAGS, visualize=True, low_latency=ll)
    d = np.abs(_np(r["mask"]) - _np(ref["mask"]))
    assert d.max() < TOL_NET and d.mean() < TOL_NET_MEAN
    flips = float((_np(r["hard"]) != _np(ref["hard_mask"])).mean())
    assert flips < 5e-3, "hard-mask flips: %.4f of the pixels" % flips
    hard = ref["hard_mask"].cuda()
    ci, cs = _cuda(img), _cuda(sk)
    coarse, fine = eng.netG(ci, ci, hard, hard, cs, FLAGS)
    for got, want in ((coarse, ref["coarse"]), (fine, ref["fine"])):
        d = np.abs(_np(got) - _np(want))
        assert d.max() < TOL_NET and d.mean() < TOL_NET_MEAN
    # against the fp32 oracle the bf16 path is a bf16 computation: reported, loosely bounded
    d32 = np.abs(_np(fine) - _np(O.netG_forward(WG, img, img, ref["hard_mask"], ref["hard_mask"], sk)[1]))
    assert d32.mean() < 2e-2
    assert torch.isfinite(r["composed"]).all()
    comp = r["fine"] * r["mask"] + ci * (1 - r["mask"])
    assert float((comp - r["composed"]).abs().max()) < 1e-6
    del ref32


def test_bf16_batch_shard_invariance_and_config5_size(eng):
    """BASELINE config 5 size (512x512): finite outputs, composite identity, image k independent of its batch."""
    img, sk = synth.make_inputs(4, 512, 512, seed=99)
    ci, cs = _cuda(img), _cuda(sk)
    r = eng.inference(ci, cs, FLAGS, visualize=True, low_latency=False)
    for k in ("composed", "mask", "fine", "coarse"):
        assert torch.isfinite(r[k]).all(), k
    assert float(r["mask"].min()) >= 0 and float(r["mask"].max()) <= 1
    comp = r["fine"] * r["mask"] + ci * (1 - r["mask"])
    assert float((comp - r["composed"]).abs().max()) < 1e-6
    one = eng.inference(ci[2:3].contiguous(), cs[2:3].contiguous(), FLAGS, low_latency=False)
    assert torch.equal(one["composed"], r["composed"][2:3])


@pytest.mark.parametrize("size", [64, 128, 256])
def test_bf16_error_triangle(eng, size):
    """|HIP_bf16 - fp32 oracle| <= 1.25 x |bf16 oracle - fp32 oracle| (max-abs and mean-abs), on the soft mask of netM and
    on both outputs of netG, all three computations fed the SAME hard mask (the fp32 oracle's)."""
    from oracle import sketchedit_oracle as O
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    B = 2 if size <= 64 else 1
    img, sk = synth.make_inputs(B, size, size, seed=1234)
    WM, WG = synth.make_state_dict("M", 0), synth.make_state_dict("G", 0)
    ref32 = O.inference(WM, WG, img, sk)
    hard = ref32["hard_mask"]
    with torch.no_grad():
        m16, _ = O.netM_forward(WM, torch.from_numpy(img), torch.from_numpy(sk), act_dtype=BF)
        c16, f16 = O.netG_forward(WG, img, img, hard, hard, sk, act_dtype=BF)
    ci, cs = _cuda(img), _cuda(sk)
    gm, _ = eng.netM(ci, cs, want_image=False)
    gc, gf = eng.netG(ci, ci, hard.cuda(), hard.cuda(), cs, FLAGS)
    report = {}
    for name, got, o16, o32 in (("mask", gm, m16, ref32["mask"]), ("coarse", gc, c16, ref32["coarse"]), ("fine", gf, f16, ref32["fine"])):
        d_hip = np.abs(_np(got).astype(np.float64) - _np(o32))
        d_or = np.abs(_np(o16).astype(np.float64) - _np(o32))
        report[name] = (d_hip.max(), d_or.max(), d_hip.mean(), d_or.mean())
    print("bf16 triangle %d: " % size + "  ".join("%s max %.2e/%.2e mean %.2e/%.2e" % ((k,) + v) for k, v in report.items()))
    for name, (hmax, omax, hmean, omean) in report.items():
        assert hmean <= TRIANGLE * omean, "%s: mean |HIP-fp32| %.3e > %.2f x mean |oracle_bf16-fp32| %.3e" % (name, hmean, TRIANGLE, omean)
        assert hmax <= TRIANGLE * omax, "%s: max |HIP-fp32| %.3e > %.2f x max |oracle_bf16-fp32| %.3e" % (name, hmax, TRIANGLE, omax)


@pytest.mark.timeout(1200)
def test_config5_full_size(eng):
    """BASELINE config 5 at ITS size -- 512x512, batch 16, bf16 -- in the suite (not only in bench.py): images 0 and 9 of
    the batch against the oracle's bf16 mode (soft mask of the batch-16 run; netG's outputs from a batch-16 netG call in
    which these two images get the oracle's hard mask, so that a threshold flip does not change their input), plus the
    size-independent properties on all 16 images."""
    from oracle import sketchedit_oracle as O
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    B, S, picks = 16, 512, (0, 9)
    img, sk = synth.make_inputs(B, S, S, seed=1234)
    WM, WG = synth.make_state_dict("M", 0), synth.make_state_dict("G", 0)
    ci, cs = _cuda(img), _cuda(sk)
    r = eng.inference(ci, cs, FLAGS, visualize=True, low_latency=False)
    for k in ("composed", "mask", "fine", "coarse"):
        assert torch.isfinite(r[k]).all(), k
    assert float(r["mask"].min()) >= 0 and float(r["mask"].max()) <= 1
    assert torch.equal(r["hard"], (r["mask"] > 0.5).float())
    comp = r["fine"] * r["mask"] + ci * (1 - r["mask"])
    assert float((comp - r["composed"]).abs().max()) < 1e-6
    hard_mix = r["hard"].clone()
    refs = {}
    for k in picks:
        refs[k] = O.inference(WM, WG, img[k:k + 1], sk[k:k + 1], act_dtype=BF)
        d = np.abs(_np(r["mask"][k:k + 1]) - _np(refs[k]["mask"]))
        assert d.max() < TOL_NET and d.mean() < TOL_NET_MEAN, (k, d.max(), d.mean())
        flips = float((_np(r["hard"][k:k + 1]) != _np(refs[k]["hard_mask"])).mean())
        assert flips < 5e-3, "image %d: hard-mask flips on %.4f of the pixels" % (k, flips)
        hard_mix[k:k + 1] = refs[k]["hard_mask"].cuda()
    coarse, fine = eng.netG(ci, ci, hard_mix, hard_mix, cs, FLAGS)
    for k in picks:
        for got, want in ((coarse[k:k + 1], refs[k]["coarse"]), (fine[k:k + 1], refs[k]["fine"])):
            d = np.abs(_np(got) - _np(want))
            assert d.max() < TOL_NET and d.mean() < TOL_NET_MEAN, (k, d.max(), d.mean())
    # an image's result does not depend on its batch: image 9 alone, same mode
    one = eng.inference(ci[9:10].contiguous(), cs[9:10].contiguous(), FLAGS, low_latency=False)
    assert torch.equal(one["composed"], r["composed"][9:10]) and torch.equal(one["mask"], r["mask"][9:10])
