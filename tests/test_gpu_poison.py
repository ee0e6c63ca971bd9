"""Poisoned scratch memory (SE_TEST_POISON): no result may depend on a byte nobody wrote.

Every kernel here reads activations that live in recycled scratch memory, and many read bytes they do not own: pad channels
of the bf16 layouts, pad columns and guard bands of the attention's E, ragged last tiles.  Whether that is harmless depends on
what the bytes held, which the other tests do not control (fresh driver memory is mostly zero -- the one value that hides it).
With SE_TEST_POISON = v the library fills every scratch region with the byte v when it hands it out, and each test here fills
the caller's workspace and the outputs it may supply with v too.

The assertion is the same everywhere: the same call with v = 0 (off), 0xFF, 0x47, 0xC7 --
  * 0xFF.. is a NaN in fp32, bf16 and fp16: every arithmetic use of a stale value, `stale x 0` included, shows;
  * 0x4747.. / 0xC7C7.. are +-5.1e4 in fp32 and bf16 (+-7.3 in fp16), finite: a stale value that enters a max, a min or a
    comparison shows (a NaN does not: v_max_f32 returns the other operand);
the three poisoned runs are torch.equal to the unpoisoned one on every output and every fp32 output is finite.  No tolerance,
no oracle: correctness of the unpoisoned run is what the other tests check, at these same shapes (the lists are theirs)."""
import numpy as np
import pytest
import torch

from sketchedit_amd import _lib, synth
from test_gpu_bf16 import RCONV, RCONV96, SHAPES
from test_gpu_parity import C24, NET_SHAPES, SMALL_SIZES, TWO_SRC, WINO, WINO24, WINO48, WINOUP

pytestmark = pytest.mark.gpu

POISONS = (0, 0xFF, 0x47, 0xC7)
FLAGS = 1 | 2 | 16   # use_cam, pool max, joint_train_inp


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    e.load_state_dict("M", synth.make_state_dict("M", 0))
    e.load_state_dict("G", synth.make_state_dict("G", 0))
    assert e.weights_ready()
    yield e
    e.close()


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _u8(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint8)).cuda()


def _bytes(t, v):
    """every byte of t := v"""
    t.view(torch.uint8).fill_(v)
    return t


def _four(seopt, call):
    """call(v) -> {name: tensor} under SE_TEST_POISON = v, for the four values; the comparison described above"""
    outs = []
    for v in POISONS:
        seopt.set("SE_TEST_POISON", v)
        outs.append({k: t.clone() for k, t in call(v).items()})
    seopt.set("SE_TEST_POISON", 0)
    torch.cuda.synchronize()
    base = outs[0]
    assert base
    for k, t in base.items():
        if t.is_floating_point():
            assert bool(torch.isfinite(t).all()), "%s of the unpoisoned run is not finite" % k
    for v, o in zip(POISONS[1:], outs[1:]):
        assert o.keys() == base.keys()
        for k, t in base.items():
            if o[k].is_floating_point():
                assert bool(torch.isfinite(o[k]).all()), "%s is not finite under poison 0x%02X" % (k, v)
            assert torch.equal(t, o[k]), "%s changes under poison 0x%02X: %d of %d elements differ" % (
                k, v, int((t != o[k]).sum()), t.numel())
    return base


# ---- per-op gated conv ------------------------------------------------------------------------------------------------------
def _conv_case(seed, tag, B, cin, cout, k, H, W):
    a = 1.5 / np.sqrt(cin * k * k)
    w = synth.uniform(seed, tag + ".w", (cout, cin, k, k), -a, a)
    b = synth.uniform(seed, tag + ".b", (cout,), -0.3, 0.3)
    x = _cuda(synth.uniform(seed, tag + ".x", (B, cin, H, W), -1, 1))
    return x, w, b


def _conv4(seopt, eng, x, w, b, **kw):
    return _four(seopt, lambda v: {"y": eng.gated_conv2d(x, w, b, **kw)})


@pytest.mark.parametrize("ll", [False, True], ids=["default", "lowlat"])
@pytest.mark.parametrize("shape", NET_SHAPES, ids=["%d-%d-s%d-d%d-u%d-k%d" % s for s in NET_SHAPES])
def test_conv_network_shapes(eng, seopt, shape, ll):
    cin, cout, s, r, up, k = shape
    H, W = (10, 14) if up else (22, 18)
    x, w, b = _conv_case(11, "ns%s" % (shape,), 3, cin, cout, k, H, W)
    _conv4(seopt, eng, x, w, b, stride=s, rate=r, upsample=up, low_latency=ll)


@pytest.mark.parametrize("f43", [1, 0])
@pytest.mark.parametrize("case", WINO24, ids=["d%d-%dx%d-%s" % c for c in WINO24])
def test_conv_winograd_f43(eng, seopt, case, f43):
    d, H, W, act = case
    seopt.set("SE_WINOGRAD_F43", f43)
    x, w, b = _conv_case(17, "w24%s" % (case,), 3, 96, 192, 3, H, W)
    _conv4(seopt, eng, x, w, b, rate=d, act=act)


@pytest.mark.parametrize("wino", [1, 0])
@pytest.mark.parametrize("case", WINO, ids=["d%d-%dx%d-%s" % c for c in WINO])
def test_conv_winograd_f22(eng, seopt, case, wino):
    d, H, W, act = case
    seopt.set("SE_WINOGRAD_F43", 0)
    seopt.set("SE_WINOGRAD", wino)
    x, w, b = _conv_case(13, "wino%s" % (case,), 3, 96, 192, 3, H, W)
    _conv4(seopt, eng, x, w, b, rate=d, act=act)


@pytest.mark.parametrize("wx", [2, 1, 0])
@pytest.mark.parametrize("case", C24, ids=["%dx%d-%s" % c for c in C24])
def test_conv_24_to_24(eng, seopt, case, wx):
    H, W, act = case
    seopt.set("SE_RTILE_WX", wx)
    x, w, b = _conv_case(23, "c24%s" % (case,), 2, 24, 24, 3, H, W)
    _conv4(seopt, eng, x, w, b, act=act)


@pytest.mark.parametrize("wino48", [1, 0])
@pytest.mark.parametrize("cin", [48, 24])
@pytest.mark.parametrize("case", WINO48, ids=["d%d-%dx%d-%s" % c for c in WINO48])
def test_conv_winograd48(eng, seopt, case, cin, wino48):
    d, H, W, act = case
    seopt.set("SE_WINOGRAD48", wino48)
    x, w, b = _conv_case(17, "wino48.%d%s" % (cin, case), 3, cin, 96, 3, H, W)
    _conv4(seopt, eng, x, w, b, rate=d, act=act)


@pytest.mark.parametrize("winoup", [1, 0])
@pytest.mark.parametrize("cin", [96, 48])
@pytest.mark.parametrize("case", WINOUP, ids=["%dx%d-%s" % c for c in WINOUP])
def test_conv_winograd_upsample(eng, seopt, case, cin, winoup):
    H, W, act = case
    seopt.set("SE_WINOGRAD_UP", winoup)
    x, w, b = _conv_case(19, "winoup%d%s" % (cin, case), 3, cin, cin, 3, H, W)
    _conv4(seopt, eng, x, w, b, upsample=True, act=act)


@pytest.mark.parametrize("form", [(False, 1), (False, 0), (True, 1)], ids=["f43", "f22", "lowlat"])
@pytest.mark.parametrize("case", TWO_SRC, ids=["%s-%dx%d" % c[:3] for c in TWO_SRC])
def test_conv_two_sources(eng, seopt, case, form):
    kind, H, W, d = case
    ll, f43 = form
    seopt.set("SE_WINOGRAD_F43", f43)
    x, w, b = _conv_case(23, "two%s" % (case,), 3, 96, 192, 3, H, W)
    w = np.concatenate([w, synth.uniform(23, "two.w1%s" % (case,), (192, 96, 3, 3), -0.03, 0.03)], 1)
    x1 = _cuda(synth.uniform(23, "two.y%s" % (case,), (3, 96, H, W) if kind == "tensor" else (3, 96), -1, 1))
    _conv4(seopt, eng, x, w, b, rate=d, x1=x1, low_latency=ll)


@pytest.mark.parametrize("vecbias", [1, 0])
@pytest.mark.parametrize("size", [(16, 16), (12, 20), (2, 8), (64, 64)], ids=lambda s: "%dx%d" % s)
def test_conv_folded_vector_source(eng, seopt, size, vecbias):
    H, W = size
    seopt.set("SE_VECBIAS", vecbias)
    x, w, b = _conv_case(53, "vb%d" % H, 3, 96, 192, 3, H, W)
    w = np.concatenate([w, synth.uniform(53, "vb.w1", (192, 96, 3, 3), -0.03, 0.03)], 1)
    v1 = _cuda(synth.uniform(53, "vb.v", (3, 96), -1, 1))
    _conv4(seopt, eng, x, w, b, x1=v1)


@pytest.mark.parametrize("dense", [1, 0])
@pytest.mark.parametrize("case", [(5, 22, 18), (3, 22, 18), (4, 22, 18), (5, 8, 16), (3, 40, 33), (4, 16, 48), (5, 9, 70)],
                         ids=lambda c: "c%d-%dx%d" % c)
def test_conv_first_layer_dense_k(eng, seopt, case, dense):
    cin, H, W = case
    seopt.set("SE_RTILE_DENSE", dense)
    x, w, b = _conv_case(47, "d5%s" % (case,), 3, cin, 48, 5, H, W)
    _conv4(seopt, eng, x, w, b)


@pytest.mark.parametrize("d5w", [1, 0])
@pytest.mark.parametrize("case", [(5, 22, 18), (3, 22, 18), (4, 22, 18), (5, 8, 16), (3, 40, 34), (4, 16, 48), (5, 9, 70), (3, 5, 2)],
                         ids=lambda c: "c%d-%dx%d" % c)
def test_conv_first_layer_winograd_along_x(eng, seopt, case, d5w):
    cin, H, W = case
    seopt.set("SE_RTILE_D5W", d5w)
    x, w, b = _conv_case(59, "d5w%s" % (case,), 2, cin, 48, 5, H, W)
    _conv4(seopt, eng, x, w, b)


def test_conv_first_layer_dense_k_sub_launches(eng, seopt):
    seopt.set("SE_TEST_OFFSET_LIMIT", 2 * 24 * 40 * 8 * 4 + 1)      # two images per sub-launch: 2 + 2 + 1
    x, w, b = _conv_case(61, "dk", 5, 5, 48, 5, 24, 40)
    _conv4(seopt, eng, x, w, b)


@pytest.mark.parametrize("ll", [False, True], ids=["default", "lowlat"])
@pytest.mark.parametrize("shape", SHAPES, ids=["%d-%d-s%d-d%d-u%d-k%d" % s for s in SHAPES])
def test_conv_bf16_network_shapes(eng, seopt, shape, ll):
    cin, cout, s, r, up, k = shape
    H, W = (10, 14) if up else (22, 18)
    x, w, b = _conv_case(31, "b16%s" % (shape,), 3, cin, cout, k, H, W)
    _conv4(seopt, eng, x, w, b, stride=s, rate=r, upsample=up, low_latency=ll, bf16=True)


RCONV_SMALL = [c for c in RCONV if c[1:3] not in ((128, 128), (128, 96))]


@pytest.mark.parametrize("case", RCONV_SMALL, ids=["d%d-%dx%d-%s" % c for c in RCONV_SMALL])
def test_conv_bf16_rconv16(eng, seopt, case):
    d, H, W, act = case
    x, w, b = _conv_case(41, "rc%s" % (case,), 2, 96, 192, 3, H, W)
    _conv4(seopt, eng, x, w, b, rate=d, act=act, bf16=True)


@pytest.mark.parametrize("case", RCONV96, ids=["c%d-u%d-%dx%d-%s" % c for c in RCONV96])
def test_conv_bf16_rconv96(eng, seopt, case):
    cin, up, H, W, act = case
    x, w, b = _conv_case(43, "r96%s" % (case,), 2, cin, 96, 3, H, W)
    _conv4(seopt, eng, x, w, b, act=act, upsample=up, bf16=True)


@pytest.mark.parametrize("kind", ["tensor", "vector"])
def test_conv_bf16_two_sources(eng, seopt, kind):
    H, W = 14, 18
    x, w, b = _conv_case(37, "b16two" + kind, 2, 96, 192, 3, H, W)
    w = np.concatenate([w, synth.uniform(37, "b16two.w1", (192, 96, 3, 3), -0.03, 0.03)], 1)
    x1 = _cuda(synth.uniform(37, "b16two.y", (2, 96, H, W) if kind == "tensor" else (2, 96), -1, 1))
    _conv4(seopt, eng, x, w, b, x1=x1, bf16=True)


# ---- per-op attention -------------------------------------------------------------------------------------------------------
ATT_SHAPES = [(2, 16, 12), (2, 16, 16), (1, 24, 40), (2, 64, 64), (1, 20, 248)]
ATT_FORMS = {"default": {}, "fused": {"SE_ATT_FUSED": 1, "SE_ATT_FUSED_BF16": 1},
             "fused-ptilde-r3": {"SE_ATT_FUSED": 1, "SE_ATT_FUSED_BF16": 1, "SE_ATT_PTILDE_LDS": 0},
             "fused-stats-r3": {"SE_ATT_FUSED": 1, "SE_ATT_FUSED_BF16": 1, "SE_ATT_STATS_LDS": 0},
             "fused-e32": {"SE_ATT_FUSED": 1, "SE_ATT_FUSED_BF16": 1, "SE_ATT_E16": 0},
             "three-pass": {"SE_ATT_FUSED": 0, "SE_ATT_FUSED_BF16": 0},
             "three-pass-e32": {"SE_ATT_FUSED": 0, "SE_ATT_FUSED_BF16": 0, "SE_ATT_E16": 0},
             "all-tiles": {"SE_ATT_SYM": 0}}


def _att_inputs(shape):
    B, h, w = shape
    x = 0.004 * synth.uniform(5, "att96s.x%d" % h, (B, 96, h, w), -1, 1)
    full = (synth.uniform(5, "att96s.m%d" % h, (B, 1, 4 * h, 4 * w), 0, 1) < 0.5).astype(np.float32)
    full[0, :, :, 2 * w:] = 1.0
    return _cuda(x), _cuda(full)


def _att4(seopt, eng, x, full, bf16, similar):
    def call(v):
        r = eng.attention(x, full, want_similar=similar, bf16=bf16)
        return {"out": r[0], "similar": r[1]} if similar else {"out": r}
    return _four(seopt, call)


def _set_form(seopt, form):
    for name, val in ATT_FORMS[form].items():
        seopt.set(name, val)


@pytest.mark.parametrize("form", list(ATT_FORMS))
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", ATT_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_attention_forms(eng, seopt, shape, bf16, form):
    _set_form(seopt, form)
    x, full = _att_inputs(shape)
    _att4(seopt, eng, x, full, bf16, False)


# `similar_out` is P itself: a call that asks for it always takes the three-pass form (launch_attention_v2_t), so the switches
# of the fused form change nothing there -- only the forms such a call can tell apart
SIMILAR_FORMS = ["default", "three-pass-e32", "all-tiles"]


@pytest.mark.parametrize("form", SIMILAR_FORMS)
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", ATT_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_attention_forms_with_similar(eng, seopt, shape, bf16, form):
    _set_form(seopt, form)
    x, full = _att_inputs(shape)
    _att4(seopt, eng, x, full, bf16, True)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", ATT_SHAPES[:4], ids=lambda s: "%dx%dx%d" % s)
def test_attention_streaming_form(eng, seopt, shape, bf16):
    seopt.set("SE_ATT_STREAM", 1)
    x, full = _att_inputs(shape)
    _att4(seopt, eng, x, full, bf16, False)


@pytest.mark.parametrize("similar", [False, True], ids=["out", "similar"])
@pytest.mark.parametrize("shape", [(1, 12, 8), (1, 42, 8), (1, 10, 80), (2, 6, 40)], ids=lambda s: "%dx%dx%d" % s)
def test_attention_bf16_pad_columns(eng, seopt, shape, similar):
    """R % 64 in 1..32 in bf16 mode: the deterministic form of test_attention_pad_columns_are_finite_in_bf16_mode -- with
    32-key tiles of the E GEMM the columns R .. Rp-1 were left unwritten and the fused passes read them."""
    B, h, w = shape
    x = _cuda(synth.uniform(9, "padc.x%d" % h, (B, 96, h, w), -1, 1))
    full = _cuda((synth.uniform(9, "padc.m%d" % h, (B, 1, 4 * h, 4 * w), 0, 1) < 0.5).astype(np.float32))
    _att4(seopt, eng, x, full, True, similar)


@pytest.mark.parametrize("similar", [False, True], ids=["out", "similar"])
@pytest.mark.parametrize("form", ["default", "fused", "fused-stats-r3", "fused-ptilde-r3", "three-pass"])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_attention_all_keys_invalid(eng, seopt, bf16, form, similar):
    """every key has kmul = 0 and the row maxima run over masked scores only.  8 x 8: wc = 4, the LDS-staged fused kernels
    (without `similar`; with it the call takes the three-pass form whatever the switches say)"""
    _set_form(seopt, form)
    x = _cuda(synth.uniform(5, "att96b.x", (1, 96, 8, 8), -1, 1))
    _att4(seopt, eng, x, _cuda(np.ones((1, 1, 32, 32), np.float32)), bf16, similar)


# ---- forwards ---------------------------------------------------------------------------------------------------------------
MODES = {"default": ("f32", False, False), "lowlat": ("f32", True, False), "bf16": ("bf16", False, False),
         "bf16-lowlat": ("bf16", True, False), "conservative": ("f32", False, True)}
FWD_SIZES = [(2, 64, 64), (1, 40, 72)] + [s for s in SMALL_SIZES if s in ((2, 24, 16), (1, 16, 40), (1, 104, 88))]


class _mode:
    """precision / conservative of the module's Engine for one test; -> low_latency"""

    def __init__(self, eng, mode):
        self.eng, (self.prec, self.ll, self.cons) = eng, MODES[mode]

    def __enter__(self):
        self.eng.set_precision(self.prec)
        self.eng.set_conservative(self.cons)
        return self.ll

    def __exit__(self, *a):
        self.eng.set_precision("f32")
        self.eng.set_conservative(False)


def _inputs(B, H, W, seed=1234):
    img, sk = synth.make_inputs(B, H, W, seed=seed)
    return _cuda(img), _cuda(sk)


def _ws_fill(eng, v, B, H, W):
    _bytes(eng.workspace(B, H, W), v)


def _empty(v, shape, dtype=torch.float32):
    return _bytes(torch.empty(shape, dtype=dtype, device="cuda"), v)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("size", FWD_SIZES, ids=lambda s: "%dx%dx%d" % s)
def test_inference(eng, seopt, size, mode):
    B, H, W = size
    ci, cs = _inputs(B, H, W)
    assert len(FWD_SIZES) == 5
    with _mode(eng, mode) as ll:
        def call(v):
            _ws_fill(eng, v, B, H, W)
            out = {"composed": _empty(v, (B, 3, H, W)), "mask": _empty(v, (B, 1, H, W))}
            return eng.inference(ci, cs, FLAGS, out=out, low_latency=ll)
        _four(seopt, call)


@pytest.mark.parametrize("mode", ["default", "bf16"])
def test_inference_every_output(eng, seopt, mode):
    B, H, W = 2, 64, 64
    ci, cs = _inputs(B, H, W)
    with _mode(eng, mode) as ll:
        def call(v):
            _ws_fill(eng, v, B, H, W)
            out = {"composed": _empty(v, (B, 3, H, W)), "mask": _empty(v, (B, 1, H, W))}
            return eng.inference(ci, cs, FLAGS, visualize=True, out=out, low_latency=ll)
        r = _four(seopt, call)
    assert set(r) == {"composed", "mask", "hard", "maskim", "coarse", "fine"}


@pytest.mark.parametrize("mode", ["default", "bf16"])
@pytest.mark.parametrize("want_image", [True, False], ids=["image", "mask-only"])
def test_netM(eng, seopt, want_image, mode):
    B, H, W = 2, 64, 64
    ci, cs = _inputs(B, H, W)
    with _mode(eng, mode):
        def call(v):
            _ws_fill(eng, v, B, H, W)
            mask, mim = eng.netM(ci, cs, want_image=want_image)
            return {"mask": mask, "maskim": mim} if want_image else {"mask": mask}
        _four(seopt, call)


@pytest.mark.parametrize("mode", ["default", "bf16"])
@pytest.mark.parametrize("taps", [False, True], ids=["netG", "netG_taps"])
def test_netG(eng, seopt, taps, mode):
    B, H, W = 2, 64, 64
    ci, cs = _inputs(B, H, W)
    hard = _cuda((synth.uniform(3, "poison.hard", (B, 1, H, W), 0, 1) < 0.5).astype(np.float32))
    with _mode(eng, mode):
        def call(v):
            _ws_fill(eng, v, B, H, W)
            if taps:
                return eng.netG_taps(ci, ci, hard, hard, cs, FLAGS)
            coarse, fine = eng.netG(ci, ci, hard, hard, cs, FLAGS)
            return {"coarse": coarse, "fine": fine}
        r = _four(seopt, call)
    assert not taps or set(r) == {"coarse", "fine", "pmconv6", "attn_out", "style_vec"}


@pytest.mark.parametrize("mode", ["default", "bf16"])
def test_inference_streaming_attention(eng, seopt, mode):
    B, H, W = 2, 64, 64
    ci, cs = _inputs(B, H, W)
    seopt.set("SE_ATT_STREAM", 1)
    with _mode(eng, mode) as ll:
        def call(v):
            _ws_fill(eng, v, B, H, W)
            out = {"composed": _empty(v, (B, 3, H, W)), "mask": _empty(v, (B, 1, H, W))}
            return eng.inference(ci, cs, FLAGS, visualize=True, out=out, low_latency=ll)
        _four(seopt, call)


@pytest.mark.parametrize("mode", ["default", "lowlat", "bf16"])
def test_large_batch_passes(eng, seopt, mode):
    """7 images with the byte range lowered to three (SE_TEST_OFFSET_LIMIT): passes of 3 + 3 + 1 in one workspace"""
    B, H, W = 7, 64, 64
    ci, cs = _inputs(B, H, W, seed=123)
    seopt.set("SE_TEST_OFFSET_LIMIT", 3 * 64 * 64 * (48 if mode == "bf16" else 96) + 1)
    with _mode(eng, mode) as ll:
        def call(v):
            _ws_fill(eng, v, B, H, W)
            out = {"composed": _empty(v, (B, 3, H, W)), "mask": _empty(v, (B, 1, H, W))}
            r = dict(eng.inference(ci, cs, FLAGS, visualize=True, out=out, low_latency=ll))
            _ws_fill(eng, v, B, H, W)
            r["rgb"], r["m8"] = eng.inference_u8(ci, cs, FLAGS, low_latency=ll)
            _ws_fill(eng, v, B, H, W)
            r["packed"] = eng.inference_packed(ci, cs, FLAGS, _empty(v, (B, 4, H, W)), low_latency=ll)
            return r
        _four(seopt, call)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("size", [(2, 64, 64), (1, 40, 72)], ids=lambda s: "%dx%dx%d" % s)
def test_inference_u8_u8io_packed(eng, seopt, size, mode):
    B, H, W = size
    rng = np.random.RandomState(7)
    iu8 = _u8(rng.randint(0, 256, (B, H, W, 3)))
    su8 = _u8((rng.rand(B, H, W) < 0.02) * 255)
    ci, cs = eng.dequantize_u8(iu8, su8)
    with _mode(eng, mode) as ll:
        def call(v):
            r = {}
            _ws_fill(eng, v, B, H, W)
            r["rgb"], r["m8"] = eng.inference_u8(ci, cs, FLAGS, low_latency=ll)
            _ws_fill(eng, v, B, H, W)
            out = (_empty(v, (B, H, W, 3), torch.uint8), _empty(v, (B, H, W), torch.uint8))
            r["rgb_io"], r["m8_io"] = eng.inference_u8io(iu8, su8, FLAGS, low_latency=ll, out=out)
            _ws_fill(eng, v, B, H, W)
            r["packed"] = eng.inference_packed(ci, cs, FLAGS, _empty(v, (B, 4, H, W)), low_latency=ll)
            return r
        r = _four(seopt, call)
    assert torch.equal(r["rgb"], r["rgb_io"]) and torch.equal(r["m8"], r["m8_io"])


@pytest.mark.parametrize("mode", ["default", "lowlat", "bf16"])
def test_edit_u8(eng, seopt, mode):
    """raw 67 x 70 (working size 64 x 64): both resizes run both passes, through the ctx-owned intermediate"""
    B, Hi, Wi = 2, 67, 70
    rng = np.random.RandomState(8)
    iu8 = _u8(rng.randint(0, 256, (B, Hi, Wi, 3)))
    su8 = _u8((rng.rand(B, 61, 75) < 0.03) * 255)
    need = eng.lib.se_edit_u8_workspace_bytes(eng.h, B, Hi, Wi)
    assert need > 0
    with _mode(eng, mode) as ll:
        def call(v):
            _bytes(eng._workspace_bytes(need), v)
            return {"rgb": eng.edit_u8(iu8, su8, FLAGS, low_latency=ll)}
        _four(seopt, call)


# ---- editing sessions: window edits at a 64 x 64 working size, unaligned origins, committed ---------------------------------
def _session(seed, window_hw):
    rng = np.random.RandomState(seed)
    hs, ws = window_hw
    frames = [rng.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((131, 157), (hs + 5, ws + 3))]
    origins = [(33, 51), (5, 3)]
    sketches = [_u8((rng.rand(hs, ws) < 0.03) * 255) for _ in frames]
    locks = []
    for f in frames:
        lk = np.zeros(f.shape[:2], np.uint8)
        lk[f.shape[0] // 3: f.shape[0] // 2, 7: f.shape[1] - 9] = 255
        locks.append(_u8(lk))
    return frames, origins, sketches, locks


def _window4(seopt, eng, kind, window_hw, mode):
    H, W = 64, 64
    frames, origins, sketches, locks = _session(21, window_hw)
    B = len(frames)
    hs, ws = window_hw
    need = {"plain": lambda: eng.lib.se_edit_window_u8_workspace_bytes(eng.h, B, H, W),
            "scaled": lambda: eng.lib.se_edit_window_scaled_u8_workspace_bytes(eng.h, B, hs, ws, H, W),
            "locked": lambda: eng.lib.se_edit_window_locked_u8_workspace_bytes(eng.h, B, hs, ws, H, W)}[kind]()
    assert need > 0
    with _mode(eng, mode) as ll:
        def call(v):
            fts = [_u8(f) for f in frames]
            _bytes(eng._workspace_bytes(need), v)
            if kind == "plain":
                rgb, m8, hits = eng.edit_window_u8(fts, origins, sketches, H, W, FLAGS, commit=True, low_latency=ll)
            elif kind == "scaled":
                rgb, m8, hits = eng.edit_window_scaled_u8(fts, origins, sketches, window_hw, H, W, FLAGS, commit=True, low_latency=ll)
            else:
                rgb, m8, hits = eng.edit_window_locked_u8(fts, origins, sketches, [locks[0], None], window_hw, H, W, FLAGS,
                                                          commit=True, low_latency=ll)
            r = {"rgb": rgb, "m8": m8, "hits": hits}
            r.update({"frame%d" % i: f for i, f in enumerate(fts)})           # the whole frames, as the window tests compare
            return r
        r = _four(seopt, call)
    assert any(not np.array_equal(r["frame%d" % i].cpu().numpy(), f) for i, f in enumerate(frames))      # (an edit was pasted)


@pytest.mark.parametrize("mode", ["default", "lowlat", "bf16"])
def test_edit_window(eng, seopt, mode):
    _window4(seopt, eng, "plain", (64, 64), mode)


@pytest.mark.parametrize("mode", ["default", "lowlat", "bf16"])
@pytest.mark.parametrize("window_hw", [(90, 77), (64, 100), (45, 64)], ids=lambda s: "%dx%d" % s)
def test_edit_window_scaled(eng, seopt, window_hw, mode):
    _window4(seopt, eng, "scaled", window_hw, mode)


@pytest.mark.parametrize("mode", ["default", "lowlat", "bf16"])
@pytest.mark.parametrize("window_hw", [(64, 64), (90, 77)], ids=lambda s: "%dx%d" % s)
def test_edit_window_locked(eng, seopt, window_hw, mode):
    _window4(seopt, eng, "locked", window_hw, mode)


def _edit_window_null_outputs(eng, frame, origin, sketch, ws_t):
    """se_edit_window_u8 with rgb_out = mask_u8_out = hits_out = NULL: the three live at the front of the workspace"""
    wins = eng._windows([frame], [origin], [sketch])
    flags = FLAGS | eng.exec_flags(1, 64, 64, True, False)
    if eng.lib.se_edit_window_u8(eng.h, eng._stream(), wins, 1, 64, 64, None, None, None, 1, _lib._ptr(ws_t), ws_t.numel(), flags):
        eng._err("se_edit_window_u8")


def test_edit_window_results_in_the_workspace(eng, seopt):
    """the entry's own rgb / mask / hits regions (the caller passed NULL): the frame, and the three regions' contents"""
    frames, origins, sketches, _ = _session(22, (64, 64))
    need = eng.lib.se_edit_window_u8_workspace_bytes(eng.h, 1, 64, 64)
    rgbw, mw = 64 * 64 * 3, 64 * 64

    def call(v):
        ft = _u8(frames[0])
        ws_t = _bytes(eng._workspace_bytes(need), v)
        _edit_window_null_outputs(eng, ft, origins[0], sketches[0], ws_t)
        return {"frame": ft, "rgb": ws_t[:rgbw], "m8": ws_t[rgbw:rgbw + mw], "hits": ws_t[rgbw + mw:rgbw + mw + 16]}
    _four(seopt, call)


@pytest.mark.parametrize("window_hw", [(64, 64), (31, 45)], ids=lambda s: "%dx%d" % s)
def test_window_save_and_swap(eng, seopt, window_hw):
    frames, origins, _, _ = _session(23, window_hw)

    def call(v):
        fts = [_u8(f) for f in frames]
        slots = eng.window_save_u8(fts, origins, window_hw)
        for f in fts:
            f[:, :, 1] += 3
        eng.window_swap_u8(fts, origins, window_hw, slots)
        r = {"frame%d" % i: f for i, f in enumerate(fts)}
        # a slot's rows are padded to 16 bytes: the pad is the journal's own and nobody reads it
        r.update({"slot%d" % i: s[:, :3 * window_hw[1]] for i, s in enumerate(slots)})
        return r
    _four(seopt, call)


# ---- the kernels between the convolutions (shapes of tests/test_gpu_glue.py) -------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("net", ["M", "G", "G-joint"])
def test_pack_inputs(eng, seopt, net, bf16):
    from test_gpu_glue import _pack_case
    x, x2, mask, mask2, guide = (_cuda(a) for a in _pack_case(5, 7))

    def call(v):
        if net == "M":
            return {"packed": eng.pack_inputs("M", x, guide, bf16=bf16)}
        coarse, style = eng.pack_inputs("G", x, guide, x2, mask, mask2, flags=16 if net == "G-joint" else 0, bf16=bf16)
        return {"coarse": coarse, "style": style}
    _four(seopt, call)


# (C, H, W): an HW < 128 pool (most splits empty), the 40 x 72 input's, a granule count that does not divide 256 at a size
# that reaches the four-loads-in-flight loop
POOLS = [(96, 4, 4), (96, 10, 18), (104, 82, 100)]


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("op", ["max", "mean", "rsqrt"])
@pytest.mark.parametrize("case", POOLS, ids=lambda c: "c%d-%dx%d" % c)
def test_column_reduce(eng, seopt, case, op, bf16):
    C, H, W = case
    x = _cuda(synth.uniform(71, "pool%s" % (case,), (3, C, H, W), -1, 1))

    def call(v):
        r = eng.column_reduce(x, op, bf16=bf16)
        return {"out": r[0], "out16": r[1]} if bf16 else {"out": r}
    _four(seopt, call)


# 2-row strips, and a 4-row-strip launch whose last strip has one row
OUTPUT_CONVS = [(3, 5, 7), (2, 12, 16), (1, 1037, 252)]


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", OUTPUT_CONVS, ids=lambda s: "%dx%dx%d" % s)
def test_output_conv(eng, seopt, shape, bf16):
    B, H, W = shape
    a = 1.5 / np.sqrt(108.0)
    w1, w3 = synth.uniform(73, "oc.w1", (1, 12, 3, 3), -a, a), synth.uniform(73, "oc.w3", (3, 12, 3, 3), -a, a)
    b1, b3 = np.float32([0.3]), np.float32([-1.0, 0.1, 1.0])
    x = _cuda(synth.uniform(73, "oc.x%s" % (shape,), (B, 12, H, W), -4, 4))
    img = _cuda(synth.uniform(73, "oc.img%s" % (shape,), (B, 3, H, W), -1, 1))
    mask = _cuda(synth.uniform(73, "oc.mask%s" % (shape,), (B, 1, H, W), 0, 1))
    lock = _u8(synth.uniform(73, "oc.lock%s" % (shape,), (B, H, W), 0, 1) < 0.3)

    def call(v):
        r = {"mask": _empty(v, (B, 1, H, W)), "hard": _empty(v, (B, 1, H, W)), "coarse": _empty(v, (B, 3, H, W)),
             "xnow": _empty(v, (B, H, W, 8), torch.int16) if bf16 else _empty(v, (B, H, W, 4)), "fine": _empty(v, (B, 3, H, W)),
             "composed": _empty(v, (B, 3, H, W)), "rgb8": _empty(v, (B, H, W, 3), torch.uint8), "m8": _empty(v, (B, H, W), torch.uint8)}
        eng.output_conv(x, w1, b1, 0, bf16=bf16, out=r["mask"], hard=r["hard"], lock=lock)
        eng.output_conv(x, w3, b3, 2, bf16=bf16, out=r["coarse"], img=img, mask=mask, xnow=r["xnow"])
        eng.output_conv(x, w3, b3, 3, bf16=bf16, out=r["fine"], img=img, mask=mask, composed=r["composed"], rgb8=r["rgb8"], m8=r["m8"])
        return r
    _four(seopt, call)


# ---- guard conditions: the harness cannot pass vacuously --------------------------------------------------------------------
def test_poisoned_forward_still_runs(eng, seopt):
    """with the option on, the forward still launches its kernels (the profiler counts them) and leaves the graph cache alone"""
    B, H, W = 1, 64, 64
    ci, cs = _inputs(B, H, W)
    seopt.set("SE_TEST_POISON", 0xFF)
    eng.profile(True)
    try:
        r = eng.inference(ci, cs, FLAGS)
        rep = eng.profile_report()
    finally:
        eng.profile(False)
    assert sum(k["launches"] for k in rep["kernels"]) >= 50 and bool(torch.isfinite(r["composed"]).all())
    # graph=True while poisoned: uncaptured every time, bit-identical to the eager call
    for _ in range(3):
        g = eng.inference(ci, cs, FLAGS, graph=True)
        assert torch.equal(g["composed"], r["composed"]) and torch.equal(g["mask"], r["mask"])


def test_poison_reaches_a_byte_nobody_writes(eng, seopt):
    """An incomplete consumer sees the poison.  The border counts of se_edit_window_u8 are B x 4 ints at the front of a
    256-byte region of the workspace when the caller passes hits_out = NULL: with B = 1 the kernel writes 16 bytes and no
    kernel writes the other 240.  They hold the caller's bytes with the option off (0, or a value outside 1..255) and the
    poison with it on."""
    frames, origins, sketches, _ = _session(22, (64, 64))
    need = eng.lib.se_edit_window_u8_workspace_bytes(eng.h, 1, 64, 64)
    at = 64 * 64 * 3 + 64 * 64
    seen = {}
    for v in (0, 0x47, 256):
        seopt.set("SE_TEST_POISON", v)
        ws_t = _bytes(eng._workspace_bytes(need), 0x11)
        _edit_window_null_outputs(eng, _u8(frames[0]), origins[0], sketches[0], ws_t)
        torch.cuda.synchronize()
        seen[v] = ws_t[at:at + 256].cpu().numpy().copy()
    assert np.array_equal(seen[0][:16], seen[0x47][:16])                       # the counts themselves
    assert (seen[0][16:] == 0x11).all() and (seen[0x47][16:] == 0x47).all()
    assert np.array_equal(seen[256], seen[0])                                  # outside 1..255: off, not a fill with zeros

