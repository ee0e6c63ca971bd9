"""Large inputs through the streaming contextual attention (se_att_stream.hip).

The materialised attention addresses its R x R matrices (R = h/2 * w/2 on the feature map) with 32-bit offsets and cannot
run where R Rp 4 >= 2^31: from 1224x1224 inputs on, 1080x1920 among them.  The streaming form runs there (and, with
SE_ATT_STREAM=1, at every size).  Its results are checked against the sampled-pixel reference (att_sample_util.py: the
oracle's arithmetic for chosen pixels), the materialised form, and the reference-held fixtures."""
import os

import numpy as np
import pytest
import torch

from att_sample_util import colreduce_rn_fp32, contextual_attention_chunked, gather_pixels, sample_pixels, sampled_attention
from sketchedit_amd import synth

pytestmark = pytest.mark.gpu

FLAGS = 1 | 2 | 16   # use_cam, pool max, joint_train_inp


@pytest.fixture(scope="module")
def eng():
    from sketchedit_amd._lib import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_w(eng):
    eng.load_state_dict("M", synth.make_state_dict("M", 0))
    eng.load_state_dict("G", synth.make_state_dict("G", 0))
    return eng


def _md(a, b):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    b = b.detach().cpu().numpy() if hasattr(b, "detach") else np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _load(golden_dir, name):
    return dict(np.load(os.path.join(golden_dir, name)))


def _inputs(B, h, w, regime, tag):
    x = synth.uniform(7, "big.x%s" % tag, (B, 96, h, w), -1, 1)
    if regime == "soft":
        x = 0.004 * x
    # valid and invalid keys: a random hole pattern at 16x16-window granularity plus a solid hole over the right third
    cells = synth.uniform(7, "big.m%s" % tag, (B, 1, h // 2 + 1, w // 2 + 1), 0, 1) < 0.4
    full = np.kron(cells.astype(np.float32), np.ones((1, 1, 8, 8), np.float32))[:, :, :4 * h, :4 * w]
    full[:, :, :, (8 * w) // 3:] = 1.0
    return np.ascontiguousarray(x), np.ascontiguousarray(full)


@pytest.mark.parametrize("regime", ["soft", "saturated"])
@pytest.mark.parametrize("hw", [(270, 480), (512, 512)], ids=["1080p", "2048sq"])
def test_op_attention_at_large_sizes_f32(eng, hw, regime):
    """1080x1920 and 2048x2048 inputs (feature maps 270x480, 512x512) against the sampled reference at >= 2000 pixels,
    borders and class-grid edges included: <= 1e-4 x max|out| in the soft regime (the large-shape bound of
    test_op_attention_soft_scores_vs_oracle).  Unscaled inputs (logits of ~25 in log2 units) are held to the project's
    1e-3 x max|out|: measured 1.1e-5 at 1080p and 4.7e-4 at 2048x2048.  The key norm is ruled out as the source of the
    2048x2048 gap: the reference run with the norm summed in the library's order (colreduce_rn_fp32) leaves it unchanged.
    Its cause is not identified."""
    h, w = hw
    x, full = _inputs(1, h, w, regime, "%dx%d" % hw)
    out = eng.attention(_cuda(x), _cuda(full))
    assert torch.isfinite(out).all()
    pix = sample_pixels(1, h, w, 2000, seed=3)
    ref = sampled_attention(x, full, pix)
    got = gather_pixels(out, pix)
    d, scale = float((got - ref).abs().max()), float(ref.abs().max())
    # the same reference with the key norm summed in the library's order (colreduce_rn_fp32): what is left is the streaming
    # kernels' own error
    ref_k = sampled_attention(x, full, pix, rn=colreduce_rn_fp32(x))
    d_k = float((got - ref_k).abs().max())
    print("%dx%d %s: max|d| %.3e (library-order key norm: %.3e)  max|out| %.3e" % (h, w, regime, d, d_k, scale))
    assert d <= (1e-4 if regime == "soft" else 1e-3) * scale


def test_op_attention_1080p_bf16_triangle(eng):
    """bf16 at 1080p: the distance from the fp32 sampled reference is at most 1.25x that of the bf16-rounded sampled
    reference (the test_bf16_error_triangle bound), in max-abs and in mean-abs."""
    h, w = 270, 480
    x, full = _inputs(1, h, w, "soft", "bf")
    xb = torch.from_numpy(x).to(torch.bfloat16).float()
    out = eng.attention(_cuda(xb.numpy()), _cuda(full), bf16=True)
    pix = sample_pixels(1, h, w, 2000, seed=4)
    ref32 = sampled_attention(x, full, pix)
    ref16 = sampled_attention(xb, full, pix, dt=torch.bfloat16)
    got = gather_pixels(out, pix)
    d_gpu, d_ref = float((got - ref32).abs().max()), float((ref16 - ref32).abs().max())
    m_gpu, m_ref = float((got - ref32).abs().mean()), float((ref16 - ref32).abs().mean())
    print("1080p bf16: |gpu - f32 ref| max %.3e mean %.3e  |bf16 ref - f32 ref| max %.3e mean %.3e" % (d_gpu, m_gpu, d_ref, m_ref))
    assert m_gpu <= 1.25 * m_ref
    assert d_gpu <= 1.25 * d_ref


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 16, 12), (2, 16, 16), (1, 24, 40), (2, 64, 64), (1, 128, 128), (1, 132, 136), (1, 20, 248)],
                         ids=lambda s: "%dx%dx%d" % s)
def test_forced_stream_matches_materialised(eng, shape, bf16, seopt):
    """SE_ATT_STREAM=1 at the shapes of test_op_attention_fused_streaming_pass: the streaming form against the
    materialised one (fp32: <= 1e-5 x max|out| below 100 rows, 1e-4 above) and, in bf16, against the bf16 oracle and the
    materialised form (max-abs), and its mean-abs error from the fp32 oracle within [0.9, 1.05] x the materialised form's."""
    from oracle import sketchedit_oracle as O
    B, h, w = shape
    x = 0.004 * synth.uniform(5, "att96s.x%d" % h, (B, 96, h, w), -1, 1)
    full = (synth.uniform(5, "att96s.m%d" % h, (B, 1, 4 * h, 4 * w), 0, 1) < 0.5).astype(np.float32)
    full[0, :, :, 2 * w:] = 1.0
    mat = eng.attention(_cuda(x), _cuda(full), bf16=bf16)
    seopt.set("SE_ATT_STREAM", 1)
    st = eng.attention(_cuda(x), _cuda(full), bf16=bf16)
    assert torch.isfinite(st).all()
    if bf16:
        ro, _ = O.contextual_attention(torch.from_numpy(x).to(torch.bfloat16).float(), torch.from_numpy(full), torch.bfloat16)
        tol = 2.0 ** -7 * float(ro.abs().max())
        assert _md(st, ro) < tol and _md(st, mat) < tol
        # mean-abs triangle against the fp32 oracle (test_bf16_error_triangle): a missing rounding point or a wrong P would
        # move the streaming form's mean error off the bf16 oracle's
        r32, _ = O.contextual_attention(torch.from_numpy(x), torch.from_numpy(full))
        m_st = float((st.cpu() - r32).abs().mean())
        m_mat = float((mat.cpu() - r32).abs().mean())
        m_ro = float((ro - r32).abs().mean())
        print("%s bf16 mean|.-f32 oracle|: streaming %.3e  materialised %.3e  bf16 oracle %.3e" % (shape, m_st, m_mat, m_ro))
        # the two forms share the bf16 rounding points (x, xn, P, P~, out); their mean errors agree to within 2 % here, while
        # both sit up to 1.3x the bf16 oracle's at the smallest shapes (the materialised form's own property)
        assert 0.9 * m_mat <= m_st <= 1.05 * m_mat
    else:
        tol = (1e-5 if h < 100 else 1e-4) * float(mat.abs().max())
        assert _md(st, mat) <= tol


def test_forced_stream_threshold_boundary_golden(eng, golden_dir, seopt):
    """The key-validity boundary of ops_r6.npz (24 / 25 / 26 / 27 hole-free pixels of 256 around th = 0.1, vectors of the
    reference's cam modules) through the streaming form: an invalid key is multiplied by zero, not dropped."""
    g = _load(golden_dir, "ops_r6.npz")
    x = 0.004 * synth.uniform(11, "att_th.x", (2, 96, 12, 16), -1, 1)
    full = np.unpackbits(g["op.att_th.mask_bits"])[: 2 * 48 * 64].reshape(2, 1, 48, 64).astype(np.float32)
    seopt.set("SE_ATT_STREAM", 1)
    out = eng.attention(_cuda(x), _cuda(full))
    assert _md(out, g["op.att_th.out"]) < 1e-5 * float(np.abs(g["op.att_th.out"]).max()) + 1e-7


def test_forced_stream_netG_64_golden(eng_w, golden_dir, seopt):
    """e2e_64.npz (reference-held): netG through the streaming attention, fed the reference's hard mask: coarse, fine and
    the attention output tap within the bounds of test_netG_intermediates_64_golden."""
    g = _load(golden_dir, "e2e_64.npz")
    img, sk = synth.make_inputs(2, 64, 64, seed=1234)
    hard = _cuda(g["hard_mask"])
    ci, cs = _cuda(img), _cuda(sk)
    seopt.set("SE_ATT_STREAM", 1)
    r = eng_w.netG_taps(ci, ci, hard, hard, cs, FLAGS)
    assert _md(r["coarse"], g["coarse"]) < 1e-3 and _md(r["fine"], g["fine"]) < 1e-3
    assert _md(r["attn_out"], g["attn_out"]) < 1e-4 * max(1.0, float(np.abs(g["attn_out"]).max()))


def test_1080p_taps_attention_vs_sampled_reference(eng_w):
    """netG at 1080x1920 (B=1, fp32): the attention output tap against the sampled reference computed from the pmconv6 tap
    of the same forward (the taps work at streaming sizes)."""
    H, W = 1080, 1920
    img, sk = synth.make_inputs(1, H, W, seed=77)
    hard_np = np.zeros((1, 1, H, W), np.float32)
    hard_np[:, :, 300:700, 600:1300] = 1.0
    ci, cs, hard = _cuda(img), _cuda(sk), _cuda(hard_np)
    r = eng_w.netG_taps(ci, ci, hard, hard, cs, FLAGS)
    assert torch.isfinite(r["fine"]).all()
    pm = r["pmconv6"].cpu()
    pix = sample_pixels(1, H // 4, W // 4, 2000, seed=5)
    ref = sampled_attention(pm, hard_np, pix)
    d, scale = float((gather_pixels(r["attn_out"], pix) - ref).abs().max()), float(ref.abs().max())
    print("1080p attn_out tap: max|d| %.3e  max|out| %.3e" % (d, scale))
    assert d <= 1e-4 * max(1.0, scale)


def test_1080p_invariants(eng_w):
    """At 1080x1920: image 0 of a B=2 call equals the same image at B=1 bit for bit; the captured graph equals eager
    execution bit for bit; the workspace stays below one R x R fp32 matrix (nothing R^2 is allocated)."""
    H, W = 1080, 1920
    img, sk = synth.make_inputs(2, H, W, seed=99)
    ci, cs = _cuda(img), _cuda(sk)
    r2 = eng_w.inference(ci, cs, FLAGS)
    r1 = eng_w.inference(ci[:1].contiguous(), cs[:1].contiguous(), FLAGS)
    assert torch.equal(r2["composed"][:1], r1["composed"]) and torch.equal(r2["mask"][:1], r1["mask"])
    rg = eng_w.inference(ci[:1].contiguous(), cs[:1].contiguous(), FLAGS, graph=True)
    assert torch.equal(rg["composed"], r1["composed"]) and torch.equal(rg["mask"], r1["mask"])
    R = (H // 8) * (W // 8)
    Rp = (R + 31) // 32 * 32
    ws = eng_w.lib.se_workspace_bytes(eng_w.h, 1, H, W)
    print("1080p workspace: %d bytes (one R x R fp32 matrix: %d)" % (ws, R * Rp * 4))
    assert 0 < ws < R * Rp * 4


def test_1080p_similar_refused(eng):
    """want_similar at a streaming size raises instead of allocating L^2 floats; the engine stays usable."""
    from sketchedit_amd._lib import SketchEditHipError
    h, w = 270, 480
    x, full = _inputs(1, h, w, "soft", "sim")
    with pytest.raises(SketchEditHipError):
        eng.attention(_cuda(x), _cuda(full), want_similar=True)
    xs, fs = _inputs(1, 16, 16, "soft", "sim16")
    out, sim = eng.attention(_cuda(xs), _cuda(fs), want_similar=True)
    assert torch.isfinite(out).all() and torch.isfinite(sim).all()
    out = eng.attention(_cuda(x), _cuda(full))
    assert torch.isfinite(out).all()


def test_1080p_similar_refused_through_the_c_abi(eng):
    """se_attention_ex itself (not the binding's pre-check) refuses a non-NULL similar_out at a streaming size with an error
    message, writes nothing, and the same ctx then runs the attention."""
    from sketchedit_amd._lib import _ptr
    h, w = 270, 480
    x, full = _inputs(1, h, w, "soft", "simc")
    L = ((h - 4) // 2 + 1) * ((w - 4) // 2 + 1)
    xc, fc = _cuda(x), _cuda(full)
    out = torch.zeros_like(xc)
    sim = torch.full((L * L,), 7.0, dtype=torch.float32, device="cuda")      # full size: a write could not go out of bounds
    rc = eng.lib.se_attention_ex(eng.h, eng._stream(), _ptr(xc), _ptr(fc), _ptr(out), _ptr(sim), 1, h, w, 0)
    torch.cuda.synchronize()
    msg = eng.lib.se_last_error(eng.h).decode()
    assert rc != 0 and "similar_out" in msg, msg
    assert bool((out == 0).all()) and bool((sim[:: 1 << 20] == 7.0).all())
    del sim
    rc = eng.lib.se_attention_ex(eng.h, eng._stream(), _ptr(xc), _ptr(fc), _ptr(out), None, 1, h, w, 0)
    torch.cuda.synchronize()
    assert rc == 0 and torch.isfinite(out).all() and float(out.abs().max()) > 0


def test_1080p_end_to_end_vs_oracle(eng_w, monkeypatch):
    """Full inference at 1080x1920, fp32, B=1, procedural weights, against the CPU oracle with its contextual_attention
    replaced (inside this test only) by the query-chunked restatement contextual_attention_chunked (checked against the
    oracle's own on the CPU: test_att_sample_util.py), so that CPU memory stays O(rows * R).  Hard-mask flips through
    composed_for_hard_mask.  Bound: max-abs <= 1e-3 on composed and mask.  CPU time of the oracle: about 15 s on 16 CPUs
    (23 s measured on 8)."""
    from oracle import sketchedit_oracle as O
    from parity_util import composed_for_hard_mask
    monkeypatch.setattr(O, "contextual_attention", lambda x, m, dt=None: contextual_attention_chunked(x, m, dt))
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    H, W = 1080, 1920
    img, sk = synth.make_inputs(1, H, W, seed=11)
    WM, WG = synth.make_state_dict("M", 0), synth.make_state_dict("G", 0)
    r = eng_w.inference(_cuda(img), _cuda(sk), FLAGS, visualize=True)
    ref = O.inference(WM, WG, img, sk)
    comp, flips = composed_for_hard_mask(O, WG, img, sk, ref["mask"], ref["hard_mask"], ref["composed"], r["hard"].cpu())
    d_c, d_m = _md(r["composed"], comp), _md(r["mask"], ref["mask"])
    print("1080p end to end vs oracle: max|composed| %.3e  max|mask| %.3e  hard-mask flips %d" % (d_c, d_m, flips))
    assert d_c <= 1e-3 and d_m <= 1e-3


@pytest.mark.parametrize("procs", ["serial", "encode_procs"])
def test_test_py_1080p(tmp_path, eng_w, procs):
    """test.py on one 1080x1920 PNG pair (--synthetic_weights; the serial loop and the encoder-process pipeline): the files it
    writes have the input's size and equal Engine.inference_u8 on the same inputs, bit for bit."""
    import importlib.util
    from PIL import Image
    H, W = 1080, 1920
    for sub in ("images", "edges"):
        os.makedirs(tmp_path / sub)
    rng = np.random.RandomState(3)
    rgb = rng.randint(0, 255, (H, W, 3), dtype=np.uint8)
    edge = ((rng.rand(H, W) < 0.005) * 255).astype(np.uint8)
    Image.fromarray(rgb).save(tmp_path / "images" / "hd.png")
    Image.fromarray(edge).save(tmp_path / "edges" / "hd.png")
    (tmp_path / "list.txt").write_text("hd.png\n")
    extra = "--nThreads 0 --serial_io" if procs == "serial" else "--nThreads 1 --encode_procs 2"
    argv = ("--batchSize 1 --name celeb --joint_train_inp --dataset_mode testimage --image_dirs {d}/images "
            "--mask_dirs {d}/edges --image_lists {d}/list.txt --image_postfix .png --mask_postfix .png --model editline2 "
            "--netG deepfillc2 --pool_type max --use_cam --which_epoch latest --output_dir {d}/results "
            "--output_mask_dir {d}/masks --synthetic_weights " + extra).format(d=tmp_path).split()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("se_test_script_1080p", os.path.join(root, "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main(argv)
    out = np.asarray(Image.open(tmp_path / "results" / "hd.png"))
    msk = np.asarray(Image.open(tmp_path / "masks" / "hd.png"))
    assert out.shape == (H, W, 3) and msk.shape == (H, W)
    img, sk = eng_w.dequantize_u8(torch.from_numpy(rgb)[None].cuda(), torch.from_numpy(edge)[None].cuda())
    want, want_m = eng_w.inference_u8(img, sk, FLAGS)
    assert np.array_equal(out, want[0].cpu().numpy()) and np.array_equal(msk, want_m[0].cpu().numpy())


def test_forced_stream_e2e_512_digest(eng_w, golden_dir, seopt):
    """e2e_512.npz (reference-held digests of the 512x512 case) with the streaming attention forced: crops, row / column
    sums and hard-mask bits within the bounds of test_inference_digest_golden (no `similar`: the streaming form has none)."""
    from test_gpu_parity import _digest_or_mask_only
    g = _load(golden_dir, "e2e_512.npz")
    img, sk = synth.make_inputs(1, 512, 512, seed=1234)
    seopt.set("SE_ATT_STREAM", 1)
    r = eng_w.inference(_cuda(img), _cuda(sk), FLAGS, visualize=True)
    _digest_or_mask_only(r, g, 512, 512)


def test_forced_stream_bf16_error_triangle_512(eng, seopt):
    """bf16 through netG with the streaming attention forced, 512x512 B=16: |HIP_bf16 - fp32 oracle| <= 1.25 x |bf16 oracle -
    fp32 oracle| in max-abs and mean-abs on coarse and fine (test_bf16_error_triangle), netG fed the fp32 oracle's hard mask."""
    from oracle import sketchedit_oracle as O
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    B, size = 16, 512
    img, sk = synth.make_inputs(B, size, size, seed=1234)
    WM, WG = synth.make_state_dict("M", 0), synth.make_state_dict("G", 0)
    with torch.no_grad():
        m32, _ = O.netM_forward(WM, torch.from_numpy(img), torch.from_numpy(sk), want_image=False)
        hard = (m32 > 0.5).float()
        c32, f32 = O.netG_forward(WG, img, img, hard, hard, sk)
        c16, f16 = O.netG_forward(WG, img, img, hard, hard, sk, act_dtype=torch.bfloat16)
    eng.load_state_dict("M", WM)
    eng.load_state_dict("G", WG)
    eng.set_precision("bf16")
    try:
        seopt.set("SE_ATT_STREAM", 1)
        ci, cs = _cuda(img), _cuda(sk)
        gc, gf = eng.netG(ci, ci, hard.cuda(), hard.cuda(), cs, FLAGS)
    finally:
        eng.set_precision("f32")
    for name, got, o16, o32 in (("coarse", gc, c16, c32), ("fine", gf, f16, f32)):
        d_hip = np.abs(got.cpu().numpy().astype(np.float64) - o32.numpy())
        d_or = np.abs(o16.numpy().astype(np.float64) - o32.numpy())
        print("bf16 triangle 512 B=16 streaming %s: max %.2e/%.2e mean %.2e/%.2e" % (name, d_hip.max(), d_or.max(), d_hip.mean(), d_or.mean()))
        assert d_hip.mean() <= 1.25 * d_or.mean() and d_hip.max() <= 1.25 * d_or.max(), name
