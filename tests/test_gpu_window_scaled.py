"""GPU tests of window edits at a working size: the gather end (the frame's window resampled straight into
the forward's inputs), the paste end (the result and its mask resampled back, pasted where the resampled mask is > 0), the
one-call scaled edit and the serving layer on top (EditSession.edit(max_side=...), BatchingServer(window=True, max_side=...)).

Every comparison is exact (bytes / bits): each step is integer or table arithmetic around an unchanged forward.  The
comparator is always the composition of the EXISTING entries on a host-made contiguous crop -- Engine.prepare_u8,
Engine.inference_u8, Engine.resize_u8 and numpy for the paste and the counts -- and, for the two resample ends, Pillow
itself."""
import threading

import numpy as np
import pytest
import torch
from PIL import Image

from sketchedit_amd import _lib, serve, synth

pytestmark = pytest.mark.gpu

ARGV = ("--batchSize 1 --name celeb --joint_train_inp --dataset_mode testimage --image_dirs x --mask_dirs x "
        "--image_lists x --model editline2 --netG deepfillc2 --pool_type max --use_cam --output_dir {d} --gpu_ids 0")


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    from sketchedit_amd import models
    from sketchedit_amd.options.test_options import TestOptions
    opt = TestOptions().parse(ARGV.format(d=tmp_path_factory.mktemp("out")).split(), quiet=True)
    opt.isSkip = True                      # no checkpoint on disk: procedural weights
    m = models.create_model(opt)
    m.netG.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict("G", 0).items()})
    m.netM.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict("M", 0).items()})
    return m.eval()


def _frame(rng, w, h):
    return rng.randint(0, 256, (h, w, 3), dtype=np.uint8)


def _sketch(rng, h, w, p=0.01):
    return ((rng.rand(h, w) < p) * 255).astype(np.uint8)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _pillow_inputs(crop, sk, H, W):
    """serve._to_tensors' arithmetic on a crop: Pillow's default resize, (v/255 - 0.5)/0.5 and v > 0"""
    x = np.array(Image.fromarray(crop).resize((W, H))).transpose((2, 0, 1))
    m = np.array(Image.fromarray(sk).resize((W, H)))
    x = (torch.from_numpy(x.astype(np.float32)) / 255 - 0.5) / 0.5
    return x[None], (torch.from_numpy(m.astype(np.float32)) > 0).float()[None, None]


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32).cpu(), b.contiguous().view(torch.int32).cpu())


# (frame (w, h), (y0, x0), (hs, ws), (H, W)): odd frames, x0 = 0..3 and odd rows so that 3 x0 + 3 y Wi takes every dword
# alignment, window sides that are not multiples of 8, ratios below, at and above 1 (per axis and mixed)
GATHER_CASES = [
    ((1921, 1081), (1, 1), (1001, 1203), (264, 320)),           # ~3.8x down
    ((1921, 1081), (3, 2), (1075, 1917), (360, 640)),           # nearly the whole frame
    ((1921, 1081), (0, 3), (517, 333), (520, 336)),             # slightly up
    ((1921, 1081), (564, 1588), (517, 333), (128, 336)),        # flush with the bottom right corner; down in y, up in x
    ((70, 67), (1, 0), (33, 35), (64, 64)),                     # ~2x up
    ((70, 67), (2, 1), (33, 35), (24, 32)),
    ((70, 67), (3, 2), (64, 61), (64, 32)),                     # rows at ratio 1: no vertical pass
    ((70, 67), (5, 3), (50, 48), (32, 48)),                     # columns at ratio 1: the horizontal pass is the identity
    ((641, 481), (7, 5), (473, 631), (16, 24)),                 # ~30 taps per output
]


def test_gather_is_prepare_of_the_crop_and_pillow(model):
    eng = model.engine()
    rng = np.random.RandomState(11)
    frames = {}
    for (w, h), (y0, x0), (hs, ws), (H, W) in GATHER_CASES:
        if (w, h) not in frames:
            f = _frame(rng, w, h)
            frames[(w, h)] = (f, _cuda(f))
        f, ft = frames[(w, h)]
        sk = _sketch(rng, hs, ws, 0.05)
        img, s = eng.window_gather_resize_u8([ft], [(y0, x0)], [_cuda(sk)], (hs, ws), H, W)
        crop = np.ascontiguousarray(f[y0:y0 + hs, x0:x0 + ws])
        ref_i, ref_s = eng.prepare_u8(_cuda(crop), _cuda(sk), H, W)
        ctx = ((w, h), (y0, x0), (hs, ws), (H, W))
        assert _same_bits(img, ref_i) and _same_bits(s, ref_s), ctx            # the fusion
        pil_i, pil_s = _pillow_inputs(crop, sk, H, W)
        assert _same_bits(img, pil_i) and _same_bits(s, pil_s), ctx            # the definition
        assert float(s.mean()) > 0, ctx
    for f, ft in frames.values():
        assert np.array_equal(ft.cpu().numpy(), f)


def test_gather_three_frames_in_one_launch(model):
    """B = 3, three different frames (one a slice of a batch: its first byte is not 4-byte aligned), odd origins"""
    eng = model.engine()
    rng = np.random.RandomState(12)
    fs = [_frame(rng, 641, 481), _frame(rng, 1283, 963), _frame(rng, 70, 67)]
    stack = _cuda(np.stack([_frame(rng, 70, 67), fs[2]]))                      # frame 2 starts 14070 bytes in
    fts = [_cuda(fs[0]), _cuda(fs[1]), stack[1]]
    (hs, ws), (H, W) = (51, 57), (24, 32)
    origins = [(333, 517), (1, 1219), (16, 13)]
    sks = [_sketch(rng, hs, ws, 0.2) for _ in fs]
    img, s = eng.window_gather_resize_u8(fts, origins, [_cuda(k) for k in sks], (hs, ws), H, W)
    for i, (f, (y0, x0)) in enumerate(zip(fs, origins)):
        crop = np.ascontiguousarray(f[y0:y0 + hs, x0:x0 + ws])
        ref_i, ref_s = eng.prepare_u8(_cuda(crop), _cuda(sks[i]), H, W)
        assert _same_bits(img[i:i + 1], ref_i) and _same_bits(s[i:i + 1], ref_s), i
        pil_i, pil_s = _pillow_inputs(crop, sks[i], H, W)
        assert _same_bits(img[i:i + 1], pil_i) and _same_bits(s[i:i + 1], pil_s), i


def _working_result(rng, B, H, W):
    """Synthetic rgb / mask at the working size, independent of the weights: ~half the mask zero in large regions, isolated
    single selected pixels inside them, fully selected rows and a fully selected block -- after the resample both the
    whole-dword and the single-byte store paths run, and runs of selected pixels start at every alignment."""
    rgb = rng.randint(0, 256, (B, H, W, 3), dtype=np.uint8)
    m8 = rng.randint(1, 256, (B, H, W)).astype(np.uint8)
    m8[:, :, : W // 2] = 0                                     # a large zero region ...
    m8[:, H // 4, 3] = 255                                     # ... with isolated single pixels in it
    m8[:, H // 2, W // 4] = 1
    m8[:, H - 3:, :] = 255                                     # fully selected rows
    m8[:, : H // 3, W // 2 + 2:] = 200                         # a fully selected block
    m8[:, H // 2:H // 2 + 2, W // 2:] = (rng.rand(B, 2, W - W // 2) < 0.5) * 255      # ragged runs
    return rgb, m8


def _paste_rule(f, y0, x0, R, M):
    want = f.copy()
    sel = M > 0
    want[y0:y0 + M.shape[0], x0:x0 + M.shape[1]][sel] = R[sel]
    return want, sel


PASTE_CASES = [
    ((1921, 1081), (1, 1), (1001, 1203), (264, 320)),
    ((1921, 1081), (564, 1588), (517, 333), (128, 336)),
    ((70, 67), (1, 0), (33, 35), (64, 64)),
    ((70, 67), (2, 1), (34, 37), (16, 16)),
    ((70, 67), (3, 2), (64, 61), (64, 32)),                     # rows at ratio 1: the vertical pass is the identity
    ((641, 481), (5, 3), (150, 48), (32, 48)),                  # columns at ratio 1: no horizontal pass
    ((641, 481), (7, 6), (203, 310), (104, 160)),
]


def test_paste_follows_the_numpy_rule(model):
    eng = model.engine()
    rng = np.random.RandomState(13)
    for (w, h), (y0, x0), (hs, ws), (H, W) in PASTE_CASES:
        f = _frame(rng, w, h)
        ft = _cuda(f)
        rgb, m8 = _working_result(rng, 1, H, W)
        R = eng.resize_u8(_cuda(rgb), (hs, ws))[0].cpu().numpy()
        M = eng.resize_u8(_cuda(m8), (hs, ws))[0].cpu().numpy()
        ctx = ((w, h), (y0, x0), (hs, ws), (H, W))
        assert np.array_equal(R, np.array(Image.fromarray(rgb[0]).resize((ws, hs)))), ctx          # the definition: Pillow
        assert np.array_equal(M, np.array(Image.fromarray(m8[0]).resize((ws, hs)))), ctx
        eng.window_paste_resize_u8([ft], [(y0, x0)], (hs, ws), _cuda(rgb), _cuda(m8))
        want, sel = _paste_rule(f, y0, x0, R, M)
        got = ft.cpu().numpy()
        assert np.array_equal(got, want), ctx                                                     # the whole frame
        keep = np.ones(f.shape[:2], bool)
        keep[y0:y0 + hs, x0:x0 + ws] = ~sel
        assert np.array_equal(got[keep], f[keep]) and 0.1 < sel.mean() < 0.9, (ctx, sel.mean())
        groups = sel[:, : ws // 4 * 4].reshape(hs, -1, 4).sum(axis=2)
        assert (groups == 4).any() and ((groups > 0) & (groups < 4)).any(), ctx                    # both store paths
    # B = 3: two disjoint windows of ONE frame and a window of another frame in one launch
    (hs, ws), (H, W) = (101, 75), (48, 40)
    fa, fb = _frame(rng, 641, 481), _frame(rng, 90, 107)
    fta, ftb = _cuda(fa), _cuda(fb)
    rgb, m8 = _working_result(rng, 3, H, W)
    origins = [(3, 7), (3, 7 + ws), (6, 0)]
    eng.window_paste_resize_u8([fta, fta, ftb], origins, (hs, ws), _cuda(rgb), _cuda(m8))
    R = eng.resize_u8(_cuda(rgb), (hs, ws)).cpu().numpy()
    M = eng.resize_u8(_cuda(m8), (hs, ws)).cpu().numpy()
    wa, _ = _paste_rule(fa, 3, 7, R[0], M[0])
    wa, _ = _paste_rule(wa, 3, 7 + ws, R[1], M[1])
    wb, _ = _paste_rule(fb, 6, 0, R[2], M[2])
    assert np.array_equal(fta.cpu().numpy(), wa) and np.array_equal(ftb.cpu().numpy(), wb)


def test_nothing_outside_the_window_is_touched(model):
    """a window flush with each frame edge and each corner; the frame is a view inside a larger poisoned buffer"""
    eng = model.engine()
    rng = np.random.RandomState(14)
    Hi, Wi, lead, tail = 97, 131, 4099, 4097
    (hs, ws), (H, W) = (45, 51), (24, 32)
    f = _frame(rng, Wi, Hi)
    rgb, m8 = _working_result(rng, 1, H, W)
    m8[:] = 255                                    # every pixel of the window is written: the widest reach of the paste
    R = eng.resize_u8(_cuda(rgb), (hs, ws))[0].cpu().numpy()
    ym, xm = (Hi - hs) // 2 | 1, (Wi - ws) // 2 | 1
    origins = [(0, 0), (0, Wi - ws), (Hi - hs, 0), (Hi - hs, Wi - ws), (0, xm), (Hi - hs, xm), (ym, 0), (ym, Wi - ws)]
    for y0, x0 in origins:
        buf = torch.full((lead + Hi * Wi * 3 + tail,), 0xA5, dtype=torch.uint8, device="cuda")
        ft = buf[lead:lead + Hi * Wi * 3].view(Hi, Wi, 3)
        ft.copy_(_cuda(f))
        sk = _sketch(rng, hs, ws, 0.1)
        img, s = eng.window_gather_resize_u8([ft], [(y0, x0)], [_cuda(sk)], (hs, ws), H, W)
        ref_i, ref_s = eng.prepare_u8(_cuda(f[y0:y0 + hs, x0:x0 + ws]), _cuda(sk), H, W)
        assert _same_bits(img, ref_i) and _same_bits(s, ref_s), (y0, x0)
        eng.window_paste_resize_u8([ft], [(y0, x0)], (hs, ws), _cuda(rgb), _cuda(m8))
        got = buf.cpu().numpy()
        assert (got[:lead] == 0xA5).all() and (got[lead + Hi * Wi * 3:] == 0xA5).all(), (y0, x0)
        want = f.copy()
        want[y0:y0 + hs, x0:x0 + ws] = R
        assert np.array_equal(got[lead:lead + Hi * Wi * 3].reshape(Hi, Wi, 3), want), (y0, x0)


def _border_numpy(m8, y0, x0, hs, ws, Hi, Wi):
    """the rule of window_border_u8 on the working-size mask; sides by the FRAME-SPACE window"""
    c = [int((m8[0] >= 128).sum()), int((m8[-1] >= 128).sum()), int((m8[:, 0] >= 128).sum()), int((m8[:, -1] >= 128).sum())]
    if y0 == 0:
        c[0] = 0
    if y0 + hs == Hi:
        c[1] = 0
    if x0 == 0:
        c[2] = 0
    if x0 + ws == Wi:
        c[3] = 0
    return c


def _composition_batch(model, fs, origins, hs, ws, H, W, sk_wins, low_latency):
    """steps 1-6 of the definition from the existing entries, for the requests of ONE call: every crop prepared into its slot
    of the batch, one forward for the batch (a batch's kernels may differ from a single image's, so a batch is compared with
    a batch) -> per request (frame after, rgb, m8 at the working size, counts, selection)"""
    eng = model.engine()
    B = len(fs)
    image = torch.empty((B, 3, H, W), dtype=torch.float32, device="cuda")
    s = torch.empty((B, 1, H, W), dtype=torch.float32, device="cuda")
    for i, (f, (y0, x0)) in enumerate(zip(fs, origins)):
        crop = np.ascontiguousarray(f[y0:y0 + hs, x0:x0 + ws])
        eng.prepare_u8(_cuda(crop), _cuda(sk_wins[i]), H, W, out=(image[i:i + 1], s[i:i + 1]))
    rgb, m8 = eng.inference_u8(image, s, _lib.flags_from_opt(model.opt), low_latency=low_latency)
    R = eng.resize_u8(rgb, (hs, ws)).cpu().numpy()
    M = eng.resize_u8(m8, (hs, ws)).cpu().numpy()
    rgb, m8 = rgb.cpu().numpy(), m8.cpu().numpy()
    out = []
    for i, (f, (y0, x0)) in enumerate(zip(fs, origins)):
        want, sel = _paste_rule(f, y0, x0, R[i], M[i])
        out.append((want, rgb[i], m8[i], _border_numpy(m8[i], y0, x0, hs, ws, f.shape[0], f.shape[1]), sel))
    return out


def _composition(model, f, y0, x0, hs, ws, H, W, sk_win, low_latency):
    return _composition_batch(model, [f], [(y0, x0)], hs, ws, H, W, [sk_win], low_latency)[0]


def _centre_sketch(rng, hs, ws, inset, p):
    sk = np.zeros((hs, ws), np.uint8)
    sk[inset:hs - inset, inset:ws - inset] = _sketch(rng, hs - 2 * inset, ws - 2 * inset, p)
    return sk


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("low_latency", [True, False])
def test_scaled_edit_end_to_end(model, low_latency, precision):
    """edit_window_scaled_u8 == the composition, commit 0 and 1, B = 1 and a batch of two frames of different sizes (one
    window flush with its frame's right edge).  The sketches are sparse strokes in the centre of the window, as in the
    unscaled end-to-end test: far from them the procedural weights' soft mask quantises to 0, so the resampled mask holds
    both selected and unselected pixels (asserted)."""
    eng = model.engine()
    eng.set_precision(precision)
    flags = _lib.flags_from_opt(model.opt)
    try:
        rng = np.random.RandomState(15)
        (hs, ws), (H, W) = (509, 515), (256, 256)
        fs = [_frame(rng, 641, 600), _frame(rng, 1283, 963)]
        origins = [(33, 71), (201, 1283 - ws)]
        sks = [_centre_sketch(rng, hs, ws, 190, 0.02) for _ in fs]
        for idx in ([0], [0, 1]):
            refs = dict(zip(idx, _composition_batch(model, [fs[i] for i in idx], [origins[i] for i in idx], hs, ws, H, W,
                                                    [sks[i] for i in idx], low_latency)))
            for want, _, m8, counts, sel in refs.values():
                print("scaled e2e: selected %d, unselected %d of %d; counts %r" % (sel.sum(), (~sel).sum(), sel.size, counts))
                assert sel.any() and (~sel).any()
            assert len(idx) == 1 or refs[1][3][3] == 0             # the flush side counts 0
            for commit in (False, True):
                fts = [_cuda(fs[i]) for i in idx]
                rgb, m8, hits = eng.edit_window_scaled_u8(fts, [origins[i] for i in idx], [_cuda(sks[i]) for i in idx], (hs, ws), H, W,
                                                          flags, commit=commit, low_latency=low_latency)
                for k, i in enumerate(idx):
                    want, r_rgb, r_m8, r_counts, _ = refs[i]
                    ctx = (idx, commit, i)
                    assert np.array_equal(rgb[k].cpu().numpy(), r_rgb) and np.array_equal(m8[k].cpu().numpy(), r_m8), ctx
                    assert hits[k].cpu().tolist() == r_counts, ctx
                    assert np.array_equal(fts[k].cpu().numpy(), want if commit else fs[i]), ctx
                if not commit:                                     # ... and the separate paste completes it
                    eng.window_paste_resize_u8(fts, [origins[i] for i in idx], (hs, ws), rgb, m8)
                    for k, i in enumerate(idx):
                        assert np.array_equal(fts[k].cpu().numpy(), refs[i][0]), (idx, i)
    finally:
        eng.set_precision("f32")


def test_scale_one_is_the_unscaled_edit(model):
    """(H, W) == (hs, ws): frame, rgb_out, mask_u8_out and counts byte-identical to edit_window_u8; likewise the two ends"""
    eng = model.engine()
    flags = _lib.flags_from_opt(model.opt)
    rng = np.random.RandomState(16)
    H, W = 128, 160
    fs = [_frame(rng, 641, 481), _frame(rng, 300, 277)]
    origins = [(101, 203), (277 - H, 3)]
    sks = [_centre_sketch(rng, H, W, 24, 0.05) for _ in fs]
    for commit in (True, False):
        a = [_cuda(f) for f in fs]
        b = [_cuda(f) for f in fs]
        ra = eng.edit_window_u8(a, origins, [_cuda(k) for k in sks], H, W, flags, commit=commit, low_latency=True)
        rb = eng.edit_window_scaled_u8(b, origins, [_cuda(k) for k in sks], (H, W), H, W, flags, commit=commit, low_latency=True)
        for x, y in zip(ra, rb):
            assert torch.equal(x, y), commit
        for x, y, f in zip(a, b, fs):
            assert torch.equal(x, y) and (commit == (not np.array_equal(x.cpu().numpy(), f))), commit
        if not commit:
            eng.window_paste_u8(a, origins, ra[0], ra[1])
            eng.window_paste_resize_u8(b, origins, (H, W), rb[0], rb[1])
            for x, y in zip(a, b):
                assert torch.equal(x, y)
    ia, sa = eng.window_gather_u8([_cuda(f) for f in fs], origins, [_cuda(k) for k in sks], H, W)
    ib, sb = eng.window_gather_resize_u8([_cuda(f) for f in fs], origins, [_cuda(k) for k in sks], (H, W), H, W)
    assert _same_bits(ia, ib) and _same_bits(sa, sb)


def test_step_entries_agree_at_scale_one(model):
    """The step entries alone, no forward: at (hs, ws) == (H, W) the gathers of 6d and 6e return the same bits, and the
    pastes of 6d, 6e and 6g (no plane at all; an all-zero plane for one frame and none for the other) leave the same bytes,
    those of the numpy rule.  B = 3: two disjoint windows of a 97 x 131 frame (a width that is no multiple of 4, odd
    origins) and one window of a 64 x 80 frame."""
    eng = model.engine()
    rng = np.random.RandomState(21)
    fs = [_frame(rng, 131, 97), _frame(rng, 80, 64)]
    for H, W in ((16, 24), (40, 48)):
        origins = [(1, 1), (H + 3, W + 3), (5, 3)]
        which = [0, 0, 1]                                          # the frame of each request

        def frames():
            fts = [_cuda(f) for f in fs]
            return fts, [fts[k] for k in which]

        sks = [_cuda(_sketch(rng, H, W, 0.2)) for _ in which]
        ia, sa = eng.window_gather_u8(frames()[1], origins, sks, H, W)
        ib, sb = eng.window_gather_resize_u8(frames()[1], origins, sks, (H, W), H, W)
        assert _same_bits(ia, ib), (H, W)
        assert _same_bits(sa, sb), (H, W)

        rgb = rng.randint(0, 256, (3, H, W, 3), dtype=np.uint8)
        m8 = rng.choice(np.array([0, 1, 255], np.uint8), size=(3, H, W))
        assert all((m8 == v).any() for v in (0, 1, 255))
        want = [f.copy() for f in fs]
        for i, (k, (y0, x0)) in enumerate(zip(which, origins)):
            want[k], _ = _paste_rule(want[k], y0, x0, rgb[i], m8[i])
        zero = torch.zeros((97, 131), dtype=torch.uint8, device="cuda")
        pastes = {
            "paste": lambda fr: eng.window_paste_u8(fr, origins, _cuda(rgb), _cuda(m8)),
            "paste_resize": lambda fr: eng.window_paste_resize_u8(fr, origins, (H, W), _cuda(rgb), _cuda(m8)),
            "paste_locked, no plane": lambda fr: eng.window_paste_locked_u8(fr, origins, [None] * 3, (H, W), _cuda(rgb), _cuda(m8)),
            "paste_locked, zero plane": lambda fr: eng.window_paste_locked_u8(fr, origins, [zero, zero, None], (H, W), _cuda(rgb), _cuda(m8)),
        }
        first = None
        for name, paste in pastes.items():
            fts, per_request = frames()
            paste(per_request)
            got = [t.cpu().numpy() for t in fts]
            first = first or got
            for k in range(2):
                assert np.array_equal(got[k], first[k]), (name, (H, W), k)          # the entries agree ...
                assert np.array_equal(got[k], want[k]), (name, (H, W), k)           # ... on the rule's bytes
        assert not np.array_equal(want[0], fs[0]) and not np.array_equal(want[1], fs[1])


def _stroke(rng, hw, box, p=0.02):
    sk = np.zeros(hw, np.uint8)
    y0, x0, y1, x1 = box
    sk[y0:y1, x0:x1] = _sketch(rng, y1 - y0, x1 - x0, p)
    sk[y0, x0] = sk[y1 - 1, x1 - 1] = 255
    return sk


def test_session_edits_at_a_working_size(model):
    """three successive edits of a 1921x1081 session with max_side=640, native windows >= 1024 on a side: each patch equals
    the composition on the frame as the previous edit left it; a region no window covers keeps its bytes"""
    rng = np.random.RandomState(17)
    w, h = 1921, 1081
    f = _frame(rng, w, h)
    s = serve.EditSession(model, f)
    cur = f.copy()
    boxes = [(300, 200, 560, 760), (350, 420, 640, 1000), (280, 100, 500, 700)]
    covered = np.zeros((h, w), bool)
    for n, box in enumerate(boxes):
        sk = _stroke(rng, (h, w), box)
        patch, (px, py), info = s.edit(sk, low_latency=True, max_side=640, max_grow=0)
        y0, x0, hs, ws = info["window"]
        H, W = info["work"]
        print("session edit %d: window %r work %r counts %r reruns %d" % (n, info["window"], info["work"], info["counts"], info["reruns"]))
        assert max(hs, ws) >= 1024 and (H, W) == serve.choose_working_size((hs, ws), 640) and max(H, W) == 640
        want, _, _, counts, sel = _composition(model, cur, y0, x0, hs, ws, H, W, sk[y0:y0 + hs, x0:x0 + ws], True)
        assert sel.any() and (~sel).any()
        assert (px, py) == (x0, y0) and np.array_equal(patch, want[y0:y0 + hs, x0:x0 + ws]), n
        assert info["counts"] == counts
        got = s.frame()
        assert np.array_equal(got, want), n
        cur = want
        covered[y0:y0 + hs, x0:x0 + ws] = True
    assert (~covered).sum() > 100000 and np.array_equal(cur[~covered], f[~covered]) and not np.array_equal(cur, f)


def test_grow_loop_at_a_working_size(model):
    """The default edit (max_grow = 2) with max_side: whatever the counts make it do, the result is the composition on the
    FINAL window of the raw frame (uncommitted runs leave no trace), at that window's working size."""
    rng = np.random.RandomState(20)
    w, h = 1283, 963
    f = _frame(rng, w, h)
    sk = _stroke(rng, (h, w), (400, 500, 520, 800), 0.05)
    s = serve.EditSession(model, f)
    patch, (px, py), info = s.edit(sk, max_side=320)
    y0, x0, hs, ws = info["window"]
    H, W = info["work"]
    print("scaled grow: window %r work %r counts %r reruns %d" % (info["window"], info["work"], info["counts"], info["reruns"]))
    assert (H, W) == serve.choose_working_size((hs, ws), 320) and max(H, W) == 320
    want, _, _, counts, _ = _composition(model, f, y0, x0, hs, ws, H, W, sk[y0:y0 + hs, x0:x0 + ws], None)
    assert np.array_equal(s.frame(), want) and np.array_equal(patch, want[y0:y0 + hs, x0:x0 + ws]) and (px, py) == (x0, y0)
    assert info["counts"] == counts and info["reruns"] <= 2
    assert info["reruns"] == 2 or not any(info["counts"])


def test_batching_server_at_a_working_size(model):
    """two sessions, frames of two sizes, equal (hs, ws, H, W) -> one batch of 2; each result equals the direct session's"""
    rng = np.random.RandomState(18)
    fs = [_frame(rng, 1921, 1081), _frame(rng, 1500, 1203)]
    boxes = [(300, 600, 560, 1160), (500, 400, 760, 960)]
    sks = [_stroke(rng, f.shape[:2], box) for f, box in zip(fs, boxes)]
    srv = serve.BatchingServer(model, max_batch=2, max_wait_s=5.0, window=True, max_grow=0, max_side=640)
    sessions = [serve.EditSession(model, f) for f in fs]
    outs = [None] * 2

    def call(i):
        outs[i] = srv.submit(sessions[i], sks[i])
    ts = [threading.Thread(target=call, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    key = srv._window_key(outs[0][2]["window"])
    pinned = srv._mode(key)
    srv.close()
    assert srv.batches == [2] and pinned == _lib.Engine.is_low_latency(2, key[4], key[5])
    for i in range(2):
        patch, pos, info = outs[i]
        assert info["window"][2:] == key[2:4] and info["work"] == key[4:6] and max(key[2:4]) >= 1024
        alone = serve.EditSession(model, fs[i])
        p1, pos1, info1 = alone.edit(sks[i], max_grow=0, low_latency=pinned, max_side=640)
        assert pos1 == pos and info1 == info and np.array_equal(p1, patch), i
        assert np.array_equal(alone.frame(), sessions[i].frame()) and not np.array_equal(alone.frame(), fs[i]), i


def test_refusals_leave_the_frame_untouched(model):
    eng = model.engine()
    rng = np.random.RandomState(19)
    f = _frame(rng, 641, 481)
    ft = _cuda(f)
    flags = _lib.flags_from_opt(model.opt)

    def sk(hs, ws):
        return _cuda(_sketch(rng, hs, ws))

    cases = [((481 - 99, 0), (100, 90), (48, 40), "y0"), ((0, 641 - 89), (100, 90), (48, 40), "x0"), ((-1, 0), (100, 90), (48, 40), "y0"),
             ((0, -2), (100, 90), (48, 40), "x0"), ((0, 0), (15, 90), (16, 40), "hs"), ((0, 0), (100, 12), (48, 16), "ws"),
             ((0, 0), (100, 90), (44, 40), "H"), ((0, 0), (100, 90), (48, 8), "W"), ((0, 0), (100, 90), (8, 40), "H")]
    for origin, (hs, ws), (H, W), what in cases:
        with pytest.raises(_lib.SketchEditHipError) as e:
            eng.edit_window_scaled_u8([ft], [origin], [sk(hs, ws)], (hs, ws), H, W, flags)
        assert what in str(e.value), (what, str(e.value))
        with pytest.raises(_lib.SketchEditHipError):
            eng.window_gather_resize_u8([ft], [origin], [sk(hs, ws)], (hs, ws), H, W)
        with pytest.raises(_lib.SketchEditHipError):
            eng.window_paste_resize_u8([ft], [origin], (hs, ws), torch.zeros((1, H, W, 3), dtype=torch.uint8, device="cuda"),
                                       torch.full((1, H, W), 255, dtype=torch.uint8, device="cuda"))
    # a tap count the resize kernels refuse: 40000 rows into 16 is a 2500x downscale, 10001 taps per output
    tall = torch.zeros((40000, 24, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.SketchEditHipError) as e:
        eng.edit_window_scaled_u8([tall], [(0, 0)], [torch.zeros((40000, 24), dtype=torch.uint8, device="cuda")], (40000, 24), 16, 24, flags)
    assert "taps" in str(e.value)
    with pytest.raises(_lib.SketchEditHipError) as e:
        eng.window_paste_resize_u8([tall], [(0, 0)], (40000, 24), torch.zeros((1, 16, 24, 3), dtype=torch.uint8, device="cuda"),
                                   torch.full((1, 16, 24), 255, dtype=torch.uint8, device="cuda"))
    assert "taps" in str(e.value) and int(tall.max()) == 0
    # overlapping windows of one frame when committing (one pixel row / column short of disjoint), in frame space
    rgb = torch.zeros((2, 48, 40, 3), dtype=torch.uint8, device="cuda")
    m8 = torch.full((2, 48, 40), 255, dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.SketchEditHipError) as e:
        eng.window_paste_resize_u8([ft, ft], [(10, 10), (109, 99)], (100, 90), rgb, m8)
    assert "overlapping" in str(e.value)
    with pytest.raises(_lib.SketchEditHipError) as e:
        eng.edit_window_scaled_u8([ft, ft], [(10, 10), (40, 40)], [sk(100, 90), sk(100, 90)], (100, 90), 48, 40, flags)
    assert "overlapping" in str(e.value)
    # (uncommitted, overlapping windows of one frame are only read: allowed; windows apart by exactly their size too)
    eng.edit_window_scaled_u8([ft, ft], [(10, 10), (40, 40)], [sk(100, 90), sk(100, 90)], (100, 90), 48, 40, flags, commit=False)
    torch.cuda.synchronize()
    assert np.array_equal(ft.cpu().numpy(), f)
