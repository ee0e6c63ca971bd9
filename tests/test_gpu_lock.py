"""GPU tests of locked regions: the forward with a lock plane against the reference's own vectors
(tests/golden/lock_64.npz) and against the existing entries bit for bit, the lock gather and the locked paste against numpy
and Pillow, the one-call locked edit against the composition of the stand-alone entries, and the serving layer on top
(EditSession.set_lock, BatchingServer(window=True)).

Apart from the comparison with the reference (TOL_E2E) every comparison is exact: a lock only replaces mask values by 0 and
removes pixels from the paste."""
import os
import threading

import numpy as np
import pytest
import torch
from PIL import Image

from sketchedit_amd import _lib, serve, synth

pytestmark = pytest.mark.gpu

TOL_E2E = 1e-3
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


@pytest.fixture(scope="module")
def golden(golden_dir):
    """lock_64.npz and its inputs on the device, shared and never written"""
    g = dict(np.load(os.path.join(golden_dir, "lock_64.npz")))
    img, sk = synth.make_inputs(2, 64, 64, seed=1234)
    return g, _cuda(img), _cuda(sk), _cuda(g["lock"])


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _md(a, b):
    return float(np.abs(a.detach().cpu().numpy().astype(np.float64) - np.asarray(b, np.float64)).max())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _frame(rng, w, h):
    return rng.randint(0, 256, (h, w, 3), dtype=np.uint8)


def _sketch(rng, h, w, p=0.05):
    return ((rng.rand(h, w) < p) * 255).astype(np.uint8)


def _plane(rng, h, w):
    """a lock plane with every kind of run: ~25 % scattered bytes of any non-zero value, a solid block, a full-height column
    and a full-width row"""
    lk = (rng.randint(1, 256, (h, w)) * (rng.rand(h, w) < 0.25)).astype(np.uint8)
    lk[h // 3:h // 3 + 9, w // 4:w // 4 + 13] = 255
    lk[:, w // 2] = 1
    lk[h // 2, :] = 128
    lk[h // 5:h // 5 + 12, : w // 3] = 0                       # ... and a region without any
    return lk


def _in_buffer(a, lead, tail, fill=0xA5):
    """`a` on the device as a view `lead` bytes into a larger poisoned buffer -> (buffer, view)"""
    buf = torch.full((lead + a.size + tail,), fill, dtype=torch.uint8, device="cuda")
    view = buf[lead:lead + a.size].view(a.shape)
    view.copy_(_cuda(a))
    return buf, view


# ---- 1. the forward against the reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("low_latency", [False, True])
def test_forward_against_the_reference(model, golden, low_latency):
    g, ci, cs, lock = golden
    r = model.engine().inference(ci, cs, _lib.flags_from_opt(model.opt), visualize=True, low_latency=low_latency, lock=lock)
    flips = int((r["hard"].cpu().numpy() != g["hard_mask"]).sum())
    d = {k: _md(r[k], g[k]) for k in ("mask", "composed", "coarse", "fine")}
    print("locked forward vs reference (low_latency=%s): flips %d, max |diff| %r" % (low_latency, flips, d))
    assert flips == 0, "hard-mask flips: %d" % flips
    for k, v in d.items():
        assert v < TOL_E2E, (k, v)


# ---- 2. the forward against the existing entries, bit for bit -----------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_forward_against_itself(model, golden, precision):
    _, ci, cs, lock = golden
    eng = model.engine()
    flags = _lib.flags_from_opt(model.opt)
    eng.set_precision(precision)
    try:
        lk = (lock > 0)[:, None]
        # Engine.netM / Engine.netG run in the default execution mode: the relation is stated there.  The unlocked entry
        # first -- the locked one is held to what it shows.
        soft, _ = eng.netM(ci, cs, want_image=False)
        u = eng.inference(ci, cs, flags, visualize=True, low_latency=False)
        assert torch.equal(_bits(u["mask"]), _bits(soft)), "unlocked: inference's mask is not Engine.netM's"
        _, uf = eng.netG(ci, ci, u["hard"], u["hard"], cs, flags)
        assert torch.equal(_bits(u["fine"]), _bits(uf)), "unlocked: inference's fine is not Engine.netG's"
        r = eng.inference(ci, cs, flags, visualize=True, low_latency=False, lock=lock)
        want_mask = torch.where(lk, torch.zeros_like(soft), soft)
        assert torch.equal(_bits(r["mask"]), _bits(want_mask))
        assert torch.equal(r["hard"], (r["mask"] > 0.5).float())
        assert int((u["hard"] != r["hard"]).sum()) > 100                  # the locks took pixels out of the hole
        coarse, fine = eng.netG(ci, ci, r["hard"], r["hard"], cs, flags)
        assert torch.equal(_bits(r["fine"]), _bits(fine)) and torch.equal(_bits(r["coarse"]), _bits(coarse))
        for ll in (False, True):
            r = eng.inference(ci, cs, flags, visualize=True, low_latency=ll, lock=lock)
            l3 = lk.expand(-1, 3, -1, -1)
            assert float(r["mask"][lk].abs().max()) == 0.0 and (_bits(r["mask"])[lk] == 0).all(), ll
            assert torch.equal(_bits(r["composed"])[l3], _bits(ci)[l3]), ll
            assert not torch.equal(r["composed"], ci)
            rgb, m8 = eng.inference_u8(ci, cs, flags, low_latency=ll, lock=lock)
            q_rgb, q_m8 = eng.quantize_u8(r["composed"], r["mask"])
            assert torch.equal(rgb, q_rgb) and torch.equal(m8, q_m8), ll
            assert int(m8[lk[:, 0]].max()) == 0
            z_rgb, z_m8 = eng.inference_u8(ci, cs, flags, low_latency=ll, lock=torch.zeros_like(lock))
            n_rgb, n_m8 = eng.inference_u8(ci, cs, flags, low_latency=ll)
            assert torch.equal(z_rgb, n_rgb) and torch.equal(z_m8, n_m8), ll
            z = eng.inference(ci, cs, flags, visualize=True, low_latency=ll, lock=torch.zeros_like(lock))
            n = eng.inference(ci, cs, flags, visualize=True, low_latency=ll)
            for k in n:
                assert torch.equal(_bits(z[k]), _bits(n[k])), (ll, k)
    finally:
        eng.set_precision("f32")


# ---- 3. passes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default", "lowlat", "bf16"])
def test_passes_advance_the_lock(model, seopt, mode):
    """3 images with the byte range lowered to two (SE_TEST_OFFSET_LIMIT): passes of 2 + 1.  Image i's result is its B = 1
    result with ITS lock plane, so a pass that took the first plane again would show."""
    eng = model.engine()
    flags = _lib.flags_from_opt(model.opt)
    ll = mode == "lowlat"
    eng.set_precision("bf16" if mode == "bf16" else "f32")
    try:
        rng = np.random.RandomState(31)
        img, sk = synth.make_inputs(3, 64, 64, seed=77)
        ci, cs = _cuda(img), _cuda(sk)
        lock = _cuda(np.stack([_plane(rng, 64, 64) for _ in range(3)]))
        lock[2, :, 40:] = 255                                            # the last image's plane is unlike the others
        ones = [(eng.inference(ci[i:i + 1].contiguous(), cs[i:i + 1].contiguous(), flags, low_latency=ll, lock=lock[i:i + 1].contiguous()),
                 eng.inference_u8(ci[i:i + 1].contiguous(), cs[i:i + 1].contiguous(), flags, low_latency=ll, lock=lock[i:i + 1].contiguous()))
                for i in range(3)]
        seopt.set("SE_TEST_OFFSET_LIMIT", 2 * 64 * 64 * (48 if mode == "bf16" else 96) + 1)
        r = eng.inference(ci, cs, flags, low_latency=ll, lock=lock)
        rgb, m8 = eng.inference_u8(ci, cs, flags, low_latency=ll, lock=lock)
        for i, (o, (o_rgb, o_m8)) in enumerate(ones):
            assert torch.equal(_bits(r["composed"][i:i + 1]), _bits(o["composed"])), i
            assert torch.equal(_bits(r["mask"][i:i + 1]), _bits(o["mask"])), i
            assert torch.equal(rgb[i:i + 1], o_rgb) and torch.equal(m8[i:i + 1], o_m8), i
            assert float(r["mask"][i, 0][lock[i] > 0].abs().max()) == 0.0, i
    finally:
        eng.set_precision("f32")


# ---- 4. the lock gather -------------------------------------------------------------------------------------------------------
def _lock_at(crop, H, W):
    """the definition: crop > 0, or Pillow's BICUBIC resize of the crop as an 'L' image, > 0"""
    if crop.shape == (H, W):
        return (crop > 0).astype(np.uint8)
    return (np.array(Image.fromarray(np.ascontiguousarray(crop)).resize((W, H), Image.BICUBIC)) > 0).astype(np.uint8)


# (hs, ws) -> (H, W): ratios below, at and above 1 per axis, and the unscaled window
SIZES = [((33, 35), (64, 64)), ((50, 48), (32, 48)), ((64, 61), (64, 32)), ((64, 64), (64, 64))]


def test_lock_gather_follows_numpy_and_pillow(model):
    eng = model.engine()
    rng = np.random.RandomState(32)
    n = 0
    for (w, h), lead in (((70, 67), 4099), ((131, 97), 4098)):
        f = _cuda(_frame(rng, w, h))
        lk = _plane(rng, h, w)
        _, lkt = _in_buffer(lk, lead, 5)                        # the plane's first byte at an odd / even offset
        for (hs, ws), (H, W) in SIZES:
            for x0 in (0, 1, 2, 3):
                for y0 in (1, 3):                               # odd rows: (y0 + r) Wi + x0 takes every alignment
                    got = eng.window_gather_lock_u8([f], [(y0, x0)], [lkt], (hs, ws), H, W)
                    want = _lock_at(lk[y0:y0 + hs, x0:x0 + ws], H, W)
                    assert got.shape == (1, H, W) and np.array_equal(got[0].cpu().numpy(), want), ((w, h), (y0, x0), (hs, ws), (H, W))
                    assert 0 < want.mean() < 1 and int(got.max()) == 1
                    n += 1
        assert np.array_equal(lkt.cpu().numpy(), lk)
    assert n == 64


def test_lock_gather_three_frames_one_without_a_lock(model):
    eng = model.engine()
    rng = np.random.RandomState(33)
    shapes = [(70, 67), (131, 97), (203, 151)]
    fs = [_cuda(_frame(rng, w, h)) for w, h in shapes]
    lks = [_plane(rng, h, w) for w, h in shapes]
    origins = [(3, 1), (31, 66), (77, 130)]
    for (hs, ws), (H, W) in SIZES:
        got = eng.window_gather_lock_u8(fs, origins, [_cuda(lks[0]), None, _cuda(lks[2])], (hs, ws), H, W).cpu().numpy()
        for i, (y0, x0) in enumerate(origins):
            want = np.zeros((H, W), np.uint8) if i == 1 else _lock_at(lks[i][y0:y0 + hs, x0:x0 + ws], H, W)
            assert np.array_equal(got[i], want), (i, (hs, ws), (H, W))


# ---- 5. the locked paste ------------------------------------------------------------------------------------------------------
def _working_result(rng, B, H, W):
    """synthetic rgb / mask at the working size: a zero region with isolated selected pixels, fully selected rows and a
    block, ragged runs -- both store paths run and runs start at every alignment"""
    rgb = rng.randint(0, 256, (B, H, W, 3), dtype=np.uint8)
    m8 = rng.randint(1, 256, (B, H, W)).astype(np.uint8)
    m8[:, :, : W // 3] = 0
    m8[:, H // 4, 3] = 255
    m8[:, H - 3:, :] = 255
    m8[:, H // 2:H // 2 + 2, W // 2:] = (rng.rand(B, 2, W - W // 2) < 0.5) * 255
    return rgb, m8


def _locked_paste_rule(f, lk, y0, x0, R, M):
    """frame[y0 + y, x0 + x] = R[y, x] where M[y, x] > 0 and lock[y0 + y, x0 + x] == 0; lk None: no lock"""
    want = f.copy()
    sel = M > 0
    if lk is not None:
        sel = sel & (lk[y0:y0 + M.shape[0], x0:x0 + M.shape[1]] == 0)
    want[y0:y0 + M.shape[0], x0:x0 + M.shape[1]][sel] = R[sel]
    return want, sel


def _resized(a, hs, ws):
    return a if a.shape[:2] == (hs, ws) else np.array(Image.fromarray(a).resize((ws, hs), Image.BICUBIC))


def test_locked_paste_follows_the_numpy_rule(model):
    eng = model.engine()
    rng = np.random.RandomState(34)
    for (w, h), lead, tail in (((70, 67), 4099, 4097), ((131, 97), 4097, 4099)):
        f = _frame(rng, w, h)
        lk = _plane(rng, h, w)
        lkt = _cuda(lk)
        for (hs, ws), (H, W) in SIZES:
            rgb, m8 = _working_result(rng, 1, H, W)
            R, M = _resized(rgb[0], hs, ws), _resized(m8[0], hs, ws)
            for x0 in (0, 1, 2, 3):
                y0 = 1 + 2 * (x0 & 1)
                buf, ft = _in_buffer(f, lead, tail)
                eng.window_paste_locked_u8([ft], [(y0, x0)], [lkt], (hs, ws), _cuda(rgb), _cuda(m8))
                want, sel = _locked_paste_rule(f, lk, y0, x0, R, M)
                got = buf.cpu().numpy()
                ctx = ((w, h), (y0, x0), (hs, ws), (H, W))
                assert (got[:lead] == 0xA5).all() and (got[lead + f.size:] == 0xA5).all(), ctx
                got = got[lead:lead + f.size].reshape(f.shape)
                assert np.array_equal(got, want), ctx
                assert np.array_equal(got[lk > 0], f[lk > 0]), ctx                          # no locked pixel changed
                unguarded = (M > 0) & (lk[y0:y0 + hs, x0:x0 + ws] > 0)
                assert sel.any() and unguarded.sum() > 50, ctx                              # the guard had something to do
                groups = sel[:, : ws // 4 * 4].reshape(hs, -1, 4).sum(axis=2)
                assert (groups == 4).any() and ((groups > 0) & (groups < 4)).any(), ctx      # both store paths
    # B = 3 in one launch: two disjoint windows of one frame (one plane), and a frame without a lock
    (hs, ws), (H, W) = (50, 48), (32, 48)
    fa, fb = _frame(rng, 131, 97), _frame(rng, 70, 67)
    la = _plane(rng, 97, 131)
    fta, ftb = _cuda(fa), _cuda(fb)
    rgb, m8 = _working_result(rng, 3, H, W)
    origins = [(3, 7), (3, 7 + ws), (5, 3)]
    eng.window_paste_locked_u8([fta, fta, ftb], origins, [_cuda(la), _cuda(la), None], (hs, ws), _cuda(rgb), _cuda(m8))
    wa, _ = _locked_paste_rule(fa, la, 3, 7, _resized(rgb[0], hs, ws), _resized(m8[0], hs, ws))
    wa, _ = _locked_paste_rule(wa, la, 3, 7 + ws, _resized(rgb[1], hs, ws), _resized(m8[1], hs, ws))
    wb, _ = _locked_paste_rule(fb, None, 5, 3, _resized(rgb[2], hs, ws), _resized(m8[2], hs, ws))
    assert np.array_equal(fta.cpu().numpy(), wa) and np.array_equal(ftb.cpu().numpy(), wb)


# ---- 6. the one-call edit against the composition of the stand-alone entries ------------------------------------------------------
def _border_numpy(m8, y0, x0, hs, ws, Hi, Wi):
    c = [int((m8[0] >= 128).sum()), int((m8[-1] >= 128).sum()), int((m8[:, 0] >= 128).sum()), int((m8[:, -1] >= 128).sum())]
    for side, on_edge in enumerate((y0 == 0, y0 + hs == Hi, x0 == 0, x0 + ws == Wi)):
        if on_edge:
            c[side] = 0
    return c


def _composition(model, f, lk, y0, x0, hs, ws, H, W, sk, low_latency):
    """host crop -> prepare_u8 -> lock gather -> inference_u8(lock=) -> two resize_u8 -> the numpy paste"""
    eng = model.engine()
    image, s = eng.prepare_u8(_cuda(f[y0:y0 + hs, x0:x0 + ws]), _cuda(sk), H, W)
    lock = eng.window_gather_lock_u8([_cuda(f)], [(y0, x0)], [_cuda(lk)], (hs, ws), H, W)
    rgb, m8 = eng.inference_u8(image, s, _lib.flags_from_opt(model.opt), low_latency=low_latency, lock=lock)
    R = eng.resize_u8(rgb, (hs, ws))[0].cpu().numpy()
    M = eng.resize_u8(m8, (hs, ws))[0].cpu().numpy()
    want, sel = _locked_paste_rule(f, lk, y0, x0, R, M)
    m8 = m8[0].cpu().numpy()
    return want, rgb[0].cpu().numpy(), m8, _border_numpy(m8, y0, x0, hs, ws, f.shape[0], f.shape[1]), sel, M


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("low_latency", [True, False])
def test_locked_edit_end_to_end(model, low_latency, precision):
    eng = model.engine()
    eng.set_precision(precision)
    flags = _lib.flags_from_opt(model.opt)
    try:
        rng = np.random.RandomState(35)
        f = _frame(rng, 131, 97)
        for (hs, ws), (H, W), (y0, x0) in (((64, 61), (64, 32), (5, 3)), ((64, 64), (64, 64), (7, 2))):
            lk = _plane(rng, 97, 131)
            lk[:, x0] = 255                                      # the window's left column is locked
            sk = _sketch(rng, hs, ws)
            want, r_rgb, r_m8, r_counts, sel, M = _composition(model, f, lk, y0, x0, hs, ws, H, W, sk, low_latency)
            ctx = ((hs, ws), (H, W))
            print("locked e2e %r: selected %d of %d, mask > 0 on locked pixels %d, counts %r" % (
                ctx, sel.sum(), sel.size, ((M > 0) & (lk[y0:y0 + hs, x0:x0 + ws] > 0)).sum(), r_counts))
            assert sel.any() and (~sel).any() and r_counts[2] == 0 and (r_m8[:, 0] == 0).all(), ctx
            for commit in (False, True):
                ft, lkt = _cuda(f), _cuda(lk)
                rgb, m8, hits = eng.edit_window_locked_u8([ft], [(y0, x0)], [_cuda(sk)], [lkt], (hs, ws), H, W, flags,
                                                          commit=commit, low_latency=low_latency)
                assert np.array_equal(rgb[0].cpu().numpy(), r_rgb) and np.array_equal(m8[0].cpu().numpy(), r_m8), (ctx, commit)
                assert hits[0].cpu().tolist() == r_counts, (ctx, commit)
                got = ft.cpu().numpy()
                assert np.array_equal(got, want if commit else f), (ctx, commit)
                assert np.array_equal(got[lk > 0], f[lk > 0]) and np.array_equal(lkt.cpu().numpy(), lk)
                if not commit:
                    eng.window_paste_locked_u8([ft], [(y0, x0)], [lkt], (hs, ws), rgb, m8)
                    assert np.array_equal(ft.cpu().numpy(), want), ctx
            # no plane for the request: the existing entries, byte for byte
            a, b = _cuda(f), _cuda(f)
            ra = eng.edit_window_scaled_u8([a], [(y0, x0)], [_cuda(sk)], (hs, ws), H, W, flags, low_latency=low_latency)
            rb = eng.edit_window_locked_u8([b], [(y0, x0)], [_cuda(sk)], [None], (hs, ws), H, W, flags, low_latency=low_latency)
            rz = eng.edit_window_locked_u8([_cuda(f)], [(y0, x0)], [_cuda(sk)], [torch.zeros((97, 131), dtype=torch.uint8, device="cuda")],
                                           (hs, ws), H, W, flags, low_latency=low_latency)
            for x, y, z in zip(ra, rb, rz):
                assert torch.equal(x, y) and torch.equal(x, z), ctx
            assert torch.equal(a, b) and not np.array_equal(a.cpu().numpy(), f)
    finally:
        eng.set_precision("f32")


# ---- 7. sessions -------------------------------------------------------------------------------------------------------------
def _stroke(rng, hw, box, p=0.05):
    sk = np.zeros(hw, np.uint8)
    y0, x0, y1, x1 = box
    sk[y0:y1, x0:x1] = _sketch(rng, y1 - y0, x1 - x0, p)
    sk[y0, x0] = sk[y1 - 1, x1 - 1] = 255
    return sk


def _session_lock(rng, h, w, box):
    """a plane that locks half of the sketch's box and scattered pixels all over the frame"""
    lk = ((rng.rand(h, w) < 0.1) * 255).astype(np.uint8)
    y0, x0, y1, x1 = box
    lk[y0:y1, x0:(x0 + x1) // 2] = 255
    return lk


def test_session_keeps_locked_pixels_through_edit_undo_redo(model):
    rng = np.random.RandomState(36)
    w, h = 331, 301
    f = _frame(rng, w, h)
    box = (120, 130, 170, 200)
    sk, lk = _stroke(rng, (h, w), box), _session_lock(rng, h, w, box)
    s = serve.EditSession(model, f, history=2)
    assert s.lock() is None
    s.set_lock(lk)
    assert np.array_equal(s.lock(), lk)
    patch, (px, py), info = s.edit(sk, max_grow=0, low_latency=True)
    y0, x0, hh, ww = info["window"]
    after = s.frame()
    assert info["locked"] is True and info["undoable"] and np.array_equal(patch, after[y0:y0 + hh, x0:x0 + ww])
    assert np.array_equal(after[lk > 0], f[lk > 0]) and not np.array_equal(after, f)
    # the edit is the composition on the window (so the lock entered the forward, not only the paste)
    want, _, _, counts, _, _ = _composition(model, f, lk, y0, x0, hh, ww, hh, ww, sk[y0:y0 + hh, x0:x0 + ww], True)
    assert np.array_equal(after, want) and info["counts"] == counts
    s.undo()
    assert np.array_equal(s.frame(), f) and np.array_equal(s.lock(), lk)          # the whole frame; the lock is not undone
    s.redo()
    assert np.array_equal(s.frame(), after)
    s.set_lock(None)                                                              # ... and freeing it is no edit either
    assert s.lock() is None and s.can_undo
    _, _, info = s.edit(sk, max_grow=0, low_latency=True)
    assert "locked" not in info and not np.array_equal(s.frame()[lk > 0], f[lk > 0])


def test_session_max_side_and_grow_loop_honour_the_lock(model):
    rng = np.random.RandomState(37)
    w, h = 421, 397
    f = _frame(rng, w, h)
    box = (150, 160, 230, 260)
    sk, lk = _stroke(rng, (h, w), box), _session_lock(rng, h, w, box)
    for kw in (dict(max_side=128, max_grow=0), dict(max_side=128), dict()):
        s = serve.EditSession(model, f)
        s.set_lock(lk)
        patch, _, info = s.edit(sk, **kw)
        y0, x0, hh, ww = info["window"]
        H, W = info.get("work", (hh, ww))
        print("locked session %r: window %r work %r counts %r reruns %d" % (kw, info["window"], (H, W), info["counts"], info["reruns"]))
        got = s.frame()
        assert np.array_equal(got[lk > 0], f[lk > 0]) and not np.array_equal(got, f), kw
        want, _, _, counts, _, _ = _composition(model, f, lk, y0, x0, hh, ww, H, W, sk[y0:y0 + hh, x0:x0 + ww], None)
        assert np.array_equal(got, want) and info["counts"] == counts and info["locked"] is True, kw
        assert "max_grow" in kw or info["reruns"] == 2 or not any(info["counts"]), kw


def test_batching_server_mixes_locked_and_unlocked_sessions(model):
    rng = np.random.RandomState(38)
    fs = [_frame(rng, 331, 301), _frame(rng, 400, 290)]
    boxes = [(120, 130, 170, 200), (100, 200, 150, 260)]
    sks = [_stroke(rng, f.shape[:2], b) for f, b in zip(fs, boxes)]
    lk = _session_lock(rng, 301, 331, boxes[0])
    srv = serve.BatchingServer(model, max_batch=2, max_wait_s=5.0, window=True, max_grow=0)
    sessions = [serve.EditSession(model, f) for f in fs]
    sessions[0].set_lock(lk)
    outs = [None] * 2

    def call(i):
        outs[i] = srv.submit(sessions[i], sks[i])
    ts = [threading.Thread(target=call, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    pinned = srv._mode(srv._window_key(outs[0][2]["window"]))
    srv.close()
    assert srv.batches == [2]
    for i in range(2):
        patch, pos, info = outs[i]
        alone = serve.EditSession(model, fs[i])
        if i == 0:
            alone.set_lock(lk)
        p1, pos1, info1 = alone.edit(sks[i], max_grow=0, low_latency=pinned)
        assert pos1 == pos and info1 == info and np.array_equal(p1, patch), i
        assert info.get("locked", False) == (i == 0)
        assert np.array_equal(alone.frame(), sessions[i].frame()) and not np.array_equal(alone.frame(), fs[i]), i
    got = sessions[0].frame()
    assert np.array_equal(got[lk > 0], fs[0][lk > 0])


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_frame_untouched(model):
    eng = model.engine()
    rng = np.random.RandomState(39)
    f = _frame(rng, 131, 97)
    ft = _cuda(f)
    lkt = _cuda(_plane(rng, 97, 131))
    alias = ft.view(-1)[7:7 + 97 * 131].view(97, 131)             # a "plane" inside the frame's own bytes
    flags = _lib.flags_from_opt(model.opt)
    rgb = torch.zeros((1, 48, 40, 3), dtype=torch.uint8, device="cuda")
    m8 = torch.full((1, 48, 40), 255, dtype=torch.uint8, device="cuda")

    def sk(hs, ws):
        return _cuda(_sketch(rng, hs, ws))

    cases = [((1, 1), (50, 45), (48, 40), alias, "locks[0]"), ((97 - 49, 0), (50, 45), (48, 40), lkt, "y0"),
             ((0, 131 - 44), (50, 45), (48, 40), lkt, "x0"), ((1, 1), (50, 45), (44, 40), lkt, "H")]
    for origin, (hs, ws), (H, W), plane, what in cases:
        with pytest.raises(_lib.SketchEditHipError) as e:
            eng.edit_window_locked_u8([ft], [origin], [sk(hs, ws)], [plane], (hs, ws), H, W, flags)
        assert what in str(e.value), (what, str(e.value))
        with pytest.raises(_lib.SketchEditHipError) as e:
            eng.window_paste_locked_u8([ft], [origin], [plane], (hs, ws), torch.zeros((1, H, W, 3), dtype=torch.uint8, device="cuda"),
                                       torch.full((1, H, W), 255, dtype=torch.uint8, device="cuda"))
        assert what in str(e.value), (what, str(e.value))
        if plane is lkt:
            with pytest.raises(_lib.SketchEditHipError) as e:
                eng.window_gather_lock_u8([ft], [origin], [plane], (hs, ws), H, W)
            assert what in str(e.value), (what, str(e.value))
    # a plane of another frame of the same call
    other = _cuda(f)
    with pytest.raises(_lib.SketchEditHipError) as e:
        eng.window_paste_locked_u8([ft, other], [(1, 1), (1, 1)], [None, ft.view(-1)[:97 * 131].view(97, 131)], (50, 45),
                                   torch.cat([rgb, rgb]), torch.cat([m8, m8]))
    assert "locks[1]" in str(e.value) and "wins[0]" in str(e.value)
    # (a call that writes no frame may read such a plane: the uncommitted edit and the gather are allowed)
    eng.edit_window_locked_u8([ft], [(1, 1)], [sk(50, 45)], [alias], (50, 45), 48, 40, flags, commit=False)
    eng.window_gather_lock_u8([ft], [(1, 1)], [alias], (50, 45), 48, 40)
    torch.cuda.synchronize()
    assert np.array_equal(ft.cpu().numpy(), f) and np.array_equal(other.cpu().numpy(), f)
