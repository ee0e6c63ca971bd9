"""GPU tests of fills: se_fill against the reference's own vectors (tests/golden/fill_64.npz) and against
Engine.netG bit for bit, the keep kernel against numpy, the one-call window fill against the composition of the existing
entries, and EditSession.fill / fill_strokes on top.

Apart from the comparison with the reference (TOL_E2E) every comparison is exact: a fill only chooses netG's mask and removes
pixels from the paste."""
import ctypes
import os

import numpy as np
import pytest
import torch
from PIL import Image

from sketchedit_amd import _lib, serve, synth
from feather_util import feather_paste
from strokes_util import spec_raster

pytestmark = pytest.mark.gpu

TOL_E2E = 1e-3          # tests/test_gpu_lock.py's bound for the same network, size and weights; no threshold here, so no flips
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
    """fill_64.npz and its inputs on the device, shared and never written"""
    g = dict(np.load(os.path.join(golden_dir, "fill_64.npz")))
    img, sk = synth.make_inputs(2, 64, 64, seed=1234)
    return g, _cuda(img), _cuda(sk), _cuda(g["fill"]), _cuda(g["lock"])


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _md(a, b):
    return float(np.abs(a.detach().cpu().numpy().astype(np.float64) - np.asarray(b, np.float64)).max())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _frame(rng, w, h):
    return rng.randint(0, 256, (h, w, 3), dtype=np.uint8)


def _plane(rng, h, w, p=0.25):
    """a byte plane with every kind of run: scattered bytes of any non-zero value, a solid block, a full-height column, a
    full-width row and a region without any"""
    a = (rng.randint(1, 256, (h, w)) * (rng.rand(h, w) < p)).astype(np.uint8)
    a[h // 3:h // 3 + 9, w // 4:w // 4 + 13] = 255
    a[:, w // 2] = 1
    a[h // 2, :] = 128
    a[h // 5:h // 5 + 12, : w // 3] = 0
    return a


def _blob(h, w, cy, cx, r):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r).astype(np.uint8) * 255


def _in_buffer(a, lead, tail, fill=0xA5):
    """`a` on the device as a view `lead` bytes into a larger sentinel buffer -> (buffer, view)"""
    buf = torch.full((lead + a.size + tail,), fill, dtype=torch.uint8, device="cuda")
    view = buf[lead:lead + a.size].view(a.shape)
    view.copy_(_cuda(a))
    return buf, view


def _netG(eng, x, hole, sk, flags, low_latency):
    """se_netG_forward(x, x, hole, hole, sk) in the given execution mode (Engine.netG drops the mode bit) -> (coarse, fine)"""
    B, _, H, W = x.shape
    ws = eng.workspace(B, H, W)
    coarse, fine = torch.empty_like(x), torch.empty_like(x)
    fl = (flags & 31) | (_lib.FLAG_BF16 if eng.precision == "bf16" else 0) | (_lib.FLAG_LOW_LATENCY if low_latency else 0)
    p = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    rc = eng.lib.se_netG_forward(eng.h, eng._stream(), p(x), p(x), p(hole), p(hole), p(sk), p(coarse), p(fine), p(ws), ws.numel(), B, H, W, fl)
    assert rc == 0, eng.lib.se_last_error(eng.h)
    return coarse, fine


def _hole_f32(fill, lock):
    h = fill > 0
    if lock is not None:
        h = h & ~(lock > 0)
    return h[:, None].float().contiguous()


# ---- 1. se_fill against the reference and against netG ------------------------------------------------------------------------
@pytest.mark.parametrize("low_latency", [False, True])
def test_fill_against_the_reference(model, golden, low_latency):
    g, ci, cs, fill, lock = golden
    r = model.engine().fill(ci, fill, _lib.flags_from_opt(model.opt), sketch=cs, lock=lock, visualize=True, low_latency=low_latency)
    d = {k: _md(r[k], g[k]) for k in ("coarse", "fine", "composed")}
    print("fill vs reference (low_latency=%s): max |diff| %r" % (low_latency, d))
    assert np.array_equal(r["hard"][:, 0].cpu().numpy(), g["hole"].astype(np.float32))
    hole = r["hard"] > 0
    assert torch.equal(_bits(r["composed"]), _bits(torch.where(hole, r["fine"], ci)))
    for k, v in d.items():
        assert v < TOL_E2E, (k, v)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("low_latency", [False, True])
def test_fill_is_netG_on_the_hole(model, golden, low_latency, precision):
    _, ci, cs, fill, lock = golden
    eng = model.engine()
    flags = _lib.flags_from_opt(model.opt)
    eng.set_precision(precision)
    try:
        r = eng.fill(ci, fill, flags, sketch=cs, lock=lock, visualize=True, low_latency=low_latency)
        hole = _hole_f32(fill, lock)
        assert torch.equal(r["hard"], hole) and int(((fill > 0) & (lock > 0)).sum()) > 100
        coarse, fine = _netG(eng, ci, hole, cs, flags, low_latency)
        assert torch.equal(_bits(r["coarse"]), _bits(coarse)) and torch.equal(_bits(r["fine"]), _bits(fine))
        assert torch.equal(_bits(r["composed"]), _bits(torch.where(hole > 0, fine, ci)))
        if not low_latency:      # Engine.netG's own mode
            c2, f2 = eng.netG(ci, ci, hole, hole, cs, flags)
            assert torch.equal(_bits(f2), _bits(fine)) and torch.equal(_bits(c2), _bits(coarse))
        # without visualize: the same composite; without a lock: another hole
        assert torch.equal(_bits(eng.fill(ci, fill, flags, sketch=cs, lock=lock, low_latency=low_latency)["composed"]), _bits(r["composed"]))
        u = eng.fill(ci, fill, flags, sketch=cs, visualize=True, low_latency=low_latency)
        assert torch.equal(u["hard"], _hole_f32(fill, None)) and not torch.equal(u["composed"], r["composed"])
    finally:
        eng.set_precision("f32")


# ---- 2. corners ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("low_latency", [False, True])
def test_fill_corners(model, low_latency):
    eng = model.engine()
    flags = _lib.flags_from_opt(model.opt)
    img, sk = synth.make_inputs(1, 64, 64, seed=99)
    ci, cs = _cuda(img), _cuda(sk)
    ones = torch.full((1, 64, 64), 3, dtype=torch.uint8, device="cuda")
    zeros = torch.zeros((1, 64, 64), dtype=torch.uint8, device="cuda")
    # an all-ones hole: no valid attention key; the scores are multiplied by the validity and stay finite
    r = eng.fill(ci, ones, flags, sketch=cs, visualize=True, low_latency=low_latency)
    coarse, fine = _netG(eng, ci, _hole_f32(ones, None), cs, flags, low_latency)
    assert torch.isfinite(r["fine"]).all() and torch.isfinite(r["coarse"]).all()
    assert torch.equal(_bits(r["fine"]), _bits(fine)) and torch.equal(_bits(r["coarse"]), _bits(coarse))
    assert torch.equal(_bits(r["composed"]), _bits(fine)) and float(r["hard"].min()) == 1.0
    # ... and a lock over everything: no hole at all
    r = eng.fill(ci, ones, flags, sketch=cs, lock=ones, visualize=True, low_latency=low_latency)
    assert float(r["hard"].max()) == 0.0 and torch.equal(_bits(r["composed"]), _bits(ci))
    # an all-zero hole: composed is the image, bit for bit
    r = eng.fill(ci, zeros, flags, sketch=cs, visualize=True, low_latency=low_latency)
    coarse, fine = _netG(eng, ci, _hole_f32(zeros, None), cs, flags, low_latency)
    assert torch.equal(_bits(r["composed"]), _bits(ci)) and torch.equal(_bits(r["fine"]), _bits(fine))
    # no sketch is a zero sketch
    hole = _cuda(_blob(64, 64, 30, 28, 14)[None])
    a = eng.fill(ci, hole, flags, sketch=None, visualize=True, low_latency=low_latency)
    b = eng.fill(ci, hole, flags, sketch=torch.zeros_like(cs), visualize=True, low_latency=low_latency)
    c = eng.fill(ci, hole, flags, sketch=cs, visualize=True, low_latency=low_latency)
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
    assert not torch.equal(a["fine"], c["fine"])                      # the sketch does guide the fill


# ---- 3. passes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default", "lowlat", "bf16"])
def test_passes_advance_both_planes(model, seopt, mode):
    """3 images with the byte range lowered to two (SE_TEST_OFFSET_LIMIT): passes of 2 + 1.  Image i's result is its B = 1
    result with ITS planes, so a pass that took the first planes again would show."""
    eng = model.engine()
    flags = _lib.flags_from_opt(model.opt)
    ll = mode == "lowlat"
    eng.set_precision("bf16" if mode == "bf16" else "f32")
    try:
        rng = np.random.RandomState(41)
        img, sk = synth.make_inputs(3, 64, 64, seed=77)
        ci, cs = _cuda(img), _cuda(sk)
        fill = _cuda(np.stack([_blob(64, 64, 20 + 12 * i, 40 - 10 * i, 12 + 3 * i) for i in range(3)]))
        lock = _cuda(np.stack([_plane(rng, 64, 64, 0.1) for _ in range(3)]))
        lock[2, :, 40:] = 255                                            # the last image's planes are unlike the others
        one = lambda t, i: t[i:i + 1].contiguous()     # noqa: E731
        ones = [eng.fill(one(ci, i), one(fill, i), flags, sketch=one(cs, i), lock=one(lock, i), visualize=True, low_latency=ll) for i in range(3)]
        seopt.set("SE_TEST_OFFSET_LIMIT", 2 * 64 * 64 * (48 if mode == "bf16" else 96) + 1)
        r = eng.fill(ci, fill, flags, sketch=cs, lock=lock, visualize=True, low_latency=ll)
        for i, o in enumerate(ones):
            for k in ("composed", "coarse", "fine", "hard"):
                assert torch.equal(_bits(r[k][i:i + 1]), _bits(o[k])), (i, k)
            assert torch.equal(r["hard"][i, 0] > 0, (fill[i] > 0) & (lock[i] == 0)), i
        assert not torch.equal(r["hard"][0], r["hard"][2])
    finally:
        eng.set_precision("f32")


# ---- 4. the keep planes -------------------------------------------------------------------------------------------------------
def _keep_rule(fill, lock, keep, y0, x0, hs, ws):
    """keep' = keep with the rectangle set to 255 where fill == 0 or lock != 0, else 0; lock None: no lock"""
    want = keep.copy()
    k = fill[y0:y0 + hs, x0:x0 + ws] == 0
    if lock is not None:
        k = k | (lock[y0:y0 + hs, x0:x0 + ws] != 0)
    want[y0:y0 + hs, x0:x0 + ws] = np.where(k, 255, 0)
    return want


def test_keep_follows_numpy(model):
    eng = model.engine()
    rng = np.random.RandomState(42)
    n = 0
    seen = {"fill": set(), "lock": set(), "keep": set(), "fill-keep": set(), "lock-keep": set(), "fill, no lock": set(), "keep, no lock": set()}
    for (h, w) in ((37, 53), (100, 90)):
        f = _cuda(_frame(rng, w, h))
        fill, lock = _plane(rng, h, w, 0.5), _plane(rng, h, w, 0.2)
        pre = rng.randint(0, 256, (h, w), dtype=np.uint8)              # what the keep plane held: bytes outside the rectangle survive
        for (hs, ws) in ((16, 16), (24, 40)):
            origins = [(0, 0), (h - hs, w - ws), (0, w - ws), (h - hs, 0), (1, 3), (2, 2), (5, 1), (h - hs - 1, 6)]
            g = n // 8                                                  # which (plane, rectangle) pair: 0 .. 3
            for k, (y0, x0) in enumerate(origins):
                # the planes' first bytes at every offset mod 4, each plane from a counter of its own: within one (plane,
                # rectangle) pair and at one origin alike each plane takes all four, and so do the differences to the keep plane
                fo, lo, ko = (g + k) % 4, (3 * g + k // 2) % 4, (g + 2 * k + k // 4) % 4
                _, ft = _in_buffer(fill, 4096 + fo, 7)
                _, lt = _in_buffer(lock, 4096 + lo, 7)
                at = 4096 + ko
                buf, kt = _in_buffer(pre, at, 4099)
                assert (ft.data_ptr() % 4, lt.data_ptr() % 4, kt.data_ptr() % 4) == (fo, lo, ko)
                use_lock = k % 4 != 3                                   # ... and requests without a lock
                seen["fill"].add(fo), seen["keep"].add(ko), seen["fill-keep"].add((fo - ko) % 4)
                if use_lock:
                    seen["lock"].add(lo), seen["lock-keep"].add((lo - ko) % 4)
                else:
                    seen["fill, no lock"].add(fo), seen["keep, no lock"].add(ko)
                out = eng.fill_keep_u8([f], [(y0, x0)], [ft], [lt] if use_lock else None, (hs, ws), keeps=[kt])
                assert out[0] is kt
                got = buf.cpu().numpy()
                ctx = ((h, w), (hs, ws), (y0, x0), (fo, lo, ko), use_lock)
                assert (got[:at] == 0xA5).all() and (got[at + pre.size:] == 0xA5).all(), ctx
                want = _keep_rule(fill, lock if use_lock else None, pre, y0, x0, hs, ws)
                assert np.array_equal(got[at:at + pre.size].reshape(h, w), want), ctx
                rect = want[y0:y0 + hs, x0:x0 + ws]
                assert set(np.unique(rect)) == {0, 255}, ctx
                assert np.array_equal(ft.cpu().numpy(), fill) and np.array_equal(lt.cpu().numpy(), lock)
                n += 1
    assert all(v == {0, 1, 2, 3} for v in seen.values()), seen
    assert n == 32
    # B = 3 in one launch: two disjoint rectangles of one keep plane (one fill plane, one lock), and a request without a lock
    h, w, hs, ws = 100, 90, 24, 40
    fa, fb = _cuda(_frame(rng, w, h)), _cuda(_frame(rng, 53, 37))
    fill_a, lock_a, fill_b = _plane(rng, h, w, 0.5), _plane(rng, h, w, 0.2), _plane(rng, 37, 53, 0.5)
    pre_a, pre_b = rng.randint(0, 256, (h, w), dtype=np.uint8), rng.randint(0, 256, (37, 53), dtype=np.uint8)
    ka, kb = _cuda(pre_a), _cuda(pre_b)
    fta, lta = _cuda(fill_a), _cuda(lock_a)
    origins = [(3, 7), (3, 7 + ws), (5, 3)]
    eng.fill_keep_u8([fa, fa, fb], origins, [fta, fta, _cuda(fill_b)], [lta, lta, None], (hs, ws), keeps=[ka, ka, kb])
    wa = _keep_rule(fill_a, lock_a, _keep_rule(fill_a, lock_a, pre_a, 3, 7, hs, ws), 3, 7 + ws, hs, ws)
    assert np.array_equal(ka.cpu().numpy(), wa) and np.array_equal(kb.cpu().numpy(), _keep_rule(fill_b, None, pre_b, 5, 3, hs, ws))
    # new planes when none are given
    out = eng.fill_keep_u8([fa], [(3, 7)], [fta], [lta], (hs, ws))
    assert out[0].shape == (h, w) and np.array_equal(out[0][3:3 + hs, 7:7 + ws].cpu().numpy(), wa[3:3 + hs, 7:7 + ws])


# ---- 5. the one-call window fill against the composition of the existing entries ------------------------------------------------
def _composition(eng, flags, frames, origins, sketches, holes, locks, window_hw, H, W, low_latency):
    """window_gather(_resize)_u8 -> window_gather_lock_u8 on each plane -> netG -> se_quantize_u8; sketches[i] None: zeros"""
    hs, ws = window_hw
    sks = [s if s is not None else torch.zeros((hs, ws), dtype=torch.uint8, device="cuda") for s in sketches]
    if (hs, ws) == (H, W):
        image, sketch = eng.window_gather_u8(frames, origins, sks, H, W)
    else:
        image, sketch = eng.window_gather_resize_u8(frames, origins, sks, (hs, ws), H, W)
    fill8 = eng.window_gather_lock_u8(frames, origins, holes, (hs, ws), H, W)
    lock8 = eng.window_gather_lock_u8(frames, origins, locks if locks is not None else [None] * len(frames), (hs, ws), H, W)
    hole = ((fill8 > 0) & (lock8 == 0))[:, None].float().contiguous()
    _, fine = _netG(eng, image, hole, sketch, flags, low_latency)
    composed = torch.where(hole > 0, fine, image).contiguous()
    rgb, m8 = eng.quantize_u8(composed, hole)
    return rgb, m8, hole


WINDOW_CASES = [((64, 64), (64, 64), [(5, 3), (7, 1)]), ((72, 96), (48, 64), [(3, 1), (9, 3)])]


@pytest.mark.parametrize("poison", [0, 0xFF])
@pytest.mark.parametrize("window_hw,work_hw,origins", WINDOW_CASES)
def test_window_fill_is_the_composition(model, seopt, window_hw, work_hw, origins, poison):
    """a 100 x 90 frame (and a second one, 131 x 97); B = 2 with one request without a lock and one without a sketch; the
    default mode pinned.  Under SE_TEST_POISON every scratch byte is a NaN pattern until somebody writes it."""
    eng = model.engine()
    flags = _lib.flags_from_opt(model.opt)
    rng = np.random.RandomState(43)
    (hs, ws), (H, W) = window_hw, work_hw
    fa, fb = _frame(rng, 100, 90), _frame(rng, 131, 97)
    fill_a = _blob(90, 100, origins[0][0] + hs // 2, origins[0][1] + ws // 2, hs // 3) | (_plane(rng, 90, 100, 0.02) > 0) * np.uint8(9)
    fill_b = _blob(97, 131, origins[1][0] + hs // 3, origins[1][1] + ws // 2, hs // 4)
    lock_a = _plane(rng, 90, 100, 0.1)
    sk_a = ((rng.rand(hs, ws) < 0.05) * 255).astype(np.uint8)
    frames, holes = [_cuda(fa), _cuda(fb)], [_cuda(fill_a), _cuda(fill_b)]
    locks, sketches = [_cuda(lock_a), None], [_cuda(sk_a), None]
    want_rgb, want_m8, hole = _composition(eng, flags, frames, origins, sketches, holes, locks, (hs, ws), H, W, False)
    frac = float(hole.mean())
    assert 0.05 < frac < 0.9 and int(((holes[0][origins[0][0]:origins[0][0] + hs, origins[0][1]:origins[0][1] + ws] > 0) &
                                      (locks[0][origins[0][0]:origins[0][0] + hs, origins[0][1]:origins[0][1] + ws] > 0)).sum()) > 20
    assert torch.equal(want_m8, (hole[:, 0] * 255).to(torch.uint8))
    if poison:
        seopt.set("SE_TEST_POISON", poison)
    rgb, m8 = eng.fill_window_u8(frames, origins, sketches, holes, locks, (hs, ws), H, W, flags, low_latency=False)
    assert torch.equal(m8, want_m8) and torch.equal(rgb, want_rgb)
    # nothing is committed, no plane is written
    assert np.array_equal(frames[0].cpu().numpy(), fa) and np.array_equal(frames[1].cpu().numpy(), fb)
    assert np.array_equal(holes[0].cpu().numpy(), fill_a) and np.array_equal(locks[0].cpu().numpy(), lock_a)
    # locks=None is a list of Nones; one request alone is its row of the batch (the default mode is pinned)
    r1, m1 = eng.fill_window_u8(frames[1:], origins[1:], None, holes[1:], None, (hs, ws), H, W, flags, low_latency=False)
    r2, m2 = eng.fill_window_u8(frames[1:], origins[1:], [None], holes[1:], [None], (hs, ws), H, W, flags, low_latency=False)
    assert torch.equal(r1, r2) and torch.equal(m1, m2) and torch.equal(m1[0], want_m8[1])


# ---- 6. sessions ------------------------------------------------------------------------------------------------------------
FW, FH = 120, 104


def _session_case(rng):
    f = _frame(rng, FW, FH)
    mask = _blob(FH, FW, 50, 60, 22) | _blob(FH, FW, 30, 90, 9)
    mask[(rng.rand(FH, FW) < 0.01)] = 255
    lock = ((rng.rand(FH, FW) < 0.08) * 255).astype(np.uint8)
    lock[40:60, 50:62] = 255                                            # a locked block inside the painted disc
    sk = np.zeros((FH, FW), np.uint8)
    sk[45:47, 40:85] = 255
    return f, mask, lock, sk


def _session(model, f, lock, lead=4099, tail=4097, **kw):
    """a session whose resident frame lies between sentinel margins -> (session, buffer, lead)"""
    s = serve.EditSession(model, f, **kw)
    buf, view = _in_buffer(f, lead, tail)
    s._frame = view
    if lock is not None:
        s.set_lock(lock)
    return s, buf


def _frame_of(buf, f, lead=4099):
    got = buf.cpu().numpy()
    assert (got[:lead] == 0xA5).all() and (got[lead + f.size:] == 0xA5).all()
    return got[lead:lead + f.size].reshape(f.shape)


def _resized(a, hs, ws):
    return a if a.shape[:2] == (hs, ws) else np.array(Image.fromarray(a).resize((ws, hs), Image.BICUBIC))


def _definition(model, f, mask, lock, sk, win, work, feather=None):
    """the numpy statement of the definition and the paste rule; the forward through the existing entries, default mode pinned"""
    eng = model.engine()
    y0, x0, h, w = win
    H, W = work or (h, w)
    mask255 = np.where(mask != 0, 255, 0).astype(np.uint8)
    rgb, m8, _ = _composition(eng, _lib.flags_from_opt(model.opt), [_cuda(f)], [(y0, x0)], [None if sk is None else _cuda(sk[y0:y0 + h, x0:x0 + w])],
                              [_cuda(mask255)], None if lock is None else [_cuda(lock)], (h, w), H, W, False)
    R, M = _resized(rgb[0].cpu().numpy(), h, w), _resized(m8[0].cpu().numpy(), h, w)
    keep = mask255 == 0
    if lock is not None:
        keep = keep | (lock != 0)
    keep = np.where(keep, 255, 0).astype(np.uint8)
    if feather:
        return feather_paste(f, (y0, x0), R, M, feather, lock=keep), M, keep
    sel = (M > 0) & (keep[y0:y0 + h, x0:x0 + w] == 0)
    want = f.copy()
    want[y0:y0 + h, x0:x0 + w][sel] = R[sel]
    return want, M, keep


@pytest.mark.parametrize("locked", [False, True])
def test_session_fill_is_the_definition_and_undoes(model, locked):
    rng = np.random.RandomState(44)
    f, mask, lock, sk = _session_case(rng)
    lock = lock if locked else None
    win = (3, 5, 64, 64)
    s, buf = _session(model, f, lock, history=2)
    patch, (px, py), info = s.fill(mask, sketch=sk, window=win, low_latency=False)
    want, M, keep = _definition(model, f, mask, lock, sk, win, None)
    after = _frame_of(buf, f)
    assert np.array_equal(after, want) and not np.array_equal(after, f)
    assert info == dict(window=win, fill=True, undoable=True, **({"locked": True} if locked else {}))
    assert (px, py) == (5, 3) and np.array_equal(patch, after[3:67, 5:69])
    assert np.array_equal(after[keep > 0], f[keep > 0])
    if locked:
        assert np.array_equal(s.lock(), lock)
    s.undo()
    assert np.array_equal(_frame_of(buf, f), f)
    s.redo()
    assert np.array_equal(_frame_of(buf, f), after)
    # the automatic window: the floored frame here (min_side 256 > the frame), and no sketch
    s, buf = _session(model, f, lock)
    _, _, info = s.fill(mask, low_latency=False)
    assert info["window"] == (0, 0, FH, FW) and "undoable" not in info
    want, _, _ = _definition(model, f, mask, lock, None, info["window"], None)
    assert np.array_equal(_frame_of(buf, f), want)


@pytest.mark.parametrize("locked", [False, True])
def test_session_fill_at_a_working_size_changes_painted_unlocked_pixels_only(model, locked):
    rng = np.random.RandomState(45)
    f, mask, lock, sk = _session_case(rng)
    lock = lock if locked else None
    win = (3, 5, 72, 96)
    s, buf = _session(model, f, lock, history=1)
    _, _, info = s.fill(mask, sketch=sk, window=win, max_side=64, low_latency=False)
    assert info["work"] == (48, 64) == serve.choose_working_size((72, 96), 64)
    want, M, keep = _definition(model, f, mask, lock, sk, win, (48, 64))
    after = _frame_of(buf, f)
    assert np.array_equal(after, want) and not np.array_equal(after, f)
    assert np.array_equal(after[keep > 0], f[keep > 0])                 # fill == 0 or lock != 0: the bytes are kept
    ringing = (M > 0) & (keep[3:75, 5:101] > 0)
    print("scaled fill: upsampled mask > 0 on %d kept pixels" % ringing.sum())
    assert ringing.sum() > 20                                           # a paste that tests the mask alone would have written those
    s.undo()
    assert np.array_equal(_frame_of(buf, f), f)


def test_session_fill_strokes_feather_and_encode(model):
    rng = np.random.RandomState(46)
    f, mask, lock, sk = _session_case(rng)
    # strokes: the fill of the rasteriser's planes
    strokes = [([(30.0, 40.5), (70.25, 60.0), (90.0, 35.0)], 14.0)]
    guides = [([(25.0, 50.0), (95.0, 52.0)], 2.0)]
    segs, _ = serve.stroke_segments(strokes, (FH, FW))
    gsegs, _ = serve.stroke_segments(guides, (FH, FW))
    win = (8, 4, 88, 112)
    for kw in (dict(), dict(max_side=64)):
        a, abuf = _session(model, f, lock)
        b, bbuf = _session(model, f, lock)
        pa, _, ia = a.fill_strokes(strokes, sketch_strokes=guides, window=win, low_latency=False, **kw)
        pb, _, ib = b.fill(spec_raster(segs, (FH, FW)), sketch=spec_raster(gsegs, (FH, FW)), window=win, low_latency=False, **kw)
        assert ia == ib and np.array_equal(pa, pb) and np.array_equal(_frame_of(abuf, f), _frame_of(bbuf, f)), kw
        assert not np.array_equal(_frame_of(abuf, f), f)
    # feather: feather_util's rule with the keep plane as its lock, at either scale
    for work, kw in ((None, dict()), ((48, 64), dict(max_side=64))):
        win = (3, 5, 72, 96) if work else (3, 5, 64, 64)
        s, buf = _session(model, f, lock, history=1)
        _, _, info = s.fill(mask, sketch=sk, window=win, feather=4, low_latency=False, **kw)
        want, _, keep = _definition(model, f, mask, lock, sk, win, work, feather=4)
        hard, _, _ = _definition(model, f, mask, lock, sk, win, work)
        after = _frame_of(buf, f)
        assert info["feather"] == 4 and np.array_equal(after, want) and not np.array_equal(after, hard), kw
        assert np.array_equal(after[keep > 0], f[keep > 0]), kw
        s.undo()
        assert np.array_equal(_frame_of(buf, f), f)
    # encode: the files frame_jpg / frame_png give for the window afterwards
    for encode, ref in (("png", lambda s, w: s.frame_png(w)), ("jpg", lambda s, w: s.frame_jpg(w)),
                        (("jpg", 70, "420", True), lambda s, w: s.frame_jpg(w, quality=70, subsampling="420", optimize=True))):
        s, buf = _session(model, f, lock, history=1)
        patch, _, info = s.fill(mask, window=(3, 5, 64, 64), encode=encode, low_latency=False)
        assert isinstance(patch, bytes) and patch == ref(s, info["window"]), encode
        s.undo()
        assert np.array_equal(_frame_of(buf, f), f)


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(model):
    eng = model.engine()
    flags = _lib.flags_from_opt(model.opt)
    rng = np.random.RandomState(47)
    f = _frame(rng, 131, 97)
    fill, lock = _plane(rng, 97, 131, 0.5), _plane(rng, 97, 131, 0.2)
    ft, ht, lt = _cuda(f), _cuda(fill), _cuda(lock)
    kt = torch.full((97, 131), 77, dtype=torch.uint8, device="cuda")
    alias = ft.view(-1)[7:7 + 97 * 131].view(97, 131)                 # a "plane" inside the frame's own bytes
    cases = [((97 - 49, 0), (50, 45), (48, 40), "y0"), ((0, 131 - 44), (50, 45), (48, 40), "x0"), ((1, 1), (50, 45), (44, 40), "H"),
             ((1, 1), (12, 45), (16, 40), "hs")]
    for origin, (hs, ws), (H, W), what in cases:
        with pytest.raises(_lib.SketchEditHipError) as e:
            eng.fill_window_u8([ft], [origin], None, [ht], [lt], (hs, ws), H, W, flags)
        assert what in str(e.value), (what, str(e.value))
        if what != "H":
            with pytest.raises(_lib.SketchEditHipError) as e:
                eng.fill_keep_u8([ft], [origin], [ht], [lt], (hs, ws), keeps=[kt])
            assert what in str(e.value), (what, str(e.value))
    # null holes, through the C entries themselves (the binding refuses them earlier)
    wins = eng._windows([ft], [(1, 1)])
    one = lambda t: (ctypes.c_void_p * 1)(t.data_ptr() if t is not None else None)     # noqa: E731
    need = eng.lib.se_fill_window_u8_workspace_bytes(eng.h, 1, 64, 64, 64, 64)
    wsp = eng._workspace_bytes(need)
    for holes, what in ((None, "holes"), (one(None), "holes[0]")):
        rc = eng.lib.se_fill_window_u8(eng.h, eng._stream(), wins, holes, one(lt), 1, 64, 64, 64, 64, None, None, ctypes.c_void_p(wsp.data_ptr()),
                                       wsp.numel() // 16 * 16, flags)
        assert rc != 0 and what in eng.lib.se_last_error(eng.h).decode()
        rc = eng.lib.se_fill_keep_u8(eng.h, eng._stream(), wins, holes, one(lt), one(kt), 1, 64, 64)
        assert rc != 0 and what in eng.lib.se_last_error(eng.h).decode()
    with pytest.raises(_lib.SketchEditHipError):
        eng.fill_window_u8([ft], [(1, 1)], None, [None], None, (64, 64), 64, 64, flags)
    # a keep plane that shares a byte with a frame, a hole or a lock plane of the call; two rectangles of one plane that meet
    for keeps, holes, locks, what in (([alias], [ht], [lt], "wins[0]"), ([ht], [ht], [lt], "holes[0]"), ([lt], [ht], [lt], "locks[0]")):
        with pytest.raises(_lib.SketchEditHipError) as e:
            eng.fill_keep_u8([ft], [(1, 1)], holes, locks, (50, 45), keeps=keeps)
        assert "keeps[0]" in str(e.value) and what in str(e.value), str(e.value)
    with pytest.raises(_lib.SketchEditHipError) as e:
        eng.fill_keep_u8([ft, ft], [(1, 1), (20, 30)], [ht, ht], None, (50, 45), keeps=[kt, kt])
    assert "keeps[0]" in str(e.value) and "keeps[1]" in str(e.value)
    # se_fill: a hole of another shape, a missing hole
    img, sk = synth.make_inputs(1, 64, 64, seed=5)
    with pytest.raises(_lib.SketchEditHipError):
        eng.fill(_cuda(img), torch.zeros((1, 64, 32), dtype=torch.uint8, device="cuda"), flags)
    with pytest.raises(_lib.SketchEditHipError):
        eng.fill(_cuda(img), None, flags)
    # the session: its refusals come before any call
    s, buf = _session(model, f, lock, history=1)
    for call in (lambda: s.fill(np.zeros((97, 131), np.uint8)), lambda: s.fill(fill, window=(60, 0, 64, 64)),
                 lambda: s.fill(fill, sketch=np.zeros((5, 5), np.uint8)), lambda: s.fill_strokes([])):
        with pytest.raises(ValueError):
            call()
    torch.cuda.synchronize()
    assert np.array_equal(_frame_of(buf, f), f) and not s.can_undo and np.array_equal(s.lock(), np.where(lock != 0, 255, 0))
    assert np.array_equal(ft.cpu().numpy(), f) and np.array_equal(ht.cpu().numpy(), fill) and np.array_equal(lt.cpu().numpy(), lock)
    assert int(kt.min()) == 77 and int(kt.max()) == 77
