"""GPU tests of the editing sessions: the window kernels (gather / border / paste), the one-call window edit
and the serving layer on top (serve.EditSession, BatchingServer(window=True)).

Every comparison is exact (bytes / bits).  The comparator is always the EXISTING whole-image path run on a host-made
contiguous crop -- `model.inference_u8({"image_u8": crop, "mask_u8": crop_sketch}, low_latency=m)` or
`Engine.dequantize_u8(crop)` -- plus numpy, never the new entry points."""
import threading

import numpy as np
import pytest
import torch

from sketchedit_amd import _lib, serve, synth

pytestmark = pytest.mark.gpu

ARGV = ("--batchSize 1 --name celeb --joint_train_inp --dataset_mode testimage --image_dirs x --mask_dirs x "
        "--image_lists x --model editline2 --netG deepfillc2 --pool_type max --use_cam --output_dir {d} --gpu_ids 0")
FRAMES = [(641, 481), (1283, 963), (70, 67)]          # (width, height)


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


def _corner_windows(Hi, Wi, H, W):
    """(y0, x0): the four corners and two odd interior positions"""
    out = [(0, 0), (0, Wi - W), (Hi - H, 0), (Hi - H, Wi - W)]
    if Hi - H >= 3 and Wi - W >= 5:
        out += [(1, 3), (Hi - H - 1, Wi - W - 3), ((Hi - H) // 2 | 1, (Wi - W) // 2 | 1)]
    return out


def _existing_path(model, crop, crop_sketch, low_latency):
    """the parent's whole-image path on a contiguous crop -> (rgb (H,W,3), mask_u8 (H,W)) numpy"""
    rgb, m8 = model.inference_u8({"image_u8": torch.from_numpy(np.ascontiguousarray(crop))[None],
                                  "mask_u8": torch.from_numpy(np.ascontiguousarray(crop_sketch))[None]}, low_latency=low_latency)
    return rgb[0].cpu().numpy(), m8[0].cpu().numpy()


def _border_numpy(m8, y0, x0, Hi, Wi):
    H, W = m8.shape
    c = [int((m8[0] >= 128).sum()), int((m8[-1] >= 128).sum()), int((m8[:, 0] >= 128).sum()), int((m8[:, -1] >= 128).sum())]
    if y0 == 0:
        c[0] = 0
    if y0 + H == Hi:
        c[1] = 0
    if x0 == 0:
        c[2] = 0
    if x0 + W == Wi:
        c[3] = 0
    return c


def test_gather_is_dequantize_of_the_crop(model):
    eng = model.engine()
    rng = np.random.RandomState(1)
    for (w, h), (H, W) in zip(FRAMES, [(256, 320), (512, 512), (64, 56)]):
        f = _frame(rng, w, h)
        ft = torch.from_numpy(f).cuda()
        for y0, x0 in _corner_windows(h, w, H, W):
            sk = _sketch(rng, H, W, 0.3)
            img, s = eng.window_gather_u8([ft], [(y0, x0)], [torch.from_numpy(sk).cuda()], H, W)
            crop = np.ascontiguousarray(f[y0:y0 + H, x0:x0 + W])
            ref_i, ref_s = eng.dequantize_u8(torch.from_numpy(crop)[None].cuda(), torch.from_numpy(sk)[None].cuda())
            assert torch.equal(img.view(torch.int32), ref_i.view(torch.int32)), ((w, h), (y0, x0))
            assert torch.equal(s.view(torch.int32), ref_s.view(torch.int32)), ((w, h), (y0, x0))
        assert np.array_equal(ft.cpu().numpy(), f)


def test_gather_three_frames_in_one_launch(model):
    """B = 3, three different frames (one of them a slice of a batch: its first byte is not 4-byte aligned), odd origins"""
    eng = model.engine()
    rng = np.random.RandomState(2)
    fs = [_frame(rng, w, h) for w, h in FRAMES]
    stack = torch.from_numpy(np.stack([_frame(rng, 70, 67), fs[2]])).cuda()       # frame 2 starts 14070 bytes in
    fts = [torch.from_numpy(fs[0]).cuda(), torch.from_numpy(fs[1]).cuda(), stack[1]]
    H, W = 48, 64
    origins = [(333, 517), (1, 1219), (19, 3)]
    sks = [_sketch(rng, H, W, 0.2) for _ in fs]
    img, s = eng.window_gather_u8(fts, origins, [torch.from_numpy(k).cuda() for k in sks], H, W)
    crops = np.stack([f[y0:y0 + H, x0:x0 + W] for f, (y0, x0) in zip(fs, origins)])
    ref_i, ref_s = eng.dequantize_u8(torch.from_numpy(crops).cuda(), torch.from_numpy(np.stack(sks)).cuda())
    assert torch.equal(img.view(torch.int32), ref_i.view(torch.int32)) and torch.equal(s.view(torch.int32), ref_s.view(torch.int32))


def test_paste_follows_the_numpy_rule(model):
    """Synthetic rgb / mask with ~50 % zeros (independent of the weights): the frame equals the numpy rule; the bytes
    outside the windows and under zeros are unchanged.  Runs of selected pixels of every length and alignment occur."""
    eng = model.engine()
    rng = np.random.RandomState(3)
    fs = [_frame(rng, w, h) for w, h in FRAMES] + [_frame(rng, 641, 481)]
    H, W = 56, 64
    origins = [(0, 0), (963 - H, 1283 - W), (11, 5), (201, 333)]
    rgb = rng.randint(0, 256, (4, H, W, 3), dtype=np.uint8)
    m8 = (rng.randint(0, 256, (4, H, W)) * (rng.rand(4, H, W) < 0.5)).astype(np.uint8)
    m8[3, :, :16] = 255                                    # whole groups of four selected: the dword path
    m8[0, :8] = 0
    fts = [torch.from_numpy(f).cuda() for f in fs]
    eng.window_paste_u8(fts, origins, torch.from_numpy(rgb).cuda(), torch.from_numpy(m8).cuda())
    for i, (f, (y0, x0)) in enumerate(zip(fs, origins)):
        want = f.copy()
        sel = m8[i] > 0
        want[y0:y0 + H, x0:x0 + W][sel] = rgb[i][sel]
        got = fts[i].cpu().numpy()
        assert np.array_equal(got, want), i
        keep = np.ones(f.shape[:2], bool)
        keep[y0:y0 + H, x0:x0 + W] = sel == 0
        assert np.array_equal(got[keep], f[keep]) and 0.3 < (sel == 0).mean() < 0.7
    # two disjoint windows of ONE frame in one launch
    f = _frame(rng, 641, 481)
    ft = torch.from_numpy(f).cuda()
    eng.window_paste_u8([ft, ft], [(3, 7), (3, 7 + W)], torch.from_numpy(rgb[:2]).cuda(), torch.from_numpy(m8[:2]).cuda())
    want = f.copy()
    for i, x0 in enumerate((7, 7 + W)):
        want[3:3 + H, x0:x0 + W][m8[i] > 0] = rgb[i][m8[i] > 0]
    assert np.array_equal(ft.cpu().numpy(), want)


def test_border_counts(model):
    """counts == numpy on the existing path's mask_u8; windows flush with two frame edges report 0 on those sides"""
    eng = model.engine()
    rng = np.random.RandomState(4)
    w, h = 641, 481
    f = _frame(rng, w, h)
    ft = torch.from_numpy(f).cuda()
    H, W = 64, 96
    origins = [(0, 0), (h - H, w - W), (h - H, 0), (101, 203)]
    masks = []
    for y0, x0 in origins:
        _, m8 = _existing_path(model, f[y0:y0 + H, x0:x0 + W], _sketch(rng, H, W), True)
        masks.append(m8)
    m = np.stack(masks)
    got = eng.window_border_u8([ft] * 4, origins, torch.from_numpy(m).cuda()).cpu().numpy().tolist()
    want = [_border_numpy(m[i], y0, x0, h, w) for i, (y0, x0) in enumerate(origins)]
    assert got == want, (got, want)
    assert got[0][0] == 0 and got[0][2] == 0 and got[1][1] == 0 and got[1][3] == 0
    # and on a synthetic mask around the threshold (127 / 128), so that the comparison itself is exercised
    syn = rng.randint(120, 136, (4, H, W)).astype(np.uint8)
    got = eng.window_border_u8([ft] * 4, origins, torch.from_numpy(syn).cuda()).cpu().numpy().tolist()
    assert got == [_border_numpy(syn[i], y0, x0, h, w) for i, (y0, x0) in enumerate(origins)]
    assert sum(got[3]) > 0 and sum(got[3]) < 2 * (H + W)


CASE = dict(frame=(641, 481), seed=5, window=(101, 203, 256, 256), inset=96, p=0.02)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("low_latency", [True, False])
def test_one_edit_end_to_end(model, low_latency, precision):
    """frame after edit(..., max_grow=0) == raw frame with rgb[mask_u8 > 0] of the existing path written into the window;
    patch == that window.  The case, picked with the CPU oracle: a 641x481 random frame (RandomState(5)), the 256x256
    window at (y0, x0) = (101, 203) -- odd origin, interior -- and a 2 % random sketch in its central 64x64.  The
    procedural weights' masks are large (hole fraction 0.66-0.85), but this far from the strokes the fp32
    oracle's soft mask falls to 3e-4, well under 1/255: 160 of the 65536 pixels quantise to 0 (seeds 5-11 give 88-161), so
    the window holds both selected and unselected pixels and the paste's selection is exercised by the network's own mask."""
    eng = model.engine()
    eng.set_precision(precision)
    try:
        rng = np.random.RandomState(CASE["seed"])
        w, h = CASE["frame"]
        y0, x0, H, W = CASE["window"]
        f = _frame(rng, w, h)
        sk = np.zeros((h, w), np.uint8)
        i = CASE["inset"]
        sk[y0 + i:y0 + H - i, x0 + i:x0 + W - i] = _sketch(rng, H - 2 * i, W - 2 * i, CASE["p"])
        rgb, m8 = _existing_path(model, f[y0:y0 + H, x0:x0 + W], sk[y0:y0 + H, x0:x0 + W], low_latency)
        print("mask_u8 > 0: %d, == 0: %d of %d" % ((m8 > 0).sum(), (m8 == 0).sum(), m8.size))
        assert (m8 > 0).any() and (m8 == 0).any()          # the existing path alone: both kinds of pixel in the window
        want = f.copy()
        want[y0:y0 + H, x0:x0 + W][m8 > 0] = rgb[m8 > 0]
        s = serve.EditSession(model, f)
        patch, (px, py), info = s.edit(sk, window=(y0, x0, H, W), max_grow=0, low_latency=low_latency)
        got = s.frame()
        assert np.array_equal(got, want)
        assert (px, py) == (x0, y0) and np.array_equal(patch, want[y0:y0 + H, x0:x0 + W])
        assert info["counts"] == _border_numpy(m8, y0, x0, h, w) and info["reruns"] == 0
        # the automatic window of the same sketch (choose_window: 256 x 256 around the strokes)
        s = serve.EditSession(model, f)
        patch, (px, py), info = s.edit(sk, max_grow=0, low_latency=low_latency)
        ay, ax, ah, aw = info["window"]
        assert (ah, aw) == (256, 256) and (px, py) == (ax, ay)
        rgb, m8 = _existing_path(model, f[ay:ay + ah, ax:ax + aw], sk[ay:ay + ah, ax:ax + aw], low_latency)
        want = f.copy()
        want[ay:ay + ah, ax:ax + aw][m8 > 0] = rgb[m8 > 0]
        assert np.array_equal(s.frame(), want) and np.array_equal(patch, want[ay:ay + ah, ax:ax + aw])
    finally:
        eng.set_precision("f32")


def test_two_edits_in_sequence(model):
    """the second edit equals the existing path run on the crop of the FIRST's result (the frame is the session's state);
    the second window overlaps the first"""
    rng = np.random.RandomState(6)
    w, h = 641, 481
    f = _frame(rng, w, h)
    s = serve.EditSession(model, f)
    cur = f.copy()
    for (y0, x0, H, W) in [(33, 71, 128, 160), (97, 151, 160, 128)]:
        sk = np.zeros((h, w), np.uint8)
        sk[y0 + 8:y0 + H - 8, x0 + 8:x0 + W - 8] = _sketch(rng, H - 16, W - 16)
        rgb, m8 = _existing_path(model, cur[y0:y0 + H, x0:x0 + W], sk[y0:y0 + H, x0:x0 + W], True)
        cur[y0:y0 + H, x0:x0 + W][m8 > 0] = rgb[m8 > 0]
        patch, _, _ = s.edit(sk, window=(y0, x0, H, W), low_latency=True)
        assert np.array_equal(patch, cur[y0:y0 + H, x0:x0 + W])
        assert np.array_equal(s.frame(), cur)
    assert not np.array_equal(cur, f)


def test_grow_loop_on_the_device(model):
    """The default edit (max_grow = 2) on the device: whatever the counts make it do, the result is the existing path on
    the FINAL window's crop of the raw frame (uncommitted runs leave no trace)."""
    rng = np.random.RandomState(7)
    w, h = 1283, 963
    f = _frame(rng, w, h)
    sk = np.zeros((h, w), np.uint8)
    sk[400:460, 600:700] = _sketch(rng, 60, 100, 0.05)
    s = serve.EditSession(model, f)
    patch, (px, py), info = s.edit(sk)
    y0, x0, H, W = info["window"]
    print("grow: window %r counts %r reruns %d" % (info["window"], info["counts"], info["reruns"]))
    rgb, m8 = _existing_path(model, f[y0:y0 + H, x0:x0 + W], sk[y0:y0 + H, x0:x0 + W], None)
    want = f.copy()
    want[y0:y0 + H, x0:x0 + W][m8 > 0] = rgb[m8 > 0]
    assert np.array_equal(s.frame(), want) and np.array_equal(patch, want[y0:y0 + H, x0:x0 + W])
    assert info["counts"] == _border_numpy(m8, y0, x0, h, w) and info["reruns"] <= 2
    assert info["reruns"] == 2 or not any(info["counts"])


def test_batching_server_windows(model):
    """three sessions, frames of three sizes, windows of one size -> ONE batch of 3; each result equals the same request
    run alone under the pinned mode"""
    rng = np.random.RandomState(8)
    fs = [_frame(rng, w, h) for w, h in [(641, 481), (1283, 963), (300, 277)]]
    sks = []
    for f, (cy, cx) in zip(fs, [(200, 300), (700, 1000), (30, 250)]):
        sk = np.zeros(f.shape[:2], np.uint8)
        sk[cy:cy + 40, cx:cx + 30] = _sketch(rng, 40, 30, 0.1)
        sk[cy, cx] = sk[cy + 39, cx + 29] = 255
        sks.append(sk)
    srv = serve.BatchingServer(model, max_batch=3, max_wait_s=5.0, window=True, max_grow=0)
    sessions = [serve.EditSession(model, f) for f in fs]
    outs = [None] * 3

    def call(i):
        outs[i] = srv.submit(sessions[i], sks[i])
    ts = [threading.Thread(target=call, args=(i,)) for i in range(3)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    pinned = srv._mode(("window", 3, 256, 256))
    srv.close()
    assert srv.batches == [3]
    assert pinned == _lib.Engine.is_low_latency(3, 256, 256)
    for i in range(3):
        patch, (px, py), info = outs[i]
        y0, x0, H, W = info["window"]
        assert (H, W) == (256, 256) and (px, py) == (x0, y0)
        rgb, m8 = _existing_path(model, fs[i][y0:y0 + H, x0:x0 + W], sks[i][y0:y0 + H, x0:x0 + W], pinned)
        want = fs[i].copy()
        want[y0:y0 + H, x0:x0 + W][m8 > 0] = rgb[m8 > 0]
        assert np.array_equal(sessions[i].frame(), want), i
        assert np.array_equal(patch, want[y0:y0 + H, x0:x0 + W]), i
        alone = serve.EditSession(model, fs[i])
        p1, _, _ = alone.edit(sks[i], max_grow=0, low_latency=pinned)
        assert np.array_equal(p1, patch) and np.array_equal(alone.frame(), want), i


def test_refusals_leave_the_frame_untouched(model):
    eng = model.engine()
    rng = np.random.RandomState(9)
    f = _frame(rng, 641, 481)
    ft = torch.from_numpy(f).cuda()
    flags = _lib.flags_from_opt(model.opt)

    def sk(H, W):
        return torch.from_numpy(_sketch(rng, H, W)).cuda()

    for origin, H, W, what in [((481 - 63, 0), 64, 64, "y0"), ((0, 641 - 63), 64, 64, "x0"), ((-1, 0), 64, 64, "y0"),
                               ((0, 0), 60, 64, "H"), ((0, 0), 64, 8, "W")]:
        with pytest.raises(_lib.SketchEditHipError) as e:
            eng.edit_window_u8([ft], [origin], [sk(H, W)], H, W, flags)
        assert what in str(e.value), (what, str(e.value))
        with pytest.raises(_lib.SketchEditHipError):
            eng.window_gather_u8([ft], [origin], [sk(H, W)], H, W)
    rgb = torch.zeros((2, 64, 64, 3), dtype=torch.uint8, device="cuda")
    m8 = torch.full((2, 64, 64), 255, dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.SketchEditHipError) as e:
        eng.window_paste_u8([ft, ft], [(10, 10), (73, 73)], rgb, m8)          # one pixel row / column short of disjoint
    assert "overlapping" in str(e.value)
    with pytest.raises(_lib.SketchEditHipError) as e:
        eng.edit_window_u8([ft, ft], [(10, 10), (40, 40)], [sk(64, 64), sk(64, 64)], 64, 64, flags)
    assert "overlapping" in str(e.value)
    # (uncommitted, overlapping windows of one frame are only read: allowed)
    eng.edit_window_u8([ft, ft], [(10, 10), (40, 40)], [sk(64, 64), sk(64, 64)], 64, 64, flags, commit=False)
    torch.cuda.synchronize()
    assert np.array_equal(ft.cpu().numpy(), f)
