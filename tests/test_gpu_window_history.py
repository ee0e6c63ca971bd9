"""GPU tests of the undo journal of the editing sessions: the two kernels (save, swap) against numpy, the
sessions' undo / redo end to end, and the server.

Every comparison is exact (bytes).  The comparator is the frame's own earlier bytes: a crop made by numpy, or a download of
the frame taken before the operation."""
import threading

import numpy as np
import pytest
import torch

from sketchedit_amd import _lib, serve, synth

pytestmark = pytest.mark.gpu

ARGV = ("--batchSize 1 --name celeb --joint_train_inp --dataset_mode testimage --image_dirs x --mask_dirs x "
        "--image_lists x --model editline2 --netG deepfillc2 --pool_type max --use_cam --output_dir {d} --gpu_ids 0")
SENTINEL = 0xA5
MARGIN = 4099                              # odd, so that the embedded frame starts at an odd address


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


def _embedded(rng, w, h, lead=MARGIN):
    """A random (h,w,3) frame inside a larger device buffer filled with a sentinel -> (buffer, frame view, numpy frame).
    `lead` bytes of sentinel precede the frame, MARGIN follow it."""
    f = rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
    buf = torch.full((lead + f.size + MARGIN,), SENTINEL, dtype=torch.uint8, device="cuda")
    view = buf[lead:lead + f.size].view(h, w, 3)
    view.copy_(torch.from_numpy(f).cuda())
    return buf, view, f


def _whole(buf_np, lead, f):
    """the buffer's expected bytes for frame content f"""
    want = np.full(buf_np.shape, SENTINEL, np.uint8)
    want[lead:lead + f.size] = f.reshape(-1)
    return want


def _windows(w, h):
    """(y0, x0, hs, ws): x0 mod 4 and ws mod 4 over 0..3 (with the odd widths and the odd lead, every dword alignment of a
    row's first and last byte), a window on each frame edge, the corners, the whole frame"""
    out = [(1 + x0, x0, 16 + x0, 16 + k) for x0 in range(4) for k in range(4)]
    out += [(h - 19 - k, 4 + k, 19 + k, 21 + k) for k in range(4)]
    out += [(0, 5, 17, 23), (h - 18, 7, 18, 30), (3, 0, 20, 27), (2, w - 29, 21, 29),            # top, bottom, left, right
            (0, 0, 16, 16), (h - 16, w - 16, 16, 16), (0, 0, h, w)]
    return out


@pytest.mark.parametrize("size", [(1921, 1081), (71, 67)])
def test_save_and_swap_against_numpy(model, size):
    eng = model.engine()
    rng = np.random.RandomState(21)
    w, h = size
    wins = _windows(w, h)
    assert {x0 % 4 for _, x0, _, _ in wins} == {0, 1, 2, 3} and {ws % 4 for _, _, _, ws in wins} == {0, 1, 2, 3}
    for lead in (MARGIN, MARGIN + 1):
        buf, view, f = _embedded(rng, w, h, lead)
        for y0, x0, hs, ws in wins:
            crop = f[y0:y0 + hs, x0:x0 + ws].reshape(hs, 3 * ws)
            slot, = eng.window_save_u8([view], [(y0, x0)], (hs, ws))
            assert slot.numel() == eng.window_saved_bytes(hs, ws) and slot.shape[1] % 16 == 0 and slot.data_ptr() % 16 == 0
            assert np.array_equal(slot.cpu().numpy()[:, :3 * ws], crop), (size, lead, y0, x0, hs, ws)
            assert np.array_equal(buf.cpu().numpy(), _whole(buf.cpu().numpy(), lead, f))          # save writes no frame byte
            # a slot with other content: after swap the rectangle holds it, the slot the old rectangle, nothing else moved
            other = rng.randint(0, 256, tuple(slot.shape), dtype=np.uint8)
            slot.copy_(torch.from_numpy(other).cuda())
            eng.window_swap_u8([view], [(y0, x0)], (hs, ws), [slot])
            want = f.copy()
            want[y0:y0 + hs, x0:x0 + ws] = other[:, :3 * ws].reshape(hs, ws, 3)
            got = buf.cpu().numpy()
            assert np.array_equal(got, _whole(got, lead, want)), (size, lead, y0, x0, hs, ws)      # whole buffer, margins too
            assert np.array_equal(slot.cpu().numpy()[:, :3 * ws], crop), (size, lead, y0, x0, hs, ws)
            # swap twice is the identity
            eng.window_swap_u8([view], [(y0, x0)], (hs, ws), [slot])
            got = buf.cpu().numpy()
            assert np.array_equal(got, _whole(got, lead, f)), (size, lead, y0, x0, hs, ws)
            assert np.array_equal(slot.cpu().numpy()[:, :3 * ws], other[:, :3 * ws])


def test_several_requests_in_one_launch_and_refusals(model):
    eng = model.engine()
    rng = np.random.RandomState(22)
    buf1, v1, f1 = _embedded(rng, 641, 481)
    buf2, v2, f2 = _embedded(rng, 71, 67, MARGIN + 2)
    hs, ws = 33, 35
    origins = [(3, 5), (3, 5 + ws), (34, 36)]              # two disjoint windows of frame 1 (touching), one of frame 2
    frames, fs = [v1, v1, v2], [f1, f1, f2]
    slots = eng.window_save_u8(frames, origins, (hs, ws))
    crops = [f[y0:y0 + hs, x0:x0 + ws].reshape(hs, 3 * ws) for f, (y0, x0) in zip(fs, origins)]
    for s, c in zip(slots, crops):
        assert np.array_equal(s.cpu().numpy()[:, :3 * ws], c)
    others = [rng.randint(0, 256, tuple(s.shape), dtype=np.uint8) for s in slots]
    for s, o in zip(slots, others):
        s.copy_(torch.from_numpy(o).cuda())
    eng.window_swap_u8(frames, origins, (hs, ws), slots)
    w1, w2 = f1.copy(), f2.copy()
    for want, (y0, x0), o in zip([w1, w1, w2], origins, others):
        want[y0:y0 + hs, x0:x0 + ws] = o[:, :3 * ws].reshape(hs, ws, 3)
    g1, g2 = buf1.cpu().numpy(), buf2.cpu().numpy()
    assert np.array_equal(g1, _whole(g1, MARGIN, w1)) and np.array_equal(g2, _whole(g2, MARGIN + 2, w2))
    for s, c in zip(slots, crops):
        assert np.array_equal(s.cpu().numpy()[:, :3 * ws], c)
    # refusals: non-zero before anything is enqueued, frames and slots untouched
    before = [s.cpu().numpy() for s in slots]

    def refused(what, fn, *a):
        with pytest.raises(_lib.SketchEditHipError) as e:
            fn(*a)
        assert what in str(e.value), (what, str(e.value))

    refused("overlapping", eng.window_swap_u8, [v1, v1], [(3, 5), (3 + hs - 1, 5 + ws - 1)], (hs, ws), slots[:2])
    refused("x0", eng.window_swap_u8, [v1], [(3, 641 - ws + 1)], (hs, ws), slots[:1])
    refused("y0", eng.window_save_u8, [v1], [(481 - hs + 1, 0)], (hs, ws))
    refused("hs=15", eng.window_save_u8, [v1], [(0, 0)], (15, 64))
    refused("ws=15", eng.window_swap_u8, [v1], [(0, 0)], (64, 15), slots[:1])
    refused("aligned", eng.window_swap_u8, [v1], [(3, 5)], (hs, ws), [torch.empty(slots[0].numel() + 16, dtype=torch.uint8, device="cuda")[8:]])
    refused("overlap", eng.window_swap_u8, [v1, v2], [(3, 5), (3, 5)], (hs, ws), [slots[0], slots[0]])
    lib, ptrs = eng.lib, (eng.lib.se_window_save_u8.argtypes[-1]._type_ * 1)(None)
    assert lib.se_window_save_u8(eng.h, eng._stream(), eng._windows([v1], [(3, 5)]), 1, hs, ws, ptrs) != 0
    assert b"slots[0] is null" in lib.se_last_error(eng.h)
    torch.cuda.synchronize()
    g1, g2 = buf1.cpu().numpy(), buf2.cpu().numpy()
    assert np.array_equal(g1, _whole(g1, MARGIN, w1)) and np.array_equal(g2, _whole(g2, MARGIN + 2, w2))
    assert all(np.array_equal(s.cpu().numpy(), b) for s, b in zip(slots, before))


def _two_sketches(rng, h, w):
    """two sketches whose default windows (256 x 256) overlap"""
    out = []
    for cy, cx in ((300, 500), (380, 560)):
        sk = np.zeros((h, w), np.uint8)
        sk[cy:cy + 60, cx:cx + 100] = ((rng.rand(60, 100) < 0.05) * 255).astype(np.uint8)
        sk[cy, cx] = sk[cy + 59, cx + 99] = 255
        out.append(sk)
    return out


@pytest.mark.parametrize("max_grow", [0, 2])
@pytest.mark.parametrize("max_side", [None, 640])
@pytest.mark.parametrize("low_latency", [True, False])
def test_sessions_undo_redo_end_to_end(model, low_latency, max_side, max_grow):
    rng = np.random.RandomState(23)
    w, h = 1283, 963
    f = rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
    skA, skB = _two_sketches(rng, h, w)
    s = serve.EditSession(model, f, history=8)
    kw = dict(max_grow=max_grow, low_latency=low_latency, max_side=max_side)
    f0 = s.frame()
    assert np.array_equal(f0, f)
    _, _, ia = s.edit(skA, **kw)
    f1 = s.frame()
    _, _, ib = s.edit(skB, **kw)
    f2 = s.frame()
    assert not np.array_equal(f1, f0) and not np.array_equal(f2, f1)          # an undo of nothing cannot pass
    assert ia["undoable"] is True and ib["undoable"] is True
    (ay, ax, ah, aw), (by, bx, bh, bw) = ia["window"], ib["window"]
    assert ay < by + bh and by < ay + ah and ax < bx + bw and bx < ax + aw      # the windows overlap
    assert s.history_bytes_used == serve.window_saved_bytes(ah, aw) + serve.window_saved_bytes(bh, bw)

    def check(out, win, want, depths):
        patch, (px, py), info = out
        y0, x0, hh, ww = win
        got = s.frame()
        assert np.array_equal(got, want)                                        # byte for byte on the whole frame
        assert np.array_equal(patch, want[y0:y0 + hh, x0:x0 + ww]) and (px, py) == (x0, y0)
        assert info == dict(window=win, undo_depth=depths[0], redo_depth=depths[1])

    check(s.undo(), ib["window"], f1, (1, 1))
    check(s.undo(), ia["window"], f0, (0, 2))
    with pytest.raises(IndexError):
        s.undo()
    check(s.redo(), ia["window"], f1, (1, 1))
    check(s.redo(), ib["window"], f2, (2, 0))
    with pytest.raises(IndexError):
        s.redo()


@pytest.mark.parametrize("max_side", [None, 640])
def test_history_does_not_change_an_edit(model, max_side):
    rng = np.random.RandomState(24)
    w, h = 1283, 963
    f = rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
    sks = _two_sketches(rng, h, w)
    results = []
    for history in (0, 8):
        s = serve.EditSession(model, f, history=history)
        patches = []
        for sk, grow in zip(sks + sks[:1], (0, 2, 0)):
            patch, pos, info = s.edit(sk, max_grow=grow, low_latency=True, max_side=max_side)
            assert ("undoable" in info) == (history > 0)
            patches.append((patch, pos, info["window"], info["counts"]))
        results.append((s.frame(), patches))
    (fa, pa), (fb, pb) = results
    assert np.array_equal(fa, fb) and not np.array_equal(fa, f)
    for (p0, pos0, w0, c0), (p1, pos1, w1, c1) in zip(pa, pb):
        assert np.array_equal(p0, p1) and pos0 == pos1 and w0 == w1 and c0 == c1


def test_server_undo_matches_standalone_sessions(model):
    """two sessions, frames of different sizes, one server; per session: edit, edit, undo, edit submitted from one thread
    (in order), the sessions' threads running concurrently.  The final frames equal those of stand-alone sessions."""
    rng = np.random.RandomState(25)
    sizes = [(1283, 963), (801, 701)]
    fs = [rng.randint(0, 256, (h, w, 3), dtype=np.uint8) for w, h in sizes]
    sks = [_two_sketches(rng, h, w) for w, h in sizes]
    srv = serve.BatchingServer(model, max_batch=2, max_wait_s=0.02, window=True, max_grow=0)
    pinned = srv._mode(("window", 3, 256, 256))
    sessions = [serve.EditSession(model, f, history=4) for f in fs]
    logs = [[], []]

    def work(i):
        a, b = sks[i]
        logs[i].append(srv.submit(sessions[i], a))
        logs[i].append(srv.submit(sessions[i], b))
        logs[i].append(srv.undo(sessions[i]))                 # undoes b
        logs[i].append(srv.submit(sessions[i], a))
        logs[i].append(srv.undo(sessions[i]))
        logs[i].append(srv.redo(sessions[i]))
    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    with pytest.raises(IndexError):
        srv.redo(sessions[0])
    srv.close()
    for i in range(2):
        alone = serve.EditSession(model, fs[i], history=4)
        a, b = sks[i]
        want = [alone.edit(a, max_grow=0, low_latency=pinned), alone.edit(b, max_grow=0, low_latency=pinned), alone.undo(),
                alone.edit(a, max_grow=0, low_latency=pinned), alone.undo(), alone.redo()]
        assert len(logs[i]) == len(want)
        for got, exp in zip(logs[i], want):
            assert np.array_equal(got[0], exp[0]) and got[1] == exp[1] and got[2]["window"] == exp[2]["window"], i
        assert logs[i][2][2] == dict(window=want[1][2]["window"], undo_depth=1, redo_depth=1)
        assert np.array_equal(sessions[i].frame(), alone.frame()) and not np.array_equal(alone.frame(), fs[i]), i
        assert sessions[i].can_undo and not sessions[i].can_redo
