"""GPU tests of `feather=` in the editing sessions against its definition: the frame after
edit(S, window=w, max_grow=0, feather=r) is the frame on which tests/feather_util.py pasted, on the host, the results of the
uncommitted model.edit_window_u8 of the same arguments (resized to the window when the edit ran at a working size).  Procedural
weights, small frames of seeded noise, one pinned execution mode (low_latency=False) on both sides."""
import io
import threading

import numpy as np
import pytest
import torch

import feather_util as FU
from sketchedit_amd import serve, synth
from strokes_util import spec_raster

pytestmark = pytest.mark.gpu

ARGV = ("--batchSize 1 --name celeb --joint_train_inp --dataset_mode testimage --image_dirs x --mask_dirs x "
        "--image_lists x --model editline2 --netG deepfillc2 --pool_type max --use_cam --output_dir {d} --gpu_ids 0")
HW = (96, 120)
WIN = (17, 25, 64, 64)                                        # (y0, x0, h, w): inside the frame, odd origin
WIN_ODD = (5, 3, 70, 90)                                      # sides that are no multiples of 8: only a working size takes them
R = 5


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
def frame():
    return np.random.RandomState(41).randint(0, 256, HW + (3,), dtype=np.uint8)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sketch(hw=HW, boxes=((40, 50, 45, 75),)):
    sk = np.zeros(hw, np.uint8)
    for y0, y1, x0, x1 in boxes:
        sk[y0:y1, x0:x1] = 255
    return sk


def _defined(model, frame, sk, win, r, max_side=None, lock=None):
    """the definition, on the host: -> (the frame it gives, the frame the hard paste of the same results gives)"""
    y0, x0, h, w = win
    ft = _cuda(frame)
    work = serve.choose_working_size((h, w), max_side) if max_side is not None else None
    rgb, m8, _ = model.edit_window_u8([ft], [(y0, x0)], [sk[y0:y0 + h, x0:x0 + w]], h, w, commit=False, low_latency=False, work_hw=work,
                                      locks=None if lock is None else [_cuda(lock)])
    if work is not None:
        assert tuple(rgb.shape[1:3]) == work and work != (h, w)
        rgb, m8 = model.engine().resize_u8(rgb, (h, w)), model.engine().resize_u8(m8, (h, w))
    assert np.array_equal(ft.cpu().numpy(), frame)                                    # nothing was committed
    rgb, m8 = rgb[0].cpu().numpy(), m8[0].cpu().numpy()
    return FU.feather_paste(frame, (y0, x0), rgb, m8, r, lock=lock), FU.feather_paste(frame, (y0, x0), rgb, m8, 0, lock=lock)


@pytest.mark.parametrize("variant", ["plain", "max_side", "lock"])
def test_edit_is_its_definition(model, frame, variant):
    sk = _sketch()
    win, kw, lock = WIN, {}, None
    if variant == "max_side":
        win, kw = WIN_ODD, dict(max_side=48)
    if variant == "lock":
        lock = np.zeros(HW, np.uint8)
        lock[30:70, 58:62] = 255                              # crosses the stroke
    for r in (R, 16):
        s = serve.EditSession(model, frame)
        if lock is not None:
            s.set_lock(lock)
        patch, (x0, y0), info = s.edit(sk, window=win, max_grow=0, low_latency=False, feather=r, **kw)
        want, hard = _defined(model, frame, sk, win, r, lock=lock, **kw)
        got = s.frame()
        assert info["feather"] == r and info["window"] == win and (y0, x0) == win[:2]
        assert np.array_equal(got, want), (variant, r, np.argwhere(got != want)[:5].tolist())
        assert np.array_equal(patch, got[win[0]:win[0] + win[2], win[1]:win[1] + win[3]])
        assert not np.array_equal(want, hard) and not np.array_equal(hard, frame)    # the soft edge decided something
        assert ((want != frame).any(2) <= (hard != frame).any(2)).all()                # and changed no pixel the hard paste leaves
        if lock is not None:
            assert info["locked"] is True and np.array_equal(got[lock > 0], frame[lock > 0])
        # feather=0 and None are the hard paste of the same results
        for f0 in (0, None) if r == R else ():
            s0 = serve.EditSession(model, frame)
            if lock is not None:
                s0.set_lock(lock)
            _, _, info0 = s0.edit(sk, window=win, max_grow=0, low_latency=False, feather=f0, **kw)
            assert "feather" not in info0 and np.array_equal(s0.frame(), hard), (variant, f0)


def test_undo_and_redo_are_byte_exact(model, frame):
    s = serve.EditSession(model, frame, history=2)
    _, _, info = s.edit(_sketch(), window=WIN, max_grow=0, low_latency=False, feather=R)
    assert info["undoable"] is True and info["feather"] == R
    f1 = s.frame()
    assert not np.array_equal(f1, frame)
    s.undo()
    assert np.array_equal(s.frame(), frame) and not s.can_undo
    s.redo()
    assert np.array_equal(s.frame(), f1) and s.can_undo and not s.can_redo


def _sequential(model, frame, sk, wins, **kw):
    s = serve.EditSession(model, frame)
    for w in wins:
        s.edit(sk, window=w, max_grow=0, low_latency=False, **kw)
    return s.frame()


def test_regions_equal_the_single_window_feathered_edits(model):
    hw = (80, 280)
    frame = np.random.RandomState(31).randint(0, 256, hw + (3,), dtype=np.uint8)
    sk = _sketch(hw, [(10, 20, 10, 20), (50, 60, 250, 260), (30, 34, 90, 130)])
    s = serve.EditSession(model, frame, history=1)
    _, _, info = s.edit_regions(sk, low_latency=False, feather=R, tile=16, min_side=64, bucket=8)
    wins = info["windows"]
    assert len(wins) == 3 and info["groups"] == 2 and info["feather"] == R and info["undoable"] is True
    got = s.frame()
    assert np.array_equal(got, _sequential(model, frame, sk, wins, feather=R))
    assert not np.array_equal(got, _sequential(model, frame, sk, wins))              # not the hard paste
    s.undo()
    assert np.array_equal(s.frame(), frame)                                           # ONE step


def test_strokes_equal_the_single_window_feathered_edits(model):
    hw = (256, 320)
    frame = np.random.RandomState(37).randint(0, 256, hw + (3,), dtype=np.uint8)
    strokes = [([(20.5, 20.5), (50.5, 50.5)], 3.0), ([(265.5, 195.5), (295.5, 225.5), (270.0, 230.0)], 4.0)]
    full = spec_raster(serve.stroke_segments(strokes, hw)[0], hw)
    s = serve.EditSession(model, frame)
    _, _, info = s.edit_strokes(strokes, low_latency=False, feather=R, min_side=64)
    assert len(info["windows"]) == 2 and info["groups"] == 1 and info["feather"] == R
    got = s.frame()
    assert np.array_equal(got, _sequential(model, frame, full, info["windows"], feather=R)) and not np.array_equal(got, frame)


def test_png_patch_is_the_feathered_window(model, frame):
    from PIL import Image
    s = serve.EditSession(model, frame)
    png, (x0, y0), info = s.edit(_sketch(), window=WIN, max_grow=0, low_latency=False, feather=R, encode="png")
    got = s.frame()
    want, _ = _defined(model, frame, _sketch(), WIN, R)
    assert np.array_equal(got, want)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(png)).convert("RGB")), got[y0:y0 + 64, x0:x0 + 64])


def test_batching_server_feathers_a_shared_group(model):
    rng = np.random.RandomState(43)
    fs = [rng.randint(0, 256, (301, 331, 3), dtype=np.uint8), rng.randint(0, 256, (290, 400, 3), dtype=np.uint8)]
    sks = [_sketch(fs[0].shape[:2], [(120, 130, 170, 200)]), _sketch(fs[1].shape[:2], [(100, 110, 200, 260)])]
    srv = serve.BatchingServer(model, max_batch=2, max_wait_s=5.0, window=True, max_grow=0, feather=R)
    sessions = [serve.EditSession(model, fs[0], history=1), serve.EditSession(model, fs[1])]
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
        alone = serve.EditSession(model, fs[i], history=1 if i == 0 else 0)
        p1, pos1, info1 = alone.edit(sks[i], max_grow=0, low_latency=pinned, feather=R)
        assert info["feather"] == R and pos1 == pos and info1 == info and np.array_equal(p1, patch), i
        assert np.array_equal(alone.frame(), sessions[i].frame()) and not np.array_equal(alone.frame(), fs[i]), i
        hard = serve.EditSession(model, fs[i])
        hard.edit(sks[i], max_grow=0, low_latency=pinned)
        assert not np.array_equal(hard.frame(), alone.frame()), i
    sessions[0].undo()
    assert np.array_equal(sessions[0].frame(), fs[0])
