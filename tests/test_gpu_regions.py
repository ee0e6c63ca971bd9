"""GPU tests of the region edits: the tile kernel against its numpy restatement (tests/sketch_tiles_util.py),
exactly, and `EditSession.edit_regions` against its definition -- the frame after the equivalent single-window edits, byte for
byte -- with history, a lock, a working size and under SE_TEST_POISON.

Shared setup of the forward tests: procedural weights, an 80 x 280 frame of seeded noise, min_side=64, bucket=8, tile=16 and
low_latency=False on both sides.  The windows are serve.choose_window's, recomputed on the host in
tests/test_regions_host.py::test_split_literals."""
import ctypes

import numpy as np
import pytest
import torch

from sketchedit_amd import _lib, serve, synth
from sketch_tiles_util import sketch_tiles

pytestmark = pytest.mark.gpu

ARGV = ("--batchSize 1 --name celeb --joint_train_inp --dataset_mode testimage --image_dirs x --mask_dirs x "
        "--image_lists x --model editline2 --netG deepfillc2 --pool_type max --use_cam --output_dir {d} --gpu_ids 0")
HW = (80, 280)
KW = dict(tile=16, min_side=64, bucket=8)
TWO = [(10, 20, 10, 20), (50, 60, 250, 260)]                  # strokes as (y0, y1, x0, x1)
THREE = TWO + [(30, 34, 90, 130)]
MERGE = [(10, 20, 10, 20), (10, 20, 70, 80)]
W1, W2, W3 = (0, 0, 64, 64), (16, 216, 64, 64), (0, 70, 64, 80)


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
    return np.random.RandomState(31).randint(0, 256, HW + (3,), dtype=np.uint8)


def _sketch(strokes, hw=HW):
    sk = np.zeros(hw, np.uint8)
    for y0, y1, x0, x1 in strokes:
        sk[y0:y1, x0:x1] = 255
    return sk


# ---- the kernel -------------------------------------------------------------------------------------------------------------
def _planes(rng, Hi, Wi, tile):
    """the sketches of one plane size: name -> (Hi,Wi) uint8"""
    out = {"empty": np.zeros((Hi, Wi), np.uint8), "full": np.full((Hi, Wi), 255, np.uint8)}
    c = np.zeros((Hi, Wi), np.uint8)
    c[0, 0], c[0, -1], c[-1, 0], c[-1, -1] = 1, 2, 128, 255
    out["corners"] = c
    c = np.zeros((Hi, Wi), np.uint8)
    c[Hi // 2, Wi - 1] = 1
    out["last_column"] = c
    c = np.zeros((Hi, Wi), np.uint8)
    ys = [y for b in range(tile, Hi, tile) for y in (b - 1, b)]
    xs = [x for b in range(tile, Wi, tile) for x in (b - 1, b)]
    for y in ys:                                              # a pixel on both sides of every boundary, along it and across it
        c[y, ::5] = 3
    for x in xs:
        c[1::7, x] = 200
    for y in ys:
        for x in xs:
            c[y, x] = 9
    out["boundaries"] = c
    out["noise"] = ((rng.rand(Hi, Wi) < 0.02) * rng.randint(1, 256, (Hi, Wi))).astype(np.uint8)
    return out


@pytest.mark.parametrize("hw", [(16, 16), (45, 67), (64, 64), (70, 130)])
def test_tiles_kernel_against_numpy(model, hw):
    eng = model.engine()
    rng = np.random.RandomState(7)
    Hi, Wi = hw
    for tile in (16, 32, 64):
        for name, sk in _planes(rng, Hi, Wi, tile).items():
            want = sketch_tiles(sk, tile)
            assert want[..., 0].sum() == (sk > 0).sum()
            assert sk.any() or name == "empty" or (name == "boundaries" and max(hw) <= tile)
            for off in (1, 2, 3):
                # the plane inside a buffer of 255s: a byte read outside it would change a count
                buf = torch.full((Hi * Wi + 64,), 255, dtype=torch.uint8, device="cuda")
                view = buf[off:off + Hi * Wi].view(Hi, Wi)
                view.copy_(torch.from_numpy(sk).cuda())
                assert view.data_ptr() % 4 == off
                out = torch.full(want.shape, -0x54545455, dtype=torch.int32, device="cuda")      # every byte 0xAB
                got = eng.sketch_tiles_u8(view, tile, out=out)
                assert got is out and np.array_equal(out.cpu().numpy(), want), (hw, tile, name, off)
                again = eng.sketch_tiles_u8(view, tile)       # the same input, the same bits (a fresh, unzeroed buffer)
                assert torch.equal(again, out)


def test_tiles_refusals_leave_the_output_untouched(model):
    eng = model.engine()
    st = ctypes.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream)
    sk = torch.full((64, 64), 255, dtype=torch.uint8, device="cuda")
    out = torch.full((4 * 4 * 5 + 1,), -0x54545455, dtype=torch.int32, device="cuda")
    call = eng.lib.se_sketch_tiles_u8
    p = ctypes.c_void_p
    cases = [((p(sk.data_ptr()), 15, 64, 16, p(out.data_ptr())), "Hi"), ((p(sk.data_ptr()), 64, 15, 16, p(out.data_ptr())), "Wi"),
             ((p(sk.data_ptr()), 64, 64, 8, p(out.data_ptr())), "tile"), ((p(sk.data_ptr()), 64, 64, 48, p(out.data_ptr())), "tile"),
             ((p(sk.data_ptr()), 64, 64, 0, p(out.data_ptr())), "tile"), ((p(sk.data_ptr()), 64, 64, 128, p(out.data_ptr())), "tile"),
             ((None, 64, 64, 16, p(out.data_ptr())), "sketch_u8"), ((p(sk.data_ptr()), 64, 64, 16, None), "tiles_out"),
             ((p(sk.data_ptr()), 64, 64, 16, p(out.data_ptr() + 2)), "tiles_out")]
    for args, word in cases:
        assert call(eng.h, st, *args) != 0, args
        assert word in eng.lib.se_last_error(eng.h).decode(), (args, eng.lib.se_last_error(eng.h))
    torch.cuda.synchronize()
    assert (out == -0x54545455).all()
    with pytest.raises(_lib.SketchEditHipError, match="tile"):
        eng.sketch_tiles_u8(sk, 24)
    with pytest.raises(_lib.SketchEditHipError):
        eng.sketch_tiles_u8(sk[None], 16)
    assert call(eng.h, st, p(sk.data_ptr()), 64, 64, 16, p(out.data_ptr())) == 0      # and the call they all resemble is accepted
    assert np.array_equal(out[:80].cpu().numpy().reshape(4, 4, 5), sketch_tiles(np.full((64, 64), 255, np.uint8), 16))


# ---- edit_regions against its definition --------------------------------------------------------------------------------
def _sequential(model, frame, sk, wins, lock=None, **kw):
    """the definition: one pinned single-window edit per window, in the order given -> the frame"""
    s = serve.EditSession(model, frame)
    if lock is not None:
        s.set_lock(lock)
    for w in wins:
        s.edit(sk, window=w, max_grow=0, low_latency=False, **kw)
    return s.frame()


def _forwards(model, monkeypatch):
    """records the batch size of every window forward of the model"""
    sizes, real = [], model.edit_window_u8

    def spy(frames, *a, **kw):
        sizes.append(len(frames))
        return real(frames, *a, **kw)
    monkeypatch.setattr(model, "edit_window_u8", spy)
    return sizes


@pytest.mark.parametrize("strokes,wins,batches", [(TWO, [W1, W2], [2]), (THREE, [W1, W3, W2], [2, 1])], ids=["two", "three"])
def test_regions_equal_the_single_window_edits(model, frame, monkeypatch, strokes, wins, batches):
    sk = _sketch(strokes)
    s = serve.EditSession(model, frame)
    sizes = _forwards(model, monkeypatch)
    patches, origins, info = s.edit_regions(sk, low_latency=False, **KW)
    assert sizes == batches and info["groups"] == len(batches)
    monkeypatch.undo()
    assert info["windows"] == wins and origins == [(w[1], w[0]) for w in wins] and len(info["counts"]) == len(wins)
    got = s.frame()
    for (y0, x0, h, w), patch in zip(wins, patches):
        assert np.array_equal(patch, got[y0:y0 + h, x0:x0 + w])
        assert not np.array_equal(patch, frame[y0:y0 + h, x0:x0 + w])           # every region was edited
    outside = np.ones(HW, bool)
    for y0, x0, h, w in wins:
        outside[y0:y0 + h, x0:x0 + w] = False
    assert np.array_equal(got[outside], frame[outside])
    assert np.array_equal(got, _sequential(model, frame, sk, wins))             # whole frame, byte for byte
    assert np.array_equal(got, _sequential(model, frame, sk, wins[::-1]))       # in either order


def test_merged_strokes_are_the_single_window_edit(model, frame):
    sk = _sketch(MERGE)
    s = serve.EditSession(model, frame)
    _, _, info = s.edit_regions(sk, low_latency=False, **KW)
    assert info["windows"] == [(0, 0, 80, 144)] and info["groups"] == 1
    ref = serve.EditSession(model, frame)
    _, _, rinfo = ref.edit(sk, window=serve.choose_window(serve.sketch_bbox(sk), HW, min_side=64, bucket=8), max_grow=0, low_latency=False)
    assert rinfo["window"] == (0, 0, 80, 144) and info["counts"] == [rinfo["counts"]]
    assert np.array_equal(s.frame(), ref.frame()) and not np.array_equal(s.frame(), frame)


def test_one_undo_takes_the_whole_region_edit_back(model, frame):
    s = serve.EditSession(model, frame, history=2)
    _, _, info = s.edit_regions(_sketch(THREE), low_latency=False, **KW)
    assert info["undoable"] is True and s.history_bytes_used == sum(serve.window_saved_bytes(w[2], w[3]) for w in (W1, W2, W3))
    f1 = s.frame()
    assert not np.array_equal(f1, frame)
    patches, origins, uinfo = s.undo()
    assert np.array_equal(s.frame(), frame) and not s.can_undo                  # ONE step, byte for byte
    assert uinfo == dict(windows=[W1, W3, W2], undo_depth=0, redo_depth=1)
    assert all(np.array_equal(p, frame[y0:y0 + p.shape[0], x0:x0 + p.shape[1]]) for p, (x0, y0) in zip(patches, origins))
    s.redo()
    assert np.array_equal(s.frame(), f1) and s.can_undo and not s.can_redo


def test_regions_with_a_lock(model, frame):
    sk = _sketch(TWO)
    lock = np.zeros(HW, np.uint8)
    lock[5:75, 12:16] = 1                                     # crosses window 1's stroke and its lower edge
    s = serve.EditSession(model, frame)
    s.set_lock(lock)
    _, _, info = s.edit_regions(sk, low_latency=False, **KW)
    assert info["locked"] is True and info["windows"] == [W1, W2]
    got = s.frame()
    assert np.array_equal(got[lock > 0], frame[lock > 0]) and not np.array_equal(got, frame)
    assert np.array_equal(got, _sequential(model, frame, sk, [W1, W2], lock=lock))
    assert not np.array_equal(got, _sequential(model, frame, sk, [W1, W2]))     # the lock decided something


def test_regions_at_a_working_size(model, frame):
    sk = _sketch(THREE)
    s = serve.EditSession(model, frame)
    _, _, info = s.edit_regions(sk, low_latency=False, max_side=32, **KW)
    assert info["work"] == [(32, 32), (24, 32), (32, 32)] and info["groups"] == 2
    got = s.frame()
    assert np.array_equal(got, _sequential(model, frame, sk, [W1, W3, W2], max_side=32)) and not np.array_equal(got, frame)


def test_regions_do_not_read_unwritten_scratch(model, frame, seopt):
    sk = _sketch(TWO)
    outs = []
    for v in (0, 0x55, 0xAA):
        seopt.set("SE_TEST_POISON", v)
        s = serve.EditSession(model, frame, history=1)
        _, _, info = s.edit_regions(sk, low_latency=False, **KW)
        outs.append((s.frame(), info["counts"]))
    seopt.set("SE_TEST_POISON", 0)
    assert not np.array_equal(outs[0][0], frame)
    for f, counts in outs[1:]:
        assert np.array_equal(f, outs[0][0]) and counts == outs[0][1]
