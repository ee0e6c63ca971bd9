"""GPU tests of the stroke edits: the rasteriser se_sketch_strokes_u8 against the integer rule's numpy statement
(tests/strokes_util.py), byte for byte, inside a buffer of sentinels; and `EditSession.edit_strokes` against its definition --
the frame after the single-window edits of the rule's full-size sketch -- with a lock, a working size, under SE_TEST_POISON, and
one undo.

Shapes: windows 16x16, 24x40, 64x72 (one 64 x 16 tile; a ragged tile in both directions; two columns of tiles, the second 8
wide) and 17x21 (rows of every alignment within one output), frames up to 96x120, every output at the four byte alignments."""
import ctypes

import numpy as np
import pytest
import torch

from sketchedit_amd import _lib, serve, synth
from strokes_util import spec_raster

pytestmark = pytest.mark.gpu

ARGV = ("--batchSize 1 --name celeb --joint_train_inp --dataset_mode testimage --image_dirs x --mask_dirs x "
        "--image_lists x --model editline2 --netG deepfillc2 --pool_type max --use_cam --output_dir {d} --gpu_ids 0")
PAD = 96                                                      # sentinel bytes on either side of sketch_out
OUT, SENTINEL = 0xAB, 0x5C


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


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
def _rasterise(eng, segs, recs, hw, ranges, off):
    """recs = [(Hi, Wi, y0, x0)] -> (B,hs,ws) uint8 on the host; the output starts `off` bytes past a 4-byte boundary, is
    pre-filled with 0xAB and lies between sentinels that must survive"""
    hs, ws = hw
    n = len(recs) * hs * ws
    buf = torch.full((PAD + 4 + n + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = buf[PAD + off:PAD + off + n]
    out.fill_(OUT)
    assert out.data_ptr() % 4 == off
    dsegs = torch.from_numpy(np.ascontiguousarray(segs, np.int32).reshape(-1, 5)).cuda()
    got = eng.sketch_strokes_u8(dsegs, [r[:2] for r in recs], [r[2:] for r in recs], hw, ranges=ranges, out=out)
    assert got is out
    host = buf.cpu().numpy()
    assert (host[:PAD + off] == SENTINEL).all() and (host[PAD + off + n:] == SENTINEL).all(), "a byte outside sketch_out was written"
    return host[PAD + off:PAD + off + n].reshape(len(recs), hs, ws)


def _want(segs, recs, hw, ranges):
    segs = np.asarray(segs, np.int64).reshape(-1, 5)
    return np.stack([spec_raster(segs[f:f + n], (Hi, Wi), (y0, x0) + tuple(hw)) for (Hi, Wi, y0, x0), (f, n) in zip(recs, ranges)])


def _check(eng, segs, recs, hw, ranges, offs=(0, 1, 2, 3)):
    want = _want(segs, recs, hw, ranges)
    for off in offs:
        got = _rasterise(eng, segs, recs, hw, ranges, off)
        assert np.array_equal(got, want), (hw, off, np.argwhere(got != want)[:5].tolist())
    return want


def _centre(y, x):
    return [4 * x + 2, 4 * y + 2]


@pytest.mark.parametrize("hw", [(16, 16), (24, 40), (64, 72), (17, 21)])
def test_kernel_against_the_rule(model, hw):
    eng = model.engine()
    hs, ws = hw
    Hi, Wi = 96, 120
    ym, xm = min(5, 90 - hs), min(7, 117 - ws)                # an origin that is no multiple of 4, inside the smaller frame too
    assert ym % 4 and xm % 4
    recs = [(Hi, Wi, 0, 0), (Hi, Wi, Hi - hs, Wi - ws), (90, 117, ym, xm)]      # top + left edge; bottom + right edge; inside
    segs = [
        _centre(0, 0) * 2 + [3],                                                # dots at r = 3: on the frame's first pixel,
        [0, 0, 0, 0, 3], [4 * Wi, 4 * Hi, 4 * Wi, 4 * Hi, 3],                   # on the rectangle's corners,
        _centre(ym + hs - 1, xm + ws - 1) * 2 + [3],                            # on the inside window's last pixel,
        _centre(ym + hs, xm + ws) * 2 + [3],                                    # and one pixel past it diagonally (misses it)
        [4 * 3, 4 * 2, 4 * (ws + 9), 4 * (hs - 3) + 1, 5],                      # a thin line across the window and out of it
        [4 * (Wi - 2), 4 * 10, 4 * (Wi - ws // 2), 4 * (Hi - 1) + 3, 23],       # a thick one along the right edge
        [4 * Wi, 0, 4 * Wi, 0, 512],                                            # r = 512 from the top right corner: 128 pixels
        [4 * (xm + ws + 3), 4 * (ym + hs - 5), 4 * (xm + ws - 5), 4 * (ym + hs + 3), 4],       # clips the inside window's corner
        [4 * (xm + ws + 30), 4 * (ym + hs + 20), 4 * (xm + ws + 40), 4 * (ym + hs + 25), 9],   # wholly outside every window
    ]
    N = len(segs)
    # B = 3 with different ranges: everything; nothing; a shared part (without the disc that covers small windows whole)
    want = _check(eng, segs, recs, hw, [(0, N), (4, 0), (3, 4)])
    assert want[0].any() and not want[1].any() and want[2].any() and not want[2].all()
    # each kind alone, on the inside window: a dot is one pixel, the clip a few pixels of the corner, the far segment nothing
    one = [recs[2]] * 4
    want = _check(eng, segs, one, hw, [(3, 1), (4, 1), (8, 1), (9, 1)], offs=(0, 3))
    assert want[0].sum() == 255 and want[0][-1, -1] == 255 and not want[1].any() and not want[3].any()
    assert 0 < (want[2] > 0).sum() <= 12 and want[2][-1, -1] == 255 and not want[2][:-4].any() and not want[2][:, :-4].any()
    # r = 512 alone: a disc of 128 pixels around the top right corner; its edge cuts the largest window at the top left
    want = _check(eng, segs, [recs[1], recs[0]], hw, [(7, 1), (7, 1)], offs=(1,))
    assert want[0].any() and want[1].any() and want[1].all() == (hw != (64, 72))


def test_more_segments_than_one_chunk(model):
    eng = model.engine()
    rng = np.random.RandomState(23)
    Hi, Wi, hw = 96, 120, (24, 40)
    N = 600                                                   # three chunks of 256, the last one ragged
    a = np.stack([rng.randint(0, 4 * Wi + 1, N), rng.randint(0, 4 * Hi + 1, N)], 1)
    d = rng.randint(-60, 61, (N, 2))
    b = np.clip(a + d, 0, [4 * Wi, 4 * Hi])
    segs = np.concatenate([a, b, rng.randint(3, 9, (N, 1))], 1)
    segs[::7, 2:4] = segs[::7, 0:2]                           # some dots
    recs = [(Hi, Wi, 33, 41), (Hi, Wi, 33, 41), (Hi, Wi, 70, 79), (Hi, Wi, 1, 2)]
    ranges = [(0, N), (250, 300), (0, N), (257, 343)]         # two requests share segments; a range across chunk boundaries
    want = _check(eng, segs, recs, hw, ranges, offs=(0, 2))
    assert all(w.any() and not w.all() for w in want) and not np.array_equal(want[0], want[1])
    # a chunk in which EVERY segment is kept, and more than a chunk of them: 300 dots inside one 16 x 16 window
    dots = np.stack([rng.randint(4 * 40, 4 * 56, 300), rng.randint(4 * 30, 4 * 46, 300)], 1)
    segs = np.concatenate([dots, dots, np.full((300, 1), 3)], 1)
    want = _check(eng, segs, [(Hi, Wi, 30, 40)], (16, 16), [(0, 300)], offs=(0,))
    assert 100 < (want > 0).sum() < 256


def test_the_64_bit_range(model):
    # only the record says 8192: corner to corner at r = 512, where cr^2 is the largest value of the rule (below 2^62)
    eng = model.engine()
    seg = [[0, 0, 4 * 8192, 4 * 8192, 512], [4 * 8192, 0, 0, 4 * 8192, 512]]
    recs = [(8192, 8192, 4000, 4173), (8192, 8192, 8176, 8176), (8192, 8192, 0, 8176), (8192, 8192, 0, 8176)]
    want = _check(eng, seg, recs, (16, 16), [(0, 1), (0, 1), (0, 1), (1, 1)], offs=(0, 1))
    edge = np.abs(np.subtract.outer(np.arange(4000, 4016), np.arange(4173, 4189))) <= 181      # 16 (x - y)^2 <= 2 * 512^2
    assert np.array_equal(want[0] > 0, edge) and edge.any() and not edge.all()
    assert want[1].all() and not want[2].any() and want[3].all()


def test_any_int32_in_the_segments_is_safe(model):
    # the limits are the caller's to keep; the kernel clamps what it loads to them: other pixels, never another address
    eng = model.engine()
    rng = np.random.RandomState(41)
    segs = rng.randint(-2 ** 31, 2 ** 31, (300, 5), dtype=np.int64)
    segs[:8] = [[-2 ** 31] * 5, [2 ** 31 - 1] * 5, [-2 ** 31, 2 ** 31 - 1] * 2 + [2 ** 31 - 1], [0, 0, 2 ** 31 - 1, 2 ** 31 - 1, -1],
                [200, 200, 200, 200, 2 ** 31 - 1], [200, 200, 200, 200, -7], [-5, 100, 300, 100, 4], [100, 100, 100, 100, 0]]
    clamped = np.concatenate([np.clip(segs[:, :4], 0, 4 * 8192), np.clip(segs[:, 4:], 0, 512)], 1)
    recs = [(96, 120, 21, 33), (96, 120, 40, 2)]
    for rngs in ([(0, 300), (0, 8)], [(5, 3), (8, 292)]):
        want = _want(clamped, recs, (24, 40), rngs)
        got = _rasterise(eng, segs.astype(np.int32), recs, (24, 40), rngs, 1)
        assert np.array_equal(got, want)


def test_refusals_leave_the_output_untouched(model):
    eng = model.engine()
    st = ctypes.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream)
    p = ctypes.c_void_p
    segs = torch.tensor([[40, 40, 80, 80, 6]] * 4, dtype=torch.int32, device="cuda")
    out = torch.full((2 * 16 * 16 + 8,), OUT, dtype=torch.uint8, device="cuda")
    call = eng.lib.se_sketch_strokes_u8

    def wins(*recs):
        return (_lib.Window * len(recs))(*[_lib.Window(None, None, *r) for r in recs])

    def rng(*v):
        return (ctypes.c_int * len(v))(*v)
    ok_w, ok_r, S, O = wins((96, 120, 3, 5), (96, 120, 80, 104)), rng(0, 4, 1, 2), p(segs.data_ptr()), p(out.data_ptr())
    cases = [((None, 2, 16, 16, S, 4, ok_r, O), "wins"), ((ok_w, 2, 16, 16, None, 4, ok_r, O), "segs"),
             ((ok_w, 2, 16, 16, S, 4, None, O), "ranges"), ((ok_w, 2, 16, 16, S, 4, ok_r, None), "sketch_out"),
             ((ok_w, 2, 15, 16, S, 4, ok_r, O), "hs"), ((ok_w, 2, 16, 15, S, 4, ok_r, O), "ws"), ((ok_w, 0, 16, 16, S, 4, ok_r, O), "B"),
             ((wins((96, 120, 3, 5), (96, 120, 81, 104)), 2, 16, 16, S, 4, ok_r, O), "wins[1].y0"),
             ((wins((96, 120, 3, 105), (96, 120, 80, 104)), 2, 16, 16, S, 4, ok_r, O), "wins[0].x0"),
             ((wins((96, 120, -1, 5), (96, 120, 80, 104)), 2, 16, 16, S, 4, ok_r, O), "wins[0].y0"),
             ((wins((96, 120, 3, 5), (96, 120, 80, -4)), 2, 16, 16, S, 4, ok_r, O), "wins[1].x0"),
             ((wins((8193, 120, 3, 5), (96, 120, 80, 104)), 2, 16, 16, S, 4, ok_r, O), "Hi"),
             ((wins((96, 120, 3, 5), (96, 8193, 80, 104)), 2, 16, 16, S, 4, ok_r, O), "Wi"),
             ((wins((0, 120, 0, 0), (96, 120, 80, 104)), 2, 16, 16, S, 4, ok_r, O), "Hi"),
             ((ok_w, 2, 16, 16, S, 4, rng(0, 5, 1, 2), O), "ranges[0]"), ((ok_w, 2, 16, 16, S, 4, rng(0, 4, 3, 2), O), "ranges[1]"),
             ((ok_w, 2, 16, 16, S, 4, rng(-1, 2, 1, 2), O), "ranges[0]"), ((ok_w, 2, 16, 16, S, 4, rng(0, 4, 1, -1), O), "ranges[1]"),
             ((ok_w, 2, 16, 16, S, -1, ok_r, O), "N"), ((ok_w, 2, 16, 16, p(segs.data_ptr() + 2), 3, ok_r, O), "segs"),
             ((ok_w, 2, 16, 16, S, 4, ok_r, p(segs.data_ptr() + 8)), "overlaps")]
    for args, word in cases:
        assert call(eng.h, st, *args) != 0, word
        assert word in eng.lib.se_last_error(eng.h).decode(), (word, eng.lib.se_last_error(eng.h))
    torch.cuda.synchronize()
    assert (out == OUT).all() and segs.cpu().tolist() == [[40, 40, 80, 80, 6]] * 4
    with pytest.raises(_lib.SketchEditHipError):
        eng.sketch_strokes_u8(segs.float(), [(96, 120)], [(0, 0)], (16, 16))
    with pytest.raises(_lib.SketchEditHipError, match="ws"):
        eng.sketch_strokes_u8(segs, [(96, 120)], [(0, 0)], (16, 8))
    assert call(eng.h, st, ok_w, 2, 16, 16, S, 4, ok_r, O) == 0      # and the call they all resemble is accepted
    got = out.cpu().numpy()
    want = _want(segs.cpu().numpy(), [(96, 120, 3, 5), (96, 120, 80, 104)], (16, 16), [(0, 4), (1, 2)])
    assert np.array_equal(got[:512].reshape(2, 16, 16), want) and (got[512:] == OUT).all() and want[0].any() and not want[1].any()


# ---- edit_strokes against its definition ------------------------------------------------------------------------------------
HW = (256, 320)
KW = dict(min_side=64)
STROKES = [([(20.5, 20.5), (50.5, 50.5)], 3.0), ([(265.5, 195.5), (295.5, 225.5), (270.0, 230.0)], 4.0)]
WINS = [(0, 0, 128, 128), (128, 192, 128, 128)]


@pytest.fixture(scope="module")
def frame():
    return np.random.RandomState(37).randint(0, 256, HW + (3,), dtype=np.uint8)


@pytest.fixture(scope="module")
def full_sketch():
    """the rule's full-size sketch of STROKES: what the definition hands to `edit`"""
    sk = spec_raster(serve.stroke_segments(STROKES, HW)[0], HW)
    assert sk[35, 35] == 255 and sk[210, 280] == 255 and 0 < (sk > 0).sum() < 2000
    return sk


def _sequential(model, frame, sk, wins, lock=None, **kw):
    """the definition: one pinned single-window edit per window, in the order given -> the frame"""
    s = serve.EditSession(model, frame)
    if lock is not None:
        s.set_lock(lock)
    for w in wins:
        s.edit(sk, window=w, max_grow=0, low_latency=False, **kw)
    return s.frame()


def test_strokes_equal_the_single_window_edits(model, frame, full_sketch, monkeypatch):
    s = serve.EditSession(model, frame)
    sizes, real = [], model.edit_window_u8
    monkeypatch.setattr(model, "edit_window_u8", lambda frames, *a, **kw: (sizes.append(len(frames)), real(frames, *a, **kw))[1])
    patches, origins, info = s.edit_strokes(STROKES, low_latency=False, **KW)
    monkeypatch.undo()
    assert sizes == [2] and info["groups"] == 1 and info["windows"] == WINS and origins == [(0, 0), (192, 128)]
    got = s.frame()
    for (y0, x0, h, w), patch in zip(WINS, patches):
        assert np.array_equal(patch, got[y0:y0 + h, x0:x0 + w]) and not np.array_equal(patch, frame[y0:y0 + h, x0:x0 + w])
    outside = np.ones(HW, bool)
    for y0, x0, h, w in WINS:
        outside[y0:y0 + h, x0:x0 + w] = False
    assert np.array_equal(got[outside], frame[outside])
    assert np.array_equal(got, _sequential(model, frame, full_sketch, WINS))        # whole frame, byte for byte
    assert np.array_equal(got, _sequential(model, frame, full_sketch, WINS[::-1]))


def test_strokes_with_a_lock(model, frame, full_sketch):
    lock = np.zeros(HW, np.uint8)
    lock[10:200, 30:36] = 1                                   # crosses the first stroke and its window's lower edge
    s = serve.EditSession(model, frame)
    s.set_lock(lock)
    _, _, info = s.edit_strokes(STROKES, low_latency=False, **KW)
    assert info["locked"] is True and info["windows"] == WINS
    got = s.frame()
    assert np.array_equal(got[lock > 0], frame[lock > 0]) and not np.array_equal(got, frame)
    assert np.array_equal(got, _sequential(model, frame, full_sketch, WINS, lock=lock))
    assert not np.array_equal(got, _sequential(model, frame, full_sketch, WINS))    # the lock decided something


def test_strokes_at_a_working_size(model, frame, full_sketch):
    s = serve.EditSession(model, frame)
    _, _, info = s.edit_strokes(STROKES, low_latency=False, max_side=64, **KW)
    assert info["work"] == [(64, 64), (64, 64)] and info["windows"] == WINS
    got = s.frame()
    assert np.array_equal(got, _sequential(model, frame, full_sketch, WINS, max_side=64)) and not np.array_equal(got, frame)


def test_strokes_do_not_read_unwritten_scratch(model, frame, full_sketch, seopt):
    outs = []
    for v in (0, 0x55, 0xAA):
        seopt.set("SE_TEST_POISON", v)
        s = serve.EditSession(model, frame, history=1)
        _, _, info = s.edit_strokes(STROKES, low_latency=False, **KW)
        outs.append((s.frame(), info["counts"]))
    want = _sequential(model, frame, full_sketch, WINS)       # (poisoned too: the last value stays set until here)
    seopt.set("SE_TEST_POISON", 0)
    assert not np.array_equal(outs[0][0], frame)
    for f, counts in outs:
        assert np.array_equal(f, want) and counts == outs[0][1]


def test_one_undo_takes_the_whole_stroke_edit_back(model, frame):
    s = serve.EditSession(model, frame, history=2)
    _, _, info = s.edit_strokes(STROKES, low_latency=False, **KW)
    assert info["undoable"] is True and s.history_bytes_used == 2 * serve.window_saved_bytes(128, 128)
    f1 = s.frame()
    assert not np.array_equal(f1, frame)
    patches, origins, uinfo = s.undo()
    assert np.array_equal(s.frame(), frame) and not s.can_undo                      # ONE step, byte for byte
    assert uinfo == dict(windows=WINS, undo_depth=0, redo_depth=1)
    assert all(np.array_equal(p, frame[y0:y0 + p.shape[0], x0:x0 + p.shape[1]]) for p, (x0, y0) in zip(patches, origins))
    s.redo()
    assert np.array_equal(s.frame(), f1) and s.can_undo and not s.can_redo
