"""GPU tests of the device JPEG encoder: se_jpg_encode_u8 against the stream's statement (tests/jpg_stream_util.py),
byte for byte, every slot of `out` between sentinels that must survive; every refusal; runs under SE_TEST_POISON; and the session
calls with encode="jpg" against the same calls without it on a twin session.

Shapes (tests/jpg_cases.py): 16x16 flat (EOB only), 33x17 (partial blocks on both axes), 80x16 (ten rows: the restart index
wraps), 16x32 at quality 100 (size-11 DC differences, the 59-bit token), 16x100 noise at quality 100 (a row of three tiles of the
row kernel's walk), 24x16 (stuffing; an FF from the padding in front of a marker), odd origins in a frame of width 53, B = 3 over
two frames; qualities 1, 50, 90, 100 over the set."""
import ctypes
import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpg_cases
import jpg_stream_util as U
from sketchedit_amd import _lib, serve, synth

pytestmark = pytest.mark.gpu

ARGV = ("--batchSize 1 --name celeb --joint_train_inp --dataset_mode testimage --image_dirs x --mask_dirs x "
        "--image_lists x --model editline2 --netG deepfillc2 --pool_type max --use_cam --output_dir {d} --gpu_ids 0")
GUARD, SENTINEL = 37, 0xA5                        # (an odd guard: the slots start at every alignment over the cases)
CASES = jpg_cases.cases()
ODD = next(c for c in CASES if c[0].startswith("x0, y0 odd"))
MANY = next(c for c in CASES if c[0].startswith("B = 3"))


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
def wanted():
    """the statement's segment of every request of every case, computed once"""
    return {name: [U.jpg_scan(jpg_cases.rectangle(frames, r, hw), q) for r in reqs] for name, frames, reqs, hw, q in CASES}


def _encode(eng, frames, reqs, hw, quality, extra=3):
    """-> the B segments on the host, after checking the sentinels around and between them.  cap = the bound + `extra`."""
    dev = [torch.from_numpy(f).cuda() for f in frames]
    B, cap = len(reqs), U.jpg_bound(*hw) + extra
    buf = torch.full((GUARD + B * cap + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = buf[GUARD:GUARD + B * cap].view(B, cap)
    got, sizes = eng.jpg_encode_u8([dev[f] for f, _, _ in reqs], [(y0, x0) for _, y0, x0 in reqs], hw, quality=quality, out=out)
    assert got is out
    sizes = sizes.cpu().tolist()
    host = buf.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + B * cap:] == SENTINEL).all(), "a byte outside out was written"
    slots = host[GUARD:GUARD + B * cap].reshape(B, cap)
    for b, n in enumerate(sizes):
        assert 0 < n <= U.jpg_bound(*hw) and (slots[b, n:] == SENTINEL).all(), "a byte behind segment %d was written" % b
    for f, d in zip(frames, dev):
        assert np.array_equal(d.cpu().numpy(), f)                         # frames are only read
    return [slots[b, :n].tobytes() for b, n in enumerate(sizes)]


@pytest.mark.parametrize("case", CASES, ids=[c[0].split(":")[0] for c in CASES])
def test_kernel_equals_the_statement(model, wanted, case):
    name, frames, reqs, hw, quality = case
    got = _encode(model.engine(), frames, reqs, hw, quality)
    for b, (g, w) in enumerate(zip(got, wanted[name])):
        assert len(g) == len(w) and g == w, (name, b, len(g), len(w), next((i for i, (x, y) in enumerate(zip(g, w)) if x != y), None))
    im = Image.open(io.BytesIO(serve.jpg_from_scan(got[-1], hw[0], hw[1], quality)))
    im.load()
    assert im.mode == "RGB" and im.size == (hw[1], hw[0])


def test_every_alignment_of_out(model, wanted):
    name, frames, reqs, hw, quality = MANY
    for extra in (0, 1, 2):                                               # cap, and with it the later slots' alignment
        assert _encode(model.engine(), frames, reqs, hw, quality, extra=extra) == wanted[name]


def test_under_poison(model, wanted, seopt):
    name, frames, reqs, hw, quality = ODD                                 # odd origins: the open words and the copy's ends
    for v in (0x55, 0xAA, 0xFF):
        seopt.set("SE_TEST_POISON", v)
        assert _encode(model.engine(), frames, reqs, hw, quality) == wanted[name]
    seopt.set("SE_TEST_POISON", 0)


def test_refusals_leave_the_output_untouched(model):
    eng = model.engine()
    st = ctypes.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream)
    p = ctypes.c_void_p
    fa = torch.zeros((40, 44, 3), dtype=torch.uint8, device="cuda")
    fb = torch.zeros((64, 70, 3), dtype=torch.uint8, device="cuda")
    hs, ws, Q = 20, 24, 90
    cap = U.jpg_bound(hs, ws)
    out = torch.full((2 * cap + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    sizes = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    need = eng.lib.se_jpg_encode_u8_workspace_bytes(eng.h, 2, hs, ws)
    assert need > 0 and need % 256 == 0
    wsp = torch.zeros((need,), dtype=torch.uint8, device="cuda")
    call = eng.lib.se_jpg_encode_u8

    def wins(*recs):
        return (_lib.Window * len(recs))(*[_lib.Window(f.data_ptr() if f is not None else None, None, f.shape[0] if f is not None else 40,
                                                       f.shape[1] if f is not None else 44, y0, x0) for f, y0, x0 in recs])
    ok = wins((fa, 1, 3), (fb, 30, 40))
    O, Z, W = p(out.data_ptr()), p(sizes.data_ptr()), p(wsp.data_ptr())
    cases = [((None, 2, hs, ws, Q, O, cap, Z, W, need), "wins"), ((ok, 2, hs, ws, Q, None, cap, Z, W, need), "out"),
             ((ok, 2, hs, ws, Q, O, cap, None, W, need), "sizes_out"), ((ok, 2, hs, ws, Q, O, cap, Z, None, need), "workspace"),
             ((wins((None, 1, 3), (fb, 30, 40)), 2, hs, ws, Q, O, cap, Z, W, need), "wins[0].frame_u8"),
             ((ok, 0, hs, ws, Q, O, cap, Z, W, need), "B"), ((ok, -1, hs, ws, Q, O, cap, Z, W, need), "B"),
             ((ok, 65536, hs, ws, Q, O, cap, Z, W, need), "B"),
             ((ok, 2, 15, ws, Q, O, cap, Z, W, need), "hs"), ((ok, 2, hs, 15, Q, O, cap, Z, W, need), "ws"),
             ((ok, 2, 8193, ws, Q, O, cap, Z, W, need), "hs"), ((ok, 2, hs, 8193, Q, O, cap, Z, W, need), "ws"),
             ((ok, 2, hs, ws, 0, O, cap, Z, W, need), "quality"), ((ok, 2, hs, ws, 101, O, cap, Z, W, need), "quality"),
             ((ok, 2, hs, ws, -90, O, cap, Z, W, need), "quality"),
             ((wins((fa, 21, 3), (fb, 30, 40)), 2, hs, ws, Q, O, cap, Z, W, need), "wins[0].y0"),
             ((wins((fa, 1, 3), (fb, 30, 47)), 2, hs, ws, Q, O, cap, Z, W, need), "wins[1].x0"),
             ((wins((fa, -1, 3), (fb, 30, 40)), 2, hs, ws, Q, O, cap, Z, W, need), "wins[0].y0"),
             ((ok, 2, hs, ws, Q, O, cap - 1, Z, W, need), "cap"), ((ok, 2, hs, ws, Q, O, cap, Z, W, need - 1), "workspace too small"),
             ((ok, 2, hs, ws, Q, O, cap, Z, p(wsp.data_ptr() + 16), need), "aligned"),
             ((ok, 2, hs, ws, Q, O, cap, p(sizes.data_ptr() + 4), W, need), "sizes_out"),
             ((ok, 2, hs, ws, Q, p(fb.data_ptr() + 100), cap, Z, W, need), "out overlaps the frame of wins[1]"),
             ((ok, 2, hs, ws, Q, p(fa.data_ptr() - cap), cap, Z, W, need), "out overlaps the frame of wins[0]"),
             ((ok, 2, hs, ws, Q, p(wsp.data_ptr() + 256), cap, Z, W, need), "out overlaps the workspace"),
             ((ok, 2, hs, ws, Q, p(sizes.data_ptr() - 8), cap, Z, W, need), "out overlaps sizes_out")]
    for args, word in cases:
        assert call(eng.h, st, *args) != 0, word
        assert word in eng.lib.se_last_error(eng.h).decode(), (word, eng.lib.se_last_error(eng.h))
    assert eng.lib.se_jpg_encode_u8_workspace_bytes(eng.h, 2, 15, ws) == 0 and "hs" in eng.lib.se_last_error(eng.h).decode()
    assert eng.lib.se_jpg_encode_u8_workspace_bytes(eng.h, 0, hs, ws) == 0 and "B" in eng.lib.se_last_error(eng.h).decode()
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (sizes == -1).all() and not fa.any() and not fb.any()
    with pytest.raises(_lib.SketchEditHipError, match="cap"):
        eng.jpg_encode_u8([fa], [(0, 0)], (hs, ws), out=torch.empty((1, cap - 1), dtype=torch.uint8, device="cuda"))
    with pytest.raises(_lib.SketchEditHipError, match="quality"):
        eng.jpg_encode_u8([fa], [(0, 0)], (hs, ws), quality=0)
    with pytest.raises(_lib.SketchEditHipError):
        eng.jpg_encode_u8([fa.float()], [(0, 0)], (hs, ws))
    assert call(eng.h, st, ok, 2, hs, ws, Q, O, cap, Z, W, need) == 0     # and the call they all resemble is accepted
    n = sizes.cpu().tolist()
    host = out.cpu().numpy()
    want = U.jpg_scan(np.zeros((hs, ws, 3), np.uint8), Q)
    assert n == [len(want)] * 2 and host[:n[0]].tobytes() == want and host[cap:cap + n[1]].tobytes() == want
    assert (host[n[0]:cap] == SENTINEL).all() and (host[cap + n[1]:] == SENTINEL).all()


# ---- sessions: encode="jpg" against the same call without it, on a twin session ---------------------------------------------------
HW = (256, 320)
KW = dict(min_side=64)
STROKES = [([(20.5, 20.5), (50.5, 50.5)], 3.0), ([(265.5, 195.5), (295.5, 225.5), (270.0, 230.0)], 4.0)]


@pytest.fixture(scope="module")
def frame():
    y, x = np.mgrid[:HW[0], :HW[1]]
    smooth = np.stack([y + x // 2, 255 - y // 2 - x // 3, (x * 3 + y) // 4], axis=2)
    return ((smooth + np.random.RandomState(37).randint(0, 12, HW + (3,))) & 255).astype(np.uint8)


def _file(raw, quality):
    return serve.jpg_from_scan(U.jpg_scan(raw, quality), raw.shape[0], raw.shape[1], quality)


def _twins(model, frame, lock=None):
    out = []
    for _ in range(2):
        s = serve.EditSession(model, frame)
        if lock is not None:
            s.set_lock(lock)
        out.append(s)
    return out


def test_edit_as_jpg(model, frame):
    sk = np.zeros(HW, np.uint8)
    sk[100:130, 140:150] = 255
    a, b = _twins(model, frame)
    raw, at0, info0 = a.edit(sk, low_latency=False)
    jpg, at1, info1 = b.edit(sk, low_latency=False, encode="jpg")
    assert at0 == at1 and info0 == info1 and isinstance(jpg, bytes) and jpg == _file(raw, 90)
    assert not np.array_equal(raw, frame[at0[1]:at0[1] + raw.shape[0], at0[0]:at0[0] + raw.shape[1]])
    fa, fb = a.frame(), b.frame()
    assert np.array_equal(fa, fb)
    assert b.frame_jpg() == _file(fb, 90)                                 # 256 x 320: 32 rows of 120 blocks
    assert b.frame_jpg((3, 5, 17, 33), quality=35) == _file(np.ascontiguousarray(fb[3:20, 5:38]), 35)
    assert np.array_equal(b.frame(), fb)


def test_edit_strokes_as_jpg_with_a_lock_and_a_working_size(model, frame):
    lock = np.zeros(HW, np.uint8)
    lock[10:200, 30:36] = 1
    a, b = _twins(model, frame, lock)
    raws, at0, info0 = a.edit_strokes(STROKES, low_latency=False, max_side=64, **KW)
    jpgs, at1, info1 = b.edit_strokes(STROKES, low_latency=False, max_side=64, encode=("jpg", 50), **KW)
    assert at0 == at1 and info0 == info1 and info0["locked"] is True and info0["work"] == [(64, 64), (64, 64)] and len(jpgs) == 2
    for raw, jpg in zip(raws, jpgs):
        assert jpg == _file(raw, 50)
    fa = a.frame()
    assert np.array_equal(fa, b.frame()) and not np.array_equal(fa, frame) and np.array_equal(fa[lock > 0], frame[lock > 0])
