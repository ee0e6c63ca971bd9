"""GPU tests of the feathered paste's kernel: se_window_paste_feather_u8 on synthetic results, masks and frames -- no
forward runs here -- against the rule's numpy statement (tests/feather_util.py).  Every frame lies between sentinel bytes and the
WHOLE buffer is compared, so a byte written outside a selected pixel fails a case like a wrong blend does."""
import ctypes

import numpy as np
import pytest
import torch

import feather_util as FU
from sketchedit_amd import _lib

pytestmark = pytest.mark.gpu

SIZES = [(16, 16), (17, 23), (33, 65), (40, 72)]          # 17x23: every row misaligned; 33x65: one pixel past a 16 x 64 tile on both axes
RADII = [1, 2, 7, 16]                                      # 16 on 16x16: the box is larger than the window
PAD = 64                                                   # sentinel bytes in front of and behind a frame
SENTINEL = 0xAB


@pytest.fixture(scope="module")
def eng():
    return _lib.shared_engine()


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _masks(rng, hs, ws):
    """name -> (hs,ws) uint8"""
    one = np.zeros((hs, ws), np.uint8)
    one[hs // 2, ws - 2] = 255
    checker = ((np.add.outer(np.arange(hs), np.arange(ws)) & 1) * 255).astype(np.uint8)
    return {"zero": np.zeros((hs, ws), np.uint8), "full": np.full((hs, ws), 255, np.uint8), "one": one, "checker": checker,
            "sparse": ((rng.random((hs, ws)) < 0.1) * 255).astype(np.uint8), "dense": ((rng.random((hs, ws)) < 0.9) * 255).astype(np.uint8),
            "values": rng.choice(np.array([0, 1, 128, 255], np.uint8), (hs, ws))}


def _origins(Hi, Wi, hs, ws):
    """inside the frame at every byte alignment of 3 x0 (y0 odd), then flush with each edge of the frame and with two corners"""
    return [(1, 0), (3, 1), (1, 2), (3, 3), (0, 3), (Hi - hs, 1), (1, Wi - ws), (0, 0), (Hi - hs, Wi - ws)]


class _Frame:
    """a frame on the device between sentinels, and the lock plane that goes with it"""

    def __init__(self, rng, Hi, Wi, lock_density=0.0):
        self.np = rng.integers(0, 256, (Hi, Wi, 3), dtype=np.uint8)
        self.buf = torch.full((Hi * Wi * 3 + 2 * PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.t = self.buf[PAD:PAD + Hi * Wi * 3].view(Hi, Wi, 3)
        self.t.copy_(_cuda(self.np))
        self.lock = ((rng.random((Hi, Wi)) < lock_density) * rng.integers(1, 256, (Hi, Wi))).astype(np.uint8) if lock_density else None
        self.lock_t = None if self.lock is None else _cuda(self.lock)

    def expect(self, want):
        """the whole buffer: the sentinels, and `want` between them"""
        got = self.buf.cpu().numpy()
        assert (got[:PAD] == SENTINEL).all() and (got[-PAD:] == SENTINEL).all()
        return np.array_equal(got[PAD:-PAD].reshape(self.np.shape), want)


def _check(eng, rng, hs, ws, r, origin, mask, frame_hw, lock_density, what):
    f = _Frame(rng, *frame_hw, lock_density=lock_density)
    rgb = rng.integers(0, 256, (hs, ws, 3), dtype=np.uint8)
    want = FU.feather_paste(f.np, origin, rgb, mask, r, lock=f.lock)
    eng.window_paste_feather_u8([f.t], [origin], None if f.lock is None else [f.lock_t], (hs, ws), r, _cuda(rgb[None]), _cuda(mask[None]))
    assert f.expect(want), (what, np.argwhere(f.t.cpu().numpy() != want)[:5].tolist())
    return f, want


@pytest.mark.parametrize("hw", SIZES, ids=lambda hw: "%dx%d" % hw)
def test_kernel_against_numpy(eng, hw):
    hs, ws = hw
    rng = np.random.default_rng(hs * 100 + ws)
    Hi, Wi = hs + 8, ws + 7
    changed = 0
    for name, mask in _masks(rng, hs, ws).items():
        for k, origin in enumerate(_origins(Hi, Wi, hs, ws)):
            for r in RADII:
                f, want = _check(eng, rng, hs, ws, r, origin, mask, (Hi, Wi), 0.3 if (k + r) % 2 else 0.0, (hw, name, origin, r))
                if name == "zero":
                    assert np.array_equal(want, f.np)
                changed += int(not np.array_equal(want, f.np))
    assert changed > 6 * 9 * 4 * 0.9                              # the cases are not vacuous: all but a few change the frame


@pytest.mark.parametrize("hw", SIZES, ids=lambda hw: "%dx%d" % hw)
def test_window_that_is_the_whole_frame(eng, hw):
    """flush with all four edges: the replicated border makes c = n under a full mask, which gives rgb itself"""
    hs, ws = hw
    rng = np.random.default_rng(5)
    for r in RADII:
        rgb = rng.integers(0, 256, (hs, ws, 3), dtype=np.uint8)
        f = _Frame(rng, hs, ws)
        eng.window_paste_feather_u8([f.t], [(0, 0)], None, (hs, ws), r, _cuda(rgb[None]), torch.full((1, hs, ws), 255, dtype=torch.uint8, device="cuda"))
        assert f.expect(rgb)
        _check(eng, rng, hs, ws, r, (0, 0), _masks(rng, hs, ws)["dense"], (hs, ws), 0.2, (hw, r))


def test_misaligned_results_and_masks(eng):
    """rgb and mask_u8 that start 1, 2, 3 bytes past a 4-byte boundary, between sentinels the kernel must not need"""
    rng = np.random.default_rng(11)
    hs, ws, r = 33, 65, 7
    for off in (1, 2, 3):
        f = _Frame(rng, hs + 5, ws + 9, lock_density=0.2)
        rgb = rng.integers(0, 256, (hs, ws, 3), dtype=np.uint8)
        mask = _masks(rng, hs, ws)["dense"]
        rbuf = torch.full((hs * ws * 3 + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        mbuf = torch.full((hs * ws + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        rt, mt = rbuf[off:off + hs * ws * 3].view(1, hs, ws, 3), mbuf[off:off + hs * ws].view(1, hs, ws)
        rt.copy_(_cuda(rgb[None]))
        mt.copy_(_cuda(mask[None]))
        assert rt.data_ptr() % 4 == off and mt.data_ptr() % 4 == off
        eng.window_paste_feather_u8([f.t], [(3, 2)], [f.lock_t], (hs, ws), r, rt, mt)
        assert f.expect(FU.feather_paste(f.np, (3, 2), rgb, mask, r, lock=f.lock)), off


def test_requests_on_three_frames_of_different_sizes(eng):
    """one launch for three frames: two with a lock plane, one without, and a fourth request that shares the first frame"""
    rng = np.random.default_rng(13)
    hs, ws, r = 33, 65, 7
    fa, fb, fc = _Frame(rng, 80, 150, 0.3), _Frame(rng, 40, 70), _Frame(rng, 33, 90, 0.3)
    frames, origins = [fa, fb, fc, fa], [(1, 3), (7, 5), (0, 25), (40, 80)]
    rgb = rng.integers(0, 256, (4, hs, ws, 3), dtype=np.uint8)
    mask = np.stack([m for n, m in _masks(rng, hs, ws).items() if n in ("dense", "sparse", "values", "checker")])
    want = {id(f): f.np for f in frames}
    for i, (f, o) in enumerate(zip(frames, origins)):
        want[id(f)] = FU.feather_paste(want[id(f)], o, rgb[i], mask[i], r, lock=f.lock)
    eng.window_paste_feather_u8([f.t for f in frames], origins, [f.lock_t for f in frames], (hs, ws), r, _cuda(rgb), _cuda(mask))
    for f in (fa, fb, fc):
        assert f.expect(want[id(f)]) and not np.array_equal(want[id(f)], f.np)
    assert np.array_equal(want[id(fa)][fa.lock > 0], fa.np[fa.lock > 0])


@pytest.mark.parametrize("hw", [(16, 16), (40, 72)], ids=lambda hw: "%dx%d" % hw)
def test_radius_0_is_the_locked_paste(eng, hw):
    hs, ws = hw
    rng = np.random.default_rng(17)
    for origin in [(1, 0), (3, 1), (1, 2), (3, 3), (0, 0)]:
        for name, mask in _masks(rng, hs, ws).items():
            f = _Frame(rng, hs + 8, ws + 7, lock_density=0.3)
            g = _Frame(rng, hs + 8, ws + 7)
            g.t.copy_(f.t)
            rgb = _cuda(rng.integers(0, 256, (1, hs, ws, 3), dtype=np.uint8))
            eng.window_paste_feather_u8([f.t], [origin], [f.lock_t], (hs, ws), 0, rgb, _cuda(mask[None]))
            eng.window_paste_locked_u8([g.t], [origin], [f.lock_t], (hs, ws), rgb, _cuda(mask[None]))
            assert torch.equal(f.buf, g.buf), (hw, origin, name)
            assert f.expect(FU.feather_paste(f.np, origin, rgb[0].cpu().numpy(), mask, 0, lock=f.lock))


def test_radius_0_after_a_resize_is_the_scaled_paste(eng):
    """24 x 40 -> 17 x 23: the paste of a working-size result is DEFINED on the resized arrays"""
    rng = np.random.default_rng(19)
    H, W, hs, ws = 24, 40, 17, 23
    for origin in [(1, 0), (3, 1), (1, 2), (3, 3)]:
        f = _Frame(rng, hs + 8, ws + 7)
        g = _Frame(rng, hs + 8, ws + 7)
        g.t.copy_(f.t)
        rgb = _cuda(rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8))
        m8 = _cuda(((rng.random((1, H, W)) < 0.5) * 255).astype(np.uint8))
        eng.window_paste_resize_u8([g.t], [origin], (hs, ws), rgb, m8)
        small_rgb, small_m = eng.resize_u8(rgb, (hs, ws)), eng.resize_u8(m8, (hs, ws))
        eng.window_paste_feather_u8([f.t], [origin], None, (hs, ws), 0, small_rgb, small_m)
        assert torch.equal(f.buf, g.buf) and not np.array_equal(f.t.cpu().numpy(), f.np), origin


def test_poison_changes_nothing(eng, seopt):
    rng = np.random.default_rng(23)
    hs, ws = 33, 65
    mask = _masks(rng, hs, ws)["dense"]
    for v in (0x55, 0xAA):
        seopt.set("SE_TEST_POISON", v)
        _check(eng, rng, hs, ws, 7, (3, 1), mask, (hs + 8, ws + 7), 0.3, ("poison", v))
    seopt.set("SE_TEST_POISON", 0)


def test_refusals_leave_the_frames_untouched(eng):
    rng = np.random.default_rng(29)
    f, g = _Frame(rng, 60, 80, 0.3), _Frame(rng, 60, 80)
    alias = f.t.view(-1)[5:5 + 60 * 80].view(60, 80)               # a "plane" inside the frame's own bytes
    call = eng.lib.se_window_paste_feather_u8
    st = ctypes.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream)
    p = ctypes.c_void_p

    def raw(frames, origins, locks, hs, ws, r, rgb=True, m8=True):
        B = len(frames)
        wins = eng._windows(frames, origins)
        lk = None if locks is None else (ctypes.c_void_p * B)(*[None if t is None else t.data_ptr() for t in locks])
        rt = torch.zeros((B, max(hs, 1), max(ws, 1), 3), dtype=torch.uint8, device="cuda")
        mt = torch.full((B, max(hs, 1), max(ws, 1)), 255, dtype=torch.uint8, device="cuda")
        rc = call(eng.h, st, wins, lk, B, hs, ws, r, p(rt.data_ptr()) if rgb else None, p(mt.data_ptr()) if m8 else None)
        return rc, eng.lib.se_last_error(eng.h).decode()

    cases = [(([f.t], [(60 - 31, 0)], None, 32, 40, 3), "y0"), (([f.t], [(0, 80 - 39)], None, 32, 40, 3), "x0"),
             (([f.t], [(-1, 0)], None, 32, 40, 3), "y0"), (([f.t], [(0, -1)], None, 32, 40, 3), "x0"),
             (([f.t], [(0, 0)], None, 15, 40, 3), "hs"), (([f.t], [(0, 0)], None, 32, 15, 3), "ws"),
             (([f.t, f.t], [(0, 0), (27, 39)], None, 32, 40, 3), "overlapping"),
             (([f.t], [(1, 1)], [alias], 32, 40, 3), "locks[0]"), (([g.t, f.t], [(1, 1), (1, 1)], [alias, None], 32, 40, 3), "locks[0]"),
             (([f.t], [(1, 1)], [f.lock_t], 32, 40, -1), "radius"), (([f.t], [(1, 1)], [f.lock_t], 32, 40, 17), "radius"),
             (([f.t], [(1, 1)], None, 32, 40, 3, False, True), "rgb"), (([f.t], [(1, 1)], None, 32, 40, 3, True, False), "mask_u8")]
    for args, word in cases:
        rc, err = raw(*args)
        assert rc != 0 and word in err, (args[1:], word, err)
    with pytest.raises(_lib.SketchEditHipError, match="radius"):
        eng.window_paste_feather_u8([f.t], [(1, 1)], None, (32, 40), 17, torch.zeros((1, 32, 40, 3), dtype=torch.uint8, device="cuda"),
                                    torch.zeros((1, 32, 40), dtype=torch.uint8, device="cuda"))
    with pytest.raises(_lib.SketchEditHipError):                  # results at another size than the window's
        eng.window_paste_feather_u8([f.t], [(1, 1)], None, (32, 40), 3, torch.zeros((1, 24, 40, 3), dtype=torch.uint8, device="cuda"),
                                    torch.zeros((1, 24, 40), dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    assert f.expect(f.np) and g.expect(g.np)
    rc, err = raw([f.t, f.t], [(0, 0), (28, 40)], [f.lock_t, None], 28, 40, 3)       # and the call they all resemble is accepted
    assert rc == 0, err
    torch.cuda.synchronize()
    assert not f.expect(f.np)
