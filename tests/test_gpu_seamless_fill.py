"""GPU tests of the seamless paste of fills: SE_FLAG_RAW_FINE of the window fill against se_quantize_u8 of
se_fill's fine_out, and EditSession.fill(..., blend="seamless") with the wrappers built on it against the statement
(blend_util.spec_blend), computed on the host from the raw patch a twin session's backend hands out.  Every comparison is exact."""
import ctypes

import numpy as np
import pytest
import torch

from sketchedit_amd import _lib, serve
import blend_util as B
import move_util as M
from strokes_util import spec_raster
from test_gpu_fill import FH, FW, _blob, _cuda, _frame, _frame_of, _in_buffer, _plane, _session, model  # noqa: F401  (model: the fixture)

pytestmark = pytest.mark.gpu


# ---- 1. the flag ----------------------------------------------------------------------------------------------------------------------------
def _window_fill(eng, frames, origins, sketches, holes, locks, hw, flags, rgb, m8):
    """se_fill_window_u8 itself, unscaled, the default mode pinned, into the caller's rgb and m8"""
    H, W = hw
    B_ = len(frames)
    wins = eng._windows(frames, origins)
    for i, sk in enumerate(sketches):
        if sk is not None:
            wins[i].sketch_u8 = sk.data_ptr()
    hp = eng._planes(holes, frames, "fill", True)
    lp = None if locks is None else eng._planes(locks, frames, "lock", False)
    need = eng.lib.se_fill_window_u8_workspace_bytes(eng.h, B_, H, W, H, W)
    assert need
    wsp = eng._workspace_bytes(need)
    p = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    rc = eng.lib.se_fill_window_u8(eng.h, eng._stream(), wins, hp, lp, B_, H, W, H, W, p(rgb), p(m8), p(wsp), wsp.numel() // 16 * 16, flags)
    assert rc == 0, eng.lib.se_last_error(eng.h)


@pytest.mark.parametrize("poison", [0, 0xFF])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("nb", [1, 2])
@pytest.mark.parametrize("hw", [(64, 64), (40, 72)])
def test_raw_fine_is_the_quantised_fine_of_se_fill(model, seopt, hw, nb, precision, poison):
    """a 100 x 90 frame and a 131 x 97 one, a disc hole in each window; request 0 has a lock and a sketch, request 1 neither
    (B = 1 runs each alone); the default mode pinned.  rgb and m8 lie between sentinels."""
    eng = model.engine()
    opt_flags = _lib.flags_from_opt(model.opt)
    rng = np.random.RandomState(61)
    H, W = hw
    origins = [(5, 3), (7, 1)]
    fa, fb = _frame(rng, 100, 90), _frame(rng, 131, 97)
    fill_a = _blob(90, 100, origins[0][0] + H // 2, origins[0][1] + W // 2, H // 3)
    fill_b = _blob(97, 131, origins[1][0] + H // 3, origins[1][1] + W // 2, H // 4)
    lock_a = _plane(rng, 90, 100, 0.1)
    sk_a = ((rng.rand(H, W) < 0.05) * 255).astype(np.uint8)
    frames, holes = [_cuda(fa), _cuda(fb)], [_cuda(fill_a), _cuda(fill_b)]
    locks, sketches = [_cuda(lock_a), None], [_cuda(sk_a), None]
    groups = [[0, 1]] if nb == 2 else [[0], [1]]
    eng.set_precision(precision)
    try:
        for idx in groups:
            fr, og, sk, ho, lk = ([t[i] for i in idx] for t in (frames, origins, sketches, holes, locks))
            n = len(idx)
            # what se_fill computes for these windows: the gathers of the existing entries, then the definition on fp32 tensors
            zero = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
            image, sketch = eng.window_gather_u8(fr, og, [s if s is not None else zero for s in sk], H, W)
            fill8 = eng.window_gather_lock_u8(fr, og, ho, (H, W), H, W)
            lock8 = eng.window_gather_lock_u8(fr, og, lk, (H, W), H, W)
            r = eng.fill(image, fill8, opt_flags, sketch=sketch, lock=lock8, visualize=True, low_latency=False)
            want_raw, want_m8 = eng.quantize_u8(r["fine"], r["hard"])
            want_comp, _ = eng.quantize_u8(r["composed"], r["hard"])
            hole = (r["hard"][:, 0] > 0)
            assert 0.05 < float(hole.float().mean()) < 0.9
            if 0 in idx:
                assert int(((fill8[0] > 0) & (lock8[0] > 0)).sum()) > 20                  # the lock does cut the hole
            if poison:
                seopt.set("SE_TEST_POISON", poison)
            flags = (opt_flags & 31) | eng.exec_flags(n, H, W, False, False)
            out = {}
            for raw in (False, True):
                rbuf, rgb = _in_buffer(np.zeros((n, H, W, 3), np.uint8), 4100, 4097)
                mbuf, m8 = _in_buffer(np.zeros((n, H, W), np.uint8), 4100, 4097)
                rgb.fill_(0x5A), m8.fill_(0x5A)
                _window_fill(eng, fr, og, sk, ho, lk, (H, W), flags | (_lib.FLAG_RAW_FINE if raw else 0), rgb, m8)
                for buf, view in ((rbuf, rgb), (mbuf, m8)):
                    got = buf.cpu().numpy()
                    assert (got[:4100] == 0xA5).all() and (got[4100 + view.numel():] == 0xA5).all(), raw
                out[raw] = (rgb.clone(), m8.clone())
            if poison:
                seopt.unset("SE_TEST_POISON")
            (comp, m_comp), (raw_rgb, m_raw) = out[False], out[True]
            # the unflagged call is what it was: the composite's quantisation, and the hole's mask
            assert torch.equal(comp, want_comp) and torch.equal(m_comp, want_m8)
            # the flagged call: fine's quantisation at every pixel, the same mask
            assert torch.equal(raw_rgb, want_raw), (hw, idx, precision, poison)
            assert torch.equal(m_raw, m_comp)
            assert torch.equal(raw_rgb[hole], comp[hole])                                  # equal on every hole pixel
            differ = int((raw_rgb[~hole] != comp[~hole]).any(dim=-1).sum())
            print("raw fine %r B=%d %s: %d of %d pixels outside the hole differ from the composite" % (hw, n, precision, differ, int((~hole).sum())))
            assert differ >= 1                                                              # ... and the generator's own outside
            # the Python layers hand the flag down
            e_rgb, e_m8 = eng.fill_window_u8(fr, og, sk, ho, lk, (H, W), H, W, opt_flags, low_latency=False, raw=True)
            assert torch.equal(e_rgb, raw_rgb) and torch.equal(e_m8, m_raw)
            c_rgb, _ = eng.fill_window_u8(fr, og, sk, ho, lk, (H, W), H, W, opt_flags, low_latency=False)
            assert torch.equal(c_rgb, comp)
            # nothing is committed, no plane is written
            assert np.array_equal(frames[0].cpu().numpy(), fa) and np.array_equal(holes[0].cpu().numpy(), fill_a)
    finally:
        eng.set_precision("f32")


def test_every_other_entry_clears_the_bit(model):
    """se_inference_u8 with the bit set gives the bytes it gives without it"""
    from sketchedit_amd import synth
    eng = model.engine()
    img, sk = synth.make_inputs(1, 64, 64, seed=62)
    ci, cs = _cuda(img), _cuda(sk)
    ws = eng.workspace(1, 64, 64)
    flags = (_lib.flags_from_opt(model.opt) & 31) | eng.exec_flags(1, 64, 64, False, False)
    p = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    got = []
    for extra in (0, _lib.FLAG_RAW_FINE):
        rgb = torch.zeros((1, 64, 64, 3), dtype=torch.uint8, device="cuda")
        m8 = torch.zeros((1, 64, 64), dtype=torch.uint8, device="cuda")
        rc = eng.lib.se_inference_u8(eng.h, eng._stream(), p(ci), p(cs), p(rgb), p(m8), p(ws), ws.numel(), 1, 64, 64, flags | extra)
        assert rc == 0, eng.lib.se_last_error(eng.h)
        got.append((rgb, m8))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]) and int(got[0][0].max()) > 0


# ---- 2. the session ---------------------------------------------------------------------------------------------------------------------------
def _cut(box, win):
    y0, x0, h, w = win
    return (max(box[0], y0), max(box[1], x0), min(box[2], y0 + h), min(box[3], x0 + w))


def _raw_patch(model, f, plane255, lock, sk, win, work):
    """P of the definition from a TWIN session's backend: run_fill(raw=True) on the twin's resident frame, resized to the
    window by se_resize_u8 when `work` is set, downloaded"""
    t = serve.EditSession(model, f)
    if lock is not None:
        t.set_lock(lock)
    be = t.backend
    y0, x0, h, w = win
    crop = None if sk is None else be.upload(sk[y0:y0 + h, x0:x0 + w])
    rgb, _ = be.run_fill([t._frame], [(y0, x0)], [crop], [be.upload(plane255)], None if lock is None else [t._lock_plane], (h, w), work, False,
                         raw=True)
    if work is not None:
        rgb = model.engine().resize_u8(rgb, (h, w))
    assert tuple(rgb.shape) == (1, h, w, 3)
    return rgb[0].cpu().numpy()


def _statement(model, f, plane, lock, sk, win, work, box):
    """the DEFINITION, on the host: spec_blend with the lift P held by the window, offset 0, no flip, the box cut to the window"""
    plane255 = np.where(plane != 0, 255, 0).astype(np.uint8)
    P = _raw_patch(model, f, plane255, lock, sk, win, work)
    return B.spec_blend(f, M.slot_of(P, (0, 0) + tuple(win[2:])), win, plane255, lock, _cut(box, win), (0, 0), 0)


def _hard(model, f, lock, call):
    """the frame a third session holds after the same call without `blend`"""
    s, buf = _session(model, f, lock)
    call(s, None)
    return _frame_of(buf, f)


def _check(model, f, lock, call, plane, sk, win, work, box, rim=True):
    """`call(session, blend)` on a session between sentinels against the statement; undo and redo restore every byte"""
    s, buf = _session(model, f, lock, history=2)
    patch, (px, py), info = call(s, "seamless")
    want = _statement(model, f, plane, lock, sk, win, work, box)
    after = _frame_of(buf, f)
    assert np.array_equal(after, want)
    y0, x0, h, w = win
    assert info["window"] == win and info["blend"] == "seamless" and info["undoable"] is True and info.get("work") == work
    assert (px, py) == (x0, y0) and np.array_equal(patch, after[y0:y0 + h, x0:x0 + w])
    if rim:                                   # a condition on the inputs: the membrane is at work in this case
        assert not np.array_equal(want, f) and not np.array_equal(want, _hard(model, f, lock, call))
    assert len(s._undo) == 1
    s.undo()
    assert np.array_equal(_frame_of(buf, f), f)
    s.redo()
    assert np.array_equal(_frame_of(buf, f), after)
    return after


def _case(seed):
    rng = np.random.RandomState(seed)
    f = _frame(rng, FW, FH)
    lock = ((rng.rand(FH, FW) < 0.05) * 255).astype(np.uint8)
    lock[30:40, 20:60] = 255                                            # a bar through the disc below
    sk = np.zeros((FH, FW), np.uint8)
    sk[33:35, 15:60] = 255
    return f, lock, sk


WIN, WIN_SCALED, WORK = (3, 5, 64, 64), (3, 5, 72, 96), (48, 64)
CASES = {
    "plain": dict(mask=_blob(FH, FW, 35, 37, 14), win=WIN),
    "lock": dict(mask=_blob(FH, FW, 35, 37, 14), win=WIN, locked=True),
    "max_side": dict(mask=_blob(FH, FW, 38, 50, 20), win=WIN_SCALED, max_side=64, locked=True),
    "frame_edge": dict(mask=_blob(FH, FW, 0, 30, 12), win=(0, 0, 64, 64)),
    "window_cuts": dict(mask=_blob(FH, FW, 35, 66, 14), win=WIN),
    "sketch": dict(mask=_blob(FH, FW, 35, 37, 14), win=(3, 5, 64, 72), sketch=True),      # 3 w is no multiple of 16: the lift is repacked
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_session_fill_seamless_is_the_statement(model, name):
    c = CASES[name]
    f, lock, sk = _case(70 + sorted(CASES).index(name))
    lock = lock if c.get("locked") else None
    sk = sk if c.get("sketch") else None
    mask, win, max_side = c["mask"], c["win"], c.get("max_side")
    work = WORK if max_side else None
    if max_side:
        assert serve.choose_working_size(win[2:], max_side) == WORK
    box = M.box_of(mask)
    if name == "window_cuts":
        assert box[3] > win[1] + win[3] and _cut(box, win) != box
    if name == "frame_edge":
        assert box[0] == 0
    after = _check(model, f, lock, lambda s, blend: s.fill(mask, sketch=sk, window=win, max_side=max_side, low_latency=False, blend=blend),
                   mask, sk, win, work, box)
    y0, x0, h, w = win
    target = mask != 0
    target[:y0], target[y0 + h:], target[:, :x0], target[:, x0 + w:] = False, False, False, False
    if lock is not None:
        target &= lock == 0
    assert np.array_equal(after[~target], f[~target]) and (after[target] != f[target]).any()


def test_each_wrapper_is_the_statement(model):
    f, lock, _ = _case(80)
    f[20:40, 20:50] = (90, 140, 200)                                    # a flat region for the selection by colour
    lock[20:40, 20:50] = 0
    lock[28:31, 20:50] = 255
    hw = (FH, FW)
    # strokes: the plane is the rasteriser's, the box the segments' bound
    strokes = [([(20.0, 25.5), (50.25, 45.0)], 9.0)]
    segs, _ = serve.stroke_segments(strokes, hw)
    _check(model, f, lock, lambda s, blend: s.fill_strokes(strokes, window=WIN, low_latency=False, blend=blend),
           spec_raster(segs, hw), None, WIN, None, serve.stroke_box(segs, hw))
    # a Selection, made on the session itself; the twin's selection gives the plane and the box
    rings = [[(18.0, 16.0), (52.0, 18.0), (40.0, 50.0)]]
    twin = serve.EditSession(model, f)
    sel = twin.select_lasso(rings, grow=2)
    _check(model, f, lock, lambda s, blend: s.fill_selection(s.select_lasso(rings, grow=2), window=WIN, low_latency=False, blend=blend),
           sel.plane.cpu().numpy(), None, WIN, None, sel.box)
    _check(model, f, lock, lambda s, blend: s.fill_lasso(rings, grow=2, window=WIN, low_latency=False, blend=blend),
           sel.plane.cpu().numpy(), None, WIN, None, sel.box)
    sim = twin.select_similar((30, 35), tolerance=0, contiguous=True, grow=2)
    assert sim.box == (18, 18, 42, 52)
    _check(model, f, lock, lambda s, blend: s.fill_similar((30, 35), tolerance=0, contiguous=True, grow=2, window=WIN, low_latency=False,
                                                           blend=blend), sim.plane.cpu().numpy(), None, WIN, None, sim.box)


def test_the_outpaint_is_the_extension_and_the_seamless_fill(model):
    f, lock, _ = _case(81)
    win = (3, 72, 64, 64)                                               # columns 72 .. 135 of the extended frame: 16 of them new
    s = serve.EditSession(model, f, history=2)
    s.set_lock(lock)
    patch, (px, py), info = s.extend_canvas(right=16, pad="edge", fill="network", window=win, low_latency=False, blend="seamless")
    assert info["canvas"] == (FH, FW + 16) and info["window"] == win and info["blend"] == "seamless" and len(s._undo) == 1
    extended = np.pad(f, ((0, 0), (0, 16), (0, 0)), mode="edge")
    elock = np.pad(lock, ((0, 0), (0, 16)))
    area = np.zeros((FH, FW + 16), np.uint8)
    area[:, FW:] = 255
    want = _statement(model, extended, area, elock, None, win, None, (0, FW, FH, FW + 16))
    after = s.frame()
    assert np.array_equal(after, want) and np.array_equal(patch, after[3:67, 72:136]) and (px, py) == (72, 3)
    h = serve.EditSession(model, f)
    h.set_lock(lock)
    h.extend_canvas(right=16, pad="edge", fill="network", window=win, low_latency=False)
    assert not np.array_equal(want, extended) and not np.array_equal(want, h.frame())
    assert np.array_equal(after[:, :FW], f)                             # the old frame is the rim, never a target
    s.undo()
    assert s.frame_hw == (FH, FW) and np.array_equal(s.frame(), f)
    s.redo()
    assert np.array_equal(s.frame(), after)


def test_encoded_patches_are_the_windows_files(model):
    f, lock, _ = _case(82)
    mask = CASES["plain"]["mask"]
    plain = serve.EditSession(model, f)
    plain.fill(mask, window=WIN, low_latency=False, blend="seamless")
    want = plain.frame()
    for encode, ref in (("png", lambda s, w: s.frame_png(w)), (("jpg", 90), lambda s, w: s.frame_jpg(w, quality=90))):
        s = serve.EditSession(model, f, history=1)
        patch, _, info = s.fill(mask, window=WIN, encode=encode, low_latency=False, blend="seamless")
        assert isinstance(patch, bytes) and patch == ref(s, info["window"]) and info["blend"] == "seamless", encode
        assert np.array_equal(s.frame(), want)
        s.undo()
        assert np.array_equal(s.frame(), f)


# ---- 3. the membrane's relaxation on small levels -------------------------------------------------------------------------------------------------
def _rect_plane(hw, y0, x0, y1, x1):
    p = np.zeros(hw, np.uint8)
    p[y0:y1, x0:x1] = 200
    return p


def _disc_plane(hw):
    yy, xx = np.mgrid[0:hw[0], 0:hw[1]]
    return np.where(((yy - hw[0] / 2.0) / (hw[0] * 0.4)) ** 2 + ((xx - hw[1] / 2.0) / (hw[1] * 0.4)) ** 2 < 1, 7, 0).astype(np.uint8)


# (frame size, selection plane, the level sizes the case is about): the levels follow from E = the box grown by one pixel, clipped
RELAX_CASES = {
    "16x16-three-pixels": ((16, 16), _rect_plane((16, 16), 8, 6, 9, 9), [(2, 3), (1, 2), (1, 1)]),
    "16x16-line": ((16, 16), _rect_plane((16, 16), 8, 1, 9, 15), [(1, 2), (1, 1)]),
    "16x16-disc": ((16, 16), _disc_plane((16, 16)), [(1, 1)]),
    "16x16-full": ((16, 16), _rect_plane((16, 16), 0, 0, 16, 16), [(2, 2), (1, 1)]),
    "18x70-line-on-the-edge": ((18, 70), _rect_plane((18, 70), 0, 1, 1, 69), [(1, 35), (1, 2), (1, 1)]),
    "18x70-disc": ((18, 70), _disc_plane((18, 70)), [(1, 2)]),
    "18x70-full": ((18, 70), _rect_plane((18, 70), 0, 0, 18, 70), [(9, 35), (1, 2)]),
    "70x18-line-on-the-edge": ((70, 18), _rect_plane((70, 18), 1, 0, 69, 1), [(35, 1), (2, 1), (1, 1)]),
    "70x18-disc": ((70, 18), _disc_plane((70, 18)), [(2, 1)]),
    "70x18-full": ((70, 18), _rect_plane((70, 18), 0, 0, 70, 18), [(35, 9), (2, 1)]),
    "level-32x80": ((40, 90), _rect_plane((40, 90), 1, 1, 31, 79), [(32, 80)]),           # the last level of ONE workgroup
    "level-33x80": ((40, 90), _rect_plane((40, 90), 1, 1, 32, 79), [(33, 80), (17, 40)]),  # the first tiled one
}


@pytest.mark.parametrize("name", sorted(RELAX_CASES))
def test_blend_on_small_levels_follows_the_statement(model, name):
    from test_gpu_blend import _Work, _blend
    from test_gpu_lasso import _Buf
    from test_gpu_move import _Slot
    import select_util as U
    eng = model.engine()
    hw, sel, want_levels = RELAX_CASES[name]
    frame, before = U._noise(hw, 3), U._noise(hw, 4)
    rng = np.random.RandomState(91)
    lock = np.where(rng.rand(*hw) < 0.2, 255, 0).astype(np.uint8)
    box, rect = M.box_of(sel), (0, 0) + hw
    slot = M.slot_of(before, rect)
    d, e = B.rects(box, (0, 0), hw)
    sizes = B.level_sizes(e[2] - e[0], e[3] - e[1])
    assert all(s in sizes for s in want_levels), (sizes, want_levels)
    wk = _Work(B.workspace_bytes(box[2] - box[0], box[3] - box[1]))
    sb, lb, pb = _Buf(hw, 1, like=sel), _Buf(hw, 3, like=lock), _Slot(slot)
    rims = 0
    for off in ((0, 0), (1, -1)):
        for lk in (None, lock):
            fb = _Buf(frame.shape, 2, like=frame)
            _blend(eng, fb.view, pb.view, rect, sb.view, None if lk is None else lb.view, box, off, 0, wk)
            want = B.spec_blend(frame, slot, rect, sel, lk, box, off, 0)
            got = fb.get()
            assert np.array_equal(got, want), (name, off, lk is not None, int((got != want).sum()))
            rims += int(not np.array_equal(want, M.spec_drop(frame, slot, rect, sel, lk, box, off, 0, 0)))
    assert rims >= 1 and wk.margins_intact() and pb.intact() and np.array_equal(sb.get(), sel) and np.array_equal(lb.get(), lock)
