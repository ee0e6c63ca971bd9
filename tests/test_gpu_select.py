"""GPU tests of the selection by colour: the three kernels of se_select.hip against the numpy statement of
tests/select_util.py on whole planes between sentinels, at every alignment, and EditSession.select_similar / fill_similar against
`fill` of the statement's mask on a twin session.  Every comparison is exact."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from sketchedit_amd import _lib, serve, synth
import select_util as U

pytestmark = pytest.mark.gpu

ARGV = ("--batchSize 1 --name celeb --joint_train_inp --dataset_mode testimage --image_dirs x --mask_dirs x "
        "--image_lists x --model editline2 --netG deepfillc2 --pool_type max --use_cam --output_dir {d} --gpu_ids 0")
SIZES = [(16, 16), (37, 53), (64, 64), (65, 129), (100, 90), (130, 70)]       # (Hi, Wi): below one tile, exactly one, ragged, three across / down
PATTERNS = {f.__name__: f for f in (U.serpentine, U.diagonal, U.two_components, U.border_region, U.blob_with_ramp)}
SENTINEL, GARBAGE = 0xA5, 0x5C
LEAD, TAIL = 4096, 4099


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
def eng(model):
    return model.engine()


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()                       # (a copy: the shared cases are read-only)


@functools.lru_cache(maxsize=None)
def _case(name, hw, t=16, contiguous=True):
    """(frame, seed, the state after similar, the state at the fixed point): computed once, shared, never written"""
    frame, seed = PATTERNS[name](hw)
    out = frame, seed, U.spec_state(frame, seed, t, contiguous, flooded=False), U.spec_state(frame, seed, t, contiguous)
    for a in (out[0], out[2], out[3]):
        a.setflags(write=False)
    return out


class _Buf:
    """an array's bytes on the device, `off` bytes past a 4-byte aligned address, between sentinel margins"""

    def __init__(self, shape, off, fill=None, like=None):
        n = int(np.prod(shape))
        self.lead, self.n = LEAD + off, n
        self.buf = torch.full((self.lead + n + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 4 == 0
        self.view = self.buf[self.lead:self.lead + n].view(shape)
        if like is not None:
            self.view.copy_(_cuda(like))
        else:
            self.view.fill_(fill)

    def get(self):
        """the array back on the host; the margins must be what they were"""
        got = self.buf.cpu().numpy()
        assert (got[:self.lead] == SENTINEL).all() and (got[self.lead + self.n:] == SENTINEL).all()
        return got[self.lead:self.lead + self.n].reshape(tuple(self.view.shape))


class _Words:
    """`n` int32 words on the device between two sentinel words, pre-filled with garbage"""

    def __init__(self, n):
        self.t = torch.full((n + 2,), -1515870811, dtype=torch.int32, device="cuda")           # 0xA5A5A5A5
        self.t[1:1 + n] = 0x5C5C5C5C
        self.view = self.t[1:1 + n]

    def get(self):
        got = self.t.cpu().numpy()
        assert got[0] == -1515870811 and got[-1] == -1515870811
        return got[1:-1].tolist()


def _flood(eng, state, passes, limit=4096):
    """se_select_flood_u8 until a call reports an idle pass -> every call's words, in order"""
    words = []
    while True:
        w = _Words(passes)
        eng.select_flood_u8(state, passes=passes, changed=w.view)
        got = w.get()
        assert set(got) <= {0, 1}, got                                                         # all written, 0 / 1
        words.append(got)
        if 0 in got:
            return words
        assert len(words) * passes <= limit


def _idle_from_the_first_idle_pass_on(words):
    flat = [v for w in words for v in w]
    return flat == sorted(flat, reverse=True)


def _select(eng, frame, seed, t, contiguous, grow, off, passes=8):
    """the three entries on planes between sentinels -> (state after similar, state at the fixed point, output plane, words)"""
    hw = frame.shape[:2]
    fb = _Buf(frame.shape, (off + 1) % 4, like=frame)
    sb = _Buf(hw, off, fill=GARBAGE)
    ob = _Buf(hw, (off + 3) % 4, fill=GARBAGE)
    eng.select_similar_u8(fb.view, seed, t, contiguous, state=sb.view)
    first = sb.get()
    words = _flood(eng, sb.view, passes) if contiguous else []
    eng.select_grow_u8(sb.view, grow, out=ob.view)
    assert np.array_equal(fb.get(), frame)
    return first, sb.get(), ob.get(), words


# ---- 1. the patterns at every size and alignment --------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", SIZES, ids=lambda hw: "%dx%d" % hw)
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_patterns_follow_the_statement(eng, name, hw):
    frame, seed, want_first, want = _case(name, hw)
    off = (sorted(PATTERNS).index(name) + SIZES.index(hw)) % 4
    first, state, plane, words = _select(eng, frame, seed, 16, True, 2, off)
    assert np.array_equal(first, want_first)
    assert np.array_equal(state, want)
    assert np.array_equal(plane, U.spec_grow(want == 255, 2))
    assert _idle_from_the_first_idle_pass_on(words)
    print("%s %dx%d: %d reached of %d similar, %d productive passes" % (name, hw[0], hw[1], (want == 255).sum(), (want > 0).sum(),
                                                                        sum(sum(w) for w in words)))
    if name == "serpentine":
        assert not (state == 1).any()                                 # all of them
    if name in ("diagonal", "two_components"):
        assert (state == 1).sum() == (state == 255).sum() > 0         # the other blob stays similar and unreached


def test_every_alignment_of_state_and_output(eng):
    frame, seed, want_first, want = _case("border_region", (37, 53))
    for off in range(4):
        first, state, plane, _ = _select(eng, frame, seed, 16, True, 3, off)
        assert np.array_equal(first, want_first) and np.array_equal(state, want), off
        assert np.array_equal(plane, U.spec_grow(want == 255, 3)), off


def test_serpentine_takes_more_than_one_call(eng):
    frame, seed, _, want = _case("serpentine", (100, 90))
    assert int((want == 255).sum()) == 4361 and not (want == 1).any()
    _, state, plane, words = _select(eng, frame, seed, 16, True, 0, 1)
    assert np.array_equal(state, want) and np.array_equal(plane, np.where(want == 255, 255, 0))
    print("serpentine 100x90: %d calls of 8 passes, %d productive passes" % (len(words), sum(sum(w) for w in words)))
    assert len(words) > 1


def test_corner_seeds(eng):
    frame, _ = U.border_region((65, 129))
    for k, seed in enumerate(((0, 0), (0, 128), (64, 0), (64, 128))):
        want = U.spec_state(frame, seed, 16, True)
        first, state, plane, _ = _select(eng, frame, seed, 16, True, 1, k)
        assert first[seed] == 255 and int((first == 255).sum()) == 1
        assert np.array_equal(state, want) and np.array_equal(plane, U.spec_grow(want == 255, 1)), seed
    # a seed that is alone: nothing else is similar at tolerance 0 in noise
    noise = U._noise((37, 53), 3)
    noise[0, 0] = (1, 2, 3)
    _, state, plane, words = _select(eng, noise, (0, 0), 0, True, 0, 2)
    assert np.array_equal(state, U.spec_state(noise, (0, 0), 0, True)) and int((plane == 255).sum()) == 1 and words == [[0] * 8]


# ---- 2. tolerance ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [0, 1, 16, 100, 254, 255])
def test_tolerance_is_chebyshev_and_inclusive(eng, t):
    hw = (37, 53)
    rng = np.random.RandomState(t)
    base = 127 if t < 128 else 0                                       # so that base + t and base + t + 1 exist wherever they can
    frame = np.full(hw + (3,), base, np.uint8)
    seed = (18, 26)
    marks = {}
    col = 2
    for c in range(3):
        for sign in (1, -1):
            for d in (t, t + 1):
                v = base + sign * d
                if 0 <= v <= 255 and not (d == 0 and sign < 0):
                    frame[18, col, c] = v                              # one channel only; the rows next to it connect past it
                    marks[(18, col)] = d <= t
                    col += 2
    frame[30:, :] = rng.randint(0, 256, (7, 53, 3))                     # and noise at every distance
    want = U.spec_state(frame, seed, t, True)
    first, state, plane, _ = _select(eng, frame, seed, t, True, 0, t % 4)
    assert np.array_equal(first, U.spec_state(frame, seed, t, True, flooded=False)) and np.array_equal(state, want)
    for at, similar in marks.items():
        assert (state[at] == 255) == similar, (at, frame[at], similar)
    assert len(marks) == {0: 9, 1: 12, 16: 12, 100: 12, 254: 6, 255: 3}[t]
    if t == 255:
        assert (state == 255).all() and (plane == 255).all()           # the whole frame
    if t == 0:
        assert set(np.unique(frame[state == 255])) == {127} and (state[30:] == 0).sum() > 300


def test_not_contiguous_is_similar_itself(eng):
    for name, hw, off in (("two_components", (65, 129), 0), ("diagonal", (37, 53), 3), ("blob_with_ramp", (130, 70), 2)):
        frame, seed, _, _ = _case(name, hw)
        want = U.spec_state(frame, seed, 16, False)
        first, state, plane, words = _select(eng, frame, seed, 16, False, 2, off)
        assert words == [] and np.array_equal(first, want) and np.array_equal(state, want) and not (want == 1).any()
        assert np.array_equal(plane, U.spec_select(frame, seed, 16, False, 2))
        # a flood of it finds a fixed point at once
        st = _cuda(want)
        assert _flood(eng, st, 3) == [[0, 0, 0]] and np.array_equal(st.cpu().numpy(), want)


# ---- 3. the passes ---------------------------------------------------------------------------------------------------------------------
def test_any_number_of_passes_per_call_gives_the_same_state(eng):
    frame, seed, first, want = _case("serpentine", (65, 129))
    productive = {}
    for passes in (1, 3, 8, 64):
        sb = _Buf(first.shape, passes % 4, like=first)
        words = _flood(eng, sb.view, passes)
        assert np.array_equal(sb.get(), want), passes
        assert _idle_from_the_first_idle_pass_on(words), (passes, words)   # 0 from the first idle pass on, inside the call too
        assert all(len(w) == passes for w in words)
        productive[passes] = sum(sum(w) for w in words)
        # at the fixed point a call stores nothing
        w = _Words(passes)
        eng.select_flood_u8(sb.view, passes=passes, changed=w.view)
        assert w.get() == [0] * passes and np.array_equal(sb.get(), want)
    print("serpentine 65x129: productive passes by passes per call: %r" % productive)
    assert productive[1] > 8                                              # the corridor crosses the tile borders row by row


# ---- 4. the grow -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [0, 1, 3, 16])
def test_grow_follows_the_statement(eng, r):
    planes = [_case("serpentine", (100, 90))[3].copy()]
    for hw in ((16, 16), (37, 53), (65, 129)):
        H, W = hw
        single = np.ones(hw, np.uint8)                                   # 1 = similar, not reached: must not grow
        states = []
        for at in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1), (H // 2, W // 2)):
            s = single.copy()
            s[at] = 255
            states.append(s)
        planes += states
        planes.append(np.full(hw, 255, np.uint8))
        planes.append(np.where(np.random.RandomState(r).rand(*hw) < 0.01, 255, np.random.RandomState(r + 1).randint(0, 255, hw)).astype(np.uint8))
    for k, st in enumerate(planes):
        sb = _Buf(st.shape, k % 4, like=st)
        ob = _Buf(st.shape, (k // 4) % 4, fill=GARBAGE)
        eng.select_grow_u8(sb.view, r, out=ob.view)
        got = ob.get()
        assert np.array_equal(got, U.spec_grow(st == 255, r)), (k, st.shape)
        assert np.array_equal(sb.get(), st)


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(eng):
    frame, seed, first, want = _case("two_components", (37, 53))
    Hi, Wi = 37, 53
    fb, sb, ob = _Buf(frame.shape, 1, like=frame), _Buf((Hi, Wi), 2, like=first), _Buf((Hi, Wi), 3, fill=GARBAGE)
    words = _Words(8)
    lib, h, st = eng.lib, eng.h, eng._stream()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else t)     # noqa: E731
    F, S, O, C = fb.view, sb.view, ob.view, words.view
    alias = fb.buf[fb.lead + 7:fb.lead + 7 + Hi * Wi]                   # a "plane" inside the frame's own bytes
    shifted = sb.buf[sb.lead + Hi * Wi - 1:]                            # shares the state's last byte
    similar = [((None, Hi, Wi, 4, 4, 16, 1, S), "frame_u8"), ((F, Hi, Wi, 4, 4, 16, 1, None), "state_u8"),
               ((F, 15, Wi, 4, 4, 16, 1, S), "Hi"), ((F, Hi, 15, 4, 4, 16, 1, S), "Wi"),
               ((F, Hi, Wi, Hi, 4, 16, 1, S), "seed"), ((F, Hi, Wi, 4, Wi, 16, 1, S), "seed"), ((F, Hi, Wi, -1, 4, 16, 1, S), "seed"),
               ((F, Hi, Wi, 4, -1, 16, 1, S), "seed"), ((F, Hi, Wi, 4, 4, -1, 1, S), "tolerance"), ((F, Hi, Wi, 4, 4, 256, 1, S), "tolerance"),
               ((F, Hi, Wi, 4, 4, 16, 1, alias), "overlaps"), ((F, Hi, Wi, 4, 4, 16, 1, fb.buf[fb.lead + 3 * Hi * Wi - 1:]), "overlaps")]
    for (f, a, b, sy, sx, t, cont, s), what in similar:
        assert lib.se_select_similar_u8(h, st, p(f), a, b, sy, sx, t, cont, p(s)) != 0, what
        assert what in lib.se_last_error(h).decode(), (what, lib.se_last_error(h).decode())
    flood = [((None, Hi, Wi, 8, C), "state_u8"), ((S, Hi, Wi, 8, None), "changed_out"), ((S, 15, Wi, 8, C), "Hi"), ((S, Hi, 8, 8, C), "Wi"),
             ((S, Hi, Wi, 0, C), "passes"), ((S, Hi, Wi, 65, C), "passes"), ((S, Hi, Wi, -3, C), "passes"),
             ((S, Hi, Wi, 2, C.data_ptr() + 2), "aligned"), ((S, Hi, Wi, 2, (sb.view.data_ptr() + 7) // 4 * 4), "overlaps")]
    for (s, a, b, n, c), what in flood:
        assert lib.se_select_flood_u8(h, st, p(s), a, b, n, p(c)) != 0, what
        assert what in lib.se_last_error(h).decode(), (what, lib.se_last_error(h).decode())
    grow = [((None, Hi, Wi, 2, O), "state_u8"), ((S, Hi, Wi, 2, None), "plane_out"), ((S, 15, Wi, 2, O), "Hi"), ((S, Hi, 15, 2, O), "Wi"),
            ((S, Hi, Wi, -1, O), "grow"), ((S, Hi, Wi, 17, O), "grow"), ((S, Hi, Wi, 2, S), "overlaps"), ((S, Hi, Wi, 2, shifted), "overlaps")]
    for (s, a, b, r, o), what in grow:
        assert lib.se_select_grow_u8(h, st, p(s), a, b, r, p(o)) != 0, what
        assert what in lib.se_last_error(h).decode(), (what, lib.se_last_error(h).decode())
    # the bindings refuse planes of another shape
    with pytest.raises(_lib.SketchEditHipError):
        eng.select_similar_u8(F, (4, 4), 16, True, state=ob.buf[:Hi * Wi].view(Wi, Hi))
    with pytest.raises(_lib.SketchEditHipError):
        eng.select_grow_u8(S, 2, out=ob.buf[:Hi * Wi].view(Wi, Hi))
    with pytest.raises(_lib.SketchEditHipError):
        eng.select_similar_u8(F, (Hi, 0), 16, True)
    torch.cuda.synchronize()
    assert np.array_equal(fb.get(), frame) and np.array_equal(sb.get(), first) and (ob.get() == GARBAGE).all()
    assert words.get() == [0x5C5C5C5C] * 8


# ---- 6. sessions ------------------------------------------------------------------------------------------------------------------------
FHW = (120, 104)


def _blob_frame():
    """a flat blob with a +-3 ramp inside it, on noise; a second blob apart; the seed in the first"""
    H, W = FHW
    f = U._noise(FHW, 7)
    yy, xx = np.mgrid[0:H, 0:W]
    blob = (yy - 60) ** 2 * 4 + (xx - 52) ** 2 <= 40 * 40
    ramp = (U.REGION + (xx % 7) - 3).astype(np.uint8)
    f[blob] = np.stack([ramp, ramp, np.full_like(ramp, U.REGION)], axis=2)[blob]
    f[4:12, 80:96] = U.REGION
    return f, (60, 52)


def _lock_plane():
    lock = np.zeros(FHW, np.uint8)
    lock[55:70, 30:60] = 255                                            # cuts the blob
    lock[::9, ::7] = 255
    return lock


def _session(model, f, lock, **kw):
    """a session whose resident frame lies between sentinel margins -> (session, _Buf)"""
    s = serve.EditSession(model, f, **kw)
    fb = _Buf(f.shape, 3, like=f)
    s._frame = fb.view
    if lock is not None:
        s.set_lock(lock)
    return s, fb


def test_session_select_similar_is_the_statement(model):
    f, seed = _blob_frame()
    s, fb = _session(model, f, _lock_plane(), history=1)
    for t, contiguous, grow in ((16, True, 0), (16, True, 3), (1, True, 0), (1, False, 2), (16, False, 16), (0, True, 1)):
        want = U.spec_select(f, seed, t, contiguous, grow)
        sel = s.select_similar(seed, tolerance=t, contiguous=contiguous, grow=grow)
        box, count = U.spec_box_count(want)
        assert (sel.box, sel.count, sel.frame_hw) == (box, count, FHW), (t, contiguous, grow)
        assert np.array_equal(sel.plane.cpu().numpy(), want)
        assert np.array_equal(sel.mask(), want[box[0]:box[2], box[1]:box[3]])
    assert np.array_equal(fb.get(), f) and not s.can_undo                # not an edit; the lock plays no part
    # the stripes of the ramp: t = 1 and contiguous reaches the seed's stripe only
    assert s.select_similar(seed, tolerance=1).count < s.select_similar(seed, tolerance=1, contiguous=False).count


SESSION_CASES = [dict(), dict(grow=0), dict(grow=3, locked=True), dict(max_side=64, locked=True), dict(feather=4, locked=True),
                 dict(grow=3, feather=4, max_side=64), dict(grow=0, window=(24, 8, 72, 88), locked=True),
                 dict(tolerance=1, contiguous=False, grow=1, locked=True)]


@pytest.mark.parametrize("poison", [0, 0xFF])
@pytest.mark.parametrize("case", SESSION_CASES, ids=lambda c: "-".join("%s=%s" % kv for kv in sorted(c.items())) or "defaults")
def test_session_fill_similar_is_fill_of_the_statement(model, seopt, case, poison):
    """a twin session fills the statement's mask through `fill`: every byte of the two frames is equal, and one undo restores
    every byte.  Under SE_TEST_POISON every scratch byte is a NaN pattern until somebody writes it."""
    case = dict(case)
    f, seed = _blob_frame()
    lock = _lock_plane() if case.pop("locked", False) else None
    sel_kw = {k: case.pop(k) for k in ("tolerance", "contiguous", "grow") if k in case}
    spec_kw = dict(dict(tolerance=16, contiguous=True, grow=2), **sel_kw)
    mask = U.spec_select(f, seed, spec_kw["tolerance"], spec_kw["contiguous"], spec_kw["grow"])
    if poison:
        seopt.set("SE_TEST_POISON", poison)
    a, abuf = _session(model, f, lock, history=2)
    b, bbuf = _session(model, f, lock, history=2)
    pa, posa, ia = a.fill_similar(seed, low_latency=False, **sel_kw, **case)
    pb, posb, ib = b.fill(mask, low_latency=False, **case)
    after = abuf.get()
    assert np.array_equal(after, bbuf.get()) and not np.array_equal(after, f)
    assert ia.pop("selected") == int((mask > 0).sum()) and ia == ib and posa == posb and np.array_equal(pa, pb)
    changed = (after != f).any(axis=2)
    assert not (changed & (mask == 0)).any() and (lock is None or not (changed & (lock != 0)).any())
    a.undo()
    assert np.array_equal(abuf.get(), f)                                 # one call is one undo step
    assert not a.can_undo
    a.redo()
    assert np.array_equal(abuf.get(), after)


def test_session_fill_selection_encode_and_reuse(model):
    f, seed = _blob_frame()
    for encode, ref in (("png", lambda s, w: s.frame_png(w)), (("jpg", 90), lambda s, w: s.frame_jpg(w, quality=90))):
        s, fb = _session(model, f, _lock_plane(), history=1)
        patch, _, info = s.fill_similar(seed, encode=encode, low_latency=False)
        assert isinstance(patch, bytes) and patch == ref(s, info["window"]), encode
        s.undo()
        assert np.array_equal(fb.get(), f)
    # a selection is a mask: it is what it was after the frame changed, and fills again
    s, fb = _session(model, f, None, history=2)
    sel = s.select_similar(seed, grow=2)
    want = U.spec_select(f, seed, 16, True, 2)
    s.fill_selection(sel, low_latency=False)
    first = fb.get()
    assert not np.array_equal(first, f) and np.array_equal(sel.plane.cpu().numpy(), want)
    _, _, info = s.fill_selection(sel, low_latency=False)
    assert info["selected"] == sel.count == int((want > 0).sum()) and info["fill"] is True
    s.undo()
    assert np.array_equal(fb.get(), first)
    other = serve.EditSession(model, np.zeros((64, 64, 3), np.uint8))
    with pytest.raises(ValueError):
        other.fill_selection(sel)
