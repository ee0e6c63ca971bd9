"""GPU tests of the device JPEG encoder with 4:2:0 sampling and per-image Huffman tables: se_jpg2_encode_u8 and
se_jpg2_code_i16 against the stream's statement (tests/jpg2_stream_util.py), byte for byte -- the segment, its size and the table
record with its padding -- every slot and every record between sentinels that must survive; flags = 0 against se_jpg_encode_u8;
every refusal; runs under SE_TEST_POISON; and the session calls with the new `encode` forms against a twin session's raw patch
run through the statement.

Shapes (tests/jpg2_cases.py): 16x16 flat (one MCU, EOB only), 17x33 (partial MCUs on both axes), 144x16 and 160x16 (nine and ten MCU rows: the
restart index wraps), 16x272 at quality 100 (102 blocks under 420: seven tiles of the row walk), 16x16 with every residue of the chroma
sums (the bias), 32x16 (stuffing and an FF from the padding under optimised tables), odd origins in a frame of width 53, B = 3 over
two frames; flags 1, 2, 3 at qualities 1, 50, 90, 100.  Coefficient planes of a few hundred blocks for the builder's and the coder's
corners: a first tree 17 deep, a token longer than 64 bits, every symbol in both classes, extreme DCs, ties, values out of range."""
import ctypes
import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpg2_cases
import jpg2_stream_util as U2
import jpg_cases
import jpg_stream_util as U
from sketchedit_amd import _lib, serve, synth

pytestmark = pytest.mark.gpu

ARGV = ("--batchSize 1 --name celeb --joint_train_inp --dataset_mode testimage --image_dirs x --mask_dirs x "
        "--image_lists x --model editline2 --netG deepfillc2 --pool_type max --use_cam --output_dir {d} --gpu_ids 0")
GUARD, TGUARD, SENTINEL = 37, 48, 0xA5            # (an odd guard: the slots start at every alignment; the records need 16)
CASES = jpg2_cases.cases()
CODE_CASES = jpg2_cases.code_cases()
ODD = jpg2_cases.by_name("x0, y0 odd", CASES)
MANY = jpg2_cases.by_name("B = 3", CASES)
SUB = {0: ("444", False), 1: ("420", False), 2: ("444", True), 3: ("420", True)}


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


_WANTED = {}


def wanted(case, quality, flags):
    """the statement's (segment, record) of every request of a case, computed once"""
    name, frames, reqs, hw, _ = case
    key = (name, quality, flags)
    if key not in _WANTED:
        _WANTED[key] = [U2.jpg2_scan(jpg2_cases.rectangle(frames, r, hw), quality, flags) for r in reqs]
    return _WANTED[key]


def _buffers(B, cap, flags):
    buf = torch.full((GUARD + B * cap + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = buf[GUARD:GUARD + B * cap].view(B, cap)
    tbuf = tables = None
    if flags & 2:
        tbuf = torch.full((TGUARD + B * 1088 + TGUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
        tables = tbuf[TGUARD:TGUARD + B * 1088].view(B, 1088)
    return buf, out, tbuf, tables


def _collect(B, cap, bound, flags, buf, tbuf, sizes):
    """-> [(segment, record or None)] on the host, after checking the sentinels around and between the slots and the records"""
    sizes = sizes.cpu().tolist()
    host = buf.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + B * cap:] == SENTINEL).all(), "a byte outside out was written"
    slots = host[GUARD:GUARD + B * cap].reshape(B, cap)
    for b, n in enumerate(sizes):
        assert 0 < n <= bound and (slots[b, n:] == SENTINEL).all(), "a byte behind segment %d was written" % b
    recs = [None] * B
    if flags & 2:
        th = tbuf.cpu().numpy()
        assert (th[:TGUARD] == SENTINEL).all() and (th[TGUARD + B * 1088:] == SENTINEL).all(), "a byte outside tables_out was written"
        recs = [th[TGUARD + b * 1088:TGUARD + (b + 1) * 1088].tobytes() for b in range(B)]
    return [(slots[b, :n].tobytes(), recs[b]) for b, n in enumerate(sizes)]


def _encode(eng, frames, reqs, hw, quality, flags, extra=3):
    dev = [torch.from_numpy(f).cuda() for f in frames]
    B, bound = len(reqs), U2.jpg2_bound(hw[0], hw[1], flags)
    cap = bound + extra
    buf, out, tbuf, tables = _buffers(B, cap, flags)
    sub, opt = SUB[flags]
    got, sizes, tab = eng.jpg2_encode_u8([dev[f] for f, _, _ in reqs], [(y0, x0) for _, y0, x0 in reqs], hw, quality=quality, subsampling=sub,
                                         optimize=opt, out=out, tables=tables)
    assert got is out and tab is tables
    res = _collect(B, cap, bound, flags, buf, tbuf, sizes)
    for f, d in zip(frames, dev):
        assert np.array_equal(d.cpu().numpy(), f)                         # frames are only read
    return res


def _same(got, want, what):
    assert len(got) == len(want)
    for b, ((gs, gt), (ws, wt)) in enumerate(zip(got, want)):
        assert gt == wt, (what, b, "tables", None if gt is None or wt is None else next(i for i, (x, y) in enumerate(zip(gt, wt)) if x != y))
        assert len(gs) == len(ws) and gs == ws, (what, b, len(gs), len(ws), next((i for i, (x, y) in enumerate(zip(gs, ws)) if x != y), None))


@pytest.mark.parametrize("flags", jpg2_cases.FLAGS)
@pytest.mark.parametrize("case", CASES, ids=[c[0].split(":")[0] for c in CASES])
def test_kernel_equals_the_statement(model, case, flags):
    name, frames, reqs, hw, qualities = case
    for quality in qualities:
        got = _encode(model.engine(), frames, reqs, hw, quality, flags)
        _same(got, wanted(case, quality, flags), (name, quality, flags))
    im = Image.open(io.BytesIO(serve.jpg_from_scan(got[-1][0], hw[0], hw[1], quality, SUB[flags][0], got[-1][1])))
    im.load()
    assert im.mode == "RGB" and im.size == (hw[1], hw[0])


def _code(eng, plane, flags, extra=3):
    coef = torch.from_numpy(plane).cuda()
    B, R, nblk = plane.shape[:3]
    bound = R * U2.row_bound(nblk, flags)
    cap = bound + extra
    buf, out, tbuf, tables = _buffers(B, cap, flags)
    sub, opt = SUB[flags]
    got, sizes, tab = eng.jpg2_code_i16(coef, subsampling=sub, optimize=opt, out=out, tables=tables)
    assert got is out and tab is tables
    res = _collect(B, cap, bound, flags, buf, tbuf, sizes)
    assert np.array_equal(coef.cpu().numpy(), plane)                      # coef is only read
    return res


@pytest.mark.parametrize("name,build", CODE_CASES, ids=[c[0] for c in CODE_CASES])
def test_code_i16_equals_the_statement(model, name, build):
    for flags in jpg2_cases.code_flags(name):
        plane = build(flags)
        _same(_code(model.engine(), plane, flags), [U2.jpg2_code(plane[0].tolist(), flags)], (name, flags))


def test_code_i16_takes_a_batch(model):
    planes = [jpg2_cases.ties(3), jpg2_cases.dc_extremes(3)]              # (1, 2, 36, 64) and (1, 1, 12, 64): the second padded
    pad = np.zeros_like(planes[0])
    pad[0, 0, :12] = planes[1][0, 0]
    both = np.concatenate([planes[0], pad])
    _same(_code(model.engine(), both, 3), [U2.jpg2_code(p[0].tolist(), 3) for p in (planes[0], pad)], "batch")


def test_flags_0_is_se_jpg_encode_u8(model):
    """se_jpg_encode_u8 forwards to the flags-0 case, so what the name stood for is checked against 6k's own statement
    (jpg_stream_util, not jpg2_stream_util as everywhere else in this file): both entries write its bytes"""
    eng = model.engine()
    for name, frames, reqs, hw, quality in jpg_cases.cases():
        dev = [torch.from_numpy(f).cuda() for f in frames]
        args = ([dev[f] for f, _, _ in reqs], [(y0, x0) for _, y0, x0 in reqs], hw)
        old, osz = eng.jpg_encode_u8(*args, quality=quality)
        got = _encode(eng, frames, reqs, hw, quality, 0)
        assert U2.jpg2_bound(hw[0], hw[1], 0) == U.jpg_bound(*hw) == eng.jpg2_bound(hw[0], hw[1], 0) == eng.jpg_bound(*hw)
        osz = osz.cpu().tolist()
        assert len(got) == len(osz) == len(reqs)
        for b, r in enumerate(reqs):
            want = U.jpg_scan(jpg_cases.rectangle(frames, r, hw), quality)
            assert got[b] == (want, None), (name, b, len(got[b][0]), len(want))
            assert osz[b] == len(want) and old[b, :osz[b]].cpu().numpy().tobytes() == want, (name, b, osz[b], len(want))


def test_every_alignment_of_out(model):
    name, frames, reqs, hw, _ = MANY
    for extra in (0, 1, 2, 3):                                            # cap, and with it the later slots' alignment
        _same(_encode(model.engine(), frames, reqs, hw, 50, 3, extra=extra), wanted(MANY, 50, 3), extra)


def test_under_poison(model, seopt):
    name, frames, reqs, hw, _ = ODD                                       # odd origins: the open words and the copy's ends
    plane = jpg2_cases.long_token(3)
    want = [U2.jpg2_code(plane[0].tolist(), 3)]
    for v in (0x55, 0xAA, 0xFF):
        seopt.set("SE_TEST_POISON", v)
        for flags in jpg2_cases.FLAGS:
            _same(_encode(model.engine(), frames, reqs, hw, 90, flags), wanted(ODD, 90, flags), (v, flags))
        _same(_code(model.engine(), plane, 3), want, v)
    seopt.set("SE_TEST_POISON", 0)


def test_refusals_leave_the_output_untouched(model):
    eng = model.engine()
    st = ctypes.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream)
    p = ctypes.c_void_p
    fa = torch.zeros((40, 44, 3), dtype=torch.uint8, device="cuda")
    fb = torch.zeros((64, 70, 3), dtype=torch.uint8, device="cuda")
    hs, ws, Q, F = 20, 24, 90, 3
    cap = U2.jpg2_bound(hs, ws, F)
    assert cap == eng.jpg2_bound(hs, ws, F) > 0
    out = torch.full((2 * cap + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    sizes = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    tabs = torch.full((2 * 1088 + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    need = eng.lib.se_jpg2_encode_u8_workspace_bytes(eng.h, 2, hs, ws, F)
    assert need > 0 and need % 256 == 0
    wsp = torch.zeros((need,), dtype=torch.uint8, device="cuda")
    call = eng.lib.se_jpg2_encode_u8

    def wins(*recs):
        return (_lib.Window * len(recs))(*[_lib.Window(f.data_ptr() if f is not None else None, None, f.shape[0] if f is not None else 40,
                                                       f.shape[1] if f is not None else 44, y0, x0) for f, y0, x0 in recs])
    ok = wins((fa, 1, 3), (fb, 30, 40))
    O, Z, T, W = p(out.data_ptr()), p(sizes.data_ptr()), p(tabs.data_ptr()), p(wsp.data_ptr())
    assert tabs.data_ptr() % 16 == 0
    zt = torch.zeros((4096,), dtype=torch.uint8, device="cuda")          # a sizes_out inside the last 16 bytes of a tables_out
    cases = [((None, 2, hs, ws, Q, F, O, cap, Z, T, W, need), "wins"), ((ok, 2, hs, ws, Q, F, None, cap, Z, T, W, need), "out"),
             ((ok, 2, hs, ws, Q, F, O, cap, None, T, W, need), "sizes_out"), ((ok, 2, hs, ws, Q, F, O, cap, Z, T, None, need), "workspace"),
             ((ok, 2, hs, ws, Q, F, O, cap, Z, None, W, need), "tables_out"), ((ok, 2, hs, ws, Q, 2, O, cap, Z, None, W, need), "tables_out"),
             ((wins((None, 1, 3), (fb, 30, 40)), 2, hs, ws, Q, F, O, cap, Z, T, W, need), "wins[0].frame_u8"),
             ((ok, 0, hs, ws, Q, F, O, cap, Z, T, W, need), "B"), ((ok, -1, hs, ws, Q, F, O, cap, Z, T, W, need), "B"),
             ((ok, 65536, hs, ws, Q, F, O, cap, Z, T, W, need), "B"),
             ((ok, 2, 15, ws, Q, F, O, cap, Z, T, W, need), "hs"), ((ok, 2, hs, 15, Q, F, O, cap, Z, T, W, need), "ws"),
             ((ok, 2, 8193, ws, Q, F, O, cap, Z, T, W, need), "hs"), ((ok, 2, hs, 8193, Q, F, O, cap, Z, T, W, need), "ws"),
             ((ok, 2, hs, ws, 0, F, O, cap, Z, T, W, need), "quality"), ((ok, 2, hs, ws, 101, F, O, cap, Z, T, W, need), "quality"),
             ((ok, 2, hs, ws, -90, F, O, cap, Z, T, W, need), "quality"),
             ((ok, 2, hs, ws, Q, 4, O, cap, Z, T, W, need), "flags"), ((ok, 2, hs, ws, Q, -1, O, cap, Z, T, W, need), "flags"),
             ((ok, 2, hs, ws, Q, 7, O, cap, Z, T, W, need), "flags"),
             ((wins((fa, 21, 3), (fb, 30, 40)), 2, hs, ws, Q, F, O, cap, Z, T, W, need), "wins[0].y0"),
             ((wins((fa, 1, 3), (fb, 30, 47)), 2, hs, ws, Q, F, O, cap, Z, T, W, need), "wins[1].x0"),
             ((wins((fa, -1, 3), (fb, 30, 40)), 2, hs, ws, Q, F, O, cap, Z, T, W, need), "wins[0].y0"),
             ((ok, 2, hs, ws, Q, F, O, cap - 1, Z, T, W, need), "cap"), ((ok, 2, hs, ws, Q, F, O, cap, Z, T, W, need - 1), "workspace too small"),
             ((ok, 2, hs, ws, Q, F, O, cap, Z, T, p(wsp.data_ptr() + 16), need), "aligned"),
             ((ok, 2, hs, ws, Q, F, O, cap, p(sizes.data_ptr() + 4), T, W, need), "sizes_out"),
             ((ok, 2, hs, ws, Q, F, O, cap, Z, p(tabs.data_ptr() + 8), W, need), "tables_out must be 16-byte aligned"),
             ((ok, 2, hs, ws, Q, F, p(fb.data_ptr() + 100), cap, Z, T, W, need), "out overlaps the frame of wins[1]"),
             ((ok, 2, hs, ws, Q, F, p(fa.data_ptr() - cap), cap, Z, T, W, need), "out overlaps the frame of wins[0]"),
             ((ok, 2, hs, ws, Q, F, p(wsp.data_ptr() + 256), cap, Z, T, W, need), "out overlaps the workspace"),
             ((ok, 2, hs, ws, Q, F, p(sizes.data_ptr() - 8), cap, Z, T, W, need), "out overlaps sizes_out"),
             ((ok, 2, hs, ws, Q, F, O, cap, Z, p(fb.data_ptr() + 160), W, need), "tables_out overlaps the frame of wins[1]"),
             ((ok, 2, hs, ws, Q, F, O, cap, Z, p(out.data_ptr() + 16), W, need), "out overlaps tables_out"),
             ((ok, 2, hs, ws, Q, F, O, cap, p(zt.data_ptr() + 2176), p(zt.data_ptr() + 16), W, need), "sizes_out overlaps tables_out"),
             ((ok, 2, hs, ws, Q, F, O, cap, Z, p(wsp.data_ptr() + 512), W, need), "the workspace overlaps tables_out")]
    for args, word in cases:
        assert call(eng.h, st, *args) != 0, word
        assert word in eng.lib.se_last_error(eng.h).decode(), (word, eng.lib.se_last_error(eng.h))
    # cap is checked against THIS call's bound: flags 3 is refused with the bound of flags 1
    assert U2.jpg2_bound(hs, ws, 1) < cap and call(eng.h, st, ok, 2, hs, ws, Q, F, O, U2.jpg2_bound(hs, ws, 1), Z, T, W, need) != 0
    wb = eng.lib.se_jpg2_encode_u8_workspace_bytes
    assert wb(eng.h, 2, 15, ws, F) == 0 and "hs" in eng.lib.se_last_error(eng.h).decode()
    assert wb(eng.h, 0, hs, ws, F) == 0 and "B" in eng.lib.se_last_error(eng.h).decode()
    assert wb(eng.h, 2, hs, ws, 4) == 0 and "flags" in eng.lib.se_last_error(eng.h).decode()
    # the per-op entry
    plane = torch.zeros((2, 2, 12, 64), dtype=torch.int16, device="cuda")
    ccap = 2 * U2.row_bound(12, F)
    cneed = eng.lib.se_jpg2_code_i16_workspace_bytes(eng.h, 2, 2, 12, F)
    assert 0 < cneed <= need and cneed % 256 == 0 and ccap <= cap
    C = p(plane.data_ptr())
    code = eng.lib.se_jpg2_code_i16
    ccases = [((None, 2, 2, 12, F, O, ccap, Z, T, W, cneed), "coef"), ((C, 0, 2, 12, F, O, ccap, Z, T, W, cneed), "B"),
              ((C, 2, 0, 12, F, O, ccap, Z, T, W, cneed), "R"), ((C, 2, 1025, 12, F, O, ccap, Z, T, W, cneed), "R"),
              ((C, 2, 2, 9, F, O, ccap, Z, T, W, cneed), "nblk"), ((C, 2, 2, 10, 2, O, ccap, Z, T, W, cneed), "nblk"),
              ((C, 2, 2, 0, F, O, ccap, Z, T, W, cneed), "nblk"), ((C, 2, 2, 3078, F, O, ccap, Z, T, W, cneed), "nblk"),
              ((C, 2, 2, 12, 4, O, ccap, Z, T, W, cneed), "flags"), ((C, 2, 2, 12, F, None, ccap, Z, T, W, cneed), "out"),
              ((C, 2, 2, 12, F, O, ccap, None, T, W, cneed), "sizes_out"), ((C, 2, 2, 12, F, O, ccap, Z, None, W, cneed), "tables_out"),
              ((C, 2, 2, 12, F, O, ccap, Z, T, None, cneed), "workspace"), ((C, 2, 2, 12, F, O, ccap - 1, Z, T, W, cneed), "cap"),
              ((C, 2, 2, 12, F, O, ccap, Z, T, W, cneed - 1), "workspace too small"),
              ((p(plane.data_ptr() + 1), 2, 2, 12, F, O, ccap, Z, T, W, cneed), "coef must be 2-byte aligned"),
              ((C, 2, 2, 12, F, p(plane.data_ptr() + 64), ccap, Z, T, W, cneed), "out overlaps coef"),
              ((C, 2, 2, 12, F, O, ccap, Z, p(plane.data_ptr() + 64), W, cneed), "tables_out overlaps coef"),
              ((C, 2, 2, 12, F, O, ccap, Z, p(tabs.data_ptr() + 4), W, cneed), "tables_out must be 16-byte aligned")]
    for args, word in ccases:
        assert code(eng.h, st, *args) != 0, word
        assert word in eng.lib.se_last_error(eng.h).decode(), (word, eng.lib.se_last_error(eng.h))
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (sizes == -1).all() and (tabs == SENTINEL).all() and not fa.any() and not fb.any() and not plane.any()
    with pytest.raises(_lib.SketchEditHipError, match="cap"):
        eng.jpg2_encode_u8([fa], [(0, 0)], (hs, ws), subsampling="420", out=torch.empty((1, U2.jpg2_bound(hs, ws, 1) - 1), dtype=torch.uint8, device="cuda"))
    with pytest.raises(_lib.SketchEditHipError, match="quality"):
        eng.jpg2_encode_u8([fa], [(0, 0)], (hs, ws), quality=0, optimize=True)
    for bad in (dict(subsampling="422"), dict(subsampling=420), dict(optimize=1), dict(optimize=None)):
        with pytest.raises(_lib.SketchEditHipError):
            eng.jpg2_encode_u8([fa], [(0, 0)], (hs, ws), **bad)
    with pytest.raises(_lib.SketchEditHipError):
        eng.jpg2_code_i16(plane.int())
    # without SE_JPG_OPTIMIZE tables_out is ignored: NULL, misaligned, overlapping -- and not written
    for tp in (None, p(tabs.data_ptr() + 3), O):
        assert call(eng.h, st, ok, 2, hs, ws, Q, 1, O, cap, Z, tp, W, need) == 0
    torch.cuda.synchronize()
    assert (tabs == SENTINEL).all()
    want = U2.jpg2_scan(np.zeros((hs, ws, 3), np.uint8), Q, 1)[0]
    n = sizes.cpu().tolist()
    host = out.cpu().numpy()
    assert n == [len(want)] * 2 and host[:n[0]].tobytes() == want and host[cap:cap + n[1]].tobytes() == want
    out.fill_(SENTINEL)
    assert call(eng.h, st, ok, 2, hs, ws, Q, F, O, cap, Z, T, W, need) == 0  # and the call they all resemble is accepted
    n = sizes.cpu().tolist()
    host, th = out.cpu().numpy(), tabs.cpu().numpy()
    want, rec = U2.jpg2_scan(np.zeros((hs, ws, 3), np.uint8), Q, F)
    assert n == [len(want)] * 2 and host[:n[0]].tobytes() == want and host[cap:cap + n[1]].tobytes() == want
    assert (host[n[0]:cap] == SENTINEL).all() and (host[cap + n[1]:] == SENTINEL).all()
    assert th[:1088].tobytes() == rec == th[1088:2176].tobytes() and (th[2176:] == SENTINEL).all()


# ---- sessions: the new encode forms against the same call without them, on a twin session ----------------------------------------
HW = (256, 320)
KW = dict(min_side=64)
STROKES = [([(20.5, 20.5), (50.5, 50.5)], 3.0), ([(265.5, 195.5), (295.5, 225.5), (270.0, 230.0)], 4.0)]


@pytest.fixture(scope="module")
def frame():
    y, x = np.mgrid[:HW[0], :HW[1]]
    smooth = np.stack([y + x // 2, 255 - y // 2 - x // 3, (x * 3 + y) // 4], axis=2)
    return ((smooth + np.random.RandomState(37).randint(0, 12, HW + (3,))) & 255).astype(np.uint8)


def _file(raw, quality, flags):
    scan, rec = U2.jpg2_scan(raw, quality, flags)
    return serve.jpg_from_scan(scan, raw.shape[0], raw.shape[1], quality, SUB[flags][0], rec)


def _twins(model, frame, lock=None):
    out = []
    for _ in range(2):
        s = serve.EditSession(model, frame)
        if lock is not None:
            s.set_lock(lock)
        out.append(s)
    return out


def test_edit_as_jpg_420_optimised(model, frame):
    sk = np.zeros(HW, np.uint8)
    sk[100:130, 140:150] = 255
    a, b = _twins(model, frame)
    raw, at0, info0 = a.edit(sk, low_latency=False)
    jpg, at1, info1 = b.edit(sk, low_latency=False, encode=("jpg", 90, "420", True))
    assert at0 == at1 and info0 == info1 and isinstance(jpg, bytes) and jpg == _file(raw, 90, 3)
    assert np.array_equal(a.frame(), b.frame())
    im = Image.open(io.BytesIO(jpg))
    im.load()
    assert im.size == (raw.shape[1], raw.shape[0])


def test_frame_jpg_420_optimised(model, frame):
    s = serve.EditSession(model, frame)
    part = np.ascontiguousarray(frame[3:52, 5:70])                        # 49 x 65: partial MCUs on both axes, odd origins
    assert s.frame_jpg((3, 5, 49, 65), quality=75, subsampling="420", optimize=True) == _file(part, 75, 3)
    assert s.frame_jpg((3, 5, 49, 65), quality=75, subsampling="420") == _file(part, 75, 1)
    assert s.frame_jpg((3, 5, 49, 65), quality=75, optimize=True) == _file(part, 75, 2)
    assert s.frame_jpg((3, 5, 49, 65), quality=75) == serve.jpg_from_scan(U.jpg_scan(part, 75), 49, 65, 75)
    assert np.array_equal(s.frame(), frame)


def test_edit_strokes_as_jpg_420_optimised_with_a_lock_and_a_working_size(model, frame):
    lock = np.zeros(HW, np.uint8)
    lock[10:200, 30:36] = 1
    a, b = _twins(model, frame, lock)
    raws, at0, info0 = a.edit_strokes(STROKES, low_latency=False, max_side=64, **KW)
    jpgs, at1, info1 = b.edit_strokes(STROKES, low_latency=False, max_side=64, encode=("jpg", 90, "420", True), **KW)
    assert at0 == at1 and info0 == info1 and info0["locked"] is True and info0["work"] == [(64, 64), (64, 64)] and len(jpgs) == 2
    for raw, jpg in zip(raws, jpgs):
        assert jpg == _file(raw, 90, 3)
    fa = a.frame()
    assert np.array_equal(fa, b.frame()) and not np.array_equal(fa, frame) and np.array_equal(fa[lock > 0], frame[lock > 0])
