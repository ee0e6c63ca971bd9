"""Paired passes: in the default mode a large pass runs as two half-batch chains, one on the caller's
stream and the main arena, one on the ctx's side stream and the side arena, between one fork and one join.

Which kernel a layer runs does not depend on the batch, and every output is addressed per image, so the pairing must not change
a bit of any result: every test here compares the same call with SE_PAIR_MIN_PIXELS = 1 (every pass of two or more images is
paired) and 0 (never), with torch.equal.  What could go wrong is ordering and memory: one half reading or overwriting the
other's scratch (the poison test), a half planned past its arena (the workspace test), the fork / join of a pass against the
next pass (the pass test), against capture (the graph test) and against the profiler's one-stream plan (the profiler test)."""
import ctypes
import re

import numpy as np
import pytest
import torch

from sketchedit_amd import _lib, synth

pytestmark = pytest.mark.gpu

CAM, POOL_MAX, JOINT = 1, 2, 16
ON, OFF = 1, 0


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    e.load_state_dict("M", synth.make_state_dict("M", 0))
    e.load_state_dict("G", synth.make_state_dict("G", 0))
    assert e.weights_ready()
    yield e
    e.close()


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _inputs(B, H, W, seed=1234):
    img, sk = synth.make_inputs(B, H, W, seed=seed)
    return _cuda(img), _cuda(sk)


def _lock(B, H, W):
    lk = np.zeros((B, H, W), np.uint8)
    lk[:, H // 4: H // 2, 5: W - 7] = 255
    lk[B - 1] = 0
    return torch.from_numpy(lk).cuda()


def _clone(r):
    return {k: t.clone() for k, t in r.items()}


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), "%s: %s differs in %d of %d elements" % (what, k, int((a[k] != b[k]).sum()), a[k].numel())


class _precision:
    def __init__(self, eng, dtype):
        self.eng, self.dtype = eng, dtype

    def __enter__(self):
        self.eng.set_precision(self.dtype)

    def __exit__(self, *a):
        self.eng.set_precision("f32")


@pytest.mark.parametrize("cam", [True, False], ids=["cam", "nocam"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 64, 64), (4, 64, 64), (5, 64, 64), (3, 40, 72)], ids=lambda s: "%dx%dx%d" % s)
def test_paired_inference_is_bit_identical(eng, seopt, shape, dtype, cam):
    """every returned tensor, paired against unpaired; at B = 5 (halves of 3 and 2) every image also against its own call"""
    B, H, W = shape
    flags = (CAM if cam else 0) | POOL_MAX | JOINT
    ci, cs = _inputs(B, H, W)
    with _precision(eng, dtype):
        seopt.set("SE_PAIR_MIN_PIXELS", OFF)
        assert not _lib.pair_rule(B, H, W)
        off = _clone(eng.inference(ci, cs, flags, visualize=True, low_latency=False))
        seopt.set("SE_PAIR_MIN_PIXELS", ON)
        assert _lib.pair_rule(B, H, W)
        on = _clone(eng.inference(ci, cs, flags, visualize=True, low_latency=False))
        assert set(on) == {"composed", "mask", "hard", "maskim", "coarse", "fine"}
        _same(off, on, "paired")
        if B == 5:
            for i in range(B):
                one = eng.inference(ci[i:i + 1].contiguous(), cs[i:i + 1].contiguous(), flags, visualize=True, low_latency=False)
                _same({k: t[i:i + 1] for k, t in on.items()}, one, "image %d alone" % i)


def _entries(eng, ci, cs, flags, lock):
    B, _, H, W = ci.shape
    r = {}
    r["packed"] = eng.inference_packed(ci, cs, flags, torch.empty((B, 4, H, W), device="cuda"), low_latency=False)
    r["rgb"], r["m8"] = eng.inference_u8(ci, cs, flags, low_latency=False)
    r["rgb_lock"], r["m8_lock"] = eng.inference_u8(ci, cs, flags, low_latency=False, lock=lock)
    r.update({"locked_" + k: t for k, t in eng.inference(ci, cs, flags, visualize=True, low_latency=False, lock=lock).items()})
    return _clone(r)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_paired_entries_are_bit_identical(eng, seopt, dtype):
    """the packed output, the uint8 entry and the locked entries at 64 x 64, B = 4"""
    B, H, W = 4, 64, 64
    flags = CAM | POOL_MAX | JOINT
    ci, cs = _inputs(B, H, W, seed=77)
    lock = _lock(B, H, W)
    with _precision(eng, dtype):
        seopt.set("SE_PAIR_MIN_PIXELS", OFF)
        off = _entries(eng, ci, cs, flags, lock)
        seopt.set("SE_PAIR_MIN_PIXELS", ON)
        on = _entries(eng, ci, cs, flags, lock)
    _same(off, on, "paired")
    for half in (slice(0, 2), slice(2, 3)):                # (the lock plane reached both halves' netM)
        assert not torch.equal(on["m8"][half], on["m8_lock"][half])
    assert torch.equal(on["locked_mask"][B - 1], on["packed"][B - 1, 3:4])      # (the last image is unlocked)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_paired_under_poison(eng, seopt, dtype):
    """SE_TEST_POISON (tests/test_gpu_poison.py): the caller's workspace and outputs and every scratch block filled with the
    byte v -- a half that reads a byte the other half (or nobody) wrote changes the result with v"""
    B, H, W = 4, 64, 64
    flags = CAM | POOL_MAX | JOINT
    ci, cs = _inputs(B, H, W)
    seopt.set("SE_PAIR_MIN_PIXELS", ON)
    outs = []
    with _precision(eng, dtype):
        for v in (0, 0xFF, 0x47, 0xC7):
            seopt.set("SE_TEST_POISON", v)
            eng.workspace(B, H, W).fill_(v)
            out = {"composed": torch.empty((B, 3, H, W), device="cuda"), "mask": torch.empty((B, 1, H, W), device="cuda")}
            for t in out.values():
                t.view(torch.uint8).fill_(v)
            r = _clone(eng.inference(ci, cs, flags, visualize=True, out=out, low_latency=False))
            eng.workspace(B, H, W).fill_(v)
            r["rgb"], r["m8"] = eng.inference_u8(ci, cs, flags, low_latency=False)
            outs.append(_clone(r))
        seopt.set("SE_TEST_POISON", 0)
        seopt.set("SE_PAIR_MIN_PIXELS", OFF)
        off = _clone(eng.inference(ci, cs, flags, visualize=True, low_latency=False))
        off["rgb"], off["m8"] = eng.inference_u8(ci, cs, flags, low_latency=False)
    for k, t in outs[0].items():
        assert not t.is_floating_point() or bool(torch.isfinite(t).all()), k
    for v, o in zip((0xFF, 0x47, 0xC7), outs[1:]):
        _same(outs[0], o, "poison 0x%02X" % v)
    _same(off, outs[0], "paired")


def _raw_inference(eng, ci, cs, flags, ws, ws_bytes, r):
    """se_inference with the caller's workspace size; -> None, or the error message"""
    B, _, H, W = ci.shape
    P = _lib._ptr
    rc = eng.lib.se_inference(eng.h, eng._stream(), P(ci), P(cs), P(r["composed"]), P(r["mask"]), None, None, None, None, P(ws),
                              ctypes.c_size_t(ws_bytes), B, H, W, flags)
    return eng.lib.se_last_error(eng.h).decode() if rc else None


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_paired_workspace_is_exact(eng, seopt, dtype):
    """A workspace of se_workspace_bytes serves the paired call.  se_workspace_bytes is the largest need over every mode of a
    shape, so the size at which THIS call is refused is the one the refusal itself names ("this call needs N", N no more than
    se_workspace_bytes): N bytes run and give the same bits, N - 256 are refused before anything is enqueued."""
    B, H, W = 4, 64, 64
    flags = CAM | POOL_MAX | JOINT | (_lib.FLAG_BF16 if dtype == "bf16" else 0)
    ci, cs = _inputs(B, H, W)
    SENT = 0x5A

    def outs():
        r = {"composed": torch.empty((B, 3, H, W), device="cuda"), "mask": torch.empty((B, 1, H, W), device="cuda")}
        for t in r.values():
            t.view(torch.uint8).fill_(SENT)
        return r

    def need_of_call(ws):
        msg = _raw_inference(eng, ci, cs, flags, ws, 256, outs())
        m = re.search(r"workspace too small: 256 bytes, this call needs (\d+)", msg or "")
        assert m, msg
        return int(m.group(1))

    seopt.set("SE_PAIR_MIN_PIXELS", OFF)
    total_off = eng.lib.se_workspace_bytes(eng.h, B, H, W)
    ws = torch.empty(total_off, dtype=torch.uint8, device="cuda")
    ref = outs()
    assert _raw_inference(eng, ci, cs, flags, ws, total_off, ref) is None
    n_off = need_of_call(ws)
    seopt.set("SE_PAIR_MIN_PIXELS", ON)
    total = eng.lib.se_workspace_bytes(eng.h, B, H, W)
    ws = torch.empty(total, dtype=torch.uint8, device="cuda")
    n = need_of_call(ws)
    assert n % 256 == 0 and 0 < n <= total and total >= total_off
    assert n != n_off      # (the paired layout is another one: the call did pair)
    for size in (total, n):
        r = outs()
        assert _raw_inference(eng, ci, cs, flags, ws, size, r) is None
        _same(ref, r, "workspace of %d bytes" % size)
    r = outs()
    msg = _raw_inference(eng, ci, cs, flags, ws, n - 256, r)
    assert msg and "workspace too small" in msg, msg
    torch.cuda.synchronize()
    for t in r.values():
        assert bool((t.view(torch.uint8) == SENT).all())      # nothing ran


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_paired_passes(eng, seopt, dtype):
    """six images with the byte range lowered to three (SE_TEST_OFFSET_LIMIT): two passes, each paired as 2 + 1"""
    B, H, W = 6, 64, 64
    flags = CAM | POOL_MAX | JOINT
    ci, cs = _inputs(B, H, W, seed=123)
    with _precision(eng, dtype):
        seopt.set("SE_PAIR_MIN_PIXELS", OFF)
        whole = _clone(eng.inference(ci, cs, flags, visualize=True, low_latency=False))
        whole["rgb"], whole["m8"] = eng.inference_u8(ci, cs, flags, low_latency=False)
        seopt.set("SE_TEST_OFFSET_LIMIT", 3 * H * W * (48 if dtype == "bf16" else 96) + 1)
        seopt.set("SE_PAIR_MIN_PIXELS", ON)
        part = _clone(eng.inference(ci, cs, flags, visualize=True, low_latency=False))
        part["rgb"], part["m8"] = eng.inference_u8(ci, cs, flags, low_latency=False)
    _same(whole, part, "two paired passes")


def test_paired_graph_replay(eng, seopt):
    """graph=True on a stream of its own: the first call runs eagerly, the second captures (the fork / join of the pass become
    parallel branches of the graph), the third replays"""
    B, H, W = 4, 64, 64
    flags = CAM | POOL_MAX | JOINT
    ci, cs = _inputs(B, H, W, seed=5)
    seopt.set("SE_PAIR_MIN_PIXELS", OFF)
    off = _clone(eng.inference(ci, cs, flags, low_latency=False))
    seopt.set("SE_PAIR_MIN_PIXELS", ON)
    eager = _clone(eng.inference(ci, cs, flags, low_latency=False))
    _same(off, eager, "paired")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for i in range(3):
            g = _clone(eng.inference(ci, cs, flags, low_latency=False, graph=True))
            _same(eager, g, "graph call %d" % i)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


def test_profiled_call_is_not_paired(eng, seopt):
    """while the profiler is on the default mode is planned on one stream: the launches of a call that would pair are the
    unpaired call's, not twice as many"""
    B, H, W = 4, 64, 64
    flags = CAM | POOL_MAX | JOINT
    ci, cs = _inputs(B, H, W)
    seopt.set("SE_PAIR_MIN_PIXELS", OFF)
    with eng.launch_forms() as off:
        r_off = _clone(eng.inference(ci, cs, flags, low_latency=False))
    seopt.set("SE_PAIR_MIN_PIXELS", ON)
    with eng.launch_forms() as on:
        r_on = _clone(eng.inference(ci, cs, flags, low_latency=False))
    assert len(off) >= 50 and on == off
    _same(r_off, r_on, "profiled")
