"""GPU tests of editing sessions as state machines: the traces of tests/session_trace_util.py run in lockstep on a real
EditSession, whose resident frame lies between sentinel margins, and on the numpy model; after every step every byte is compared --
the frame, the lock plane, the selections made, what the call returned, the journal's state -- and the model against whole-frame
snapshots.  What the other session tests do once on a fresh frame happens here in sequence: mixed journal entries undone to depth,
evictions and unjournalled commits, overlapping rectangles, selections and locks that outlive edits, device buffers freed as the
trace goes on.  The forward itself is the engine's: the model asks the engine for it, uncommitted, on its own copy of the frame (the
parity tests cover it); everything around it -- save, paste, drop, journal -- is the model's own.  Every comparison is exact.
A failure names its seed and step: session_trace_util.replay rebuilds the model there, on the CPU."""
import time

import numpy as np
import pytest
import torch

from sketchedit_amd import serve
import session_trace_util as T
from test_gpu_lasso import _session, model  # noqa: F401

pytestmark = pytest.mark.gpu


def _engine_forward(model):
    """the model's `forward` hook: the engine's own entries, never committing, on uploads of the model's arrays"""
    be = serve._ModelBackend(model)

    def up(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def forward(entry, frames, origins, sketches, holes, locks, window_hw, work_hw, low_latency):
        fr, sk = [up(f) for f in frames], [up(s) for s in sketches]
        lk = None if locks is None else [up(p) for p in locks]
        counts = None
        if entry == "run":
            rgb, m8, counts = be.run(fr, origins, sk, window_hw[0], window_hw[1], False, low_latency)
        elif entry == "run_scaled":
            rgb, m8, counts = be.run_scaled(fr, origins, sk, window_hw, work_hw, False, low_latency)
        elif entry == "run_locked":
            rgb, m8, counts = be.run_locked(fr, origins, sk, lk, window_hw, work_hw, False, low_latency)
        else:
            rgb, m8 = be.run_fill(fr, origins, sk, [up(h) for h in holes], lk, window_hw, work_hw, low_latency)
        return rgb.cpu().numpy(), m8.cpu().numpy(), counts
    return forward


def _pair(model, case):
    """-> (the device session, its frame's reader, the model session)"""
    dev, fb = _session(model, T.make_frame(case["hw"])[0], None, history=case["history"], history_bytes=case["history_bytes"])
    return dev, fb.get, T.model_session(case, _engine_forward(model))


def _lockstep(model, case, low_latency=None, what=""):
    dev, reader, ms = _pair(model, case)
    stats = {}
    t0 = time.time()
    T.run_lockstep(dev, reader, ms, T.case_trace(case), context=T.case_id(case) + what, low_latency=low_latency, stats=stats)
    print("%s%s: %d steps, %d changed the frame, %d refused, %.2f s"
          % (T.case_id(case), what, stats["steps"], stats.get("the frame changed", 0), stats.get("refused", 0), time.time() - t0))
    assert stats["steps"] == case["steps"] and stats.get("the frame changed", 0) >= 5


@pytest.mark.parametrize("case", T.EXACT_CASES, ids=T.case_id)
def test_exact_tier(model, seopt, case):
    """selections, locks, clones, transforms, filters, adjustments, undo and redo: no forward runs.  Every other pair of cases runs
    with every scratch byte poisoned until somebody writes it."""
    if T.EXACT_CASES.index(case) // 2 % 2:
        seopt.set("SE_TEST_POISON", 0xFF)
    _lockstep(model, case)


@pytest.mark.parametrize("case", T.NETWORK_CASES, ids=T.case_id)
def test_network_tier(model, case):
    """... and fills, moves and transforms that mend their hole, edits and stroke edits: the forwards are the engine's, in both
    execution modes"""
    low_latency = bool(T.NETWORK_CASES.index(case) // 2 % 2)
    _lockstep(model, case, low_latency, " low_latency=%s" % low_latency)


def test_network_tier_bf16(model):
    """the session path takes the engine's precision as it is: one trace with bf16 forwards"""
    eng = model.engine()
    eng.set_precision("bf16")
    try:
        _lockstep(model, T.NETWORK_CASES[1], False, " bf16")
    finally:
        eng.set_precision("f32")


def test_two_sessions_interleaved(model):
    """two sessions of the two frame sizes on one model take their steps in turn: the engine's workspace and scratch are shared, and
    each session must still be its own model's, byte for byte"""
    runs = []
    for case in (T.NETWORK_CASES[2], T.NETWORK_CASES[5]):
        dev, reader, ms = _pair(model, case)
        runs.append(T.iter_lockstep(dev, reader, ms, T.case_trace(case), context="interleaved, " + T.case_id(case), low_latency=False))
    assert T.NETWORK_CASES[2]["hw"] != T.NETWORK_CASES[5]["hw"]
    t0 = time.time()
    while runs:
        for it in list(runs):
            if next(it, None) is None:
                runs.remove(it)
    print("interleaved: %.2f s" % (time.time() - t0))
