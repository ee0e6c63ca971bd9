"""Session traces without a GPU: the committed traces on the numpy model alone.  These are the conditions that keep
tests/test_gpu_session_trace.py from passing vacuously: the traces are reproducible, few of their steps are refused, every kind of
step and every hard state of the journal occurs, the snapshot oracle holds at every step -- and each of six planted defects makes a
trace fail.  The defects are planted by monkeypatch, on the one session the test makes."""
import types

import numpy as np
import pytest

from sketchedit_amd import serve
import session_trace_util as T

TIERS = dict(exact=T.EXACT_CASES, network=T.NETWORK_CASES)
EXACT_KINDS = sorted(T.EXACT_WEIGHTS)
NETWORK_KINDS = sorted(T.NETWORK_WEIGHTS)
EVERY = ["filter " + k for k in serve.FILTER_KINDS] + ["adjust " + f for f in ("lut", "matrix", "levels", "equalize", "match", "rim")] + \
        ["flip %s" % f for f in T.FLIPS] + ["combine " + op for op in serve.COMBINE_OPS]
THRICE = ["undo at depth 2 or more", "a redo after an undo", "an edit discards a redo stack", "eviction by history", "eviction by history_bytes",
          "an unjournalled commit clears a history", "a step under a lock set from a selection", "an undo across a set_lock",
          "a selection at least 3 edits old is used", "the selection of a move or transform is used"]
NETWORK_THRICE = ["a _Sequence entry whose rectangles overlap", "a _Regions entry with two windows"]


def _run(case, stats=None):
    s = T.model_session(case)
    T.run_lockstep(None, None, s, T.case_trace(case), context=T.case_id(case), stats=stats)
    return s


def test_the_same_seed_gives_the_same_trace():
    for case in (T.EXACT_CASES[1], T.NETWORK_CASES[2]):
        a = T.make_trace(case["seed"], case["steps"], case["hw"], case["tier"], case["history"], case["history_bytes"])
        assert a == T.case_trace(case) and len(a) == case["steps"]
        assert a != T.make_trace(case["seed"] + 1, case["steps"], case["hw"], case["tier"], case["history"], case["history_bytes"])
    assert serve.window_saved_bytes(120, 104) == 38400
    assert {c["hw"] for c in T.EXACT_CASES} == set(T.FRAMES) == {c["hw"] for c in T.NETWORK_CASES}
    assert {c["history"] for c in T.EXACT_CASES} == {0, 1, 3} and {c["history_bytes"] for c in T.EXACT_CASES} == {None, 60000, 20000, 8000}


def test_the_traces_reach_what_they_are_for():
    """the oracle holds at every step of every trace (run_lockstep raises otherwise); few steps of the set are refused; every kind of
    a tier occurs 5 times in the tier's traces; over the whole set every filter, adjustment, flip and combination occurs, and every
    hard state of the journal 3 times"""
    total = {}
    for tier in ("exact", "network"):
        stats = {}
        for case in TIERS[tier]:
            _run(case, stats)
        print("%s tier: %d steps in %d traces, %d refused" % (tier, stats["steps"], len(TIERS[tier]), stats.get("refused", 0)))
        for name in sorted(stats):
            print("  %-50s %d" % (name, stats[name]))
            total[name] = total.get(name, 0) + stats[name]
        for k in (EXACT_KINDS if tier == "exact" else NETWORK_KINDS):
            assert stats.get("kind " + k, 0) >= 5, (tier, k)
        for name in NETWORK_THRICE if tier == "network" else []:
            assert stats.get(name, 0) >= 3, name
    share = total.get("refused", 0) / float(total["steps"])
    print("refused: %d of %d steps, %.1f %%" % (total.get("refused", 0), total["steps"], 100 * share))
    assert share <= 0.05
    for name in EVERY:
        assert total.get(name, 0) >= 1, name
    for name in THRICE:
        assert total.get(name, 0) >= 3, name


# ---- planted defects: each must make a trace of the set fail against the unmodified model ------------------------------------------------------
def _forward_order(s, monkeypatch):
    real = s._exchange_sequence
    monkeypatch.setattr(s, "_exchange_sequence", lambda src, dst, reverse: real(src, dst, False))


def _drop_the_newest(s, monkeypatch):
    def push(self, entry):
        self._undo.append(entry)
        while len(self._undo) > self.history or (self.history_bytes is not None and self._bytes_used() > self.history_bytes):
            self._undo.pop()
    monkeypatch.setattr(s, "_push", types.MethodType(push, s))


class _NeverCleared(list):
    def clear(self):
        pass


def _keep_the_redo_list(s, monkeypatch):
    monkeypatch.setattr(s, "_redo", _NeverCleared())


def _drop_ignores_the_lock(s, monkeypatch):
    be = s.backend
    move, warp = be.move_drop, be.warp_drop
    monkeypatch.setattr(be, "move_drop", lambda frame, lift, rect, plane, lock, *a: move(frame, lift, rect, plane, None, *a))
    monkeypatch.setattr(be, "warp_drop", lambda frame, lift, rect, plane, lock, *a: warp(frame, lift, rect, plane, None, *a))


def _lock_keeps_the_plane(s, monkeypatch):
    monkeypatch.setattr(s.backend, "copy", lambda plane: plane)


def _swap_misses_a_pixel(s, monkeypatch):
    real = s.backend.swap

    def swap(frames, origins, window_hw, slots):
        h, w = window_hw
        last = [f[y0:y0 + h, x0 + w - 1].copy() for f, (y0, x0) in zip(frames, origins)]
        tails = [slot[:, 3 * (w - 1):3 * w].copy() for slot in slots]
        real(frames, origins, window_hw, slots)
        for f, (y0, x0), slot, px, tail in zip(frames, origins, slots, last, tails):      # the last pixel of each row stays where it was
            f[y0:y0 + h, x0 + w - 1] = px
            slot[:, 3 * (w - 1):3 * w] = tail
    monkeypatch.setattr(s.backend, "swap", swap)


def _scribble(index, step, pools):
    """behind a set_lock(selection): the selection's plane is changed in place, through each side's own backend -- a lock that is a
    copy does not notice"""
    if step["kind"] == "set_lock" and step["lock"] is not None and step["lock"][0] == "selection":
        for pool in pools:
            sel = pool[step["lock"][1]]
            sel.plane[...] = sel._backend.combine(sel.plane, None, serve.COMBINE_INVERT)[0]


DEFECTS = [("a _Sequence entry undone in forward order", "network", _forward_order, None),
           ("_push drops the newest entry", "exact", _drop_the_newest, None),
           ("the redo list survives a new edit", "exact", _keep_the_redo_list, None),
           ("the drop ignores the lock plane", "exact", _drop_ignores_the_lock, None),
           ("set_lock(selection) keeps the selection's plane", "exact", _lock_keeps_the_plane, _scribble),
           ("swap exchanges ws - 1 of the ws pixels of a row", "exact", _swap_misses_a_pixel, None)]


@pytest.mark.parametrize("defect", DEFECTS, ids=lambda d: d[0])
def test_a_planted_defect_is_caught(defect, monkeypatch):
    name, tier, plant, after = defect
    for case in TIERS[tier]:
        bad, good = T.model_session(case), T.model_session(case)
        with monkeypatch.context() as m:
            plant(bad, m)
            try:
                T.run_lockstep(bad, bad.frame, good, T.case_trace(case), context=T.case_id(case), after=after)
            except T.Mismatch as e:
                print("%s: caught by seed %d at step %d (%s): %s" % (name, case["seed"], e.index, (e.step or {}).get("kind"), e.what))
                return
    pytest.fail("%s: no trace of the %s tier noticed" % (name, tier))


def test_the_scribble_alone_changes_nothing_the_traces_compare():
    """the fifth defect's helper on two sound sessions: the lock is a copy, so the run passes"""
    case = next(c for c in T.EXACT_CASES if any(s["kind"] == "set_lock" and s["lock"] and s["lock"][0] == "selection" for s in T.case_trace(c)))
    a, b = T.model_session(case), T.model_session(case)
    T.run_lockstep(a, a.frame, b, T.case_trace(case), context=T.case_id(case), after=_scribble)


def test_replay_rebuilds_the_model_at_a_step():
    case = T.EXACT_CASES[0]
    s, pool, steps = T.replay(case, 17)
    full = T.model_session(case)
    T.run_lockstep(None, None, full, T.case_trace(case)[:17])
    assert len(steps) == 17 and np.array_equal(s.frame(), full.frame()) and s.history_bytes_used == full.history_bytes_used
    assert len(pool) <= T.POOL
