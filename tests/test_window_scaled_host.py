"""Host-side logic of window edits at a working size, no GPU: the policy `serve.choose_working_size`, the grow
loop of `serve.EditSession.edit(max_side=...)` and the grouping of `BatchingServer(window=True, max_side=...)` against a
scripted stand-in for the device side."""
import threading

import numpy as np
import pytest

from sketchedit_amd import serve


def test_choose_working_size_sweep():
    rng = np.random.RandomState(0)
    cases = [(16, 16), (17, 23), (640, 640), (641, 640), (2000, 2000), (1080, 1920), (16, 4000), (4000, 16), (67, 70), (24, 5000)]
    cases += [(rng.randint(16, 5000), rng.randint(16, 5000)) for _ in range(300)]
    for hs, ws in cases:
        for max_side in (16, 64, 256, 640, 1000, 1024):
            H, W = serve.choose_working_size((hs, ws), max_side)
            ctx = (hs, ws, max_side, H, W)
            assert H % 8 == 0 and W % 8 == 0 and H >= 16 and W >= 16, ctx
            if max(hs, ws) <= max_side:                          # identity under the cap, up to the flooring
                assert (H, W) == (hs // 8 * 8, ws // 8 * 8), ctx
                continue
            assert max(H, W) <= max_side and H <= hs and W <= ws, ctx      # never above the cap, never an upscale
            # the rule itself, in exact arithmetic: floor(side * max_side / long side) floored to 8, at least 16
            long_side = max(hs, ws)
            assert H == max((hs * max_side // long_side) // 8 * 8, 16) and W == max((ws * max_side // long_side) // 8 * 8, 16), ctx
            assert max(H, W) == max(max_side // 8 * 8, 16), ctx               # the long side lands on the cap
            # aspect preserved up to the flooring: the short side is within 8 of its exact scaled value (or raised to 16)
            for side, got in ((hs, H), (ws, W)):
                exact = side * max_side / long_side
                assert got == 16 or exact - 8 < got <= exact, ctx


def test_choose_working_size_values_and_refusals():
    assert serve.choose_working_size((2000, 2000), 640) == (640, 640)
    assert serve.choose_working_size((1080, 1920), 640) == (360, 640)
    assert serve.choose_working_size((1216, 1080), 640) == (640, 568)
    assert serve.choose_working_size((512, 512), 640) == (512, 512)
    assert serve.choose_working_size((67, 70), 640) == (64, 64)
    assert serve.choose_working_size((16, 4000), 640) == (16, 640)
    for hw, cap in (((15, 400), 640), ((400, 15), 640), ((400, 400), 15), ((400, 400), 0)):
        with pytest.raises(ValueError):
            serve.choose_working_size(hw, cap)


class _Stub:
    """Scripted device side of a session: frames are numpy arrays; every run returns the next scripted border counts.  The
    scaled calls are recorded apart from the unscaled ones, so a test sees which path was taken."""

    def __init__(self, script):
        self.script = list(script)
        self.calls, self.uploads = [], []

    def upload(self, a):
        self.uploads.append(tuple(a.shape))
        return np.array(a)

    def _counts(self, n):
        return [list(self.script.pop(0) if self.script else [0, 0, 0, 0]) for _ in range(n)]

    def run(self, frames, origins, sketches, h, w, commit, low_latency):
        assert all(s.shape == (h, w) for s in sketches)
        self.calls.append(("run", [(y0, x0, h, w) for y0, x0 in origins], bool(commit)))
        rgb, m8 = np.full((len(frames), h, w, 3), 7, np.uint8), np.full((len(frames), h, w), 255, np.uint8)
        if commit:
            self._write(frames, origins, (h, w))
        return rgb, m8, self._counts(len(frames))

    def paste(self, frames, origins, rgb, m8):
        self.calls.append(("paste", [(y0, x0) + tuple(rgb.shape[1:3]) for y0, x0 in origins]))
        self._write(frames, origins, rgb.shape[1:3])

    def run_scaled(self, frames, origins, sketches, window_hw, work_hw, commit, low_latency):
        assert all(s.shape == tuple(window_hw) for s in sketches)          # the sketch travels at frame scale
        H, W = work_hw
        self.calls.append(("run_scaled", [(y0, x0) + tuple(window_hw) for y0, x0 in origins], tuple(work_hw), bool(commit)))
        rgb, m8 = np.full((len(frames), H, W, 3), 7, np.uint8), np.full((len(frames), H, W), 255, np.uint8)      # working size
        if commit:
            self._write(frames, origins, window_hw)
        return rgb, m8, self._counts(len(frames))

    def paste_scaled(self, frames, origins, window_hw, rgb, m8):
        self.calls.append(("paste_scaled", [(y0, x0) + tuple(window_hw) for y0, x0 in origins], tuple(rgb.shape[1:3])))
        self._write(frames, origins, window_hw)

    def _write(self, frames, origins, hw):
        for f, (y0, x0) in zip(frames, origins):
            f[y0:y0 + hw[0], x0:x0 + hw[1]] = 7

    def select(self, t, idx):
        return t[list(idx)]

    def crop(self, frame, y0, x0, h, w):
        return frame[y0:y0 + h, x0:x0 + w].copy()

    def download(self, frame):
        return frame.copy()


HW = (2161, 3841)
BOX = (900, 1500, 1100, 2100)          # a long stroke: 200 x 600, windows of 832 x 1216 and up


def _session(script, hw=HW, box=BOX):
    stub = _Stub(script)
    s = serve.EditSession(None, np.zeros(hw + (3,), np.uint8), backend=stub)
    sk = np.zeros(hw, np.uint8)
    sk[box[0]:box[2], box[1]:box[3]] = 255
    return s, stub, sk


def test_scaled_edit_follows_the_grow_loop():
    hit = [0, 3, 0, 0]
    s, stub, sk = _session([hit] * 10)
    patch, (x0, y0), info = s.edit(sk, max_grow=2, max_side=640)
    wins = [serve.choose_window(BOX, HW, margin=m) for m in (0.5, 1.0, 2.0)]
    assert len({w[2:] for w in wins}) == 3 and all(max(w[2:]) > 640 for w in wins)          # three large windows, all scaled
    works = [serve.choose_working_size(w[2:], 640) for w in wins]
    assert stub.calls == [("run_scaled", [wins[0]], works[0], False), ("run_scaled", [wins[1]], works[1], False),
                          ("run_scaled", [wins[2]], works[2], True)]          # the last allowed run commits in the same call
    assert all(max(w) == 640 for w in works)
    assert info["work"] == works[2] and info["window"] == wins[2] and info["reruns"] == 2 and info["margin"] == 2.0
    assert patch.shape == wins[2][2:] + (3,) and (x0, y0) == (wins[2][1], wins[2][0]) and (patch == 7).all()
    # only the window's sketch goes up, at frame scale
    assert stub.uploads == [HW + (3,)] + [w[2:] for w in wins]


def test_scaled_edit_pastes_through_the_scaled_paste():
    # the hits stop after one rerun: that run was not committed, so the scaled paste follows with the working-size result
    s, stub, sk = _session([[1, 0, 0, 0], [0, 0, 0, 0]])
    _, _, info = s.edit(sk, max_grow=5, max_side=640)
    wins = [serve.choose_window(BOX, HW, margin=m) for m in (0.5, 1.0)]
    works = [serve.choose_working_size(w[2:], 640) for w in wins]
    assert stub.calls == [("run_scaled", [wins[0]], works[0], False), ("run_scaled", [wins[1]], works[1], False),
                          ("paste_scaled", [wins[1]], works[1])]
    assert info["reruns"] == 1 and info["counts"] == [0, 0, 0, 0] and info["work"] == works[1]
    # max_grow = 0: the counts cannot matter, one committed call
    s, stub, sk = _session([[5, 5, 5, 5]])
    _, _, info = s.edit(sk, max_grow=0, max_side=640)
    assert stub.calls == [("run_scaled", [wins[0]], works[0], True)] and info["counts"] == [5, 5, 5, 5] and info["reruns"] == 0


def test_scaled_edit_under_the_cap_and_given_windows():
    # a small sketch: the working size is the window itself, still through the scaled entry (scale 1 there is the old path)
    s, stub, sk = _session([], hw=(1081, 1921), box=(500, 900, 560, 1000))
    _, _, info = s.edit(sk, max_grow=0, max_side=640)
    assert stub.calls == [("run_scaled", [(402, 822, 256, 256)], (256, 256), True)] and info["work"] == (256, 256)
    # a given window needs no multiple-of-8 sides when the forward runs at a working size; it never grows
    s, stub, sk = _session([[9, 9, 9, 9]], hw=(1081, 1921), box=(500, 900, 560, 1000))
    _, (x0, y0), info = s.edit(sk, window=(3, 5, 1001, 1203), max_grow=3, max_side=320)
    assert stub.calls == [("run_scaled", [(3, 5, 1001, 1203)], serve.choose_working_size((1001, 1203), 320), True)]
    assert info["work"] == (264, 320) and (x0, y0) == (5, 3)
    with pytest.raises(ValueError):
        s.edit(sk, window=(3, 5, 1001, 1203))                     # without max_side the window feeds the network directly
    with pytest.raises(ValueError):
        s.edit(sk, window=(3, 5, 15, 1203), max_side=320)
    with pytest.raises(ValueError):
        s.edit(sk, window=(100, 5, 1001, 1203), max_side=320)     # outside the frame


def test_max_side_none_makes_todays_calls():
    hit = [0, 3, 0, 0]
    s, stub, sk = _session([hit, [0, 0, 0, 0]], hw=(1081, 1921), box=(500, 900, 560, 1000))
    _, _, info = s.edit(sk, max_grow=5, max_side=None)
    wins = [serve.choose_window((500, 900, 560, 1000), (1081, 1921), margin=m) for m in (0.5, 1.0)]
    assert stub.calls == [("run", [wins[0]], False), ("run", [wins[1]], False), ("paste", [wins[1]])]
    assert "work" not in info and info["reruns"] == 1
    s, stub, sk = _session([hit], hw=(1081, 1921), box=(500, 900, 560, 1000))
    _, _, info = s.edit(sk, max_grow=0)
    assert stub.calls == [("run", [wins[0]], True)] and sorted(info) == ["counts", "margin", "reruns", "window"]


def _submit_all(srv, jobs):
    outs = [None] * len(jobs)

    def call(i):
        outs[i] = srv.submit(*jobs[i])
    ts = [threading.Thread(target=call, args=(i,)) for i in range(len(jobs))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    return outs


def test_server_groups_by_window_and_working_size():
    """two sessions, frames of different sizes, equal (hs, ws, H, W) -> ONE scaled run of two requests"""
    stub = _Stub([])
    sessions, sks = [], []
    for hw, (cy, cx) in (((2161, 3841), (700, 1200)), ((1801, 2403), (300, 500))):
        sessions.append(serve.EditSession(None, np.zeros(hw + (3,), np.uint8), backend=stub))
        sk = np.zeros(hw, np.uint8)
        sk[cy:cy + 500, cx:cx + 600] = 255
        sks.append(sk)
    srv = serve.BatchingServer(object(), max_batch=2, max_wait_s=5.0, window=True, max_grow=0, max_side=640)
    for s in sessions:
        s.model = srv.model
    outs = _submit_all(srv, list(zip(sessions, sks)))
    srv.close()
    assert srv.batches == [2]
    runs = [c for c in stub.calls if c[0] == "run_scaled"]
    assert len(runs) == 1 and len(runs[0][1]) == 2 and runs[0][3] is True and [c[0] for c in stub.calls] == ["run_scaled"]
    wins = [serve.choose_window((cy, cx, cy + 500, cx + 600), hw) for hw, (cy, cx) in (((2161, 3841), (700, 1200)), ((1801, 2403), (300, 500)))]
    assert sorted(runs[0][1]) == sorted(wins) and wins[0][2:] == wins[1][2:] == (1152, 1216)
    assert runs[0][2] == serve.choose_working_size((1152, 1216), 640) == (600, 640)
    for (patch, (x0, y0), info), win in zip(outs, wins):
        assert info["window"] == win and info["work"] == (600, 640) and patch.shape == (1152, 1216, 3) and (x0, y0) == (win[1], win[0])
    # the group key carries both sizes: equal windows under different caps do not share a forward
    assert srv._window_key(wins[0]) == ("window", 3, 1152, 1216, 600, 640)
    assert serve.BatchingServer._window_key(type("S", (), dict(max_side=None))(), wins[0]) == ("window", 3, 1152, 1216)


def test_server_keeps_a_sessions_edits_in_order():
    """two edits of ONE session never share a group, and run in the order they were submitted; a request that grows is
    queued again under its larger window's key and still precedes the session's next edit"""
    stub = _Stub([[1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]])
    s = serve.EditSession(None, np.zeros(HW + (3,), np.uint8), backend=stub)
    sk1 = np.zeros(HW, np.uint8)
    sk1[BOX[0]:BOX[2], BOX[1]:BOX[3]] = 255
    sk2 = np.zeros(HW, np.uint8)
    sk2[100:700, 200:900] = 255
    srv = serve.BatchingServer(object(), max_batch=4, max_wait_s=0.05, window=True, max_grow=1, max_side=640)
    s.model = srv.model
    first = threading.Thread(target=lambda: srv.submit(s, sk1))
    first.start()
    while not srv._queue and not stub.calls:          # the first edit is queued (or already running) before the second arrives
        pass
    out2 = srv.submit(s, sk2)
    first.join()
    srv.close()
    w1 = [serve.choose_window(BOX, HW, margin=m) for m in (0.5, 1.0)]
    w2 = serve.choose_window((100, 200, 700, 900), HW)
    runs = [c for c in stub.calls if c[0] == "run_scaled"]
    assert [c[1] for c in runs] == [[w1[0]], [w1[1]], [w2]]          # grown rerun of edit 1 before edit 2
    assert [c[3] for c in runs] == [False, True, False] or [c[3] for c in runs] == [False, True, True]
    assert out2[2]["window"] == w2 and out2[2]["work"] == serve.choose_working_size(w2[2:], 640)
    assert srv.batches == [1, 1, 1]


def test_max_side_needs_window_mode():
    with pytest.raises(ValueError):
        serve.BatchingServer(object(), max_side=640)
