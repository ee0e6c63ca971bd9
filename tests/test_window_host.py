"""Host-side logic of the editing sessions, no GPU: the window policy `serve.choose_window` over a randomised
sweep, and the grow loop of `serve.EditSession.edit` against a scripted stand-in for the device side."""
import numpy as np
import pytest

from sketchedit_amd import serve


def _boxes(rng, Hi, Wi):
    """boxes touching each frame edge, a box covering the frame, one pixel, and random ones: (y0, x0, y1, x1) half open"""
    out = [(0, 0, Hi, Wi), (0, Wi // 3, max(1, Hi // 5), Wi // 3 + max(1, Wi // 4)), (Hi - max(1, Hi // 5), 0, Hi, max(1, Wi // 2)),
           (Hi // 4, 0, Hi // 4 + 1, 1), (Hi // 2, Wi - 1, Hi // 2 + 1, Wi), (Hi - 1, Wi - 1, Hi, Wi), (0, 0, 1, 1)]
    for _ in range(6):
        y0, x0 = rng.randint(0, Hi), rng.randint(0, Wi)
        out.append((y0, x0, rng.randint(y0 + 1, Hi + 1), rng.randint(x0 + 1, Wi + 1)))
    return out


def test_choose_window_sweep():
    rng = np.random.RandomState(0)
    sizes = [(16, 16), (17, 23), (4100, 4099), (16, 4100), (4100, 17), (1081, 1921), (67, 70), (255, 257)]
    sizes += [(rng.randint(16, 4101), rng.randint(16, 4101)) for _ in range(60)]
    for Hi, Wi in sizes:
        fh, fw = Hi // 8 * 8, Wi // 8 * 8
        for box in _boxes(rng, Hi, Wi):
            for margin, bucket, min_side in ((0.5, 64, 256), (1.0, 64, 256), (0.0, 8, 16), (0.25, 128, 64), (4.0, 64, 256)):
                win = serve.choose_window(box, (Hi, Wi), margin=margin, bucket=bucket, min_side=min_side)
                assert win == serve.choose_window(box, (Hi, Wi), margin=margin, bucket=bucket, min_side=min_side)      # deterministic
                y0, x0, h, w = win
                ctx = (Hi, Wi, box, margin, bucket, min_side, win)
                assert h % 8 == 0 and w % 8 == 0 and h >= 16 and w >= 16, ctx
                assert 0 <= y0 and y0 + h <= Hi and 0 <= x0 and x0 + w <= Wi, ctx
                assert h % bucket == 0 or h == fh, ctx              # multiples of the bucket unless capped by the frame
                assert w % bucket == 0 or w == fw, ctx
                assert h <= fh and w <= fw, ctx
                if box[2] - box[0] <= fh:                           # contains the box whenever the floored frame can
                    assert y0 <= box[0] and box[2] <= y0 + h, ctx
                if box[3] - box[1] <= fw:
                    assert x0 <= box[1] and box[3] <= x0 + w, ctx
                # the side is what the rule says: extent + 2 ceil(margin max(bh, bw)), floor min_side, bucket, cap
                pad = int(np.ceil(margin * max(box[2] - box[0], box[3] - box[1])))
                for side, lo, hi, cap in ((h, box[0], box[2], fh), (w, box[1], box[3], fw)):
                    want = max(hi - lo + 2 * pad, min_side, 16)
                    assert side == min(-(-want // bucket) * bucket, cap), ctx


def test_choose_window_defaults_and_refusals():
    assert serve.choose_window((500, 900, 560, 1000), (1081, 1921)) == (402, 822, 256, 256)
    # a 300 x 200 stroke in a 1080p frame, pad ceil(0.5 * 300) = 150: 300 + 300 = 600 -> 640 and 200 + 300 = 500 -> 512
    assert serve.choose_window((400, 800, 700, 1000), (1081, 1921))[2:] == (640, 512)
    assert serve.choose_window(None, (1081, 1921)) is None
    assert serve.choose_window((5, 5, 5, 9), (1081, 1921)) is None
    assert serve.sketch_bbox(np.zeros((40, 50), np.uint8)) is None
    sk = np.zeros((40, 50), np.uint8)
    sk[7, 9] = 1
    sk[30, 3] = 255
    assert serve.sketch_bbox(sk) == (7, 3, 31, 10)
    for hw in ((15, 400), (400, 15), (8, 8)):
        with pytest.raises(ValueError):
            serve.choose_window((0, 0, 4, 4), hw)
    with pytest.raises(ValueError):
        serve.choose_window((0, 0, 4, 4), (64, 64), bucket=12)


class _Stub:
    """Scripted device side of a session: frames are numpy arrays; every run returns the next scripted border counts."""

    def __init__(self, script):
        self.script = list(script)
        self.runs, self.pastes, self.uploads = [], 0, []

    def upload(self, a):
        self.uploads.append(tuple(a.shape))
        return np.array(a)

    def run(self, frames, origins, sketches, h, w, commit, low_latency):
        assert len(frames) == len(origins) == len(sketches) == 1 and sketches[0].shape == (h, w)
        self.runs.append(dict(window=(origins[0][0], origins[0][1], h, w), commit=bool(commit)))
        counts = self.script.pop(0) if self.script else [0, 0, 0, 0]
        rgb, m8 = np.full((1, h, w, 3), 7, np.uint8), np.full((1, h, w), 255, np.uint8)
        if commit:
            self.paste(frames, origins, rgb, m8)
        return rgb, m8, [list(counts)]

    def paste(self, frames, origins, rgb, m8):
        self.pastes += 1
        y0, x0 = origins[0]
        frames[0][y0:y0 + rgb.shape[1], x0:x0 + rgb.shape[2]] = rgb[0]

    def crop(self, frame, y0, x0, h, w):
        return frame[y0:y0 + h, x0:x0 + w].copy()

    def download(self, frame):
        return frame.copy()


def _session(script, hw=(1081, 1921)):
    stub = _Stub(script)
    s = serve.EditSession(None, np.zeros(hw + (3,), np.uint8), backend=stub)
    sk = np.zeros(hw, np.uint8)
    sk[500:560, 900:1000] = 255
    return s, stub, sk


def test_edit_without_hits_runs_once_and_pastes_once():
    s, stub, sk = _session([[0, 0, 0, 0]])
    patch, (x0, y0), info = s.edit(sk)
    assert len(stub.runs) == 1 and stub.pastes == 1 and info["reruns"] == 0
    assert info["window"] == (402, 822, 256, 256) and (x0, y0) == (822, 402) and patch.shape == (256, 256, 3)
    assert stub.uploads == [(1081, 1921, 3), (256, 256)]          # the frame once, then only the window's sketch


def test_grow_loop_doubles_margin_and_is_bounded():
    hit = [0, 3, 0, 0]
    s, stub, sk = _session([hit] * 10)
    _, _, info = s.edit(sk, max_grow=2)
    assert info["reruns"] == 2 and len(stub.runs) == 3 and stub.pastes == 1
    wins = [r["window"] for r in stub.runs]
    box = (500, 900, 560, 1000)
    # margin 0.5 gives 256; doubling to 1.0 gives 100 + 200 = 300 -> 320; to 2.0: 100 + 400 = 500 -> 512
    assert wins == [serve.choose_window(box, (1081, 1921), margin=m) for m in (0.5, 1.0, 2.0)]
    assert [w[2:] for w in wins] == [(256, 256), (320, 320), (512, 512)] and info["margin"] == 2.0
    assert [r["commit"] for r in stub.runs] == [False, False, True]      # the last allowed run commits at once
    # the hits stop: no further rerun
    s, stub, sk = _session([hit, [0, 0, 0, 0]])
    _, _, info = s.edit(sk, max_grow=5)
    assert info["reruns"] == 1 and len(stub.runs) == 2 and stub.pastes == 1 and info["counts"] == [0, 0, 0, 0]
    # max_grow = 0: one committed run whatever the counts
    s, stub, sk = _session([hit])
    _, _, info = s.edit(sk, max_grow=0)
    assert info["reruns"] == 0 and stub.runs == [dict(window=(402, 822, 256, 256), commit=True)] and stub.pastes == 1
    assert info["counts"] == hit


def test_grow_loop_stops_at_the_floored_frame():
    hit = [1, 1, 1, 1]
    stub = _Stub([hit] * 20)
    s = serve.EditSession(None, np.zeros((301, 333, 3), np.uint8), backend=stub)
    sk = np.zeros((301, 333), np.uint8)
    sk[100:140, 100:150] = 1
    _, _, info = s.edit(sk, max_grow=10)
    assert info["window"] == (0, 0, 296, 328) or info["window"][2:] == (296, 328)
    assert stub.pastes == 1 and len(stub.runs) == info["reruns"] + 1 <= 11
    sizes = [r["window"][2:] for r in stub.runs]
    assert sizes[0] == (256, 256) and sizes[-1] == (296, 328) and len(set(sizes)) == len(sizes)      # every rerun grew
    assert stub.runs[-1]["commit"] and not any(r["commit"] for r in stub.runs[:-1])


def test_session_state_and_refusals():
    s, stub, sk = _session([])
    patch, (x0, y0), _ = s.edit(sk, window=(8, 16, 64, 32), max_grow=3)      # a given window never grows
    assert len(stub.runs) == 1 and stub.runs[0] == dict(window=(8, 16, 64, 32), commit=True) and (x0, y0) == (16, 8)
    f = s.frame()
    assert (f[8:72, 16:48] == 7).all() and f.sum() == 7 * 64 * 32 * 3 and np.array_equal(patch, f[8:72, 16:48])
    with pytest.raises(ValueError):
        s.edit(np.zeros((1080, 1920), np.uint8))          # another size: the whole-frame path's case
    with pytest.raises(ValueError):
        s.edit(np.zeros((1081, 1921), np.uint8))          # empty
    with pytest.raises(ValueError):
        s.edit(sk, window=(0, 0, 60, 64))
    with pytest.raises(ValueError):
        s.edit(sk, window=(1080, 0, 16, 16))
    with pytest.raises(ValueError):
        serve.EditSession(None, np.zeros((15, 300, 3), np.uint8), backend=stub)
