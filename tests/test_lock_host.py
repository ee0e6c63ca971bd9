"""Host tests of locked regions: the oracle composed per the definition against the vectors the reference's
own netM and netG gave (tests/golden/make_golden_lock.py), and the host logic of EditSession.set_lock with a scripted backend.
CPU only."""
import os

import numpy as np
import pytest
import torch

from oracle import sketchedit_oracle as O
from sketchedit_amd import serve, synth

TOL = 2e-6                         # the bound tests/test_oracle_golden.py holds the oracle to


def _maxdiff(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def test_oracle_follows_the_definition(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "lock_64.npz")))
    gain, wseed, iseed, B, H, W = g["meta"]
    WM, WG = synth.make_state_dict("M", 0, float(gain)), synth.make_state_dict("G", 0, float(gain))
    img, sk = synth.make_inputs(int(B), int(H), int(W), seed=int(iseed))
    lock = torch.from_numpy(g["lock"] > 0)[:, None]
    # the fixture's locks: a 20 x 24 rectangle, a full-height column and scattered pixels, different per image
    assert g["lock"].shape == (2, 64, 64) and g["lock"].dtype == np.uint8 and not np.array_equal(g["lock"][0], g["lock"][1])
    assert 0.05 < lock.float().mean() < 0.5
    with torch.no_grad():
        soft, _ = O.netM_forward(WM, img, sk)
        mask = torch.where(lock, torch.zeros_like(soft), soft)
        hard = (mask > 0.5).float()
        coarse, fine = O.netG_forward(WG, img, img, hard, hard, sk)
        image = torch.from_numpy(img)
        composed = fine * mask + image * (1 - mask)
    assert _maxdiff(mask, g["mask"]) < TOL
    assert np.array_equal(hard.numpy(), g["hard_mask"])
    assert _maxdiff(coarse, g["coarse"]) < TOL and _maxdiff(fine, g["fine"]) < TOL
    assert _maxdiff(composed, g["composed"]) < TOL
    # what the definition promises, in the reference's own vectors
    l3 = np.broadcast_to(lock.numpy(), g["composed"].shape)
    assert (g["mask"][lock.numpy()] == 0).all() and (g["hard_mask"][lock.numpy()] == 0).all()
    assert np.array_equal(g["composed"][l3].view(np.int32), img[l3].view(np.int32))
    e2e = dict(np.load(os.path.join(golden_dir, "e2e_64.npz")))
    assert np.array_equal(g["mask"][~lock.numpy()], e2e["mask"][~lock.numpy()])
    assert _maxdiff(g["fine"], e2e["fine"]) > 1e-2             # the lock changed what netG was given, not only the paste


HW = (400, 600)


class _Stub:
    """A scripted device: frames and planes are numpy arrays; every backend call is logged"""

    def __init__(self):
        self.calls = []

    def upload(self, a):
        return np.array(a)

    def _ret(self, n, h, w):
        return np.zeros((n, h, w, 3), np.uint8), np.full((n, h, w), 255, np.uint8), [[0, 0, 0, 0] for _ in range(n)]

    def run(self, frames, origins, sketches, h, w, commit, low_latency):
        self.calls.append(("run", bool(commit)))
        return self._ret(len(frames), h, w)

    def run_scaled(self, frames, origins, sketches, window_hw, work_hw, commit, low_latency):
        self.calls.append(("run_scaled", bool(commit)))
        return self._ret(len(frames), *work_hw)

    def paste(self, frames, origins, rgb, m8):
        self.calls.append(("paste",))

    def paste_scaled(self, frames, origins, window_hw, rgb, m8):
        self.calls.append(("paste_scaled",))

    def run_locked(self, frames, origins, sketches, locks, window_hw, work_hw, commit, low_latency):
        self.calls.append(("run_locked", bool(commit), work_hw, [None if t is None else int((t > 0).sum()) for t in locks]))
        return self._ret(len(frames), *(work_hw or window_hw))

    def paste_locked(self, frames, origins, locks, window_hw, rgb, m8):
        self.calls.append(("paste_locked", [None if t is None else int((t > 0).sum()) for t in locks]))

    def crop(self, frame, y0, x0, h, w):
        return frame[y0:y0 + h, x0:x0 + w].copy()

    def download(self, frame):
        return frame.copy()


class _OldStub(_Stub):
    """the backend of the older host tests: it has no locked calls at all"""
    run_locked = paste_locked = None


def _sketch():
    sk = np.zeros(HW, np.uint8)
    sk[200:210, 300:330] = 255
    return sk


def test_a_session_without_a_lock_issues_no_lock_call():
    stub = _OldStub()
    s = serve.EditSession(None, np.zeros(HW + (3,), np.uint8), backend=stub)
    assert s.lock() is None and not s.locked
    _, _, info = s.edit(_sketch(), max_grow=0)
    _, _, info2 = s.edit(_sketch(), max_grow=0, max_side=32)
    assert "locked" not in info and "locked" not in info2
    assert stub.calls == [("run", True), ("run_scaled", True)]


def test_set_lock_routes_every_path_and_none_returns():
    stub = _Stub()
    s = serve.EditSession(None, np.zeros(HW + (3,), np.uint8), backend=stub)
    plane = np.zeros(HW, np.uint8)
    plane[10:20, 30:50] = 7                                   # any non-zero byte locks
    s.set_lock(plane)
    got = s.lock()
    assert s.locked and got.dtype == np.uint8 and np.array_equal(got, (plane > 0) * np.uint8(255))
    _, _, info = s.edit(_sketch(), max_grow=0)                                        # committed in the call
    assert info["locked"] is True and stub.calls == [("run_locked", True, None, [200])]
    stub.calls.clear()
    _, _, info = s.edit(_sketch(), max_grow=1)                                        # an uncommitted run, then the paste
    assert info["locked"] is True and [c[0] for c in stub.calls] == ["run_locked", "paste_locked"] and stub.calls[0][1] is False
    stub.calls.clear()
    _, _, info = s.edit(_sketch(), max_grow=0, max_side=32)                           # at a working size
    assert stub.calls == [("run_locked", True, info["work"], [200])] and max(info["work"]) == 32
    stub.calls.clear()
    from PIL import Image
    s.set_lock(Image.fromarray(plane))                                                # a PIL 'L' image
    assert np.array_equal(s.lock(), got)
    s.set_lock(plane > 0)                                                             # a bool array
    assert np.array_equal(s.lock(), got)
    s.set_lock(None)
    assert s.lock() is None and not s.locked
    _, _, info = s.edit(_sketch(), max_grow=0)
    assert "locked" not in info and stub.calls == [("run", True)]


def test_set_lock_refuses_other_shapes_and_types():
    from PIL import Image
    s = serve.EditSession(None, np.zeros(HW + (3,), np.uint8), backend=_Stub())
    with pytest.raises(ValueError):
        s.set_lock(np.zeros((HW[0], HW[1] + 1), np.uint8))
    with pytest.raises(ValueError):
        s.set_lock(np.zeros(HW + (3,), np.uint8))
    with pytest.raises(TypeError):
        s.set_lock(np.zeros(HW, np.float32))
    with pytest.raises(TypeError):
        s.set_lock(np.zeros(HW, np.int32))
    with pytest.raises(ValueError):
        s.set_lock(Image.new("RGB", (HW[1], HW[0])))
    assert s.lock() is None                                    # a refused lock leaves the session as it was


def test_lock_is_not_an_edit_for_the_journal():
    """set_lock between edits neither adds a journal entry nor is undone by undo()"""

    class _J(_Stub):
        def save(self, frames, origins, window_hw):
            self.calls.append(("save",))
            return [np.zeros(1, np.uint8) for _ in frames]

        def swap(self, frames, origins, window_hw, slots):
            self.calls.append(("swap",))

    s = serve.EditSession(None, np.zeros(HW + (3,), np.uint8), backend=_J(), history=2)
    s.edit(_sketch(), max_grow=0)
    plane = np.zeros(HW, np.uint8)
    plane[0, 0] = 1
    s.set_lock(plane)
    assert len(s._undo) == 1 and not s.can_redo
    s.undo()
    assert s.locked and s.lock()[0, 0] == 255
