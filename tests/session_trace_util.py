"""Session traces: random sequences of EditSession operations, run in lockstep on a session under test and on a numpy
model of it, with every byte compared after every step.  Nothing here needs a GPU.

  ModelBackend    a session backend that really edits a numpy frame.  Every frame-changing call is a statement of tests/*_util.py,
                  taken through the scripted stubs of the host tests; the pastes are the rules the GPU tests state in numpy (the hard
                  paste under a lock or keep plane, Pillow's bicubic resize back to the window, feather_util.feather_paste).  The
                  forwards cannot be computed here: `forward` is a hook that returns their result (the GPU test calls the engine on
                  the model's own frame, uncommitted); without one they return a fixed pattern.
  SnapshotOracle  undo and redo as a stack of whole-frame copies, driven by what the calls report: independent of both journals.
  make_trace      a deterministic list of plain-data steps; apply() performs one on any session.
  run_lockstep    the comparison.  replay() rebuilds the model at step k of a case."""
import functools

import numpy as np
from PIL import Image

from sketchedit_amd import serve
import select_util as U
from feather_util import feather_paste
from sketch_tiles_util import sketch_tiles
from strokes_util import spec_raster
from test_adjust_host import _Stub as _StatementStub

POOL = 8                                     # live selections a trace keeps; the oldest is dropped
FRAMES = [(120, 104), (93, 131)]             # the second: rows begin at every byte alignment, and its floored window is smaller
EDITS = ("clone_selection", "transform_selection", "filter_selection", "adjust_selection", "fill_selection", "move_selection", "edit",
         "edit_strokes")
FLIPS = (None, "h", "v", "hv")


# ---- the model ------------------------------------------------------------------------------------------------------------------------------
class _NoLog(list):
    """the stubs' call log, which a trace does not need"""

    def append(self, item):
        pass


def _resized(a, hs, ws):
    """a result at a working size back at the window: Pillow's BICUBIC, as tests/test_gpu_window_scaled.py states it"""
    return a if a.shape[:2] == (hs, ws) else np.array(Image.fromarray(np.ascontiguousarray(a)).resize((ws, hs), Image.BICUBIC))


class ModelBackend(_StatementStub):
    """The scripted backends of the host tests (select, lasso, combine, outline, move, warp, filter, adjust, save and swap: each the
    statement itself, in place on numpy arrays) with what they fake done properly: the pastes, the keep plane, and the forwards
    through `forward(entry, frames, origins, sketches, holes, locks, window_hw, work_hw, low_latency) -> (rgb, m8, counts)`."""

    def __init__(self, forward=None):
        super().__init__()
        self.calls = _NoLog()
        self.forward = forward
        self.forwards = 0

    # -- the forwards: never computed here ----------------------------------------------------------------------------------------------------
    def _forward(self, entry, frames, origins, sketches, holes, locks, window_hw, work_hw, low_latency):
        if self.forward is not None:
            return self.forward(entry, frames, origins, sketches, holes, locks, tuple(window_hw), work_hw, low_latency)
        self.forwards += 1                   # a fixed pattern, another one for every call: a paste always has something to change
        H, W = work_hw or window_hw
        yy, xx = np.mgrid[0:H, 0:W]
        rgb = np.stack([(3 * yy + 5 * xx + 70 * c + 11 * self.forwards) & 255 for c in range(3)], axis=-1).astype(np.uint8)
        inner = (yy >= 2) & (yy < H - 2) & (xx >= 2) & (xx < W - 2)
        m8 = np.where(inner & ((yy + 2 * xx) % 5 != 0), 255, 0).astype(np.uint8)
        n = len(frames)
        return np.stack([rgb] * n), np.stack([m8] * n), [[0, 0, 0, 0] for _ in range(n)]

    def run(self, frames, origins, sketches, h, w, commit, low_latency):
        rgb, m8, counts = self._forward("run", frames, origins, sketches, None, None, (h, w), None, low_latency)
        if commit:
            self.paste(frames, origins, rgb, m8)
        return rgb, m8, counts

    def run_scaled(self, frames, origins, sketches, window_hw, work_hw, commit, low_latency):
        rgb, m8, counts = self._forward("run_scaled", frames, origins, sketches, None, None, window_hw, work_hw, low_latency)
        if commit:
            self.paste_scaled(frames, origins, window_hw, rgb, m8)
        return rgb, m8, counts

    def run_locked(self, frames, origins, sketches, locks, window_hw, work_hw, commit, low_latency):
        rgb, m8, counts = self._forward("run_locked", frames, origins, sketches, None, locks, window_hw, work_hw, low_latency)
        if commit:
            self.paste_locked(frames, origins, locks, window_hw, rgb, m8)
        return rgb, m8, counts

    def run_fill(self, frames, origins, sketches, holes, locks, window_hw, work_hw, low_latency):
        return self._forward("run_fill", frames, origins, sketches, holes, locks, window_hw, work_hw, low_latency)[:2]

    # -- the pastes: the rules of tests/test_gpu_fill.py (_definition), test_gpu_lock.py and test_gpu_window_scaled.py --------------------------
    def _paste_rule(self, frames, origins, locks, window_hw, rgb, m8, radius=None):
        h, w = window_hw
        for i, (f, (y0, x0)) in enumerate(zip(frames, origins)):
            R, M = _resized(np.asarray(rgb[i]), h, w), _resized(np.asarray(m8[i]), h, w)
            lock = None if locks is None else locks[i]
            if radius:
                f[...] = feather_paste(f, (y0, x0), R, M, radius, lock=lock)
                continue
            sel = M > 0
            if lock is not None:
                sel = sel & (lock[y0:y0 + h, x0:x0 + w] == 0)
            f[y0:y0 + h, x0:x0 + w][sel] = R[sel]

    def paste(self, frames, origins, rgb, m8):
        self._paste_rule(frames, origins, None, np.asarray(m8).shape[1:3], rgb, m8)

    def paste_scaled(self, frames, origins, window_hw, rgb, m8):
        self._paste_rule(frames, origins, None, window_hw, rgb, m8)

    def paste_locked(self, frames, origins, locks, window_hw, rgb, m8):
        self._paste_rule(frames, origins, locks, window_hw, rgb, m8)

    def paste_feather(self, frames, origins, locks, window_hw, radius, rgb, m8):
        self._paste_rule(frames, origins, locks, window_hw, rgb, m8, radius)

    def fill_keep(self, frames, origins, holes, locks, window_hw):
        """255 where the hole is 0 or the lock is not (the rule of tests/test_gpu_fill.py), on the whole plane"""
        return [np.where((h == 0) | (False if locks is None or locks[i] is None else locks[i] != 0), 255, 0).astype(np.uint8)
                for i, h in enumerate(holes)]

    # -- what the chain leaves out --------------------------------------------------------------------------------------------------------------
    def tiles(self, sketch, tile):
        return sketch_tiles(sketch, tile)

    def select(self, t, idx):
        return t if list(idx) == list(range(t.shape[0])) else np.ascontiguousarray(t[list(idx)])


def make_frame(frame_hw):
    """procedural noise with a flat blob that carries a +-3 ramp (tests/test_gpu_lasso.py's _blob_frame at any size) -> (frame, a
    pixel of the blob)"""
    H, W = frame_hw
    f = U._noise(frame_hw, 7)
    yy, xx = np.mgrid[0:H, 0:W]
    cy, cx = H // 2, W // 2
    blob = (yy - cy) ** 2 * 4 + (xx - cx) ** 2 <= (W // 3) ** 2
    ramp = (U.REGION + (xx % 7) - 3).astype(np.uint8)
    f[blob] = np.stack([ramp, ramp, np.full_like(ramp, U.REGION)], axis=2)[blob]
    return f, (cy, cx)


def model_session(case, forward=None):
    return serve.EditSession(None, make_frame(case["hw"])[0], backend=ModelBackend(forward), history=case["history"],
                             history_bytes=case["history_bytes"])


# ---- the snapshot oracle -----------------------------------------------------------------------------------------------------------------------
class SnapshotOracle:
    """undo and redo as whole-frame copies.  A step that reports undoable pushes the frame from before it and clears the redo
    stack; one that reports not undoable clears both; entries leave from the old end until the depth is the session's; undo and
    redo must leave the frame equal to the popped copy.  Each entry carries a `tag` of the caller's."""

    def __init__(self):
        self.undo, self.redo = [], []

    def edited(self, before, info, depth, tag=None):
        """-> None, or what is wrong"""
        if "undoable" not in info:
            return None if not (self.undo or self.redo) else "a session without history has entries"
        self.redo.clear()
        if info["undoable"]:
            self.undo.append((before, tag))
        else:
            self.undo.clear()
        if depth > len(self.undo):
            return "the session holds %d undo entries, %d edits can be taken back" % (depth, len(self.undo))
        del self.undo[:len(self.undo) - depth]
        return None

    def exchanged(self, what, before, after):
        """an undo or redo that succeeded -> (None or what is wrong, the entry's tag)"""
        src, dst = (self.undo, self.redo) if what == "undo" else (self.redo, self.undo)
        if not src:
            return "%s succeeded with nothing to %s" % (what, what), None
        want, tag = src.pop()
        dst.append((before, tag))
        return _frame_diff(after, want, "after %s" % what, ("is", "the snapshot")), tag

    def state(self, session):
        got = (session.can_undo, session.can_redo, len(session._undo), len(session._redo))
        want = (bool(self.undo), bool(self.redo), len(self.undo), len(self.redo))
        return None if got == want else "can_undo, can_redo, undo_depth, redo_depth are %r, the snapshots say %r" % (got, want)


# ---- steps -------------------------------------------------------------------------------------------------------------------------------------
def lock_plane(frame_hw, seed):
    """the plane of a ("plane", seed) lock: two rectangles and a lattice of single pixels"""
    rng = np.random.RandomState(seed)
    H, W = frame_hw
    plane = np.zeros(frame_hw, np.uint8)
    for _ in range(2):
        y0, x0 = int(rng.randint(0, H - 8)), int(rng.randint(0, W - 8))
        plane[y0:y0 + int(rng.randint(4, H // 2)), x0:x0 + int(rng.randint(4, W // 2))] = 255
    plane[int(rng.randint(0, 9))::9, int(rng.randint(0, 7))::7] = 255
    return plane if seed % 2 else plane != 0


def stroke_sketch(strokes, frame_hw):
    """the full-size 0 / 255 sketch of polylines, by the rasteriser's rule"""
    return spec_raster(serve.stroke_segments(strokes, frame_hw)[0], frame_hw)


def _strokes(step):
    return [([tuple(p) for p in pts], width) for pts, width in step["strokes"]]


def step_selections(step):
    """the pool indices a step reads"""
    out = [step[k] for k in ("sel", "a", "b") if isinstance(step.get(k), int)]
    if isinstance(step.get("reference"), int):
        out.append(step["reference"])
    if step["kind"] == "set_lock" and step["lock"] is not None and step["lock"][0] == "selection":
        out.append(step["lock"][1])
    return out


def apply(session, step, pool, low_latency=None):
    """One step on any session.  -> dict(value, made, error): what the call returned, the Selections it made (appended to `pool`,
    whose oldest entries leave above POOL) and, for a refused step, (exception type name, message)."""
    k = step["kind"]
    kw = {key: step[key] for key in step.get("kw", ())}
    made, value = [], None
    try:
        if k == "select_lasso":
            value = session.select_lasso([[tuple(p) for p in ring] for ring in step["rings"]], grow=step["grow"])
            made = [value]
        elif k == "select_similar":
            value = session.select_similar(tuple(step["seed"]), tolerance=step["tolerance"], contiguous=step["contiguous"], grow=step["grow"])
            made = [value]
        elif k == "combine":
            value = session.combine(pool[step["a"]], pool[step["b"]], step["op"])
            made = [value]
        elif k == "invert":
            value = session.invert(pool[step["a"]])
            made = [value]
        elif k == "set_lock":
            what = step["lock"]
            session.set_lock(None if what is None else pool[what[1]] if what[0] == "selection" else lock_plane(session.frame_hw, what[1]))
        elif k == "clone_selection":
            value = session.clone_selection(pool[step["sel"]], tuple(step["offset"]), **kw)
        elif k == "move_selection":
            value = session.move_selection(pool[step["sel"]], tuple(step["offset"]), low_latency=low_latency, **kw)
        elif k == "transform_selection":
            if "offset" in kw:
                kw["offset"] = tuple(kw["offset"])
            if isinstance(kw.get("scale"), list):
                kw["scale"] = tuple(kw["scale"])
            value = session.transform_selection(pool[step["sel"]], low_latency=low_latency, **kw)
        elif k == "filter_selection":
            value = session.filter_selection(pool[step["sel"]], step["filter"], **kw)
        elif k == "adjust_selection":
            if "lut_args" in step:
                lut = serve.adjust_lut(**step["lut_args"])
                kw["lut"] = lut[0] if step.get("lut_row") else lut
            if "matrix_args" in step:
                kw["matrix"] = serve.adjust_matrix(**step["matrix_args"])
            ref = step.get("reference")
            if ref is not None:
                kw["reference"] = pool[ref] if isinstance(ref, int) else tuple(ref)
            value = session.adjust_selection(pool[step["sel"]], **kw)
        elif k == "fill_selection":
            sk = stroke_sketch(_strokes(step), session.frame_hw) if "strokes" in step else None
            value = session.fill_selection(pool[step["sel"]], sketch=sk, low_latency=low_latency, **kw)
        elif k == "edit":
            value = session.edit(stroke_sketch(_strokes(step), session.frame_hw), low_latency=low_latency, **kw)
        elif k == "edit_strokes":
            value = session.edit_strokes(_strokes(step), low_latency=low_latency, **kw)
        elif k == "histogram":
            value = session.histogram(None if step["sel"] is None else pool[step["sel"]])
        elif k == "rings":
            value = pool[step["sel"]].rings()
        elif k == "lock_rings":
            value = session.lock_rings()
        elif k in ("undo", "redo"):
            value = getattr(session, k)()
        else:
            raise KeyError(k)
    except (ValueError, TypeError, IndexError) as e:
        return dict(value=None, made=[], error=(type(e).__name__, str(e)))
    if k in ("clone_selection", "move_selection", "transform_selection"):
        made = [value[2]["selection"]]
    pool.extend(made)
    del pool[:-POOL]
    return dict(value=value, made=made, error=None)


# ---- the generator -----------------------------------------------------------------------------------------------------------------------------
EXACT_WEIGHTS = dict(select_lasso=6, select_similar=5, combine=6, invert=2, set_lock=6, clone_selection=9, transform_selection=9,
                     filter_selection=9, adjust_selection=10, histogram=2, rings=2, lock_rings=2, undo=10, redo=5)
NETWORK_WEIGHTS = dict(select_lasso=4, select_similar=4, combine=4, invert=4, set_lock=5, clone_selection=4, transform_selection=4,
                       filter_selection=4, adjust_selection=5, histogram=4, rings=4, lock_rings=4, fill_selection=7, move_selection=8,
                       transform_hole=7, edit=6, edit_strokes=6, undo=8, redo=4)


def _quarter(v):
    return float(np.floor(4.0 * v + 0.5) / 4.0)


def _offset(rng, box, frame_hw):
    """a move's offset: 0 and +-1, somewhere inside the frame, or over one of its four edges"""
    (y0, x0, y1, x1), (H, W) = box, frame_hw
    h, w = y1 - y0, x1 - x0
    mode = int(rng.randint(0, 7))
    if mode == 0:
        return [int(rng.randint(-1, 2)), int(rng.randint(-1, 2))]
    if mode in (1, 6):
        return [int(rng.randint(-y0, H - y1 + 1)), int(rng.randint(-x0, W - x1 + 1))]
    small = int(rng.randint(-3, 4))
    if mode == 2:
        return [-y0 - int(rng.randint(1, max(h, 2))), small]
    if mode == 3:
        return [H - y1 + int(rng.randint(1, max(h, 2))), small]
    if mode == 4:
        return [small, -x0 - int(rng.randint(1, max(w, 2)))]
    return [small, W - x1 + int(rng.randint(1, max(w, 2)))]


def _stroke(rng, frame_hw, at=None, reach=25):
    H, W = frame_hw
    x, y = (float(rng.randint(4, W - 4)), float(rng.randint(4, H - 4))) if at is None else at
    x1 = min(max(x + float(rng.randint(-reach, reach + 1)), 1.0), W - 1.0)
    y1 = min(max(y + float(rng.randint(-reach, reach + 1)), 1.0), H - 1.0)
    return [[[x, y], [x1, y1]], float(rng.randint(4, 11)) / 2.0]


def _window(rng, frame_hw, near):
    """a given 64 x 64 window, in the style of (3, 5, 64, 64), that holds the pixel `near`"""
    H, W = frame_hw
    return [int(min(max(near[0] - int(rng.randint(8, 56)), 0), H - 64)), int(min(max(near[1] - int(rng.randint(8, 56)), 0), W - 64)), 64, 64]


def _hole_kw(rng, frame_hw, box, step):
    """what a fill of a hole takes: a given window or the automatic one, a working size, a soft edge"""
    kw = {}
    if rng.rand() < 0.5:
        kw["window"] = _window(rng, frame_hw, ((box[0] + box[2]) // 2, (box[1] + box[3]) // 2))
    if rng.rand() < 0.3:
        kw["max_side"] = 64
    if rng.rand() < 0.3:
        kw["feather"] = 4
    step.update(kw)
    return list(kw)


def _draw(rng, kind, s, pool, seed_px, turn):
    """one step of `kind` for the session as it is now -> the descriptor (plain data), or None when the kind has nothing to work on.
    `turn(name, values)` takes the values of a short list in turn, from a start the seed chose: a set of traces meets them all."""
    H, W = hw = s.frame_hw
    live = [i for i, p in enumerate(pool) if p.box is not None]

    def pick():
        """a selection that is not empty -- now and then any, an empty one too, which the session refuses"""
        if pool and rng.rand() < 0.04:
            return int(rng.randint(0, len(pool)))
        if live and rng.rand() < 0.35:                       # the oldest: a selection several edits old is used
            return live[0]
        return live[int(rng.randint(0, len(live)))] if live else None

    if kind == "select_lasso":
        ring = [[_quarter(rng.uniform(-0.15, 1.15) * W), _quarter(rng.uniform(-0.15, 1.15) * H)] for _ in range(int(rng.randint(3, 7)))]
        return dict(kind=kind, rings=[ring], grow=int(rng.randint(0, 3)))
    if kind == "select_similar":
        seed = list(seed_px) if rng.rand() < 0.4 else [int(rng.randint(0, H)), int(rng.randint(0, W))]
        return dict(kind=kind, seed=seed, tolerance=int(rng.randint(0, 121)), contiguous=bool(rng.randint(0, 2)), grow=int(rng.randint(0, 3)))
    if kind == "lock_rings":
        return dict(kind=kind)
    if kind == "set_lock":
        r = rng.rand()
        if r < 0.2:
            return dict(kind=kind, lock=None)
        if r < 0.55 or not live:
            return dict(kind=kind, lock=["plane", int(rng.randint(0, 1 << 16))])
        return dict(kind=kind, lock=["selection", live[int(rng.randint(0, len(live)))]])
    if kind == "histogram":
        return dict(kind=kind, sel=None if not pool or rng.rand() < 0.3 else int(rng.randint(0, len(pool))))
    if kind in ("undo", "redo"):
        return dict(kind=kind) if (s.can_undo if kind == "undo" else s.can_redo) else None
    if not pool:
        return None
    if kind == "invert":
        return dict(kind=kind, a=int(rng.randint(0, len(pool))))
    if kind == "combine":
        return dict(kind=kind, a=int(rng.randint(0, len(pool))), b=int(rng.randint(0, len(pool))), op=turn("op", ["add", "subtract", "intersect", "xor"]))
    if kind == "rings":
        return dict(kind=kind, sel=int(rng.randint(0, len(pool))))
    i = pick()
    if i is None:
        return None
    box = pool[i].box or (0, 0, 16, 16)
    feather_of = lambda values: values[int(rng.randint(0, len(values)))]            # noqa: E731
    if kind in ("clone_selection", "move_selection"):
        step = dict(kind=kind, sel=i, offset=_offset(rng, box, hw), flip=turn("flip", FLIPS), kw=["flip"])
        if kind == "clone_selection":
            step["feather"] = feather_of([None, None, 1, 5, 16])
            step["kw"].append("feather")
        else:
            step["hole_grow"] = int(rng.randint(0, 5))
            step["kw"] += ["hole_grow"] + _hole_kw(rng, hw, box, step)
        return step
    if kind in ("transform_selection", "transform_hole"):
        for _ in range(6):
            scale = round(float(rng.uniform(0.5, 2.0)), 3)
            if rng.rand() < 0.25:
                scale = [scale, round(float(rng.uniform(0.5, 2.0)), 3)]
            angle = 90.0 * int(rng.randint(-3, 4)) if rng.rand() < 0.3 else round(float(rng.uniform(-180, 180)), 2)
            offset = [int(rng.randint(-40, 41)) / 2.0, int(rng.randint(-40, 41)) / 2.0]
            flip = turn("flip", FLIPS) if rng.rand() < 0.4 else None
            m = serve.warp_matrix(box, tuple(scale) if isinstance(scale, list) else scale, angle, tuple(offset), flip)
            if serve.warp_rect(box, m, hw) is not None:
                break
        if rng.rand() < 0.25:
            step = dict(kind="transform_selection", sel=i, matrix=[int(v) for v in m], kw=["matrix"])
        else:
            step = dict(kind="transform_selection", sel=i, scale=scale, angle=angle, offset=offset, flip=flip, kw=["scale", "angle", "offset", "flip"])
        step["keep_source"] = kind == "transform_selection"
        step["kw"].append("keep_source")
        if kind == "transform_hole":
            step["hole_grow"] = int(rng.randint(0, 5))
            step["kw"] += ["hole_grow"] + _hole_kw(rng, hw, box, step)
        return step
    if kind == "filter_selection":
        f = turn("filter", serve.FILTER_KINDS)
        step = dict(kind=kind, sel=i, filter=f, feather=feather_of([None, 3]), kw=["feather"])
        if f == "pixelate":
            step.update(cell=int(rng.randint(2, 21)))
            step["kw"].append("cell")
        else:
            step.update(radius=int(rng.randint(1, 13)))
            step["kw"].append("radius")
            if f != "box" and rng.rand() < 0.3:
                step.update(sigma=round(float(rng.uniform(0.5, step["radius"])), 2) if step["radius"] > 1 else 0.5)
                step["kw"].append("sigma")
            if f == "sharpen":
                step.update(amount=round(float(rng.uniform(0.3, 3.0)), 2))
                step["kw"].append("amount")
        return step
    if kind == "adjust_selection":
        form = turn("adjust", ["lut", "matrix", "levels", "equalize", "match", "rim"])
        step = dict(kind=kind, sel=i, form=form, feather=feather_of([None, 3]), kw=["feather"])
        if form == "lut":
            step["lut_args"] = dict(brightness=int(rng.randint(-80, 81)), contrast=int(rng.randint(-50, 51)), gamma=round(float(rng.uniform(0.5, 2.0)), 2),
                                    invert=bool(rng.randint(0, 2)))
            step["lut_row"] = bool(rng.randint(0, 2))
        if form == "matrix" or (form in ("lut", "equalize") and rng.rand() < 0.3):
            step["matrix_args"] = dict(saturation=round(float(rng.uniform(0.0, 2.0)), 2), hue=float(rng.randint(-180, 181)))
        if form == "matrix" or rng.rand() < 0.3:
            step.update(amount=round(float(rng.uniform(0.1, 0.95)), 2))
            step["kw"].append("amount")
        if form in ("levels", "equalize", "match", "rim"):
            step.update(auto="levels" if form == "levels" else "equalize" if form == "equalize" else "match", which=["luma", "channels"][int(rng.randint(0, 2))])
            step["kw"] += ["auto", "which"]
        if form == "levels":
            step.update(clip=int(rng.randint(0, 51)))
            step["kw"].append("clip")
        if form == "match":
            step["reference"] = live[int(rng.randint(0, len(live)))] if live else 0
        if form == "rim":
            step["reference"] = ["rim", 8]
        return step
    if kind == "fill_selection":
        step = dict(kind=kind, sel=i, kw=[])
        step["kw"] += _hole_kw(rng, hw, box, step)
        if rng.rand() < 0.3:
            step["strokes"] = [_stroke(rng, hw, (float((box[1] + box[3]) // 2), float((box[0] + box[2]) // 2)), 10)]
        return step
    raise KeyError(kind)


def _draw_sketch_step(rng, kind, s):
    H, W = hw = s.frame_hw
    if kind == "edit":
        stroke = _stroke(rng, hw)
        step = dict(kind=kind, strokes=[stroke], kw=[])
        if rng.rand() < 0.5:
            step["window"] = _window(rng, hw, (int(stroke[0][0][1]), int(stroke[0][0][0])))
            step["kw"].append("window")
    else:                                    # two short strokes in opposite corners, windows as small as the call accepts
        a = _stroke(rng, hw, (float(rng.randint(6, 16)), float(rng.randint(6, 16))), 5)
        b = _stroke(rng, hw, (float(W - rng.randint(6, 16)), float(H - rng.randint(6, 16))), 5)
        step = dict(kind=kind, strokes=[a, b], min_side=16, bucket=8, kw=["min_side", "bucket"])
    if rng.rand() < 0.3:
        step["max_side"] = 64
        step["kw"].append("max_side")
    if rng.rand() < 0.3:
        step["feather"] = 4
        step["kw"].append("feather")
    return step


def make_trace(seed, steps, frame_hw, tier, history=3, history_bytes=None):
    """A trace: `steps` plain-data descriptors (a kind, literal arguments, selections by their index in the pool), a function of
    the arguments alone.  The generator runs the model beside it, so that a step refers to selections that exist, an undo to an
    entry that is there, an offset to the box it moves; it keeps a few steps the session refuses.  `history` and `history_bytes`
    are the session's, which decide what can be undone."""
    assert tier in ("exact", "network")
    rng = np.random.RandomState(seed)
    case = dict(hw=tuple(frame_hw), history=history, history_bytes=history_bytes)
    s = model_session(case)
    seed_px = make_frame(frame_hw)[1]
    weights = EXACT_WEIGHTS if tier == "exact" else NETWORK_WEIGHTS
    kinds = sorted(weights)
    p = np.array([weights[k] for k in kinds], np.float64)
    p /= p.sum()
    pool, trace, turns = [], [], {}

    def turn(name, values):
        turns[name] = turns.get(name, seed) + 1
        return values[turns[name] % len(values)]

    while len(trace) < steps:
        if sum(q.box is not None for q in pool) < 2:
            kind = "select_lasso" if rng.rand() < 0.5 else "select_similar"
        elif trace and trace[-1]["kind"] in ("undo", "redo") and rng.rand() < 0.6:       # undo and redo come in runs: depth, and a partial undo
            kind = "undo" if rng.rand() < 0.5 else "redo"
        else:
            kind = kinds[int(rng.choice(len(kinds), p=p))]
        step = _draw_sketch_step(rng, kind, s) if kind in ("edit", "edit_strokes") else _draw(rng, kind, s, pool, seed_px, turn)
        if step is None:
            continue
        apply(s, step, pool)
        trace.append(step)
    return trace


# ---- the cases both test files run ----------------------------------------------------------------------------------------------------------------
def _cases(tier, steps, rows):
    return [dict(tier=tier, steps=steps, seed=seed, hw=FRAMES[k % 2], history=h, history_bytes=hb) for k, (seed, h, hb) in enumerate(rows)]


# window_saved_bytes(120, 104) = 38400: 20000 commits a whole-frame step unjournalled, 8000 evicts on most steps
EXACT_CASES = _cases("exact", 40, [(101, 3, None), (102, 3, 60000), (103, 1, None), (104, 3, 20000), (105, 3, 8000), (106, 0, None),
                                   (107, 3, 20000), (108, 1, 8000), (109, 3, 60000), (110, 3, 8000), (111, 1, 20000), (112, 3, None)])
NETWORK_CASES = _cases("network", 25, [(271, 3, None), (272, 3, 60000), (273, 3, 20000), (274, 1, None), (275, 3, 60000), (276, 3, 20000),
                                       (277, 3, None), (278, 1, 60000)])


def case_id(case):
    return "seed%d-%dx%d-h%d-b%s" % (case["seed"], case["hw"][0], case["hw"][1], case["history"], case["history_bytes"])


@functools.lru_cache(maxsize=None)
def _trace_of(key):
    seed, steps, hw, tier, history, history_bytes = key
    return make_trace(seed, steps, hw, tier, history, history_bytes)


def case_trace(case):
    """the case's trace, generated once (read-only: the steps are shared)"""
    return _trace_of((case["seed"], case["steps"], case["hw"], case["tier"], case["history"], case["history_bytes"]))


# ---- the comparison ----------------------------------------------------------------------------------------------------------------------------
class Mismatch(AssertionError):
    def __init__(self, context, index, step, what):
        super().__init__("%s, step %d %r: %s" % (context, index, step, what))
        self.index, self.step, self.what = index, step, what


def _frame_diff(got, want, what, names):
    if got.shape != want.shape:
        return "%s: shapes %r and %r" % (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    if bad.shape[0] == 0:
        return None
    at = tuple(int(v) for v in bad[0])
    return "%s: %d bytes differ, the first at (y, x, channel) = %r: %s %d, %s %d" % (what, bad.shape[0], at, names[0], got[at], names[1], want[at])


def _plane_of(sel):
    return np.asarray(sel._backend.download(sel.plane))


def _same(a, b, what):
    """None, or how the device's `a` and the model's `b` differ"""
    if isinstance(a, serve.Selection) or isinstance(b, serve.Selection):
        if not (isinstance(a, serve.Selection) and isinstance(b, serve.Selection)):
            return "%s: %s and %s" % (what, type(a).__name__, type(b).__name__)
        if (a.box, a.count, a.frame_hw) != (b.box, b.count, b.frame_hw):
            return "%s: box, count, frame_hw %r and %r" % (what, (a.box, a.count, a.frame_hw), (b.box, b.count, b.frame_hw))
        pa, pb = _plane_of(a), _plane_of(b)
        if pa.shape != pb.shape or not np.array_equal(pa, pb):
            return "%s: the planes differ in %d bytes" % (what, int((pa != pb).sum()) if pa.shape == pb.shape else -1)
        return None
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.asarray(a), np.asarray(b)
        if a.shape != b.shape or a.dtype != b.dtype:
            return "%s: %s %r and %s %r" % (what, a.dtype, a.shape, b.dtype, b.shape)
        if a.ndim == 3:
            return _frame_diff(a, b, what, ("the device", "the model"))
        return None if np.array_equal(a, b) else "%s: %d values differ" % (what, int((a != b).sum()))
    if isinstance(a, dict) and isinstance(b, dict):
        if sorted(a) != sorted(b):
            return "%s: keys %r and %r" % (what, sorted(a), sorted(b))
        return next((d for d in (_same(a[k], b[k], "%s[%r]" % (what, k)) for k in sorted(a)) if d), None)
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        if len(a) != len(b) or type(a) is not type(b):
            return "%s: %r and %r" % (what, a, b)
        return next((d for d in (_same(x, y, "%s[%d]" % (what, i)) for i, (x, y) in enumerate(zip(a, b))) if d), None)
    return None if type(a) is type(b) and a == b else "%s: %r and %r" % (what, a, b)


def _info_of(value):
    return value[2] if isinstance(value, tuple) and len(value) == 3 and isinstance(value[2], dict) else None


def _overlap(wins):
    return len(wins) == 2 and serve._windows_intersect(wins[0], wins[1])


def iter_lockstep(dev_session, dev_frame_reader, model, trace, context="", low_latency=None, stats=None, after=None):
    """run_lockstep as a generator that yields behind every step, so that two runs can be interleaved; its return value is
    run_lockstep's.

    Applies every step of `trace` to the session under test (`dev_session`, whose whole frame `dev_frame_reader()` returns; None:
    the model alone) and to the model session, and compares after every step: the frame, the lock plane, every Selection the step
    made, what it returned, the journal's public state; and the model against a SnapshotOracle.  A refused step must be refused
    alike and change nothing.  `stats`: a dict that counts what the trace did (on the model).  `after(index, step, pools)` runs
    behind every step.  -> the two pools.  Raises Mismatch."""
    dpool, mpool, meta = [], [], []
    oracle = SnapshotOracle()
    stats = stats if stats is not None else {}
    edits = epoch = 0                        # frame-changing steps and set_locks so far
    lock_from_selection = False

    def count(name):
        stats[name] = stats.get(name, 0) + 1

    for index, step in enumerate(trace):
        kind = step["kind"]

        def check(diff):
            if diff:
                raise Mismatch(context, index, step, diff)

        before = model.frame()
        undo_before, redo_before = len(model._undo), len(model._redo)
        used = [meta[i] for i in step_selections(step) if i < len(meta)]
        m = apply(model, step, mpool, low_latency)
        after_frame = model.frame()
        count("steps")
        if not np.array_equal(after_frame, before):
            count("the frame changed")
        count("kind "+ ("transform_hole" if kind == "transform_selection" and not step["keep_source"] else kind))
        if dev_session is not None:
            d = apply(dev_session, step, dpool, low_latency)
            check(None if d["error"] == m["error"] else "refusals: the device %r, the model %r" % (d["error"], m["error"]))
            check(_frame_diff(dev_frame_reader(), after_frame, "the frame", ("the device", "the model")))
            dl, ml = dev_session.lock(), model.lock()
            check(None if (dl is None) == (ml is None) and (dl is None or np.array_equal(dl, ml)) else "the lock planes differ")
            check(_same(d["made"], m["made"], "the selections made"))
            check(_same(d["value"], m["value"], "returned"))
            got = (dev_session.can_undo, dev_session.can_redo, len(dev_session._undo), len(dev_session._redo), dev_session.history_bytes_used)
            want = (model.can_undo, model.can_redo, len(model._undo), len(model._redo), model.history_bytes_used)
            check(None if got == want else "can_undo, can_redo, undo_depth, redo_depth, history_bytes_used: the device %r, the model %r" % (got, want))
        info = _info_of(m["value"])
        if m["error"] is not None:
            count("refused")
            check(_frame_diff(after_frame, before, "a refused step changed the frame", ("now", "before")))
        elif kind in EDITS:
            evicted = info.get("undoable") and len(model._undo) < undo_before + 1
            check(oracle.edited(before, info, len(model._undo), epoch))
            edits += 1
            if redo_before:
                count("an edit discards a redo stack")
            if evicted:
                count("eviction by history" if undo_before + 1 > model.history else "eviction by history_bytes")
            if info.get("undoable") is False and (undo_before or redo_before):
                count("an unjournalled commit clears a history")
            if info.get("undoable") and kind in ("move_selection", "transform_selection") and _overlap(info["windows"]):
                count("a _Sequence entry whose rectangles overlap")
            if info.get("undoable") and kind == "edit_strokes" and len(info["windows"]) == 2:
                count("a _Regions entry with two windows")
            if lock_from_selection and model.locked:
                count("a step under a lock set from a selection")
            if any(edits - 1 - u["born"] >= 3 for u in used):
                count("a selection at least 3 edits old is used")
            if any(u["origin"] in ("move_selection", "transform_selection", "clone_selection") for u in used):
                count("the selection of a move or transform is used")
            if kind == "filter_selection":
                count("filter " + step["filter"])
            if kind == "adjust_selection":
                count("adjust " + step["form"])
            if "flip" in step:
                count("flip %s" % step["flip"])
        elif kind in ("undo", "redo"):
            diff, tag = oracle.exchanged(kind, before, after_frame)
            check(diff)
            check(None if (info["undo_depth"], info["redo_depth"]) == (len(oracle.undo), len(oracle.redo)) else "info reports depths %r" % (info,))
            edits += 1
            if kind == "undo" and info["redo_depth"] >= 2:
                count("undo at depth 2 or more")
            if kind == "redo":
                count("a redo after an undo")
            if kind == "undo" and tag != epoch:
                count("an undo across a set_lock")
        else:
            check(_frame_diff(after_frame, before, "a step that is no edit changed the frame", ("now", "before")))
            if kind == "set_lock":
                epoch += 1
                lock_from_selection = step["lock"] is not None and step["lock"][0] == "selection"
            if kind == "combine":
                count("combine " + step["op"])
        check(oracle.state(model))
        meta.extend(dict(born=edits, origin=kind) for _ in m["made"])
        del meta[:-POOL]
        if after is not None:
            after(index, step, (dpool, mpool))
        yield index
    if dev_session is not None:              # selections are immutable: what is still in the pool is what it was made as
        for i, (a, b) in enumerate(zip(dpool, mpool)):
            diff = _same(a, b, "at the end, selection %d of the pool" % i)
            if diff:
                raise Mismatch(context, len(trace), None, diff)
    return dpool, mpool


def run_lockstep(*args, **kw):
    """iter_lockstep, run to its end -> (the pool of the session under test, the model's pool)"""
    it = iter_lockstep(*args, **kw)
    while True:
        try:
            next(it)
        except StopIteration as e:
            return e.value


def replay(case, upto, forward=None, low_latency=None):
    """the model session of `case` as it is before step `upto` of its trace -> (session, pool, the steps taken): what a failure is
    examined with, on the CPU"""
    s = model_session(case, forward)
    steps = case_trace(case)[:upto]
    _, pool = run_lockstep(None, None, s, steps, context="replay of %s" % case_id(case), low_latency=low_latency)
    return s, pool, steps
