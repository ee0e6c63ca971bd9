"""Demo-path probe: the per-request wall time of serve.process_image (demo.py:39-73) with the host steps (Pillow + torch
around the forward, device_io=False) and with the steps on the device (device_io=True), B=1, in both execution modes, at
641x481, 1283x963 and 1921x1081; plus the resize kernels' times and effective bandwidth (the bytes each pass must move:
input read once, output written once) from se_profile_report over one device-path request.  Prints one JSON line.

    python tools/serve_probe.py [--reps N] [--out FILE]

--window: the editing-session leg instead.  One process, B=1, low-latency mode, a 1921x1081 frame with a sketch
whose default window is 512x512; wall time per request ending in the download, median / min / max over --reps:
  (a) whole_frame_device_io: serve.process_image(device_io=True) on the whole frame,
  (b) whole_512_device_io:   the same whole-frame path on a 512x512 request (the window's crop),
  (c) edit_session:          serve.EditSession.edit (the frame resident, only the window's sketch up and the patch down),
plus se_profile_report's per-kernel times of one session edit.

    python tools/serve_probe.py --window [--reps N] [--out FILE]

--window-scaled: window edits at a working size, same protocol (one process, B=1, low-latency mode, wall time per
request ending in the download, own warm-up per leg, median of three rounds' medians).  A 1921x1081 frame and a sketch whose
native window is the floored frame, 1080x1920:
  (a) edit_native:        EditSession.edit(max_grow=0): one forward at 1080x1920,
  (b) edit_scaled:        EditSession.edit(max_grow=0, max_side=640): the fused ends around a forward at 360x640,
  (c) chained_entries:    the same request handled with the existing entries chained from Python: the session's own parsing of
                          the sketch (box, window, working size), then a crop copy, prepare_u8, inference_u8, two resize_u8 and
                          window_paste_u8 at the frame's resolution -- what (b) would cost without the fused ends,
  (d) edit_scaled_default_grow: edit(max_side=640) with the default grow loop (this window is the floored frame: it cannot grow),
  (e) edit_512_scale_1:   edit(max_grow=0) on the 512x512 sketch of --window (the unscaled path, which this must not slow),
and the grow loop where it does grow, on that 512x512 sketch: edit_512_default_grow (three forwards, the last at 1080x1216) and
edit_512_default_grow_scaled (the same with max_side=640); plus se_profile_report's per-kernel times of one (b) request.
(b) and (c) are checked to leave the same frame.

    python tools/serve_probe.py --window-scaled [--reps N] [--out FILE]

--window-history: the undo journal, same protocol.  On the 512x512 sketch of --window:
  (a) edit_h0:    EditSession(history=0).edit(max_grow=0) -- the session without a journal (the leg that is compared with the
                  parent commit's build, run with --window-history-parent there: only this leg, no journal call),
  (b) edit_h8:    the same with history=8 (one window_save launch in front of the committing call),
  (c) undo_redo:  undo() and redo() alternating on that session, one exchange per request,
and (d) big_edit_h0 / (e) big_edit_h8 / (f) big_undo_redo: the same three at --window-scaled's input (1080x1920 window,
max_side=640; the slot is 6.2 MB); plus se_profile_report's window_save / window_swap times and bytes.

    python tools/serve_probe.py --window-history [--reps N] [--out FILE]

--window-lock: locked regions, same protocol.  On the 512x512 sketch of --window:
  (a) edit_unlocked: EditSession.edit(max_grow=0) of a session without a lock (the leg that is compared with the parent
                     commit's build, run with --window-lock-parent there: the unlocked legs only, no lock call),
  (b) edit_locked:   the same after set_lock of a plane that locks the left half of the 512x512 window,
and (c) big_edit_unlocked / (d) big_edit_locked: the same two at --window-scaled's input (1080x1920 window, max_side=640, the
left half of the window locked); plus se_profile_report's window_* kernel times and bytes of one (b) and one (d) request.

    python tools/serve_probe.py --window-lock [--reps N] [--out FILE]

--regions: region edits, same protocol.  A 1921x1081 frame and a sketch of two 40-pixel strokes near opposite
corners, whose single window is the floored frame:
  (a) edit_one_window: EditSession.edit(max_grow=0): one forward at 1080x1920 (the leg that is compared with the parent
                       commit's build, run with --regions-parent there: only this leg, no region call),
  (b) edit_regions:    EditSession.edit_regions: the tile pass, then ONE forward with B = 2 on two 256x256 windows,
  (c) tiles_device / tiles_host: the tiles step alone -- the sketch's upload, se_sketch_tiles_u8 and the grid's download --
                       against serve.sketch_bbox plus a vectorised numpy tile pass on the host;
plus se_profile_report's per-kernel times of one (b) request.

    python tools/serve_probe.py --regions [--reps N] [--out FILE]

--strokes: strokes as polylines, same protocol.  The frame of --regions and its two 40-pixel strokes stated as
polylines (a 3-pixel brush, 20 points each, the same boxes and so the same two 256x256 windows):
  (a) edit_regions: EditSession.edit_regions of the full-size sketch the rule draws for the polylines (the leg that is compared
                    with the parent commit's build, run with --strokes-parent there: only this leg, no stroke call),
  (b) edit_strokes: EditSession.edit_strokes of the polylines: the segments' upload, ONE rasteriser call, ONE forward with B = 2,
  (c) raster_device / raster_host: the two windows' sketches alone -- the segments' upload and se_sketch_strokes_u8 (with a
                    synchronisation, which the edit does not need) -- against the numpy rule on the strokes' boxes;
plus se_profile_report's per-kernel times of one (b) request.

    python tools/serve_probe.py --strokes [--reps N] [--out FILE]

--png: patches as PNG, encoded on the device, same protocol.  A 1921x1081 frame of smooth content with a little
noise (a flat or a noise frame would flatter one encoder or the other), one edit through a fixed 512x512 window per request:
  (a) edit_then_host_png: EditSession.edit, then png_worker.png_bytes_fast of the patch on the host (the leg that is compared
                          with the parent commit's build, run with --png-parent there: only this leg, no encoder call),
  (b) edit_png:           EditSession.edit(encode="png"),
  (c) encode_device / encode_host: the encoders alone -- se_png_encode_u8 of the window with the download of its stream, against
                          the download of the window's pixels and png_bytes_fast of them;
plus the bytes each request downloads, both files' sizes, and se_profile_report's per-kernel times of one (b) request.

    python tools/serve_probe.py --png [--reps N] [--out FILE]

--jpg: patches as baseline JPEG at quality 90, encoded on the device, the same frame, window and protocol:
  (a) edit_then_host_jpg: EditSession.edit, then Pillow's encoder (quality 90, 4:4:4, standard tables) on the patch on the host
                          (the leg that is compared with the parent commit's build, run with --jpg-parent there: only this leg),
  (b) edit_jpg:           EditSession.edit(encode="jpg"),
  (c) encode_device / encode_host: the encoders alone -- se_jpg_encode_u8 of the window with the download of its segment, against
                          the download of the window's pixels and Pillow's encoder on them;
plus the bytes each request downloads, both files' sizes, the PNG's size for the same patch, the PSNR of both decoded files
against the raw patch, and se_profile_report's per-kernel times of one (b) request.

    python tools/serve_probe.py --jpg [--reps N] [--out FILE]

--jpg2: the JPEG forms of DESIGN.md 6l next to 6k's in one build, the same frame, window, quality and protocol: EditSession.edit
with encode=("jpg", 90) (edit_jpg: the leg that is compared with the parent commit's --jpg run, whose leg (b) it is),
("jpg", 90, "420"), ("jpg", 90, "444", True) and ("jpg", 90, "420", True); plus each form's file size, the bytes its request
downloads (the segment and, with per-image tables, the 1088-byte record), its PSNR against the raw patch, that Pillow decodes
the two 4:2:0 files to the same pixels, and se_profile_report's per-kernel times of one request of each form.

    python tools/serve_probe.py --jpg2 [--reps N] [--out FILE]

--feather: the feathered paste: one 512 x 512 window edit of the 1921 x 1081 frame, without and with max_side=640
(which leaves a 512 x 512 window at its own size: the scaled entry, nothing to resample), and the floored frame's window at
max_side=640 (360 x 640: the resizes run), the same protocol:
  (a) edit / edit_max_side / edit_frame_scaled: EditSession.edit(window=..., max_grow=0) without feather (the legs that are compared
                                          with the parent commit's build, run with --feather-parent there: only these legs),
  (b) the same three with _feather:       feather=8 -- the uncommitted run, (resampled) two resizes, one feather launch;
plus se_profile_report's per-kernel times of one (b) request of each kind and that feather=0 leaves the frame of (a).

    python tools/serve_probe.py --feather [--reps N] [--out FILE]

--fill: fills of a painted region, netG alone: the 512 x 512 window of --feather on the 1921 x 1081 frame and the
floored frame's window at max_side=640, the same protocol, all in one build:
  (a) edit / edit_frame_scaled: EditSession.edit(window=..., max_grow=0) (the legs that are compared with the parent commit's
                                build, run with --fill-parent there: only these legs),
  (b) fill / fill_frame_scaled: EditSession.fill of a painted disc in the same window with the same sketch -- the upload of the
                                frame-sized mask, the keep launch, the forward without netM, one locked paste;
plus se_profile_report's per-kernel times of one request of each leg and the pixels each changes.

    python tools/serve_probe.py --fill [--reps N] [--out FILE]

--select: the selection by colour: a flat-coloured disc of about 50 000 pixels on noise in the 1921 x 1081 frame,
filled through the 512 x 512 window of --fill, the same protocol, all in one build; the frame is put back (a device copy, not
timed) in front of every timed call, because a fill changes the colour under the seed:
  (a) edit:         EditSession.edit(window=..., max_grow=0), the unchanged control (run with --select-parent on the parent
                    commit's build: only this leg),
  (b) fill_similar: EditSession.fill_similar(seed, grow=2, window=...) -- state plane, flood passes, grow and tile records on the
                    device, then the fill; nothing frame-sized crosses the bus,
  (c) host_route:   session.frame() (the 6 MB download), the flood and the grow on the host (scipy.ndimage where it is installed,
                    else plain numpy), EditSession.fill(mask, window=...) (the 2 MB upload),
plus the host route's three parts timed alone, the passes the disc took, that (b) and (c) leave the same frame, and
se_profile_report's per-kernel times of one (b) request.

    python tools/serve_probe.py --select [--reps N] [--out FILE]

--lasso: lasso selections: the outline of a disc of --select's size as a polygon of 300 vertices, filled through
the 512 x 512 window of --fill, the same protocol, all in one build; the frame is put back (a device copy, not timed) in front
of every timed call:
  (a) edit:       EditSession.edit(window=..., max_grow=0), the unchanged control (run with --lasso-parent on the parent commit's
                  build: only this leg),
  (b) fill_lasso: EditSession.fill_lasso([outline], grow=2, window=...) -- the edges go up, the even-odd fill, the grow and the
                  tile records on the device, then the fill; nothing frame-sized crosses the bus,
  (c) host_route: PIL.ImageDraw.polygon into an 'L' image of the frame's size, EditSession.fill(mask, window=...) (the scan and
                  the 2 MB upload),
plus the host route's two parts timed alone, select_lasso and a combine alone, the pixels on which the two routes' masks differ
(Pillow's rule at an edge is not the header's), and se_profile_report's per-kernel times of one (b) request and of one combine.

    python tools/serve_probe.py --lasso [--reps N] [--out FILE]

--outline: the outline of a selection: --select's disc on a 1921x1081 frame, selected by colour, then outlined:
  (a) edit:         EditSession.edit(window=..., max_grow=0), the unchanged control (run with --outline-parent on the parent commit's
                    build: only this leg),
  (b) rings:        select_similar then Selection.rings() -- the boundary runs extracted on the device, 16 bytes per run come down,
                    linked into rings on the host,
  (c) mask_route:   select_similar then Selection.mask() -- the box's crop of the plane comes down -- and the rings traced from its
                    pixels on the host by tests/outline_util.spec_rings, in the same build;
plus the parts timed alone (select_similar, rings(), edges(), mask(), the two host linkings, a combine for 6p's comparison), the
bytes each route downloads, whether the two routes' rings are equal, and the in-library profile of one rings() call:
    python tools/serve_probe.py --outline [--reps N] [--out FILE]

--move: move a selection: --select's disc on a 1921x1081 frame, selected by colour once (not timed), moved by
(150, 300) with its hole filled through the 512 x 512 window of --fill; the frame is put back (a device copy, not timed) in front
of every timed call:
  (a) edit:       EditSession.edit(window=..., max_grow=0), the unchanged control (run with --move-parent on the parent commit's
                  build: only this leg),
  (b) move:       EditSession.move_selection(selection, (150, 300), window=...) -- lift, grow, fill, drop, shift and the tile
                  records on the device; the two patches come down,
  (c) host_route: session.frame() (the 6 MB download), the disc's pixels copied to the destination in numpy, a NEW session of the
                  result (the 6 MB upload), EditSession.fill(grown mask, window=...) (the 2 MB upload) -- what a front end does
                  without move_selection, and it loses the undo journal on the way,
plus the parts timed alone (fill_selection of the grown selection, a combine, clone_selection, the move with history on and its
undo), and se_profile_report's per-kernel times of one (b) request:
    python tools/serve_probe.py --move [--reps N] [--out FILE]

--warp: scale and rotate a selection: --move's frame, disc, window and offset; the frame is put back (a device copy,
not timed) in front of every timed call:
  (a) edit:               EditSession.edit(window=..., max_grow=0), the unchanged control,
  (b) move:               EditSession.move_selection(selection, (150, 300), window=...), as --move times it,
  (c) transform_identity: EditSession.transform_selection(selection, offset=(150, 300), window=...) -- the same bytes through the
                          resampling drop,
  (d) transform:          the same with scale=1.5, angle=30,
  (e) host_route:         session.frame() (the 6 MB download), the object and its mask through Pillow's Image.transform (affine,
                          bilinear) and a composite in numpy, a NEW session of the result (the 6 MB upload), EditSession.fill(grown
                          mask, window=...) -- what a front end does without transform_selection; the undo journal is lost,
plus se_profile_report's per-kernel times of one (c) and one (d) request (warp_drop, plane_warp among them):
    python tools/serve_probe.py --warp [--reps N] [--out FILE]

--filter: blur, sharpen or pixelate a selection: --move's frame, disc and window; the frame is put back (a device
copy, not timed) in front of every timed call:
  (a) edit:        EditSession.edit(window=..., max_grow=0), the unchanged control,
  (b) blur_r8:     EditSession.filter_selection(selection, "blur"), radius 8,
  (c) blur_r32:    the same at radius 32, the largest tile of LDS,
  (d) pixelate_16: filter_selection(selection, "pixelate"), cell 16,
  (e) sharpen:     filter_selection(selection, "sharpen"), radius 2, amount 1.0,
  (f) host_route:  session.frame() (the 6 MB download), PIL.ImageFilter.GaussianBlur of the selection's box composited through
                   the mask in numpy, a NEW session of the result (the 6 MB upload) -- what a front end does without
                   filter_selection; the undo journal, the lock plane and every Selection are lost,
plus se_profile_report's per-kernel times of one (b), (c) and (d) request (filter_blur, filter_mosaic, window_save among them).
--move on the parent commit's build in the same job is the comparison leg (its clone_selection: a lift, one small launch, one
patch download):
    python tools/serve_probe.py --filter [--reps N] [--out FILE]

--adjust: adjust a selection's tone and colour: --move's frame and disc; every leg but the histograms runs on the FLAT
disc (select_similar's selection: every lane of a histogram wave on one counter) and on a disc of the same size in the NOISE (a
lasso); the frame is put back (a device copy, not timed) in front of every timed call:
  (a) edit:        EditSession.edit(window=..., max_grow=0), the unchanged control,
  (b) blur_r8:     EditSession.filter_selection(selection, "blur"), radius 8 -- the leg --filter has on the parent commit's build,
  (c) manual:      EditSession.adjust_selection(selection, lut=adjust_lut(brightness=30, contrast=20), matrix=adjust_matrix(1.3)),
  (d) levels:      adjust_selection(selection, auto="levels", clip=5),
  (e) match_rim8:  adjust_selection(selection, auto="match", reference=("rim", 8)),
  (f) histogram:   EditSession.histogram(selection), the 4 KB download,
  (g) host_route:  session.frame() (the 6 MB download), the table applied through the mask in numpy, a NEW session of the result
                   (the 6 MB upload) -- what a front end does without adjust_selection; the undo journal, the lock plane and
                   every Selection are lost,
plus se_profile_report's per-kernel times of one (c), (d), (e) and (f) request (adjust, hist_tiles, hist_sum, adjust_lut, window_save
among them).  --filter on the parent commit's build in the same job is the comparison leg:
    python tools/serve_probe.py --adjust [--reps N] [--out FILE]

--blend: seamless move and clone: --move's frame, disc (253 x 253), window and offset; the frame is put back (a device
copy, outside the clock) in front of every call, each call ends in the patches' download.  Legs:
  (a) edit:             EditSession.edit(window=..., max_grow=0), the unchanged control,
  (b) clone:            EditSession.clone_selection(selection, (150, 300)), the hard drop -- the two legs --blend-parent runs on the
                        parent commit's build in the same job, before and after, for the comparison and its own spread,
  (c) clone_seamless:   clone_selection(..., blend="seamless"): the lift of the grown box, the fixed schedule, the shift,
  (d) move_seamless:    move_selection(..., window=..., blend="seamless"),
and, once under the profiler, the launches and device time of the blend kernels of (c).  The expectation to confirm or refute:
(c) costs (b) plus the device time of its small launches.
    python tools/serve_probe.py --blend [--reps N] [--out FILE]

--modify: expand, contract, border and smooth a selection: --move's frame and its disc of 49 861 pixels, selected by
colour; nothing changes the frame, every timed call ends in the download of the tile records:
  (a) combine:       EditSession.combine(selection, lasso, "subtract"), the unchanged control: one launch and the tile records,
  (b) expand_r2 / expand_r32, contract_r2 / contract_r32, smooth_r2 / smooth_r32: EditSession.modify_selection,
  (c) border_r8:     modify_selection(selection, "border", 8): two modifications, one subtraction, one download,
  (d) grow_r16:      the backend's Chebyshev grow by 16 and the tile records -- the kernel an expand is measured against,
  (e) host_route:    selection.mask() (the box's download), scipy.ndimage.binary_dilation by the disc of radius 8, the result
                     pasted into a frame-sized mask and uploaded -- what a front end does without modify_selection (no box and
                     no count come of it); only where scipy is installed,
plus se_profile_report's per-kernel times of one request of every kind (modify_disc, modify_vote, plane_combine, select_grow,
sketch_tiles).  --modify-parent runs (a) alone, with the calls a build without modifications has: the comparison leg on the parent
commit's build in the same job:
    python tools/serve_probe.py --modify [--reps N] [--out FILE]

--canvas: crop, extend, rotate and flip the canvas: the 1921 x 1081 noise frame with a lock plane; the session's frame,
size and lock plane are put back (three pointers, outside the clock) in front of every call, and every timed call ends in a
device synchronisation -- a canvas call downloads nothing.  Legs:
  (a) edit:            EditSession.edit(window=..., max_grow=0), the unchanged control -- the one leg --canvas-parent runs, with the
                       calls a build without the canvas has: the comparison leg on the parent commit's build in the same job,
  (b) orient_cw / crop / extend: orient_canvas("cw"), crop_canvas((100, 200, 800, 1400)), extend_canvas(64 on every side, "reflect"),
  (c) host_orient_cw / host_crop / host_extend: frame() and lock() (the downloads), numpy, a new EditSession and set_lock (the
      uploads) -- what a front end does without the canvas calls; the undo journal and every Selection are lost,
plus, under the profiler, the device time of canvas_turn (a quarter turn) and canvas_map (a half turn) of the same frame, their
ratio and the bytes per second each moves:
    python tools/serve_probe.py --canvas [--reps N] [--out FILE]

--seamless-fill: fills pasted through the membrane: --blend's frame, disc (253 x 253) and window; the disc's mask goes
up with every call (a fill's one upload), the frame is put back (a device copy, outside the clock) in front of every call, each
call ends in the patch's download.  Legs:
  (a) edit:                 EditSession.edit(window=..., max_grow=0), the unchanged control,
  (b) fill / fill_scaled:   EditSession.fill(mask, window=...), the hard paste, at the frame's scale and with max_side=256 -- the
                            three legs --seamless-fill-parent runs on the parent commit's build in the same job, before and after,
                            for the comparison and its own spread,
  (c) fill_seamless / fill_scaled_seamless: the same with blend="seamless": the raw forward, the lift (one resize when scaled), the
                            fixed schedule on the disc's box,
and, once under the profiler, the kernels of (c)'s two calls: the blend kernels' launches and device time, the resize's.  The
expectation to confirm or refute: (c) costs (b) plus the membrane's device time for the hole's box, plus one resize when scaled.
    python tools/serve_probe.py --seamless-fill [--reps N] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((641, 481), (1283, 963), (1921, 1081))
ARGV = ("--batchSize 1 --name celeb --joint_train_inp --dataset_mode testimage --image_dirs x --mask_dirs x "
        "--image_lists x --model editline2 --netG deepfillc2 --pool_type max --use_cam --output_dir {d} --gpu_ids 0")


def make_model(out_dir):
    import torch
    from sketchedit_amd import models, synth
    from sketchedit_amd.options.test_options import TestOptions
    opt = TestOptions().parse(ARGV.format(d=out_dir).split(), quiet=True)
    opt.isSkip = True
    m = models.create_model(opt)
    m.netG.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict("G", 0).items()})
    m.netM.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict("M", 0).items()})
    return m.eval()


def wall_ms(fn, reps):
    fn()
    fn()                                   # warm-up: plans, workspace, coefficient tables, code objects
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()                               # ends in a device-to-host copy: the request is complete
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return dict(median=round(ts[len(ts) // 2], 3), min=round(ts[0], 3), max=round(ts[-1], 3))


def window_leg(model, reps):
    """(a), (b), (c) of the module docstring"""
    import numpy as np
    from PIL import Image
    from sketchedit_amd import serve
    rng = np.random.RandomState(0)
    w, h = 1921, 1081
    frame = rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
    sk = np.zeros((h, w), np.uint8)
    sk[400:640, 800:1040] = ((rng.rand(240, 240) < 0.01) * 255).astype(np.uint8)      # 240 + 2 * 120 = 480 -> the 512 bucket
    sk[400, 800] = sk[639, 1039] = 255
    win = serve.choose_window(serve.sketch_bbox(sk), (h, w))
    assert win[2:] == (512, 512), win
    y0, x0 = win[:2]
    img, skim = Image.fromarray(frame), Image.fromarray(sk)
    img512 = Image.fromarray(np.ascontiguousarray(frame[y0:y0 + 512, x0:x0 + 512]))
    sk512 = Image.fromarray(np.ascontiguousarray(sk[y0:y0 + 512, x0:x0 + 512]))
    session = serve.EditSession(model, frame)
    legs = dict(whole_frame_device_io=lambda: serve.process_image(model, img, skim, low_latency=True, device_io=True),
                whole_512_device_io=lambda: serve.process_image(model, img512, sk512, low_latency=True, device_io=True),
                edit_session=lambda: session.edit(sk, max_grow=0, low_latency=True))
    legs["edit_session_default_grow"] = lambda: session.edit(sk, low_latency=True)     # max_grow = 2: counts read before the paste
    # three rounds over the legs, each leg timed back to back after its own warm-up (wall_ms): the first small request
    # after a 1080p one pays for the switch, which is not what a leg is about; the rounds show the run-to-run spread
    rounds = [{k: wall_ms(fn, reps) for k, fn in legs.items()} for _ in range(3)]
    out = {}
    for k in legs:
        meds = sorted(r[k]["median"] for r in rounds)
        out[k] = dict(median=meds[1], round_medians=[r[k]["median"] for r in rounds], min=min(r[k]["min"] for r in rounds),
                      max=max(r[k]["max"] for r in rounds))
    info = session.edit(sk, low_latency=True)[2]
    eng = model.engine()
    eng.profile(True)
    session.edit(sk, max_grow=0, low_latency=True)
    rep = eng.profile_report()
    eng.profile(False)
    kernels = {k["kernel"]: dict(launches=k["launches"], ms=round(k["total_ms"], 4)) for k in rep["kernels"]}
    eng.profile(True)
    legs["whole_512_device_io"]()
    rep = eng.profile_report()
    eng.profile(False)
    whole512 = round(sum(k["total_ms"] for k in rep["kernels"]), 3)
    return dict(tool="serve_probe --window", B=1, reps=reps, mode="low_latency", frame=[w, h], window=list(win),
                ms=out, default_edit_info=dict(counts=info["counts"], reruns=info["reruns"], window=list(info["window"])),
                edit_kernels_profiled=kernels, edit_kernels_total_ms=round(sum(k["ms"] for k in kernels.values()), 3), whole_512_kernels_total_ms=whole512)


def big_sketch(rng, h=1081, w=1921):
    """a sketch whose default window is the floored 1921x1081 frame"""
    import numpy as np
    sk = np.zeros((h, w), np.uint8)
    sk[200:880, 300:1620] = ((rng.rand(680, 1320) < 0.01) * 255).astype(np.uint8)
    sk[200, 300] = sk[879, 1619] = 255
    return sk


def rounds_of(legs, reps):
    """three rounds over the legs, each leg timed back to back after its own warm-up -> per leg the median of the rounds'
    medians, the rounds' medians (their spread is the run-to-run noise), min and max"""
    rounds = [{k: wall_ms(fn, reps) for k, fn in legs.items()} for _ in range(3)]
    out = {}
    for k in legs:
        meds = sorted(r[k]["median"] for r in rounds)
        out[k] = dict(median=meds[1], round_medians=[r[k]["median"] for r in rounds], min=min(r[k]["min"] for r in rounds),
                      max=max(r[k]["max"] for r in rounds))
    return out


def window_scaled_leg(model, reps, max_side=640):
    """(a) - (e) of the module docstring"""
    import numpy as np
    import torch
    from sketchedit_amd import _lib, serve
    rng = np.random.RandomState(0)
    w, h = 1921, 1081
    frame = rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
    sk512 = np.zeros((h, w), np.uint8)
    sk512[400:640, 800:1040] = ((rng.rand(240, 240) < 0.01) * 255).astype(np.uint8)
    sk512[400, 800] = sk512[639, 1039] = 255
    assert serve.choose_window(serve.sketch_bbox(sk512), (h, w))[2:] == (512, 512)
    sk = big_sketch(rng)
    y0, x0, hs, ws = win = serve.choose_window(serve.sketch_bbox(sk), (h, w))
    assert (hs, ws) == (h // 8 * 8, w // 8 * 8), win
    H, W = work = serve.choose_working_size((hs, ws), max_side)
    eng = model.engine()
    flags = _lib.flags_from_opt(model.opt)
    session = serve.EditSession(model, frame)
    chained_frame = _lib.upload_u8(frame, torch.device("cuda", eng.device))

    def chained():
        f = chained_frame
        _, bbox = session._request(sk)                 # the host side of a request, as edit() does it
        assert serve.choose_window(bbox, (h, w)) == win and serve.choose_working_size((hs, ws), max_side) == work
        crop = f[y0:y0 + hs, x0:x0 + ws].contiguous()
        sku = _lib.upload_u8(sk[y0:y0 + hs, x0:x0 + ws], f.device)
        image, s = eng.prepare_u8(crop, sku, H, W)
        rgb, m8 = eng.inference_u8(image, s, flags, low_latency=True)
        eng.window_paste_u8([f], [(y0, x0)], eng.resize_u8(rgb, (hs, ws)), eng.resize_u8(m8, (hs, ws)))
        return f[y0:y0 + hs, x0:x0 + ws].contiguous().cpu().numpy()

    # (b) and (c) compute the same thing: one request each on a fresh frame
    check = serve.EditSession(model, frame)
    same = bool(np.array_equal(check.edit(sk, max_grow=0, low_latency=True, max_side=max_side)[0], chained()))
    chained_frame.copy_(_lib.upload_u8(frame, chained_frame.device))
    legs = dict(edit_native=lambda: session.edit(sk, max_grow=0, low_latency=True),
                edit_scaled=lambda: session.edit(sk, max_grow=0, low_latency=True, max_side=max_side),
                chained_entries=chained,
                edit_scaled_default_grow=lambda: session.edit(sk, low_latency=True, max_side=max_side),
                edit_512_scale_1=lambda: session.edit(sk512, max_grow=0, low_latency=True),
                edit_512_default_grow=lambda: session.edit(sk512, low_latency=True),
                edit_512_default_grow_scaled=lambda: session.edit(sk512, low_latency=True, max_side=max_side))
    out = rounds_of(legs, reps)
    info = session.edit(sk, low_latency=True, max_side=max_side)[2]
    info512 = session.edit(sk512, low_latency=True, max_side=max_side)[2]
    eng.profile(True)
    session.edit(sk, max_grow=0, low_latency=True, max_side=max_side)
    rep = eng.profile_report()
    eng.profile(False)
    kernels = {k["kernel"]: dict(launches=k["launches"], ms=round(k["total_ms"], 4), bytes=int(k["bytes"])) for k in rep["kernels"]}
    return dict(tool="serve_probe --window-scaled", B=1, reps=reps, mode="low_latency", frame=[w, h], window=list(win), work=list(work),
                max_side=max_side, ms=out, scaled_equals_chained=same,
                speedup_native_over_scaled=round(out["edit_native"]["median"] / out["edit_scaled"]["median"], 2),
                default_edit_info=dict(counts=info["counts"], reruns=info["reruns"], window=list(info["window"]), work=list(info["work"])),
                default_edit_512_info=dict(counts=info512["counts"], reruns=info512["reruns"], window=list(info512["window"]), work=list(info512["work"])),
                scaled_edit_kernels_profiled=kernels, scaled_edit_kernels_total_ms=round(sum(k["ms"] for k in kernels.values()), 3))


def window_history_leg(model, reps, parent=False, max_side=640):
    """(a) - (f) of the module docstring; parent=True: legs (a) and (d) only, with the calls a build without the journal has"""
    import numpy as np
    from sketchedit_amd import serve
    rng = np.random.RandomState(0)
    w, h = 1921, 1081
    frame = rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
    sk512 = np.zeros((h, w), np.uint8)
    sk512[400:640, 800:1040] = ((rng.rand(240, 240) < 0.01) * 255).astype(np.uint8)
    sk512[400, 800] = sk512[639, 1039] = 255
    assert serve.choose_window(serve.sketch_bbox(sk512), (h, w))[2:] == (512, 512)
    big = big_sketch(rng)
    s0 = serve.EditSession(model, frame)
    legs = dict(edit_h0=lambda: s0.edit(sk512, max_grow=0, low_latency=True),
                big_edit_h0=lambda: s0.edit(big, max_grow=0, low_latency=True, max_side=max_side))
    if not parent:
        s8, b8 = serve.EditSession(model, frame, history=8), serve.EditSession(model, frame, history=8)
        s8.edit(sk512, max_grow=0, low_latency=True)
        b8.edit(big, max_grow=0, low_latency=True, max_side=max_side)

        def flip(s):
            return s.undo() if s.can_undo else s.redo()
        legs.update(edit_h8=lambda: s8.edit(sk512, max_grow=0, low_latency=True), undo_redo=lambda: flip(u8),
                    big_edit_h8=lambda: b8.edit(big, max_grow=0, low_latency=True, max_side=max_side),
                    big_undo_redo=lambda: flip(ub))
        u8, ub = serve.EditSession(model, frame, history=1), serve.EditSession(model, frame, history=1)
        u8.edit(sk512, max_grow=0, low_latency=True)
        ub.edit(big, max_grow=0, low_latency=True, max_side=max_side)
    out = dict(tool="serve_probe --window-history" + ("-parent" if parent else ""), B=1, reps=reps, mode="low_latency",
               frame=[w, h], max_side=max_side, ms=rounds_of(legs, reps))
    if not parent:
        eng = model.engine()
        prof = {}
        for tag, s, sk, kw in (("512", s8, sk512, {}), ("big", b8, big, dict(max_side=max_side))):
            eng.profile(True)
            s.edit(sk, max_grow=0, low_latency=True, **kw)
            s.undo()
            rep = eng.profile_report()
            eng.profile(False)
            prof[tag] = {k["kernel"]: dict(launches=k["launches"], ms=round(k["total_ms"], 4), bytes=int(k["bytes"]))
                         for k in rep["kernels"] if k["kernel"].startswith("window_")}
            prof[tag]["all_kernels_ms"] = round(sum(k["total_ms"] for k in rep["kernels"]), 3)
        out.update(journal_kernels_profiled=prof, slot_bytes={"512": serve.window_saved_bytes(512, 512),
                                                               "big": serve.window_saved_bytes(1080, 1920)})
    return out


def window_lock_leg(model, reps, parent=False, max_side=640):
    """(a) - (d) of the module docstring; parent=True: legs (a) and (c) only, with the calls a build without locks has"""
    import numpy as np
    from sketchedit_amd import serve
    rng = np.random.RandomState(0)
    w, h = 1921, 1081
    frame = rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
    sk512 = np.zeros((h, w), np.uint8)
    sk512[400:640, 800:1040] = ((rng.rand(240, 240) < 0.01) * 255).astype(np.uint8)
    sk512[400, 800] = sk512[639, 1039] = 255
    win512 = serve.choose_window(serve.sketch_bbox(sk512), (h, w))
    assert win512[2:] == (512, 512)
    big = big_sketch(rng)
    winbig = serve.choose_window(serve.sketch_bbox(big), (h, w))
    s0 = serve.EditSession(model, frame)
    legs = dict(edit_unlocked=lambda: s0.edit(sk512, max_grow=0, low_latency=True),
                big_edit_unlocked=lambda: s0.edit(big, max_grow=0, low_latency=True, max_side=max_side))
    if not parent:
        def half(win):
            lk = np.zeros((h, w), np.uint8)
            lk[win[0]:win[0] + win[2], win[1]:win[1] + win[3] // 2] = 255
            return lk
        sl, bl = serve.EditSession(model, frame), serve.EditSession(model, frame)
        sl.set_lock(half(win512))
        bl.set_lock(half(winbig))
        legs.update(edit_locked=lambda: sl.edit(sk512, max_grow=0, low_latency=True),
                    big_edit_locked=lambda: bl.edit(big, max_grow=0, low_latency=True, max_side=max_side))
    out = dict(tool="serve_probe --window-lock" + ("-parent" if parent else ""), B=1, reps=reps, mode="low_latency",
               frame=[w, h], max_side=max_side, ms=rounds_of(legs, reps))
    if not parent:
        eng = model.engine()
        prof = {}
        for tag, s, sk, kw in (("512", sl, sk512, {}), ("big", bl, big, dict(max_side=max_side))):
            eng.profile(True)
            s.edit(sk, max_grow=0, low_latency=True, **kw)
            rep = eng.profile_report()
            eng.profile(False)
            prof[tag] = {k["kernel"]: dict(launches=k["launches"], ms=round(k["total_ms"], 4), bytes=int(k["bytes"]))
                         for k in rep["kernels"] if k["kernel"].startswith("window_")}
            prof[tag]["all_kernels_ms"] = round(sum(k["total_ms"] for k in rep["kernels"]), 3)
            locked = s.lock() > 0
            prof[tag]["locked_pixels_unchanged"] = bool(np.array_equal(s.frame()[locked], frame[locked]))
        out.update(lock_kernels_profiled=prof)
    return out


def host_tiles(sk, tile):
    """the tile records of serve.split_regions from a host array, vectorised numpy (what a host-only policy would run)"""
    import numpy as np
    Hi, Wi = sk.shape
    nty, ntx = -(-Hi // tile), -(-Wi // tile)
    p = np.zeros((nty * tile, ntx * tile), bool)
    p[:Hi, :Wi] = sk > 0
    b = p.reshape(nty, tile, ntx, tile)
    n = b.sum((1, 3), dtype=np.int32)
    rows, cols = b.any(3), b.any(1)                            # (nty, tile, ntx), (nty, ntx, tile)
    oy, ox = (np.arange(nty) * tile)[:, None], (np.arange(ntx) * tile)[None, :]
    rec = np.stack([n, oy + rows.argmax(1), ox + cols.argmax(2), oy + tile - rows[:, ::-1].argmax(1), ox + tile - cols[:, :, ::-1].argmax(2)], -1)
    return np.where(n[..., None] > 0, rec, 0).astype(np.int32)


def regions_leg(model, reps, parent=False, tile=32):
    """(a) - (c) of the module docstring; parent=True: leg (a) only, with the calls a build without region edits has"""
    import numpy as np
    from sketchedit_amd import serve
    rng = np.random.RandomState(0)
    w, h = 1921, 1081
    frame = rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
    sk = np.zeros((h, w), np.uint8)
    sk[30:70, 30:70] = ((rng.rand(40, 40) < 0.2) * 255).astype(np.uint8)
    sk[1000:1040, 1850:1890] = ((rng.rand(40, 40) < 0.2) * 255).astype(np.uint8)
    sk[30, 30] = sk[69, 69] = sk[1000, 1850] = sk[1039, 1889] = 255
    win = serve.choose_window(serve.sketch_bbox(sk), (h, w))
    assert win == (0, 0, 1080, 1920), win
    s1 = serve.EditSession(model, frame)
    legs = dict(edit_one_window=lambda: s1.edit(sk, max_grow=0, low_latency=True))
    out = dict(tool="serve_probe --regions" + ("-parent" if parent else ""), B=1, reps=reps, mode="low_latency", frame=[w, h],
               one_window=list(win))
    if not parent:
        s2 = serve.EditSession(model, frame)
        be = s2.backend

        def tiles_device():
            return be.tiles(be.upload(sk), tile)

        def tiles_host():
            return serve.sketch_bbox(sk), host_tiles(sk, tile)
        assert np.array_equal(tiles_device(), tiles_host()[1])
        legs.update(edit_regions=lambda: s2.edit_regions(sk, low_latency=True, tile=tile), tiles_device=tiles_device, tiles_host=tiles_host)
    out["ms"] = rounds_of(legs, reps)
    if not parent:
        info = s2.edit_regions(sk, low_latency=True, tile=tile)[2]
        eng = model.engine()
        eng.profile(True)
        s2.edit_regions(sk, low_latency=True, tile=tile)
        rep = eng.profile_report()
        eng.profile(False)
        kernels = {k["kernel"]: dict(launches=k["launches"], ms=round(k["total_ms"], 4)) for k in rep["kernels"]}
        out.update(tile=tile, windows=[list(v) for v in info["windows"]], groups=info["groups"], counts=info["counts"],
                   speedup_one_window_over_regions=round(out["ms"]["edit_one_window"]["median"] / out["ms"]["edit_regions"]["median"], 2),
                   regions_kernels_profiled=kernels, regions_kernels_total_ms=round(sum(k["ms"] for k in kernels.values()), 3))
    return out


def probe_strokes():
    """the two strokes of --regions as polylines: zigzags inside [31.5, 68.5]^2 and [1001.5, 1038.5] x [1851.5, 1888.5] at a
    3-pixel brush, so that their boxes are the 40-pixel boxes of --regions"""
    out = []
    for y0, x0 in ((30, 30), (1000, 1850)):
        pts = [(x0 + 1.5 + 37.0 * (i % 2 if i % 4 < 2 else 1 - i % 2) * 0.6 + 37.0 * 0.4 * i / 19.0, y0 + 1.5 + 37.0 * i / 19.0) for i in range(20)]
        pts[0], pts[-1] = (x0 + 1.5, y0 + 1.5), (x0 + 38.5, y0 + 38.5)
        out.append((pts, 3.0))
    return out


def host_segments(strokes):
    """serve.stroke_segments without the checks and the clamp (the probe's strokes need neither): also runs on a build without it"""
    import numpy as np
    segs = []
    for pts, width in strokes:
        q = np.floor(4.0 * np.asarray(pts, np.float64) + 0.5).astype(np.int64)
        r = int(np.floor(2.0 * width + 0.5))
        segs += [[q[i, 0], q[i, 1], q[i + 1, 0], q[i + 1, 1], r] for i in range(len(q) - 1)]
    return np.asarray(segs, np.int32)


def host_raster(segs, hw):
    """the rule of DESIGN.md 6i in numpy int64, each segment over its own box only (what a host-only front end would run)"""
    import numpy as np
    sk = np.zeros(hw, np.uint8)
    for ax, ay, bx, by, r in np.asarray(segs, np.int64):
        y0, y1 = max((min(ay, by) - r - 2 + 3) // 4, 0), min((max(ay, by) + r - 2) // 4 + 1, hw[0])
        x0, x1 = max((min(ax, bx) - r - 2 + 3) // 4, 0), min((max(ax, bx) + r - 2) // 4 + 1, hw[1])
        px, py = (4 * np.arange(x0, x1) + 2)[None, :], (4 * np.arange(y0, y1) + 2)[:, None]
        dx, dy, ex, ey = bx - ax, by - ay, px - ax, py - ay
        t, dd, cr = ex * dx + ey * dy, dx * dx + dy * dy, ex * dy - ey * dx
        hit = np.where(t <= 0, ex * ex + ey * ey <= r * r, np.where(t >= dd, (ex - dx) ** 2 + (ey - dy) ** 2 <= r * r, cr * cr <= r * r * dd))
        sk[y0:y1, x0:x1][hit] = 255
    return sk


def strokes_leg(model, reps, parent=False, tile=32):
    """(a) - (c) of the module docstring; parent=True: leg (a) only, with the calls a build without stroke edits has"""
    import numpy as np
    import torch
    from sketchedit_amd import serve
    rng = np.random.RandomState(0)
    w, h = 1921, 1081
    frame = rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
    strokes = probe_strokes()
    segs = host_segments(strokes)
    sk = host_raster(segs, (h, w))
    s1 = serve.EditSession(model, frame)
    legs = dict(edit_regions=lambda: s1.edit_regions(sk, low_latency=True, tile=tile))
    out = dict(tool="serve_probe --strokes" + ("-parent" if parent else ""), B=1, reps=reps, mode="low_latency", frame=[w, h],
               segments=int(len(segs)), sketch_pixels=int((sk > 0).sum()))
    if not parent:
        assert np.array_equal(serve.stroke_segments(strokes, (h, w))[0], segs)
        s2 = serve.EditSession(model, frame)
        be = s2.backend
        wins = s1.edit_regions(sk, low_latency=True, tile=tile)[2]["windows"]

        def raster_device():
            crops = be.strokes(be.upload(segs), (h, w), wins)
            torch.cuda.synchronize()
            return crops
        whole = be.strokes(be.upload(segs), (h, w), [(0, 0, h, w)])[0].cpu().numpy()
        assert np.array_equal(whole, sk)                     # the device's whole-frame raster is the numpy rule's
        legs.update(edit_strokes=lambda: s2.edit_strokes(strokes, low_latency=True), raster_device=raster_device,
                    raster_host=lambda: host_raster(segs, (h, w)))
    out["ms"] = rounds_of(legs, reps)
    info = s1.edit_regions(sk, low_latency=True, tile=tile)[2]
    out.update(regions_windows=[list(v) for v in info["windows"]])
    if not parent:
        s3, s4 = serve.EditSession(model, frame), serve.EditSession(model, frame)
        s3.edit_regions(sk, low_latency=True, tile=tile)
        info = s4.edit_strokes(strokes, low_latency=True)[2]
        eng = model.engine()
        eng.profile(True)
        s2.edit_strokes(strokes, low_latency=True)
        rep = eng.profile_report()
        eng.profile(False)
        kernels = {k["kernel"]: dict(launches=k["launches"], ms=round(k["total_ms"], 4)) for k in rep["kernels"]}
        out.update(windows=[list(v) for v in info["windows"]], groups=info["groups"], counts=info["counts"],
                   frames_identical=bool(np.array_equal(s3.frame(), s4.frame())),
                   regions_minus_strokes_ms=round(out["ms"]["edit_regions"]["median"] - out["ms"]["edit_strokes"]["median"], 3),
                   strokes_kernels_profiled=kernels, strokes_kernels_total_ms=round(sum(k["ms"] for k in kernels.values()), 3))
    return out


def png_leg(model, reps, parent=False, side=512):
    """(a) - (c) of the module docstring; parent=True: leg (a) only, with the calls a build without the encoder has"""
    import io
    import numpy as np
    from PIL import Image
    from sketchedit_amd import png_worker, serve
    rng = np.random.RandomState(0)
    w, h = 1921, 1081
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([96 + 64 * np.sin(xx / 97.0) + 48 * np.cos(yy / 61.0), 128 + 90 * np.sin((xx + yy) / 143.0),
                     110 + 70 * np.cos(xx / 53.0) * np.sin(yy / 77.0)], axis=2)
    frame = np.clip(base + rng.randint(-2, 3, (h, w, 3)), 0, 255).astype(np.uint8)
    win = (283, 705, side, side)
    sk = np.zeros((h, w), np.uint8)
    sk[win[0] + 200:win[0] + 240, win[1] + 250:win[1] + 256] = 255
    s1 = serve.EditSession(model, frame)
    edit = lambda s, **kw: s.edit(sk, window=win, max_grow=0, low_latency=True, **kw)      # noqa: E731
    legs = dict(edit_then_host_png=lambda: png_worker.png_bytes_fast(edit(s1)[0]))
    out = dict(tool="serve_probe --png" + ("-parent" if parent else ""), B=1, reps=reps, mode="low_latency", frame=[w, h],
               window=list(win), raw_bytes_downloaded=side * side * 3)
    if not parent:
        s2 = serve.EditSession(model, frame)
        be = s2.backend
        legs.update(edit_png=lambda: edit(s2, encode="png"), encode_device=lambda: be.crop_png([s2._frame], [win]),
                    encode_host=lambda: png_worker.png_bytes_fast(be.crop(s2._frame, *win)))
    out["ms"] = rounds_of(legs, reps)
    patch = edit(s1)[0]
    out.update(host_png_bytes=len(png_worker.png_bytes_fast(patch)))
    if not parent:
        s3, s4 = serve.EditSession(model, frame), serve.EditSession(model, frame)
        raw, png = edit(s3)[0], edit(s4, encode="png")[0]
        eng = model.engine()
        eng.profile(True)
        edit(s2, encode="png")
        rep = eng.profile_report()
        eng.profile(False)
        kernels = {k["kernel"]: dict(launches=k["launches"], ms=round(k["total_ms"], 4)) for k in rep["kernels"] if k["kernel"].startswith("png_")}
        framing = len(serve.png_from_zlib(b"", side, side))
        out.update(device_png_bytes=len(png), png_bytes_downloaded=len(png) - framing, png_kernels_profiled=kernels,
                   decodes_to_the_raw_patch=bool(np.array_equal(np.asarray(Image.open(io.BytesIO(png))), raw)),
                   frames_identical=bool(np.array_equal(s3.frame(), s4.frame())),
                   host_minus_device_request_ms=round(out["ms"]["edit_then_host_png"]["median"] - out["ms"]["edit_png"]["median"], 3))
    return out


def jpg_leg(model, reps, parent=False, side=512, quality=90):
    """(a) - (c) of the module docstring; parent=True: leg (a) only, with the calls a build without the encoder has"""
    import io
    import numpy as np
    from PIL import Image
    from sketchedit_amd import serve
    rng = np.random.RandomState(0)
    w, h = 1921, 1081
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([96 + 64 * np.sin(xx / 97.0) + 48 * np.cos(yy / 61.0), 128 + 90 * np.sin((xx + yy) / 143.0),
                     110 + 70 * np.cos(xx / 53.0) * np.sin(yy / 77.0)], axis=2)
    frame = np.clip(base + rng.randint(-2, 3, (h, w, 3)), 0, 255).astype(np.uint8)
    win = (283, 705, side, side)
    sk = np.zeros((h, w), np.uint8)
    sk[win[0] + 200:win[0] + 240, win[1] + 250:win[1] + 256] = 255

    def host_jpg(a):
        f = io.BytesIO()
        Image.fromarray(a).save(f, format="JPEG", quality=quality, subsampling=0, optimize=False)
        return f.getvalue()

    def psnr(data, a):
        d = np.asarray(Image.open(io.BytesIO(data))).astype(np.float64) - a
        return round(float(10 * np.log10(255.0 ** 2 / np.mean(d ** 2))), 3)
    s1 = serve.EditSession(model, frame)
    edit = lambda s, **kw: s.edit(sk, window=win, max_grow=0, low_latency=True, **kw)      # noqa: E731
    legs = dict(edit_then_host_jpg=lambda: host_jpg(edit(s1)[0]))
    out = dict(tool="serve_probe --jpg" + ("-parent" if parent else ""), B=1, reps=reps, mode="low_latency", frame=[w, h],
               window=list(win), quality=quality, raw_bytes_downloaded=side * side * 3)
    if not parent:
        s2 = serve.EditSession(model, frame)
        be = s2.backend
        legs.update(edit_jpg=lambda: edit(s2, encode=("jpg", quality)), encode_device=lambda: be.crop_jpg([s2._frame], [win], quality),
                    encode_host=lambda: host_jpg(be.crop(s2._frame, *win)))
    out["ms"] = rounds_of(legs, reps)
    patch = edit(s1)[0]
    out.update(host_jpg_bytes=len(host_jpg(patch)), host_jpg_psnr=psnr(host_jpg(patch), patch))
    if not parent:
        s3, s4 = serve.EditSession(model, frame), serve.EditSession(model, frame)
        raw, jpg = edit(s3)[0], edit(s4, encode=("jpg", quality))[0]
        eng = model.engine()
        eng.profile(True)
        edit(s2, encode=("jpg", quality))
        rep = eng.profile_report()
        eng.profile(False)
        kernels = {k["kernel"]: dict(launches=k["launches"], ms=round(k["total_ms"], 4)) for k in rep["kernels"] if k["kernel"].startswith("jpg_")}
        headers = len(serve.jpg_from_scan(b"", side, side, quality))
        out.update(device_jpg_bytes=len(jpg), jpg_bytes_downloaded=len(jpg) - headers, jpg_kernels_profiled=kernels,
                   device_png_bytes=len(be.crop_png([s4._frame], [win])[0]), device_jpg_psnr=psnr(jpg, raw),
                   frames_identical=bool(np.array_equal(s3.frame(), s4.frame())),
                   host_minus_device_request_ms=round(out["ms"]["edit_then_host_jpg"]["median"] - out["ms"]["edit_jpg"]["median"], 3))
    return out


def jpg2_leg(model, reps, side=512, quality=90):
    """the four forms of the module docstring"""
    import io
    import numpy as np
    from PIL import Image
    from sketchedit_amd import serve
    rng = np.random.RandomState(0)
    w, h = 1921, 1081
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([96 + 64 * np.sin(xx / 97.0) + 48 * np.cos(yy / 61.0), 128 + 90 * np.sin((xx + yy) / 143.0),
                     110 + 70 * np.cos(xx / 53.0) * np.sin(yy / 77.0)], axis=2)
    frame = np.clip(base + rng.randint(-2, 3, (h, w, 3)), 0, 255).astype(np.uint8)
    win = (283, 705, side, side)
    sk = np.zeros((h, w), np.uint8)
    sk[win[0] + 200:win[0] + 240, win[1] + 250:win[1] + 256] = 255
    forms = dict(edit_jpg=("jpg", quality), edit_jpg_420=("jpg", quality, "420"), edit_jpg_444_opt=("jpg", quality, "444", True),
                 edit_jpg_420_opt=("jpg", quality, "420", True))

    def pixels(data):
        return np.asarray(Image.open(io.BytesIO(data))).astype(np.float64)

    def scan_bytes(data):
        """the bytes between the SOS segment and EOI: what the device wrote"""
        i = 2
        while data[i + 1] != 0xDA:
            i += 2 + ((data[i + 2] << 8) | data[i + 3])
        return len(data) - (i + 2 + ((data[i + 2] << 8) | data[i + 3])) - 2
    edit = lambda s, **kw: s.edit(sk, window=win, max_grow=0, low_latency=True, **kw)      # noqa: E731
    sessions = {k: serve.EditSession(model, frame) for k in forms}
    out = dict(tool="serve_probe --jpg2", B=1, reps=reps, mode="low_latency", frame=[w, h], window=list(win), quality=quality,
               raw_bytes_downloaded=side * side * 3)
    out["ms"] = rounds_of({k: (lambda k=k: edit(sessions[k], encode=forms[k])) for k in forms}, reps)
    raw = edit(serve.EditSession(model, frame))[0]
    eng = model.engine()
    files = {}
    for k, form in forms.items():
        s = serve.EditSession(model, frame)
        files[k] = edit(s, encode=form)[0]
        eng.profile(True)
        edit(sessions[k], encode=form)
        rep = eng.profile_report()
        eng.profile(False)
        kernels = {r["kernel"]: dict(launches=r["launches"], ms=round(r["total_ms"], 4)) for r in rep["kernels"] if r["kernel"].startswith("jpg")}
        out[k] = dict(file_bytes=len(files[k]), bytes_downloaded=scan_bytes(files[k]) + (1088 if len(form) > 3 and form[3] else 0),
                      kernels_profiled=kernels, kernels_total_ms=round(sum(v["ms"] for v in kernels.values()), 4),
                      psnr=round(float(10 * np.log10(255.0 ** 2 / np.mean((pixels(files[k]) - raw) ** 2))), 3),
                      ratio_to_edit_jpg=round(len(files[k]) / len(files["edit_jpg"]), 4),
                      frame_identical=bool(np.array_equal(s.frame(), sessions["edit_jpg"].frame())))
    out.update(decoded_420_equal_with_and_without_tables=bool(np.array_equal(pixels(files["edit_jpg_420"]), pixels(files["edit_jpg_420_opt"]))),
               decoded_444_equal_with_and_without_tables=bool(np.array_equal(pixels(files["edit_jpg"]), pixels(files["edit_jpg_444_opt"]))),
               table_record_bytes_downloaded=1088)
    for k in forms:
        out[k]["minus_edit_jpg_ms"] = round(out["ms"][k]["median"] - out["ms"]["edit_jpg"]["median"], 3)
    return out


def feather_leg(model, reps, parent=False, side=512, radius=8, max_side=640):
    """(a), (b) of the module docstring; parent=True: the legs (a) only, with the calls a build without the feathered paste has"""
    import numpy as np
    from sketchedit_amd import serve
    rng = np.random.RandomState(0)
    w, h = 1921, 1081
    frame = rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
    win = (283, 705, side, side)
    sk = np.zeros((h, w), np.uint8)
    sk[win[0] + 200:win[0] + 240, win[1] + 250:win[1] + 256] = 255
    big = (0, 0, h // 8 * 8, w // 8 * 8)
    bsk = big_sketch(rng)
    s1, s2 = serve.EditSession(model, frame), serve.EditSession(model, frame)
    edit = lambda s, **kw: s.edit(sk, window=win, max_grow=0, low_latency=True, **kw)                            # noqa: E731
    edit_big = lambda s, **kw: s.edit(bsk, window=big, max_grow=0, low_latency=True, max_side=max_side, **kw)     # noqa: E731
    s5 = serve.EditSession(model, frame)
    legs = dict(edit=lambda: edit(s1), edit_max_side=lambda: edit(s5, max_side=max_side), edit_frame_scaled=lambda: edit_big(s2))
    out = dict(tool="serve_probe --feather" + ("-parent" if parent else ""), B=1, reps=reps, mode="low_latency", frame=[w, h],
               window=list(win), scaled_window=list(big), max_side=max_side)
    if not parent:
        s3, s4, s6 = serve.EditSession(model, frame), serve.EditSession(model, frame), serve.EditSession(model, frame)
        legs.update(edit_feather=lambda: edit(s3, feather=radius), edit_max_side_feather=lambda: edit(s6, max_side=max_side, feather=radius),
                    edit_frame_scaled_feather=lambda: edit_big(s4, feather=radius))
    out["ms"] = rounds_of(legs, reps)
    if not parent:
        eng = model.engine()
        kernels = {}
        for name in ("edit_feather", "edit_frame_scaled_feather"):
            eng.profile(True)
            legs[name]()
            rep = eng.profile_report()
            eng.profile(False)
            kernels[name] = {k["kernel"]: dict(launches=k["launches"], ms=round(k["total_ms"], 4)) for k in rep["kernels"]
                             if k["kernel"].startswith(("window_", "resize_"))}
        a, b, c = serve.EditSession(model, frame), serve.EditSession(model, frame), serve.EditSession(model, frame)
        edit(a), edit(b, feather=0), edit(c, feather=radius)
        fa, fb, fc = a.frame(), b.frame(), c.frame()
        out.update(radius=radius, work=list(edit_big(s4, feather=radius)[2]["work"]), window_kernels_profiled=kernels,
                   feather_0_is_the_hard_paste=bool(np.array_equal(fa, fb)),
                   pixels_changed=dict(hard=int((fa != frame).any(2).sum()), feather=int((fc != frame).any(2).sum()),
                                       differ=int((fa != fc).any(2).sum())),
                   feather_minus_hard_ms={k: round(out["ms"][k + "_feather"]["median"] - out["ms"][k]["median"], 3)
                                          for k in ("edit", "edit_max_side", "edit_frame_scaled")})
    return out


def fill_leg(model, reps, parent=False, side=512, max_side=640):
    """(a), (b) of the module docstring; parent=True: the legs (a) only, with the calls a build without fills has"""
    import numpy as np
    from sketchedit_amd import serve
    rng = np.random.RandomState(0)
    w, h = 1921, 1081
    frame = rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
    win = (283, 705, side, side)
    sk = np.zeros((h, w), np.uint8)
    sk[win[0] + 200:win[0] + 240, win[1] + 250:win[1] + 256] = 255
    big = (0, 0, h // 8 * 8, w // 8 * 8)
    bsk = big_sketch(rng)
    yy, xx = np.mgrid[0:h, 0:w]
    disc = ((yy - (win[0] + side // 2)) ** 2 + (xx - (win[1] + side // 2)) ** 2 <= (side // 4) ** 2).astype(np.uint8) * 255
    big_disc = ((yy - h // 2) ** 2 + (xx - w // 2) ** 2 <= (h // 4) ** 2).astype(np.uint8) * 255
    s1, s2 = serve.EditSession(model, frame), serve.EditSession(model, frame)
    legs = dict(edit=lambda: s1.edit(sk, window=win, max_grow=0, low_latency=True),
                edit_frame_scaled=lambda: s2.edit(bsk, window=big, max_grow=0, low_latency=True, max_side=max_side))
    out = dict(tool="serve_probe --fill" + ("-parent" if parent else ""), B=1, reps=reps, mode="low_latency", frame=[w, h],
               window=list(win), scaled_window=list(big), max_side=max_side)
    if not parent:
        s3, s4 = serve.EditSession(model, frame), serve.EditSession(model, frame)
        legs.update(fill=lambda: s3.fill(disc, sketch=sk, window=win, low_latency=True),
                    fill_frame_scaled=lambda: s4.fill(big_disc, sketch=bsk, window=big, low_latency=True, max_side=max_side))
    out["ms"] = rounds_of(legs, reps)
    if not parent:
        eng = model.engine()
        kernels = {}
        for name in legs:
            eng.profile(True)
            legs[name]()
            rep = eng.profile_report()
            eng.profile(False)
            ks = {k["kernel"]: dict(launches=k["launches"], ms=round(k["total_ms"], 4)) for k in rep["kernels"]}
            kernels[name] = dict(total_ms=round(sum(k["ms"] for k in ks.values()), 3), launches=sum(k["launches"] for k in ks.values()),
                                 around_the_forward={n: k for n, k in ks.items() if n.startswith(("window_", "resize_", "fill_"))})
        out.update(work=list(legs["fill_frame_scaled"]()[2]["work"]), kernels_profiled=kernels,
                   pixels_painted=dict(fill=int((disc > 0).sum()), fill_frame_scaled=int((big_disc > 0).sum())),
                   pixels_changed={k: int((s.frame() != frame).any(2).sum()) for k, s in (("edit", s1), ("edit_frame_scaled", s2), ("fill", s3),
                                                                                          ("fill_frame_scaled", s4))},
                   fill_minus_edit_ms={k: round(out["ms"][k.replace("edit", "fill")]["median"] - out["ms"][k]["median"], 3)
                                       for k in ("edit", "edit_frame_scaled")})
    return out


def host_select(frame, seed, tolerance, grow):
    """the selection of DESIGN.md 6o on the host -> (mask (H,W) uint8 of 0 / 255, the route's name)"""
    import numpy as np
    sim = np.abs(frame.astype(np.int16) - frame[seed[0], seed[1]].astype(np.int16)).max(axis=2) <= tolerance
    try:
        from scipy import ndimage
        labels, _ = ndimage.label(sim)
        reached = labels == labels[seed[0], seed[1]]
        if grow:
            reached = ndimage.maximum_filter(reached.view(np.uint8), size=2 * grow + 1, mode="constant") > 0
        return np.where(reached, np.uint8(255), np.uint8(0)), "scipy.ndimage"
    except ImportError:
        pass
    reached = np.zeros(sim.shape, bool)
    reached[seed[0], seed[1]] = True
    for step in range(sim.size):
        near = reached.copy()
        near[1:] |= reached[:-1]
        near[:-1] |= reached[1:]
        near[:, 1:] |= reached[:, :-1]
        near[:, :-1] |= reached[:, 1:]
        near &= sim
        if step and np.array_equal(near, reached):
            break
        reached = near | reached
    out = reached.copy()
    for _ in range(grow):                      # r steps of the 3 x 3 box = the (2r + 1)^2 box
        g = out.copy()
        g[1:] |= out[:-1]
        g[:-1] |= out[1:]
        out = g.copy()
        out[:, 1:] |= g[:, :-1]
        out[:, :-1] |= g[:, 1:]
    return np.where(out, np.uint8(255), np.uint8(0)), "numpy"


def select_leg(model, reps, parent=False, side=512, tolerance=16, grow=2):
    """(a), (b), (c) of the module docstring; parent=True: the leg (a) only, with the calls a build without selections has"""
    import numpy as np
    import torch
    from sketchedit_amd import serve
    rng = np.random.RandomState(0)
    w, h = 1921, 1081
    frame = rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
    frame[..., 0] = frame[..., 0] % 90                               # no noise pixel is similar to the disc's colour
    win = (283, 705, side, side)
    seed = (win[0] + side // 2, win[1] + side // 2)
    yy, xx = np.mgrid[0:h, 0:w]
    disc = (yy - seed[0]) ** 2 + (xx - seed[1]) ** 2 <= 126 ** 2
    frame[disc] = 128
    sk = np.zeros((h, w), np.uint8)
    sk[win[0] + 200:win[0] + 240, win[1] + 250:win[1] + 256] = 255
    dev0 = torch.from_numpy(frame).cuda()

    def fresh(session):
        def put_back():
            session._frame.copy_(dev0)
            torch.cuda.synchronize()
        return put_back

    def timed(fn, put_back):
        def rounds():
            for _ in range(2):                 # warm-up: plans, workspace, code objects
                put_back()
                fn()
            ts = []
            for _ in range(reps):
                put_back()
                t0 = time.perf_counter()
                fn()                           # ends in a device-to-host copy: the request is complete
                ts.append((time.perf_counter() - t0) * 1e3)
            ts.sort()
            return dict(median=round(ts[len(ts) // 2], 3), min=round(ts[0], 3), max=round(ts[-1], 3))
        return rounds

    s1 = serve.EditSession(model, frame)
    legs = dict(edit=timed(lambda: s1.edit(sk, window=win, max_grow=0, low_latency=True), fresh(s1)))
    out = dict(tool="serve_probe --select" + ("-parent" if parent else ""), B=1, reps=reps, mode="low_latency", frame=[w, h],
               window=list(win), seed=list(seed), tolerance=tolerance, grow=grow, disc_pixels=int(disc.sum()))
    if not parent:
        s2, s3 = serve.EditSession(model, frame), serve.EditSession(model, frame)

        def host_route():
            mask, _ = host_select(s3.frame(), seed, tolerance, grow)
            return s3.fill(mask, window=win, low_latency=True)
        legs.update(fill_similar=timed(lambda: s2.fill_similar(seed, tolerance=tolerance, grow=grow, window=win, low_latency=True), fresh(s2)),
                    host_route=timed(host_route, fresh(s3)))
        mask, route = host_select(frame, seed, tolerance, grow)
        parts = dict(frame_download=timed(lambda: s3.frame(), lambda: None), host_select=timed(lambda: host_select(frame, seed, tolerance, grow),
                                                                                                 lambda: None),
                     fill_of_the_mask=timed(lambda: s3.fill(mask, window=win, low_latency=True), fresh(s3)),
                     select_similar=timed(lambda: s2.select_similar(seed, tolerance=tolerance, grow=grow), fresh(s2)))
    rounds = [{k: fn() for k, fn in legs.items()} for _ in range(3)]
    out["ms"] = {}
    for k in legs:
        meds = sorted(r[k]["median"] for r in rounds)
        out["ms"][k] = dict(median=meds[1], round_medians=[r[k]["median"] for r in rounds], min=min(r[k]["min"] for r in rounds),
                            max=max(r[k]["max"] for r in rounds))
    if not parent:
        out["parts_ms"] = {k: fn() for k, fn in parts.items()}
        # the passes the disc takes, one launch per call
        state = model.select_similar_u8(dev0, seed, tolerance, True)
        passes = 0
        while model.select_flood_u8(state, passes=1).cpu().tolist()[0]:
            passes += 1
        fresh(s2)()
        fresh(s3)()
        eng = model.engine()
        eng.profile(True)
        _, _, info = s2.fill_similar(seed, tolerance=tolerance, grow=grow, window=win, low_latency=True)
        rep = eng.profile_report()
        eng.profile(False)
        host_route()
        ks = {k["kernel"]: dict(launches=k["launches"], ms=round(k["total_ms"], 4)) for k in rep["kernels"]}
        out.update(host_select_route=route, productive_passes=passes, flood_calls_of_8=passes // 8 + 1, selected=info["selected"],
                   selected_by_the_host=int((mask > 0).sum()), same_frame_as_the_host_route=bool(np.array_equal(s2.frame(), s3.frame())),
                   pixels_changed=int((s2.frame() != frame).any(2).sum()),
                   kernels_profiled=dict(total_ms=round(sum(k["ms"] for k in ks.values()), 3), launches=sum(k["launches"] for k in ks.values()),
                                         around_the_forward={n: k for n, k in ks.items()
                                                             if n.startswith(("window_", "resize_", "fill_", "select_", "sketch_"))}),
                   fill_similar_minus_host_route_ms=round(out["ms"]["fill_similar"]["median"] - out["ms"]["host_route"]["median"], 3),
                   fill_similar_minus_edit_ms=round(out["ms"]["fill_similar"]["median"] - out["ms"]["edit"]["median"], 3))
    return out


def lasso_leg(model, reps, parent=False, side=512, grow=2, vertices=300):
    """(a), (b), (c) of the module docstring; parent=True: the leg (a) only, with the calls a build without lassos has"""
    import math
    import numpy as np
    import torch
    from PIL import Image, ImageDraw
    from sketchedit_amd import serve
    rng = np.random.RandomState(0)
    w, h = 1921, 1081
    frame = rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
    win = (283, 705, side, side)
    cy, cx = win[0] + side // 2 + 0.5, win[1] + side // 2 + 0.5
    ring = [(cx + 126 * math.cos(2 * math.pi * k / vertices), cy + 126 * math.sin(2 * math.pi * k / vertices)) for k in range(vertices)]
    sk = np.zeros((h, w), np.uint8)
    sk[win[0] + 200:win[0] + 240, win[1] + 250:win[1] + 256] = 255
    dev0 = torch.from_numpy(frame).cuda()

    def fresh(session):
        def put_back():
            session._frame.copy_(dev0)
            torch.cuda.synchronize()
        return put_back

    def timed(fn, put_back):
        def rounds():
            for _ in range(2):                 # warm-up: plans, workspace, code objects
                put_back()
                fn()
            ts = []
            for _ in range(reps):
                put_back()
                t0 = time.perf_counter()
                fn()                           # ends in a device-to-host copy: the request is complete
                ts.append((time.perf_counter() - t0) * 1e3)
            ts.sort()
            return dict(median=round(ts[len(ts) // 2], 3), min=round(ts[0], 3), max=round(ts[-1], 3))
        return rounds

    def host_lasso():
        """the outline rasterised on the host, grown as the device grows it -> the (H,W) uint8 mask"""
        img = Image.new("L", (w, h), 0)
        ImageDraw.Draw(img).polygon(ring, fill=255)
        mask = np.asarray(img)
        if grow:
            try:
                from scipy import ndimage
                mask = ndimage.maximum_filter(mask, size=2 * grow + 1, mode="constant")
            except ImportError:
                from PIL import ImageFilter
                mask = np.asarray(img.filter(ImageFilter.MaxFilter(2 * grow + 1)))
        return mask

    s1 = serve.EditSession(model, frame)
    legs = dict(edit=timed(lambda: s1.edit(sk, window=win, max_grow=0, low_latency=True), fresh(s1)))
    out = dict(tool="serve_probe --lasso" + ("-parent" if parent else ""), B=1, reps=reps, mode="low_latency", frame=[w, h],
               window=list(win), vertices=vertices, grow=grow)
    if not parent:
        s2, s3 = serve.EditSession(model, frame), serve.EditSession(model, frame)

        def host_route():
            return s3.fill(host_lasso(), window=win, low_latency=True)
        legs.update(fill_lasso=timed(lambda: s2.fill_lasso([ring], grow=grow, window=win, low_latency=True), fresh(s2)),
                    host_route=timed(host_route, fresh(s3)))
        mask = host_lasso()
        sel = s2.select_lasso([ring], grow=grow)
        other = s2.select_lasso([[(x + 60.0, y) for x, y in ring]])

        def combine():
            return s2.combine(sel, other, "subtract").count
        parts = dict(host_polygon=timed(host_lasso, lambda: None), fill_of_the_mask=timed(lambda: s3.fill(mask, window=win, low_latency=True), fresh(s3)),
                     select_lasso=timed(lambda: s2.select_lasso([ring], grow=grow), lambda: None), combine=timed(combine, lambda: None))
    rounds = [{k: fn() for k, fn in legs.items()} for _ in range(3)]
    out["ms"] = {}
    for k in legs:
        meds = sorted(r[k]["median"] for r in rounds)
        out["ms"][k] = dict(median=meds[1], round_medians=[r[k]["median"] for r in rounds], min=min(r[k]["min"] for r in rounds),
                            max=max(r[k]["max"] for r in rounds))
    if not parent:
        out["parts_ms"] = {k: fn() for k, fn in parts.items()}
        fresh(s2)()
        fresh(s3)()
        eng = model.engine()
        eng.profile(True)
        _, _, info = s2.fill_lasso([ring], grow=grow, window=win, low_latency=True)
        rep = eng.profile_report()
        eng.profile(False)
        eng.profile(True)
        combine()
        rep2 = eng.profile_report()
        eng.profile(False)
        ks = {k["kernel"]: dict(launches=k["launches"], ms=round(k["total_ms"], 4)) for k in rep["kernels"]}
        ks2 = {k["kernel"]: dict(launches=k["launches"], ms=round(k["total_ms"], 4)) for k in rep2["kernels"]}
        out.update(selected=info["selected"], selected_by_the_host=int((mask > 0).sum()),
                   masks_differ_on_pixels=int((sel.plane.cpu().numpy() != mask).sum()),
                   pixels_changed=int((s2.frame() != frame).any(2).sum()),
                   kernels_profiled=dict(total_ms=round(sum(k["ms"] for k in ks.values()), 3), launches=sum(k["launches"] for k in ks.values()),
                                         around_the_forward={n: k for n, k in ks.items()
                                                             if n.startswith(("window_", "resize_", "fill_", "select_", "sketch_", "lasso_", "plane_"))}),
                   combine_profiled=ks2,
                   fill_lasso_minus_host_route_ms=round(out["ms"]["fill_lasso"]["median"] - out["ms"]["host_route"]["median"], 3),
                   fill_lasso_minus_edit_ms=round(out["ms"]["fill_lasso"]["median"] - out["ms"]["edit"]["median"], 3))
    return out


def outline_leg(model, reps, parent=False, side=512, tolerance=16):
    """(a), (b), (c) of the module docstring; parent=True: the leg (a) only, with the calls a build without outlines has"""
    import numpy as np
    import torch
    from sketchedit_amd import serve
    rng = np.random.RandomState(0)
    w, h = 1921, 1081
    frame = rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
    frame[..., 0] = frame[..., 0] % 90                               # no noise pixel is similar to the disc's colour
    win = (283, 705, side, side)
    seed = (win[0] + side // 2, win[1] + side // 2)
    yy, xx = np.mgrid[0:h, 0:w]
    disc = (yy - seed[0]) ** 2 + (xx - seed[1]) ** 2 <= 126 ** 2
    frame[disc] = 128
    sk = np.zeros((h, w), np.uint8)
    sk[win[0] + 200:win[0] + 240, win[1] + 250:win[1] + 256] = 255
    dev0 = torch.from_numpy(frame).cuda()

    def fresh(session):
        def put_back():
            session._frame.copy_(dev0)
            torch.cuda.synchronize()
        return put_back

    def timed(fn, put_back=lambda: None):
        def rounds():
            for _ in range(2):                 # warm-up: plans, workspace, code objects
                put_back()
                fn()
            ts = []
            for _ in range(reps):
                put_back()
                t0 = time.perf_counter()
                fn()                           # ends in a device-to-host copy or on the host: the request is complete
                ts.append((time.perf_counter() - t0) * 1e3)
            ts.sort()
            return dict(median=round(ts[len(ts) // 2], 3), min=round(ts[0], 3), max=round(ts[-1], 3))
        return rounds

    s1 = serve.EditSession(model, frame)
    legs = dict(edit=timed(lambda: s1.edit(sk, window=win, max_grow=0, low_latency=True), fresh(s1)))
    out = dict(tool="serve_probe --outline" + ("-parent" if parent else ""), B=1, reps=reps, mode="low_latency", frame=[w, h],
               window=list(win), seed=list(seed), tolerance=tolerance, disc_pixels=int(disc.sum()))
    if not parent:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
        import outline_util
        s2 = serve.EditSession(model, frame)

        def mask_rings(sel):
            y0, x0 = sel.box[:2]
            return [[(x + x0, y + y0) for x, y in r] for r in outline_util.spec_rings(sel.mask())]
        legs.update(rings=timed(lambda: s2.select_similar(seed, tolerance=tolerance).rings()),
                    mask_route=timed(lambda: mask_rings(s2.select_similar(seed, tolerance=tolerance))))
        sel = s2.select_similar(seed, tolerance=tolerance)
        other = s2.select_lasso([[(seed[1] - 40.0, seed[0] - 40.0), (seed[1] + 90.0, seed[0] - 30.0), (seed[1] + 10.0, seed[0] + 95.0)]])
        records, crop = sel.edges(), sel.mask()
        parts = dict(select_similar=timed(lambda: s2.select_similar(seed, tolerance=tolerance)), rings=timed(sel.rings), edges=timed(sel.edges),
                     mask=timed(sel.mask), link_records_on_host=timed(lambda: serve.outline_rings(records)),
                     trace_mask_on_host=timed(lambda: outline_util.spec_rings(crop)),
                     combine=timed(lambda: s2.combine(sel, other, "subtract").count))
    rounds = [{k: fn() for k, fn in legs.items()} for _ in range(3)]
    out["ms"] = {}
    for k in legs:
        meds = sorted(r[k]["median"] for r in rounds)
        out["ms"][k] = dict(median=meds[1], round_medians=[r[k]["median"] for r in rounds], min=min(r[k]["min"] for r in rounds),
                            max=max(r[k]["max"] for r in rounds))
    if not parent:
        out["parts_ms"] = {k: fn() for k, fn in parts.items()}
        eng = model.engine()
        eng.profile(True)
        rings = sel.rings()
        rep = eng.profile_report()
        eng.profile(False)
        ks = {k["kernel"]: dict(launches=k["launches"], ms=round(k["total_ms"], 4)) for k in rep["kernels"]}
        back = s2.select_lasso(rings)
        out.update(selected=sel.count, box=list(sel.box), records=int(records.shape[0]), rings=len(rings), ring_points=sum(len(r) for r in rings),
                   bytes_down_rings=8 + 16 * 4096 if records.shape[0] <= 4096 else 2 * 8 + 16 * (4096 + int(records.shape[0])),
                   bytes_of_the_records=16 * int(records.shape[0]), bytes_down_mask=int(crop.size),
                   same_rings_as_the_mask_route=bool(rings == mask_rings(sel)),
                   round_trip_is_the_plane=bool(torch.equal(back.plane, sel.plane) and (back.box, back.count) == (sel.box, sel.count)),
                   svg_path_chars=len(serve.rings_svg_path(rings)), rings_profiled=ks,
                   rings_minus_mask_route_ms=round(out["ms"]["rings"]["median"] - out["ms"]["mask_route"]["median"], 3),
                   rings_alone_minus_combine_ms=round(out["parts_ms"]["rings"]["median"] - out["parts_ms"]["combine"]["median"], 3))
    return out


def move_leg(model, reps, parent=False, side=512, tolerance=16, offset=(150, 300)):
    """(a), (b), (c) of the module docstring; parent=True: the leg (a) only, with the calls a build without moves has"""
    import numpy as np
    import torch
    from sketchedit_amd import serve
    rng = np.random.RandomState(0)
    w, h = 1921, 1081
    frame = rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
    frame[..., 0] = frame[..., 0] % 90                               # no noise pixel is similar to the disc's colour
    win = (283, 705, side, side)
    seed = (win[0] + side // 2, win[1] + side // 2)
    yy, xx = np.mgrid[0:h, 0:w]
    disc = (yy - seed[0]) ** 2 + (xx - seed[1]) ** 2 <= 126 ** 2
    frame[disc] = 128
    sk = np.zeros((h, w), np.uint8)
    sk[win[0] + 200:win[0] + 240, win[1] + 250:win[1] + 256] = 255
    dev0 = torch.from_numpy(frame).cuda()

    def fresh(session):
        def put_back():
            session._frame.copy_(dev0)
            torch.cuda.synchronize()
        return put_back

    def timed(fn, put_back=lambda: None):
        def rounds():
            for _ in range(2):                 # warm-up: plans, workspace, code objects
                put_back()
                fn()
            ts = []
            for _ in range(reps):
                put_back()
                t0 = time.perf_counter()
                fn()                           # ends in a device-to-host copy: the request is complete
                ts.append((time.perf_counter() - t0) * 1e3)
            ts.sort()
            return dict(median=round(ts[len(ts) // 2], 3), min=round(ts[0], 3), max=round(ts[-1], 3))
        return rounds

    s1 = serve.EditSession(model, frame)
    legs = dict(edit=timed(lambda: s1.edit(sk, window=win, max_grow=0, low_latency=True), fresh(s1)))
    out = dict(tool="serve_probe --move" + ("-parent" if parent else ""), B=1, reps=reps, mode="low_latency", frame=[w, h],
               window=list(win), seed=list(seed), tolerance=tolerance, offset=list(offset), disc_pixels=int(disc.sum()))
    if not parent:
        s2, s3, s4 = serve.EditSession(model, frame), serve.EditSession(model, frame), serve.EditSession(model, frame, history=4)
        sel = s2.select_similar(seed, tolerance=tolerance)
        grown = s2.select_similar(seed, tolerance=tolerance, grow=2)
        other = s2.select_lasso([[(seed[1] - 40.0, seed[0] - 40.0), (seed[1] + 90.0, seed[0] - 30.0), (seed[1] + 10.0, seed[0] + 95.0)]])
        sel4 = s4.select_similar(seed, tolerance=tolerance)
        dy, dx = offset

        def host_route():
            f = s3.frame()
            mask = (np.abs(f.astype(np.int16) - f[seed]).max(axis=2) <= tolerance)          # (the disc: no flood on this route)
            ys, xs = np.nonzero(mask)
            f[ys + dy, xs + dx] = f[ys, xs]
            hole = np.zeros((h, w), bool)
            for ey in range(-2, 3):            # the grow by 2, as shifts
                for ex in range(-2, 3):
                    hole[max(ey, 0):h + min(ey, 0), max(ex, 0):w + min(ex, 0)] |= mask[max(-ey, 0):h + min(-ey, 0), max(-ex, 0):w + min(-ex, 0)]
            return serve.EditSession(model, f).fill(hole, window=win, low_latency=True)

        def journalled():
            s4.move_selection(sel4, offset, window=win, low_latency=True)
            s4.undo()
        legs.update(move=timed(lambda: s2.move_selection(sel, offset, window=win, low_latency=True), fresh(s2)),
                    host_route=timed(host_route, fresh(s3)))
        parts = dict(fill_selection=timed(lambda: s2.fill_selection(grown, window=win, low_latency=True), fresh(s2)),
                     combine=timed(lambda: s2.combine(sel, other, "subtract").count),
                     clone_selection=timed(lambda: s2.clone_selection(sel, offset), fresh(s2)),
                     clone_selection_feather8=timed(lambda: s2.clone_selection(sel, offset, feather=8), fresh(s2)),
                     move_and_undo_with_history=timed(journalled, fresh(s4)))
    rounds = [{k: fn() for k, fn in legs.items()} for _ in range(3)]
    out["ms"] = {}
    for k in legs:
        meds = sorted(r[k]["median"] for r in rounds)
        out["ms"][k] = dict(median=meds[1], round_medians=[r[k]["median"] for r in rounds], min=min(r[k]["min"] for r in rounds),
                            max=max(r[k]["max"] for r in rounds))
    if not parent:
        out["parts_ms"] = {k: fn() for k, fn in parts.items()}
        eng = model.engine()
        fresh(s2)()
        eng.profile(True)
        _, _, info = s2.move_selection(sel, offset, window=win, low_latency=True)
        rep = eng.profile_report()
        eng.profile(False)
        ks = {k["kernel"]: dict(launches=k["launches"], ms=round(k["total_ms"], 4)) for k in rep["kernels"]}
        fill_plus_combine = out["parts_ms"]["fill_selection"]["median"] + out["parts_ms"]["combine"]["median"]
        out.update(selected=sel.count, box=list(sel.box), windows=[list(v) for v in info["windows"]], moved_box=list(info["selection"].box),
                   moved_count=info["selection"].count, move_profiled={k: v for k, v in ks.items() if v["ms"] >= 0.001},
                   move_minus_host_route_ms=round(out["ms"]["move"]["median"] - out["ms"]["host_route"]["median"], 3),
                   fill_selection_plus_combine_ms=round(fill_plus_combine, 3),
                   move_minus_fill_selection_plus_combine_ms=round(out["ms"]["move"]["median"] - fill_plus_combine, 3))
    return out


def warp_leg(model, reps, side=512, tolerance=16, offset=(150, 300), scale=1.5, angle=30.0):
    """(a) .. (e) of the module docstring"""
    import numpy as np
    import torch
    from PIL import Image
    from sketchedit_amd import serve
    rng = np.random.RandomState(0)
    w, h = 1921, 1081
    frame = rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
    frame[..., 0] = frame[..., 0] % 90                               # no noise pixel is similar to the disc's colour
    win = (283, 705, side, side)
    seed = (win[0] + side // 2, win[1] + side // 2)
    yy, xx = np.mgrid[0:h, 0:w]
    disc = (yy - seed[0]) ** 2 + (xx - seed[1]) ** 2 <= 126 ** 2
    frame[disc] = 128
    sk = np.zeros((h, w), np.uint8)
    sk[win[0] + 200:win[0] + 240, win[1] + 250:win[1] + 256] = 255
    dev0 = torch.from_numpy(frame).cuda()

    def fresh(session):
        def put_back():
            session._frame.copy_(dev0)
            torch.cuda.synchronize()
        return put_back

    def timed(fn, put_back=lambda: None):
        def rounds():
            for _ in range(2):                 # warm-up: plans, workspace, code objects
                put_back()
                fn()
            ts = []
            for _ in range(reps):
                put_back()
                t0 = time.perf_counter()
                fn()                           # ends in a device-to-host copy: the request is complete
                ts.append((time.perf_counter() - t0) * 1e3)
            ts.sort()
            return dict(median=round(ts[len(ts) // 2], 3), min=round(ts[0], 3), max=round(ts[-1], 3))
        return rounds

    s1, s2, s3 = serve.EditSession(model, frame), serve.EditSession(model, frame), serve.EditSession(model, frame)
    sel = s2.select_similar(seed, tolerance=tolerance)
    m = serve.warp_matrix(sel.box, scale, angle, offset)
    one = float(serve.WARP_ONE)
    # Pillow's affine data (a, b, c, d, e, f): input (x, y) = (a x + b y + c, d x + e y + f) on pixel CORNERS; m is on centres
    a, b, d, e = m[4] / one, m[3] / one, m[1] / one, m[0] / one
    data = (a, b, m[5] / one + 0.5 - 0.5 * (a + b), d, e, m[2] / one + 0.5 - 0.5 * (d + e))

    def host_route():
        f = s3.frame()
        mask = (np.abs(f.astype(np.int16) - f[seed]).max(axis=2) <= tolerance)              # (the disc: no flood on this route)
        rgba = Image.fromarray(np.dstack([f * mask[..., None], np.where(mask, 255, 0).astype(np.uint8)]), "RGBA")
        got = np.asarray(rgba.transform((w, h), Image.AFFINE, data, resample=Image.BILINEAR)).astype(np.int32)
        alpha = got[..., 3:]                                                                 # premultiplied: the object's rim by its coverage
        f = ((got[..., :3] * 255 + (255 - alpha) * f + 127) // 255).astype(np.uint8)
        hole = np.zeros((h, w), bool)
        for ey in range(-2, 3):                # the grow by 2, as shifts
            for ex in range(-2, 3):
                hole[max(ey, 0):h + min(ey, 0), max(ex, 0):w + min(ex, 0)] |= mask[max(-ey, 0):h + min(-ey, 0), max(-ex, 0):w + min(-ex, 0)]
        return serve.EditSession(model, f).fill(hole, window=win, low_latency=True)

    legs = dict(edit=timed(lambda: s1.edit(sk, window=win, max_grow=0, low_latency=True), fresh(s1)),
                move=timed(lambda: s2.move_selection(sel, offset, window=win, low_latency=True), fresh(s2)),
                transform_identity=timed(lambda: s2.transform_selection(sel, offset=offset, window=win, low_latency=True), fresh(s2)),
                transform=timed(lambda: s2.transform_selection(sel, scale=scale, angle=angle, offset=offset, window=win, low_latency=True), fresh(s2)),
                host_route=timed(host_route, fresh(s3)))
    out = dict(tool="serve_probe --warp", B=1, reps=reps, mode="low_latency", frame=[w, h], window=list(win), seed=list(seed), tolerance=tolerance,
               offset=list(offset), scale=scale, angle=angle, matrix=list(m), disc_pixels=int(disc.sum()))
    rounds = [{k: fn() for k, fn in legs.items()} for _ in range(3)]
    out["ms"] = {}
    for k in legs:
        meds = sorted(r[k]["median"] for r in rounds)
        out["ms"][k] = dict(median=meds[1], round_medians=[r[k]["median"] for r in rounds], min=min(r[k]["min"] for r in rounds),
                            max=max(r[k]["max"] for r in rounds))
    eng = model.engine()
    for name, kw in (("transform_identity", dict()), ("transform", dict(scale=scale, angle=angle))):
        fresh(s2)()
        eng.profile(True)
        _, _, info = s2.transform_selection(sel, offset=offset, window=win, low_latency=True, **kw)
        rep = eng.profile_report()
        eng.profile(False)
        ks = {k["kernel"]: dict(launches=k["launches"], ms=round(k["total_ms"], 4)) for k in rep["kernels"]}
        out[name + "_profiled"] = {k: v for k, v in ks.items() if v["ms"] >= 0.001}
        out[name + "_windows"] = [list(v) for v in info["windows"]]
        out[name + "_count"] = info["selection"].count
    fresh(s2)()
    _, _, moved = s2.move_selection(sel, offset, window=win, low_latency=True)
    after_move = s2._frame.clone()
    fresh(s2)()
    _, _, ident = s2.transform_selection(sel, offset=offset, window=win, low_latency=True)
    out.update(selected=sel.count, box=list(sel.box),
               identity_is_the_move=bool(torch.equal(after_move, s2._frame) and torch.equal(moved["selection"].plane, ident["selection"].plane)),
               transform_minus_move_ms=round(out["ms"]["transform"]["median"] - out["ms"]["move"]["median"], 3),
               transform_minus_host_route_ms=round(out["ms"]["transform"]["median"] - out["ms"]["host_route"]["median"], 3))
    return out


def filter_leg(model, reps, side=512, tolerance=16):
    """(a) .. (f) of the module docstring"""
    import numpy as np
    import torch
    from PIL import Image, ImageFilter
    from sketchedit_amd import serve
    rng = np.random.RandomState(0)
    w, h = 1921, 1081
    frame = rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
    frame[..., 0] = frame[..., 0] % 90                               # no noise pixel is similar to the disc's colour
    win = (283, 705, side, side)
    seed = (win[0] + side // 2, win[1] + side // 2)
    yy, xx = np.mgrid[0:h, 0:w]
    disc = (yy - seed[0]) ** 2 + (xx - seed[1]) ** 2 <= 126 ** 2
    frame[disc] = 128
    frame[disc & ((yy // 8 + xx // 8) % 2 == 0), 1] = 140            # a pattern inside the disc, within the tolerance: a filter has work to do
    sk = np.zeros((h, w), np.uint8)
    sk[win[0] + 200:win[0] + 240, win[1] + 250:win[1] + 256] = 255
    dev0 = torch.from_numpy(frame).cuda()

    def fresh(session):
        def put_back():
            session._frame.copy_(dev0)
            torch.cuda.synchronize()
        return put_back

    def timed(fn, put_back=lambda: None):
        def rounds():
            for _ in range(2):                 # warm-up: plans, workspace, code objects
                put_back()
                fn()
            ts = []
            for _ in range(reps):
                put_back()
                t0 = time.perf_counter()
                fn()                           # ends in a device-to-host copy: the request is complete
                ts.append((time.perf_counter() - t0) * 1e3)
            ts.sort()
            return dict(median=round(ts[len(ts) // 2], 3), min=round(ts[0], 3), max=round(ts[-1], 3))
        return rounds

    s1, s2, s3 = serve.EditSession(model, frame), serve.EditSession(model, frame), serve.EditSession(model, frame)
    sel = s2.select_similar(seed, tolerance=tolerance)
    by0, bx0, by1, bx1 = sel.box

    def host_route():
        f = s3.frame()
        mask = (np.abs(f.astype(np.int16) - f[seed]).max(axis=2) <= tolerance)              # (the disc: no flood on this route)
        y0, x0, y1, x1 = max(by0 - 8, 0), max(bx0 - 8, 0), min(by1 + 8, h), min(bx1 + 8, w)
        soft = np.asarray(Image.fromarray(f[y0:y1, x0:x1]).filter(ImageFilter.GaussianBlur(8 / 3.0)))
        f = f.copy()
        crop = f[y0:y1, x0:x1]
        crop[mask[y0:y1, x0:x1]] = soft[mask[y0:y1, x0:x1]]
        s = serve.EditSession(model, f)
        return s._frame[by0:by1, bx0:bx1].contiguous().cpu().numpy()                        # the patch a front end shows

    F = s2.filter_selection
    legs = dict(edit=timed(lambda: s1.edit(sk, window=win, max_grow=0, low_latency=True), fresh(s1)),
                blur_r8=timed(lambda: F(sel, "blur", radius=8), fresh(s2)),
                blur_r32=timed(lambda: F(sel, "blur", radius=32), fresh(s2)),
                pixelate_16=timed(lambda: F(sel, "pixelate", cell=16), fresh(s2)),
                sharpen=timed(lambda: F(sel, "sharpen"), fresh(s2)),
                host_route=timed(host_route, fresh(s3)))
    out = dict(tool="serve_probe --filter", B=1, reps=reps, mode="low_latency", frame=[w, h], window=list(win), seed=list(seed), tolerance=tolerance,
               disc_pixels=int(disc.sum()))
    rounds = [{k: fn() for k, fn in legs.items()} for _ in range(3)]
    out["ms"] = {}
    for k in legs:
        meds = sorted(r[k]["median"] for r in rounds)
        out["ms"][k] = dict(median=meds[1], round_medians=[r[k]["median"] for r in rounds], min=min(r[k]["min"] for r in rounds),
                            max=max(r[k]["max"] for r in rounds))
    eng = model.engine()
    for name, kw in (("blur_r8", dict(kind="blur", radius=8)), ("blur_r32", dict(kind="blur", radius=32)), ("pixelate_16", dict(kind="pixelate", cell=16))):
        fresh(s2)()
        eng.profile(True)
        _, _, info = F(sel, **kw)
        rep = eng.profile_report()
        eng.profile(False)
        out[name + "_profiled"] = {k["kernel"]: dict(launches=k["launches"], ms=round(k["total_ms"], 4)) for k in rep["kernels"]}
        out[name + "_windows"] = [list(v) for v in info["windows"]]
        out[name + "_changed_bytes"] = int((s2._frame != dev0).sum())
    out.update(selected=sel.count, box=list(sel.box),
               blur_r8_minus_host_route_ms=round(out["ms"]["blur_r8"]["median"] - out["ms"]["host_route"]["median"], 3))
    return out


def adjust_leg(model, reps, side=512, tolerance=16):
    """(a) .. (g) of the module docstring"""
    import numpy as np
    import torch
    from sketchedit_amd import serve
    rng = np.random.RandomState(0)
    w, h = 1921, 1081
    frame = rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
    frame[..., 0] = frame[..., 0] % 90                               # no noise pixel is similar to the disc's colour
    win = (283, 705, side, side)
    seed = (win[0] + side // 2, win[1] + side // 2)
    yy, xx = np.mgrid[0:h, 0:w]
    disc = (yy - seed[0]) ** 2 + (xx - seed[1]) ** 2 <= 126 ** 2
    frame[disc] = 128
    sk = np.zeros((h, w), np.uint8)
    sk[win[0] + 200:win[0] + 240, win[1] + 250:win[1] + 256] = 255
    dev0 = torch.from_numpy(frame).cuda()

    def fresh(session):
        def put_back():
            session._frame.copy_(dev0)
            torch.cuda.synchronize()
        return put_back

    def timed(fn, put_back=lambda: None):
        def rounds():
            for _ in range(2):                 # warm-up: plans, workspace, code objects
                put_back()
                fn()
            ts = []
            for _ in range(reps):
                put_back()
                t0 = time.perf_counter()
                fn()                           # ends in a device-to-host copy: the request is complete
                ts.append((time.perf_counter() - t0) * 1e3)
            ts.sort()
            return dict(median=round(ts[len(ts) // 2], 3), min=round(ts[0], 3), max=round(ts[-1], 3))
        return rounds

    s1, s2, s3 = serve.EditSession(model, frame), serve.EditSession(model, frame), serve.EditSession(model, frame)
    flat = s2.select_similar(seed, tolerance=tolerance)
    cy, cx = 300, 300                                                # a disc of the same radius in the noise, as a lasso of 256 points
    ring = [(cx + 0.5 + 126.2 * np.cos(t), cy + 0.5 + 126.2 * np.sin(t)) for t in np.linspace(0, 2 * np.pi, 256, endpoint=False)]
    noise = s2.select_lasso([ring])
    table, matrix = serve.adjust_lut(brightness=30, contrast=20), serve.adjust_matrix(1.3)

    def host_route():
        f = s3.frame()
        mask = (np.abs(f.astype(np.int16) - f[seed]).max(axis=2) <= tolerance)              # (the disc: no flood on this route)
        by0, bx0, by1, bx1 = flat.box
        f = f.copy()
        crop = f[by0:by1, bx0:bx1]
        m = mask[by0:by1, bx0:bx1]
        crop[m] = table[0][crop[m]]
        s = serve.EditSession(model, f)
        return s._frame[by0:by1, bx0:bx1].contiguous().cpu().numpy()                        # the patch a front end shows

    T = s2.adjust_selection
    legs = dict(edit=timed(lambda: s1.edit(sk, window=win, max_grow=0, low_latency=True), fresh(s1)),
                blur_r8=timed(lambda: s2.filter_selection(flat, "blur", radius=8), fresh(s2)),
                host_route=timed(host_route, fresh(s3)))
    for name, sel in (("flat", flat), ("noise", noise)):
        legs["manual_" + name] = timed(lambda sel=sel: T(sel, lut=table, matrix=matrix), fresh(s2))
        legs["levels_" + name] = timed(lambda sel=sel: T(sel, auto="levels", clip=5), fresh(s2))
        legs["match_rim8_" + name] = timed(lambda sel=sel: T(sel, auto="match", reference=("rim", 8)), fresh(s2))
        legs["histogram_" + name] = timed(lambda sel=sel: s2.histogram(sel))
    out = dict(tool="serve_probe --adjust", B=1, reps=reps, mode="low_latency", frame=[w, h], window=list(win), seed=list(seed), tolerance=tolerance,
               disc_pixels=int(disc.sum()))
    rounds = [{k: fn() for k, fn in legs.items()} for _ in range(3)]
    out["ms"] = {}
    for k in legs:
        meds = sorted(r[k]["median"] for r in rounds)
        out["ms"][k] = dict(median=meds[1], round_medians=[r[k]["median"] for r in rounds], min=min(r[k]["min"] for r in rounds),
                            max=max(r[k]["max"] for r in rounds))
    eng = model.engine()
    for name, sel in (("flat", flat), ("noise", noise)):
        for leg, call in (("manual", lambda sel=sel: T(sel, lut=table, matrix=matrix)), ("levels", lambda sel=sel: T(sel, auto="levels", clip=5)),
                          ("match_rim8", lambda sel=sel: T(sel, auto="match", reference=("rim", 8))), ("histogram", lambda sel=sel: s2.histogram(sel))):
            fresh(s2)()
            eng.profile(True)
            call()
            rep = eng.profile_report()
            eng.profile(False)
            out["%s_%s_profiled" % (leg, name)] = {k["kernel"]: dict(launches=k["launches"], ms=round(k["total_ms"], 4)) for k in rep["kernels"]}
            out["%s_%s_changed_bytes" % (leg, name)] = int((s2._frame != dev0).sum())
    out.update(selected=dict(flat=flat.count, noise=noise.count), box=dict(flat=list(flat.box), noise=list(noise.box)),
               manual_minus_blur_r8_ms=round(out["ms"]["manual_flat"]["median"] - out["ms"]["blur_r8"]["median"], 3),
               manual_minus_host_route_ms=round(out["ms"]["manual_flat"]["median"] - out["ms"]["host_route"]["median"], 3))
    return out


def blend_leg(model, reps, parent=False, side=512, tolerance=16, offset=(150, 300)):
    """(a) .. (d) of the module docstring; parent=True: the legs (a) and (b) only, with the calls a build without the blend has"""
    import numpy as np
    import torch
    from sketchedit_amd import serve
    rng = np.random.RandomState(0)
    w, h = 1921, 1081
    frame = rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
    frame[..., 0] = frame[..., 0] % 90                               # no noise pixel is similar to the disc's colour
    win = (283, 705, side, side)
    seed = (win[0] + side // 2, win[1] + side // 2)
    yy, xx = np.mgrid[0:h, 0:w]
    disc = (yy - seed[0]) ** 2 + (xx - seed[1]) ** 2 <= 126 ** 2
    frame[disc] = 128
    sk = np.zeros((h, w), np.uint8)
    sk[win[0] + 200:win[0] + 240, win[1] + 250:win[1] + 256] = 255
    dev0 = torch.from_numpy(frame).cuda()

    def timed(fn, session):
        def rounds():
            ts = []
            for k in range(2 + reps):              # two warm-ups: plans, workspace, code objects
                session._frame.copy_(dev0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()                               # ends in a device-to-host copy: the request is complete
                ts.append((time.perf_counter() - t0) * 1e3)
            ts = sorted(ts[2:])
            return dict(median=round(ts[len(ts) // 2], 3), min=round(ts[0], 3), max=round(ts[-1], 3))
        return rounds

    s1, s2 = serve.EditSession(model, frame), serve.EditSession(model, frame)
    sel = s2.select_similar(seed, tolerance=tolerance)
    legs = dict(edit=timed(lambda: s1.edit(sk, window=win, max_grow=0, low_latency=True), s1),
                clone=timed(lambda: s2.clone_selection(sel, offset), s2))
    if not parent:
        legs.update(clone_seamless=timed(lambda: s2.clone_selection(sel, offset, blend="seamless"), s2),
                    move_seamless=timed(lambda: s2.move_selection(sel, offset, window=win, low_latency=True, blend="seamless"), s2))
    out = dict(tool="serve_probe --blend" + ("-parent" if parent else ""), B=1, reps=reps, mode="low_latency", frame=[w, h], window=list(win),
               seed=list(seed), tolerance=tolerance, offset=list(offset), selected=sel.count, box=list(sel.box))
    rounds = [{k: fn() for k, fn in legs.items()} for _ in range(3)]
    out["ms"] = {}
    for k in legs:
        meds = sorted(r[k]["median"] for r in rounds)
        out["ms"][k] = dict(median=meds[1], round_medians=[r[k]["median"] for r in rounds], min=min(r[k]["min"] for r in rounds),
                            max=max(r[k]["max"] for r in rounds))
    if not parent:
        eng = model.engine()
        s2._frame.copy_(dev0)
        eng.profile(True)
        s2.clone_selection(sel, offset, blend="seamless")
        rep = eng.profile_report()
        eng.profile(False)
        ks = {k["kernel"]: dict(launches=k["launches"], ms=round(k["total_ms"], 4)) for k in rep["kernels"]}
        blend = {k: v for k, v in ks.items() if k.startswith("blend_")}
        out.update(clone_seamless_profiled=ks, blend_launches=sum(v["launches"] for v in blend.values()),
                   blend_device_ms=round(sum(v["ms"] for v in blend.values()), 4),
                   clone_seamless_minus_clone_ms=round(out["ms"]["clone_seamless"]["median"] - out["ms"]["clone"]["median"], 3))
    return out


def seamless_fill_leg(model, reps, parent=False, side=512, max_side=256):
    """(a) .. (c) of the module docstring; parent=True: the legs (a) and (b) only, with the calls a build without the flag has"""
    import numpy as np
    import torch
    from sketchedit_amd import serve
    rng = np.random.RandomState(0)
    w, h = 1921, 1081
    frame = rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
    win = (283, 705, side, side)
    centre = (win[0] + side // 2, win[1] + side // 2)
    yy, xx = np.mgrid[0:h, 0:w]
    mask = ((yy - centre[0]) ** 2 + (xx - centre[1]) ** 2 <= 126 ** 2).astype(np.uint8)
    sk = np.zeros((h, w), np.uint8)
    sk[win[0] + 200:win[0] + 240, win[1] + 250:win[1] + 256] = 255
    dev0 = torch.from_numpy(frame).cuda()
    s1 = serve.EditSession(model, frame)

    def timed(fn):
        def rounds():
            ts = []
            for k in range(2 + reps):              # two warm-ups: plans, workspace, code objects
                s1._frame.copy_(dev0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()                               # ends in a device-to-host copy: the request is complete
                ts.append((time.perf_counter() - t0) * 1e3)
            ts = sorted(ts[2:])
            return dict(median=round(ts[len(ts) // 2], 3), min=round(ts[0], 3), max=round(ts[-1], 3))
        return rounds

    legs = dict(edit=timed(lambda: s1.edit(sk, window=win, max_grow=0, low_latency=True)),
                fill=timed(lambda: s1.fill(mask, window=win, low_latency=True)),
                fill_scaled=timed(lambda: s1.fill(mask, window=win, max_side=max_side, low_latency=True)))
    if not parent:
        legs.update(fill_seamless=timed(lambda: s1.fill(mask, window=win, low_latency=True, blend="seamless")),
                    fill_scaled_seamless=timed(lambda: s1.fill(mask, window=win, max_side=max_side, low_latency=True, blend="seamless")))
    ys, xs = np.nonzero(mask)
    out = dict(tool="serve_probe --seamless-fill" + ("-parent" if parent else ""), B=1, reps=reps, mode="low_latency", frame=[w, h],
               window=list(win), max_side=max_side, selected=int(mask.sum()), box=[int(ys.min()), int(xs.min()), int(ys.max()) + 1, int(xs.max()) + 1])
    rounds = [{k: fn() for k, fn in legs.items()} for _ in range(3)]
    out["ms"] = {}
    for k in legs:
        meds = sorted(r[k]["median"] for r in rounds)
        out["ms"][k] = dict(median=meds[1], round_medians=[r[k]["median"] for r in rounds], min=min(r[k]["min"] for r in rounds),
                            max=max(r[k]["max"] for r in rounds))
    if not parent:
        eng = model.engine()
        for key, kw in (("fill_seamless", dict()), ("fill_scaled_seamless", dict(max_side=max_side))):
            s1._frame.copy_(dev0)
            eng.profile(True)
            s1.fill(mask, window=win, low_latency=True, blend="seamless", **kw)
            rep = eng.profile_report()
            eng.profile(False)
            ks = {k["kernel"]: dict(launches=k["launches"], ms=round(k["total_ms"], 4)) for k in rep["kernels"]}
            blend = {k: v for k, v in ks.items() if k.startswith("blend_")}
            out[key + "_profiled"] = dict(kernels=ks, blend_launches=sum(v["launches"] for v in blend.values()),
                                          blend_device_ms=round(sum(v["ms"] for v in blend.values()), 4),
                                          resize_device_ms=round(sum(v["ms"] for k, v in ks.items() if "resize" in k), 4),
                                          device_ms=round(sum(v["ms"] for v in ks.values()), 4))
        out["fill_seamless_minus_fill_ms"] = round(out["ms"]["fill_seamless"]["median"] - out["ms"]["fill"]["median"], 3)
        out["fill_scaled_seamless_minus_fill_scaled_ms"] = round(out["ms"]["fill_scaled_seamless"]["median"] - out["ms"]["fill_scaled"]["median"], 3)
    return out


def canvas_leg(model, reps, parent=False, side=512):
    """(a) .. (c) of the module docstring; parent=True: the leg (a) only, with the calls a build without the canvas has"""
    import numpy as np
    import torch
    from sketchedit_amd import serve
    rng = np.random.RandomState(0)
    w, h = 1921, 1081
    frame = rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
    lock = np.zeros((h, w), np.uint8)
    lock[100:300, 200:900] = 255
    win = (283, 705, side, side)
    sk = np.zeros((h, w), np.uint8)
    sk[win[0] + 200:win[0] + 240, win[1] + 250:win[1] + 256] = 255
    s1 = serve.EditSession(model, frame)
    legs = dict(edit=lambda: wall_ms(lambda: s1.edit(sk, window=win, max_grow=0, low_latency=True), reps))
    out = dict(tool="serve_probe --canvas" + ("-parent" if parent else ""), B=1, reps=reps, mode="low_latency", frame=[w, h], window=list(win))
    if not parent:
        s2 = serve.EditSession(model, frame)
        s2.set_lock(lock)
        state = (s2._frame, s2.frame_hw, s2._lock_plane)

        def timed(fn):
            def rounds():
                ts = []
                for k in range(2 + reps):              # two warm-ups: code objects, the allocator's blocks
                    s2._frame, s2.frame_hw, s2._lock_plane = state
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()           # the new frame and lock plane are made
                    ts.append((time.perf_counter() - t0) * 1e3)
                ts = sorted(ts[2:])
                return dict(median=round(ts[len(ts) // 2], 3), min=round(ts[0], 3), max=round(ts[-1], 3))
            return rounds

        def host(fn):
            def route():
                f, lk = s2.frame(), s2.lock()
                s = serve.EditSession(model, np.ascontiguousarray(fn(f)))
                s.set_lock(np.ascontiguousarray(fn(lk)))
            return route
        legs.update(orient_cw=timed(lambda: s2.orient_canvas("cw")), crop=timed(lambda: s2.crop_canvas((100, 200, 800, 1400))),
                    extend=timed(lambda: s2.extend_canvas(64, 64, 64, 64, pad="reflect")),
                    host_orient_cw=timed(host(lambda a: np.rot90(a, -1))), host_crop=timed(host(lambda a: a[100:900, 200:1600])),
                    host_extend=timed(host(lambda a: np.pad(a, ((64, 64), (64, 64)) + ((0, 0),) * (a.ndim - 2), mode="reflect"))))
    rounds = [{k: fn() for k, fn in legs.items()} for _ in range(3)]
    out["ms"] = {}
    for k in legs:
        meds = sorted(r[k]["median"] for r in rounds)
        out["ms"][k] = dict(median=meds[1], round_medians=[r[k]["median"] for r in rounds], min=min(r[k]["min"] for r in rounds),
                            max=max(r[k]["max"] for r in rounds))
    if not parent:
        eng = model.engine()
        dev = {}
        for name, op, label in (("turn_cw", "cw", "canvas_turn"), ("map_180", "180", "canvas_map")):
            ts = []
            for _ in range(5):
                s2._frame, s2.frame_hw, s2._lock_plane = state[0], state[1], None
                eng.profile(True)
                s2.orient_canvas(op)
                rep = eng.profile_report()
                eng.profile(False)
                ks = {k["kernel"]: k for k in rep["kernels"]}
                assert list(ks) == [label] and ks[label]["launches"] == 1, ks
                ts.append(ks[label]["total_ms"])
            ts.sort()
            dev[name] = dict(kernel=label, device_ms=round(ts[2], 4), min=round(ts[0], 4), max=round(ts[-1], 4),
                             gbps=round(2 * 3 * h * w / (ts[2] * 1e-3) / 1e9, 1) if ts[2] else None)
        out.update(device=dev, turn_over_map=round(dev["turn_cw"]["device_ms"] / dev["map_180"]["device_ms"], 3) if dev["map_180"]["device_ms"] else None)
        for k in ("orient_cw", "crop", "extend"):
            out["host_over_device_" + k] = round(out["ms"]["host_" + k]["median"] / out["ms"][k]["median"], 1)
    return out


def modify_leg(model, reps, parent=False, side=512, tolerance=16):
    """(a) .. (e) of the module docstring; parent=True: the leg (a) only, with the calls a build without modifications has"""
    import numpy as np
    import torch
    from sketchedit_amd import serve
    rng = np.random.RandomState(0)
    w, h = 1921, 1081
    frame = rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
    frame[..., 0] = frame[..., 0] % 90                               # no noise pixel is similar to the disc's colour
    win = (283, 705, side, side)
    seed = (win[0] + side // 2, win[1] + side // 2)
    yy, xx = np.mgrid[0:h, 0:w]
    disc = (yy - seed[0]) ** 2 + (xx - seed[1]) ** 2 <= 126 ** 2
    frame[disc] = 128

    def timed(fn):
        def rounds():
            for _ in range(2):                 # warm-up: code objects, the allocator's blocks
                fn()
            ts = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()                           # ends in a device-to-host copy (or, host_route, an upload waited for)
                ts.append((time.perf_counter() - t0) * 1e3)
            ts.sort()
            return dict(median=round(ts[len(ts) // 2], 3), min=round(ts[0], 3), max=round(ts[-1], 3))
        return rounds

    s = serve.EditSession(model, frame)
    sel = s.select_similar(seed, tolerance=tolerance)
    other = s.select_lasso([[(seed[1] - 40.0, seed[0] - 40.0), (seed[1] + 90.0, seed[0] - 30.0), (seed[1] + 10.0, seed[0] + 95.0)]])
    legs = dict(combine=timed(lambda: s.combine(sel, other, "subtract").count))
    out = dict(tool="serve_probe --modify" + ("-parent" if parent else ""), B=1, reps=reps, frame=[w, h], seed=list(seed), tolerance=tolerance,
               disc_pixels=int(disc.sum()), selected=sel.count, box=list(sel.box))
    not_measured = []
    if not parent:
        be = s.backend
        for kind in ("expand", "contract", "smooth"):
            for r in (2, 32):
                legs["%s_r%d" % (kind, r)] = timed(lambda kind=kind, r=r: s.modify_selection(sel, kind, r).count)
        legs["border_r8"] = timed(lambda: s.modify_selection(sel, "border", 8).count)
        legs["grow_r16"] = timed(lambda: serve.tiles_box(be.tiles(be.grow(sel.plane, 16), 32)))
        try:
            from scipy import ndimage
        except ImportError:
            ndimage = None
            not_measured.append("host_route: scipy is not installed")
        if ndimage is not None:
            dd = np.arange(-8, 9)
            structure = dd[:, None] ** 2 + dd[None, :] ** 2 <= 64

            def host_route():
                y0, x0, y1, x1 = sel.box
                m = np.zeros((h, w), bool)
                m[y0:y1, x0:x1] = sel.mask() != 0
                grown = ndimage.binary_dilation(m[y0 - 8:y1 + 8, x0 - 8:x1 + 8], structure=structure)
                full = np.zeros((h, w), np.uint8)
                full[y0 - 8:y1 + 8, x0 - 8:x1 + 8] = np.where(grown, 255, 0)
                be.upload(full)
                torch.cuda.synchronize()
            legs["host_route"] = timed(host_route)
    rounds = [{k: fn() for k, fn in legs.items()} for _ in range(3)]
    out["ms"] = {}
    for k in legs:
        meds = sorted(r[k]["median"] for r in rounds)
        out["ms"][k] = dict(median=meds[1], round_medians=[r[k]["median"] for r in rounds], min=min(r[k]["min"] for r in rounds),
                            max=max(r[k]["max"] for r in rounds))
    if not parent:
        eng = model.engine()
        calls = {"%s_r%d" % (kind, r): (lambda kind=kind, r=r: s.modify_selection(sel, kind, r)) for kind in ("expand", "contract", "smooth") for r in (2, 32)}
        calls.update(border_r8=lambda: s.modify_selection(sel, "border", 8), grow_r16=lambda: be.tiles(be.grow(sel.plane, 16), 32),
                     combine=lambda: s.combine(sel, other, "subtract"))
        out["profiled"] = {}
        for name, call in calls.items():       # one request each: the profiler's records start afresh when it is turned on
            eng.profile(True)
            call()
            rep = eng.profile_report()
            eng.profile(False)
            out["profiled"][name] = {k["kernel"]: dict(launches=k["launches"], ms=round(k["total_ms"], 4)) for k in rep["kernels"]}
        out["expand_r32_minus_combine_ms"] = round(out["ms"]["expand_r32"]["median"] - out["ms"]["combine"]["median"], 3)
        out["not_measured"] = not_measured
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", action="store_true", help="the editing-session leg (see the module docstring)")
    ap.add_argument("--window-scaled", action="store_true", help="window edits at a working size (see the module docstring)")
    ap.add_argument("--window-history", action="store_true", help="the undo journal (see the module docstring)")
    ap.add_argument("--window-history-parent", action="store_true", help="the history=0 legs of --window-history only")
    ap.add_argument("--window-lock", action="store_true", help="locked regions (see the module docstring)")
    ap.add_argument("--window-lock-parent", action="store_true", help="the unlocked legs of --window-lock only")
    ap.add_argument("--regions", action="store_true", help="region edits (see the module docstring)")
    ap.add_argument("--regions-parent", action="store_true", help="the single-window leg of --regions only")
    ap.add_argument("--strokes", action="store_true", help="strokes as polylines (see the module docstring)")
    ap.add_argument("--strokes-parent", action="store_true", help="the edit_regions leg of --strokes only")
    ap.add_argument("--png", action="store_true", help="patches as PNG, encoded on the device (see the module docstring)")
    ap.add_argument("--png-parent", action="store_true", help="the edit + host encoder leg of --png only")
    ap.add_argument("--jpg", action="store_true", help="patches as JPEG, encoded on the device (see the module docstring)")
    ap.add_argument("--jpg-parent", action="store_true", help="the edit + host encoder leg of --jpg only")
    ap.add_argument("--jpg2", action="store_true", help="JPEG patches in 4:2:0 and with per-image Huffman tables (see the module docstring)")
    ap.add_argument("--feather", action="store_true", help="the feathered paste (see the module docstring)")
    ap.add_argument("--feather-parent", action="store_true", help="the legs of --feather without a feathered paste only")
    ap.add_argument("--fill", action="store_true", help="fills of a painted region (see the module docstring)")
    ap.add_argument("--fill-parent", action="store_true", help="the edit legs of --fill only")
    ap.add_argument("--select", action="store_true", help="the selection by colour (see the module docstring)")
    ap.add_argument("--select-parent", action="store_true", help="the edit leg of --select only")
    ap.add_argument("--lasso", action="store_true", help="lasso selections (see the module docstring)")
    ap.add_argument("--lasso-parent", action="store_true", help="the edit leg of --lasso only")
    ap.add_argument("--outline", action="store_true", help="the outline of a selection (see the module docstring)")
    ap.add_argument("--outline-parent", action="store_true", help="the edit leg of --outline only")
    ap.add_argument("--move", action="store_true", help="move a selection (see the module docstring)")
    ap.add_argument("--move-parent", action="store_true", help="the edit leg of --move only")
    ap.add_argument("--warp", action="store_true", help="scale and rotate a selection (see the module docstring)")
    ap.add_argument("--filter", action="store_true", help="blur, sharpen or pixelate a selection (see the module docstring)")
    ap.add_argument("--adjust", action="store_true", help="adjust a selection's tone and colour (see the module docstring)")
    ap.add_argument("--modify", action="store_true", help="expand, contract, border and smooth a selection (see the module docstring)")
    ap.add_argument("--modify-parent", action="store_true", help="the combine leg of --modify only")
    ap.add_argument("--blend", action="store_true", help="seamless move and clone (see the module docstring)")
    ap.add_argument("--blend-parent", action="store_true", help="the edit and the plain clone legs of --blend only")
    ap.add_argument("--canvas", action="store_true", help="crop, extend, rotate and flip the canvas (see the module docstring)")
    ap.add_argument("--canvas-parent", action="store_true", help="the edit leg of --canvas only")
    ap.add_argument("--seamless-fill", action="store_true", help="fills pasted through the membrane (see the module docstring)")
    ap.add_argument("--seamless-fill-parent", action="store_true", help="the edit and the hard fill legs of --seamless-fill only")
    args = ap.parse_args()
    import tempfile
    import numpy as np
    import torch
    from PIL import Image
    from sketchedit_amd import serve
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    model = make_model(tempfile.mkdtemp())
    if (args.window or args.window_scaled or args.window_history or args.window_history_parent or args.window_lock or args.window_lock_parent
            or args.regions or args.regions_parent or args.strokes or args.strokes_parent or args.png or args.png_parent
            or args.jpg or args.jpg_parent or args.jpg2 or args.feather or args.feather_parent or args.fill or args.fill_parent
            or args.select or args.select_parent or args.lasso or args.lasso_parent or args.outline or args.outline_parent
            or args.move or args.move_parent or args.warp or args.filter or args.adjust or args.modify or args.modify_parent
            or args.blend or args.blend_parent or args.canvas or args.canvas_parent or args.seamless_fill or args.seamless_fill_parent):
        if args.seamless_fill or args.seamless_fill_parent:
            res = seamless_fill_leg(model, args.reps, parent=args.seamless_fill_parent)
        elif args.canvas or args.canvas_parent:
            res = canvas_leg(model, args.reps, parent=args.canvas_parent)
        elif args.blend or args.blend_parent:
            res = blend_leg(model, args.reps, parent=args.blend_parent)
        elif args.modify or args.modify_parent:
            res = modify_leg(model, args.reps, parent=args.modify_parent)
        elif args.adjust:
            res = adjust_leg(model, args.reps)
        elif args.filter:
            res = filter_leg(model, args.reps)
        elif args.warp:
            res = warp_leg(model, args.reps)
        elif args.move or args.move_parent:
            res = move_leg(model, args.reps, parent=args.move_parent)
        elif args.outline or args.outline_parent:
            res = outline_leg(model, args.reps, parent=args.outline_parent)
        elif args.lasso or args.lasso_parent:
            res = lasso_leg(model, args.reps, parent=args.lasso_parent)
        elif args.select or args.select_parent:
            res = select_leg(model, args.reps, parent=args.select_parent)
        elif args.fill or args.fill_parent:
            res = fill_leg(model, args.reps, parent=args.fill_parent)
        elif args.feather or args.feather_parent:
            res = feather_leg(model, args.reps, parent=args.feather_parent)
        elif args.jpg2:
            res = jpg2_leg(model, args.reps)
        elif args.jpg or args.jpg_parent:
            res = jpg_leg(model, args.reps, parent=args.jpg_parent)
        elif args.png or args.png_parent:
            res = png_leg(model, args.reps, parent=args.png_parent)
        elif args.strokes or args.strokes_parent:
            res = strokes_leg(model, args.reps, parent=args.strokes_parent)
        elif args.regions or args.regions_parent:
            res = regions_leg(model, args.reps, parent=args.regions_parent)
        elif args.window_lock or args.window_lock_parent:
            res = window_lock_leg(model, args.reps, parent=args.window_lock_parent)
        elif args.window_history or args.window_history_parent:
            res = window_history_leg(model, args.reps, parent=args.window_history_parent)
        else:
            res = window_scaled_leg(model, args.reps) if args.window_scaled else window_leg(model, args.reps)
        line = json.dumps(res)
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return
    eng = model.engine()
    rng = np.random.RandomState(0)
    cases = []
    for w, h in SIZES:
        img = Image.fromarray(rng.randint(0, 256, (h, w, 3), dtype=np.uint8))
        sk = Image.fromarray(((rng.rand(h, w) < 0.01) * 255).astype(np.uint8))
        case = dict(w=w, h=h, working=[w // 8 * 8, h // 8 * 8])
        for ll in (True, False):
            tag = "low_latency" if ll else "default"
            host = wall_ms(lambda: serve.process_image(model, img, sk, low_latency=ll), args.reps)
            dev = wall_ms(lambda: serve.process_image(model, img, sk, low_latency=ll, device_io=True), args.reps)
            same = np.array_equal(np.asarray(serve.process_image(model, img, sk, low_latency=ll)),
                                  np.asarray(serve.process_image(model, img, sk, low_latency=ll, device_io=True)))
            case[tag] = dict(host_ms=host, device_io_ms=dev, speedup=round(host["median"] / dev["median"], 2), identical=same)
        eng.profile(True)
        serve.process_image(model, img, sk, device_io=True)
        rep = eng.profile_report()
        eng.profile(False)
        for k in rep["kernels"]:
            if k["kernel"] in ("resize_h", "resize_v"):
                case[k["kernel"]] = dict(launches=k["launches"], ms=round(k["total_ms"], 4), bytes=int(k["bytes"]),
                                         gbps=round(k["bytes"] / (k["total_ms"] * 1e-3) / 1e9, 1) if k["total_ms"] else None)
        cases.append(case)
        print(json.dumps(case), file=sys.stderr, flush=True)
    res = dict(tool="serve_probe", B=1, reps=args.reps, torch_threads=torch.get_num_threads(), hbm_peak_gbps_measured=6290,
               cases=cases)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
