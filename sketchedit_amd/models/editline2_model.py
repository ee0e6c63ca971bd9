"""EditLine2Model: the wrapper test.py / demo.py call (reference: models/editline2_model.py:49-147,
184-200,223-242,338-370).  Only the inference-side modes exist here ('inference', 'visualize'); the
training modes of the reference ('generator', 'discriminator') depend on code it never released.

    model = create_model(opt); model.eval()
    composed, mask = model({'image': (B,3,H,W) in [-1,1], 'mask': (B,1,H,W) sketch in {0,1}}, mode='inference')

inference = netM -> mask_inpaint = (mask > 0.5) -> netG(inputs, inputs, mask_inpaint, mask_inpaint, line)
-> composed = fake*mask + inputs*(1-mask) with the SOFT mask (:132), all inside one se_inference call.
"""
import torch

from .. import _lib
from ..util import util
from . import networks


class EditLine2Model(torch.nn.Module):
    @staticmethod
    def modify_commandline_options(parser, is_train):
        networks.modify_commandline_options(parser, is_train)
        # no reference counterpart: SE_FLAG_CONSERVATIVE of the C-ABI (include/sketchedit_hip.h, INTEGRATION.md "Precision
        # choice") -- the mask predictor on the F(2x2,3x3) Winograd form; for checkpoints whose mask logits sit at 0.5
        parser.add_argument("--precision", type=str, default="f32", choices=["f32", "bf16"],
                            help="f32: the reference's arithmetic (1e-3 parity bound); bf16: SE_FLAG_BF16 -- bf16 storage and MFMA, fp32 accumulate "
                                 "(BASELINE config 5; compared against the oracle's bf16 mode, not the 1e-3 bound)")
        parser.add_argument("--conservative_mask", action="store_true",
                            help="netM on the conservative Winograd form (fewer hard-mask flips vs the fp32 CPU reference, +1.7 %% time)")
        return parser

    def __init__(self, opt):
        super().__init__()
        if getattr(opt, "isTrain", False):
            raise NotImplementedError("sketchedit_amd implements the inference path only")
        self.opt = opt
        self.netM, self.netG = self.initialize_networks(opt)
        self._engine = None

    def use_gpu(self):
        return len(self.opt.gpu_ids) > 0

    def initialize_networks(self, opt):
        netG = networks.define_G(opt)
        saved = opt.netG
        opt.netG = "MD"                                   # editline2_model.py:186-188
        netM = networks.define_G(opt)
        opt.netG = saved
        if not hasattr(opt, "isSkip"):                    # :195-197 (isSkip bypasses the checkpoint load)
            netG = util.load_network(netG, "G", opt.which_epoch, opt)
            netM = util.load_network(netM, "M", opt.which_epoch, opt)
            if self.use_gpu():
                netG.cuda()
                netM.cuda()
        return netM, netG

    def engine(self):
        if not self.use_gpu() or not torch.cuda.is_available():
            raise _lib.SketchEditHipError("EditLine2Model: this path needs an MI355X (--gpu_ids 0); the reference's "
                                          "--gpu_ids -1 CPU mode has no counterpart here")
        if self._engine is None:
            self._engine = _lib.Engine(self.opt.gpu_ids[0])
            self._engine.set_conservative(getattr(self.opt, "conservative_mask", False))
            self._engine.set_precision(getattr(self.opt, "precision", "f32") or "f32")
            self.netG.bind_engine(self._engine)
            self.netM.bind_engine(self._engine)
        self.netG.engine()                                # (re)upload weights if they changed
        self.netM.engine()
        return self._engine

    def preprocess_input(self, data):
        """:223-242.  gt / edgegt are filled from image / mask when absent (the reference only does so
        on the GPU branch and raises KeyError on CPU)."""
        dev = torch.device("cuda", self.opt.gpu_ids[0]) if self.use_gpu() else torch.device("cpu")
        data["image"] = data["image"].to(dev)
        data["gt"] = data["gt"].to(dev) if "gt" in data else data["image"]
        data["mask"] = data["mask"].to(dev)
        data["edgegt"] = data["edgegt"].to(dev) if "edgegt" in data else data["mask"]
        return data["image"], data["gt"], data["mask"], data["edgegt"], None

    def _mode_for(self, B, H, W, low_latency):
        """Execution mode of a call of B images: the caller's pin, else by the call's OWN size (an interactive caller that
        configured --batchSize 8 and sends single images keeps the low-latency kernels)."""
        return _lib.Engine.is_low_latency(int(B), H, W, low_latency)

    def batch_mode(self, H, W):
        """The mode a FULL --batchSize batch of H x W images takes -- what a batching loop pins for every batch of its file
        list.  test.py --batchSize 8 over 20 files runs batches of 8, 8, 4: chosen from each call's own size the last one
        would cross LOW_LATENCY_MAX_PIXELS into the other mode (other kernels: fp32-rounding differences, possibly another
        hard-mask pixel) -- an image's PNG must not depend on where the file list ends, so test.py passes
        `low_latency=model.batch_mode(H, W)`."""
        return _lib.Engine.is_low_latency(int(getattr(self.opt, "batchSize", 1) or 1), H, W)

    def inference_u8(self, data, low_latency=None):
        """mode='inference' followed by test.py:25-27 -- `((generated + 1) / 2 * 255).astype(uint8)` in HWC order and
        `(mask * 255).astype(uint8)` -- as ONE library call: the quantisation is fused into the forward's last kernel, so
        only uint8 leaves the device.  -> (rgb (B,H,W,3) uint8, mask (B,H,W) uint8), both on the device."""
        if self.training:
            raise NotImplementedError("call model.eval() first: only the eval branch of generate_fake exists here")
        if "image_u8" in data:
            # uint8 all the way (the dataset's u8 mode, data/testimage_dataset.py): the normalisation of
            # /root/reference/data/testimage_dataset.py:89-111 happens on the device too (table lookup, bit-identical)
            dev = torch.device("cuda", self.opt.gpu_ids[0])
            iu8, su8 = data["image_u8"].to(dev, non_blocking=True), data["mask_u8"].to(dev, non_blocking=True)
            B, H, W, _ = iu8.shape
            with torch.no_grad():
                return self.engine().inference_u8io(iu8.contiguous(), su8.contiguous(), _lib.flags_from_opt(self.opt),
                                                    low_latency=self._mode_for(B, H, W, low_latency))
        inputs, _, line, _, _ = self.preprocess_input(data)
        eng = self.engine()
        with torch.no_grad():
            return eng.inference_u8(inputs.float().contiguous(), line.float().contiguous(), _lib.flags_from_opt(self.opt),
                                    low_latency=self._mode_for(inputs.shape[0], inputs.shape[2], inputs.shape[3], low_latency))

    def edit_u8(self, image_u8, sketch_u8, low_latency=None):
        """demo.py:39-73 (process_image) after the image decode: raw uint8 arrays in, the edited image at the raw size out,
        every step on the device in one library call (se_edit_u8) -- the resizes to and from the working size
        (Hi//8*8, Wi//8*8) are Pillow's BICUBIC bit for bit, so the result is byte-identical to the host steps.
        image_u8 (Hi,Wi,3) RGB and sketch_u8 (Hs,Ws) 'L' (numpy arrays or tensors; the sketch's raw size may differ), or the
        same with a leading batch dimension for B requests of one raw size -> rgb uint8 on the device, same layout.
        `low_latency` as in forward, by the forward's size at the working resolution."""
        if self.training:
            raise NotImplementedError("call model.eval() first: only the eval branch of generate_fake exists here")
        dev = torch.device("cuda", self.opt.gpu_ids[0])
        iu8, su8 = _lib.upload_u8(image_u8, dev), _lib.upload_u8(sketch_u8, dev)
        single = iu8.dim() == 3
        if single:
            iu8, su8 = iu8[None], su8[None]
        rgb = self.engine().edit_u8(iu8, su8, _lib.flags_from_opt(self.opt),
                                    low_latency=self._mode_for(iu8.shape[0], iu8.shape[1] // 8 * 8, iu8.shape[2] // 8 * 8,
                                                               low_latency))
        return rgb[0] if single else rgb

    def edit_window_u8(self, frames, origins, sketches, H, W, commit=True, low_latency=None, work_hw=None, locks=None):
        """A window edit of resident frames (no reference counterpart; DESIGN.md 6d, serve.EditSession is the caller-facing
        form): frames[i] (Hi,Wi,3) uint8 ON THE DEVICE, edited in place; origins[i] = (y0, x0) of the H x W window;
        sketches[i] the window's (H,W) uint8 sketch (array or tensor; uploaded here).  The result is this model's inference
        on the contiguous crop, pasted where its uint8 mask is > 0 (commit).  -> (rgb (B,H,W,3), mask_u8 (B,H,W), hits (B,4)
        int32) on the device.  `low_latency` as in forward, by the size of the forward: B windows of H x W.
        work_hw = (Hw, Ww): the forward runs at that working size instead -- the window (any H, W >= 16) is
        resampled into it and the result and its mask are resampled back before the paste, all Pillow's BICUBIC bit for
        bit; rgb and mask_u8 are then returned at the working size, and the mode follows B forwards of Hw x Ww.
        locks: one (Hi,Wi) uint8 lock plane ON THE DEVICE per frame, or None for a frame without one -- no
        edit changes a pixel whose byte is non-zero; the lock enters the forward where the mask is made, and the paste."""
        if self.training:
            raise NotImplementedError("call model.eval() first: only the eval branch of generate_fake exists here")
        dev = torch.device("cuda", self.opt.gpu_ids[0])
        sks = [_lib.upload_u8(s, dev) for s in sketches]
        Hw, Ww = (int(v) for v in work_hw) if work_hw is not None else (H, W)      # the size of the forward
        args = (Hw, Ww, _lib.flags_from_opt(self.opt))
        with torch.no_grad():
            eng = self.engine()
            kw = dict(commit=commit, low_latency=self._mode_for(len(frames), Hw, Ww, low_latency))
            if locks is not None and any(t is not None for t in locks):
                return eng.edit_window_locked_u8(frames, origins, sks, locks, (H, W), *args, **kw)
            if work_hw is not None:
                return eng.edit_window_scaled_u8(frames, origins, sks, (H, W), *args, **kw)
            return eng.edit_window_u8(frames, origins, sks, *args, **kw)

    def window_paste_feather_u8(self, frames, origins, locks, window_hw, radius, rgb, m8):
        """The feathered paste that belongs to an uncommitted edit_window_u8: rgb (B,H,W,3) and m8 (B,H,W) as
        it returned them -- at a working size they are first resized to the window's (hs, ws) with Pillow's BICUBIC
        (Engine.resize_u8), the arrays the paste of 6e is defined on -- are blended into the frames with radius 0 .. 16
        (Engine.window_paste_feather_u8).  locks: a plane or None per request, or None."""
        hs, ws = (int(v) for v in window_hw)
        with torch.no_grad():
            eng = self.engine()
            if tuple(m8.shape[1:3]) != (hs, ws):
                rgb, m8 = eng.resize_u8(rgb, (hs, ws)), eng.resize_u8(m8, (hs, ws))
            eng.window_paste_feather_u8(frames, origins, locks, (hs, ws), radius, rgb, m8)

    def fill(self, image, hole, sketch=None, lock=None, visualize=False, low_latency=None):
        """A fill (no inference entry of the reference; its generate_fake trains netG on such masks, editline2_model.py:338-370;
        DESIGN.md 6n): netG alone on the hole the caller gives, netM never runs.  image (B,3,H,W) in [-1,1]; hole (B,H,W)
        uint8, non-zero = fill; sketch (B,1,H,W) in {0,1} or None; lock (B,H,W) uint8 or None, non-zero = never a hole.
        -> composed, or with visualize dict(composed, coarse, fine, hard) (Engine.fill)."""
        if self.training:
            raise NotImplementedError("call model.eval() first: only the eval branch of generate_fake exists here")
        dev = torch.device("cuda", self.opt.gpu_ids[0])
        image = image.to(dev).float().contiguous()
        sketch = None if sketch is None else sketch.to(dev).float().contiguous()
        hole = _lib.upload_u8(hole, dev)
        lock = None if lock is None else _lib.upload_u8(lock, dev)
        with torch.no_grad():
            r = self.engine().fill(image, hole, _lib.flags_from_opt(self.opt), sketch=sketch, lock=lock, visualize=visualize,
                                   low_latency=self._mode_for(image.shape[0], image.shape[2], image.shape[3], low_latency))
        return r if visualize else r["composed"]

    def fill_window_u8(self, frames, origins, sketches, holes, H, W, low_latency=None, work_hw=None, locks=None, raw=False):
        """The fill of windows of resident frames (serve.EditSession.fill is the caller-facing form): as
        edit_window_u8(commit=False) with the hole taken from holes[i], the frame's (Hi,Wi) uint8 fill plane ON THE DEVICE,
        instead of netM.  sketches[i]: the window's (H,W) uint8 sketch or None; sketches may be None.  -> (rgb, mask_u8) on the
        device, at the working size with work_hw; nothing is pasted (Engine.fill_window_u8).  raw: rgb is netG's own prediction
        at every pixel, uncomposed."""
        if self.training:
            raise NotImplementedError("call model.eval() first: only the eval branch of generate_fake exists here")
        dev = torch.device("cuda", self.opt.gpu_ids[0])
        sks = None if sketches is None else [None if s is None else _lib.upload_u8(s, dev) for s in sketches]
        Hw, Ww = (int(v) for v in work_hw) if work_hw is not None else (H, W)
        with torch.no_grad():
            return self.engine().fill_window_u8(frames, origins, sks, holes, locks, (H, W), Hw, Ww, _lib.flags_from_opt(self.opt),
                                                low_latency=self._mode_for(len(frames), Hw, Ww, low_latency), raw=raw)

    def fill_keep_u8(self, frames, origins, holes, locks, window_hw, keeps=None):
        """The keep planes a fill's paste takes in place of the locks: 255 where holes[i] is 0 or locks[i] is
        non-zero, over the window's rectangle only (Engine.fill_keep_u8)."""
        return self.engine().fill_keep_u8(frames, origins, holes, locks, window_hw, keeps=keeps)

    def select_similar_u8(self, frame, seed, tolerance, contiguous, state=None):
        """Selection by colour (serve.EditSession.select_similar is the caller-facing form): the state plane of a
        resident frame and a seed (y, x) -- 255 at the seed, 1 (contiguous) or 255 where a pixel's colour is within
        `tolerance` of the seed's in every channel, else 0 (Engine.select_similar_u8)."""
        return self.engine().select_similar_u8(frame, seed, tolerance, contiguous, state=state)

    def select_flood_u8(self, state, passes=8, changed=None):
        """`passes` flood passes over a state plane, in place -> the (passes,) int32 `changed` words on the device, 0 from the
        first pass that stored nothing (Engine.select_flood_u8)."""
        return self.engine().select_flood_u8(state, passes=passes, changed=changed)

    def select_grow_u8(self, state, grow, out=None):
        """A state plane -> the fill plane: 255 within Chebyshev distance `grow` of a reached byte (Engine.select_grow_u8)."""
        return self.engine().select_grow_u8(state, grow, out=out)

    def lasso_fill_u8(self, edges, Hi, Wi, out=None):
        """A lasso selection (serve.EditSession.select_lasso is the caller-facing form): the (N,4) int32 edges of
        closed rings, in quarter pixels, on the device -> the (Hi,Wi) fill plane of their even-odd interior (Engine.lasso_fill_u8)."""
        return self.engine().lasso_fill_u8(edges, Hi, Wi, out=out)

    def plane_combine_u8(self, a, b, op, out=None):
        """Two selection planes -> a op b as 0 / 255; op = _lib.COMBINE_ADD / SUBTRACT / INTERSECT / XOR, or COMBINE_INVERT with
        b None (Engine.plane_combine_u8)."""
        return self.engine().plane_combine_u8(a, b, op, out=out)

    def plane_modify_u8(self, plane, op, radius, out=None):
        """A selection plane expanded or contracted by a disc of `radius`, or smoothed by the majority vote in it (DESIGN.md 6w;
        serve.EditSession.modify_selection is the caller-facing form): a new 0 / 255 plane; op = _lib.MODIFY_EXPAND / CONTRACT /
        SMOOTH (Engine.plane_modify_u8)."""
        return self.engine().plane_modify_u8(plane, op, radius, out=out)

    def outline_u8(self, plane, cap):
        """The outline of a selection plane (serve.Selection.rings is the caller-facing form): ONE int32 device
        tensor, [total, written] and then the first min(total, cap) boundary records in the lasso's edge format
        (Engine.outline_u8)."""
        return self.engine().outline_u8(plane, cap)

    def move_drop_u8(self, frame, lift, lift_rect, sel, lock, box, offset, flip=0, radius=0):
        """The drop of a moved selection (serve.EditSession.move_selection is the caller-facing form): the selected
        pixels of `box`, as the journal slot `lift` of `lift_rect` holds them, blended into the resident frame `offset` away
        (Engine.move_drop_u8)."""
        self.engine().move_drop_u8(frame, lift, lift_rect, sel, lock, box, offset, flip=flip, radius=radius)

    def move_blend_u8(self, frame, lift, lift_rect, sel, lock, box, offset, flip=0):
        """The seamless drop of a move, in place on a resident frame: move_drop_u8's arguments without the radius;
        the lifted pixels plus a membrane that matches them to the place they land in (Engine.move_blend_u8)."""
        self.engine().move_blend_u8(frame, lift, lift_rect, sel, lock, box, offset, flip=flip)

    def plane_shift_u8(self, sel, box, offset, flip=0, out=None):
        """A selection plane moved as move_drop_u8 moves its pixels: a new 0 / 255 plane (Engine.plane_shift_u8)."""
        return self.engine().plane_shift_u8(sel, box, offset, flip=flip, out=out)

    def canvas_u8(self, src, out_hw, origin=(0, 0), orient=0, pad=0, pad_rgb=0, src_hw=None, out=None):
        """The canvas of a session (serve.EditSession.canvas is the caller-facing form): a NEW frame or plane, the
        rectangle `out_hw` at `origin` of `src` oriented by `orient` and padded by `pad`; src None: the plane of the new area's
        form, of a `src_hw` plane of zeros (Engine.canvas_u8)."""
        return self.engine().canvas_u8(src, out_hw, origin=origin, orient=orient, pad=pad, pad_rgb=pad_rgb, src_hw=src_hw, out=out)

    def warp_drop_u8(self, frame, lift, lift_rect, sel, lock, box, rect, m):
        """The drop of a scaled or turned selection (serve.EditSession.transform_selection is the caller-facing
        form): the selected pixels of `box`, as the journal slot `lift` of `lift_rect` holds them, gathered through the inverse
        map `m` and blended into `rect` of the resident frame (Engine.warp_drop_u8)."""
        self.engine().warp_drop_u8(frame, lift, lift_rect, sel, lock, box, rect, m)

    def plane_warp_u8(self, sel, box, m, out=None):
        """A selection plane warped as warp_drop_u8 warps its pixels: a new 0 / 255 plane (Engine.plane_warp_u8)."""
        return self.engine().plane_warp_u8(sel, box, m, out=out)

    def filter_blur_u8(self, frame, lift, lift_rect, sel, lock, box, taps, amount=-256, feather=0):
        """The blur or unsharp mask of a selection (serve.EditSession.filter_selection is the caller-facing form):
        the selected pixels of `box` become the separable filter `taps` of the frame as the journal slot `lift` of `lift_rect`
        holds it (Engine.filter_blur_u8)."""
        self.engine().filter_blur_u8(frame, lift, lift_rect, sel, lock, box, taps, amount=amount, feather=feather)

    def filter_mosaic_u8(self, frame, lift, lift_rect, sel, lock, box, cell, amount=-256, feather=0):
        """The mosaic of a selection: the selected pixels of `box` become the mean of their `cell` x `cell` block of
        the lift (Engine.filter_mosaic_u8)."""
        self.engine().filter_mosaic_u8(frame, lift, lift_rect, sel, lock, box, cell, amount=amount, feather=feather)

    def adjust_u8(self, frame, lift, lift_rect, sel, lock, box, lut=None, matrix=None, amount=256, feather=0):
        """The tone and colour of a selection (serve.EditSession.adjust_selection is the caller-facing form): the
        selected pixels of `box` become the table `lut`, then the `matrix`, of the frame as the journal slot `lift` of `lift_rect`
        holds it (Engine.adjust_u8)."""
        self.engine().adjust_u8(frame, lift, lift_rect, sel, lock, box, lut=lut, matrix=matrix, amount=amount, feather=feather)

    def adjust_hist_u8(self, frame, sel, box, out=None):
        """The histogram of the selected pixels of `box`: a (4, 256) int32 tensor on the device, rows R, G, B and
        luma (Engine.adjust_hist_u8)."""
        return self.engine().adjust_hist_u8(frame, sel, box, out=out)

    def adjust_lut_u8(self, hist_src, hist_ref, mode, which, clip=0, out=None):
        """A table for adjust_u8 made on the device from one or two hist records: stretch, equalize or match
        (Engine.adjust_lut_u8)."""
        return self.engine().adjust_lut_u8(hist_src, hist_ref, mode, which, clip=clip, out=out)

    def window_save_u8(self, frames, origins, window_hw):
        """The undo journal's save: the (hs, ws) rectangle at origins[i] of every resident frame -> one new
        slot tensor per request; called in front of a committing edit_window_u8 it keeps the bytes the paste replaces."""
        return self.engine().window_save_u8(frames, origins, window_hw)

    def window_swap_u8(self, frames, origins, window_hw, slots):
        """Undo / redo: exchanges each frame's rectangle with its slot, in place."""
        self.engine().window_swap_u8(frames, origins, window_hw, slots)

    def sketch_tiles_u8(self, sketch_u8, tile):
        """Where a full-size sketch is drawn: the (Hi,Wi) uint8 plane ON THE DEVICE -> (ceil(Hi / tile),
        ceil(Wi / tile), 5) int32 there, [count, y0, x0, y1, x1] per tile (Engine.sketch_tiles_u8)."""
        return self.engine().sketch_tiles_u8(sketch_u8, tile)

    def sketch_strokes_u8(self, segs, frame_hws, origins, window_hw, ranges=None):
        """The windows' sketches from segments: `segs` (N,5) int32 ON THE DEVICE -> (B,hs,ws) uint8 there, one
        slice per window at origins[i] of a frame of frame_hws[i] (Engine.sketch_strokes_u8)."""
        return self.engine().sketch_strokes_u8(segs, frame_hws, origins, window_hw, ranges=ranges)

    def png_encode_u8(self, frames, origins, window_hw):
        """Patches as PNG: the (hs, ws) rectangle at origins[i] of every resident frame -> the zlib stream of its
        PNG, encoded ON THE DEVICE; -> (out (B, cap) uint8, sizes (B,) int64) there (Engine.png_encode_u8)."""
        return self.engine().png_encode_u8(frames, origins, window_hw)

    def jpg_encode_u8(self, frames, origins, window_hw, quality=90):
        """Patches as JPEG: the (hs, ws) rectangle at origins[i] of every resident frame -> the entropy-coded
        segment of its baseline JPEG, encoded ON THE DEVICE; -> (out (B, cap) uint8, sizes (B,) int64) there
        (Engine.jpg_encode_u8)."""
        return self.engine().jpg_encode_u8(frames, origins, window_hw, quality=quality)

    def jpg2_encode_u8(self, frames, origins, window_hw, quality=90, subsampling="444", optimize=False):
        """Patches as JPEG with chroma at half resolution (subsampling="420") and/or four Huffman tables made for each image
        (optimize=True), encoded ON THE DEVICE; -> (out (B, cap) uint8, sizes (B,) int64, tables (B, 1088) uint8
        or None) there (Engine.jpg2_encode_u8)."""
        return self.engine().jpg2_encode_u8(frames, origins, window_hw, quality=quality, subsampling=subsampling, optimize=optimize)

    def forward(self, data, mode, low_latency=None):
        """`low_latency` (no reference counterpart): None = by this call's own size, True / False = pinned.  Results are
        bit-identical across batch compositions only WITHIN one mode (include/sketchedit_hip.h), so callers whose batch size
        varies per request (serve.BatchingServer, shard.sharded_inference, test.py's loop through batch_mode) pin it."""
        inputs, real_image, line, line_full, _ = self.preprocess_input(data)
        if mode not in ("inference", "visualize"):
            raise ValueError("|mode| is invalid")
        if self.training:
            raise NotImplementedError("call model.eval() first: only the eval branch of generate_fake exists here")
        eng = self.engine()
        flags = _lib.flags_from_opt(self.opt)
        with torch.no_grad():
            r = eng.inference(inputs.float().contiguous(), line.float().contiguous(), flags,
                              visualize=(mode == "visualize"),
                              low_latency=self._mode_for(inputs.shape[0], inputs.shape[2], inputs.shape[3], low_latency))
        if mode == "inference":
            return r["composed"], r["mask"]
        return {"mask": r["hard"], "maskim": r["maskim"], "coarse": r["coarse"], "fine": r["fine"],
                "composed": r["composed"]}                # :134-145
