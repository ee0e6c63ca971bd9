/* libsketchedit_hip.so -- C-ABI of the MI355X (gfx950) SketchEdit inference path.
 *
 * The reference (zengxianyu/sketchedit) has no FFI: its de-facto boundary is Python,
 *   models.create_model(opt)(data, mode='inference')     models/editline2_model.py:107-133
 *   netM(x, guide) -> (mask, mask_image)                 models/networks/editline2_g.py:59-94
 *   netG(x, x2, mask, mask2, guide) -> (coarse, fine)    models/networks/editline_g.py:119-221
 * and below it torch.nn.functional.  This header is what a ctypes binding on the reference side
 * binds instead of that arithmetic; sketchedit_amd/_lib.py is that binding.
 *
 * Conventions
 *  - every tensor pointer is a DEVICE pointer owned by the caller (e.g. torch tensor.data_ptr()),
 *    fp32, contiguous NCHW exactly as the reference's tensors; weights are HOST pointers.
 *  - `stream` is a hipStream_t (torch.cuda.current_stream().cuda_stream); calls only enqueue work,
 *    there is no hidden device synchronisation and no allocation inside a forward: the caller
 *    passes a workspace of at least se_workspace_bytes(ctx, B, H, W) bytes.
 *  - return value 0 = ok, non-zero = error (se_last_error(ctx) describes it); no C++ exception
 *    crosses the boundary.  A context serialises its own forwards with an internal mutex, so one
 *    ctx may be shared by threads (demo.py:120 runs Flask threaded) -- one ctx per stream is faster.
 *  - H and W must be multiples of 8 (demo.py:43-45 enforces the same for the reference).
 *  - Any batch size: the kernels address one tensor with 32-bit byte offsets, so a forward over more images than fit
 *    2^31 bytes of its largest activation (96 bytes per pixel in fp32: 341 images at 256x256) runs as several passes of
 *    the same plan over image ranges; an image's result is bit-identical whatever pass (or batch) it is in.  A single
 *    image beyond that range, and a per-op call beyond it, is an error -- never a silently wrong result.
 */
#ifndef SKETCHEDIT_HIP_H
#define SKETCHEDIT_HIP_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct se_ctx se_ctx;

enum { SE_NET_G = 0, SE_NET_M = 1 };

/* netG option flags: models/networks/editline_g.py:15-23, options/base_options.py:19 */
enum {
  SE_FLAG_USE_CAM = 1,         /* --use_cam */
  SE_FLAG_POOL_MAX = 2,        /* --pool_type max (unset: avg) */
  SE_FLAG_NO_MASK_CC = 4,      /* --no_mask_cc */
  SE_FLAG_NO_MASK_COARSE = 8,  /* --no_mask_coarse */
  SE_FLAG_JOINT_TRAIN_INP = 16, /* --joint_train_inp */
  /* execution options (no reference counterpart; the results agree with the default mode to fp32 rounding, and an
   * image's result is bit-identical across batch positions / ranks WITHIN one mode):
   * LOW_LATENCY: for one or two images per call (test_celeb.sh:2 --batchSize 1, demo.py:59): small-grid kernel shapes that
   * put every CU to work and the independent branches of netG on two streams (the ctx's side stream is ordered after /
   * before the caller's stream through events -- no host synchronisation).
   * GRAPH (se_inference only): capture the forward for these exact arguments into a hipGraph on its second use and
   * replay it afterwards; the caller keeps every pointer argument (inputs, outputs, workspace) stable. */
  SE_FLAG_LOW_LATENCY = 32,
  SE_FLAG_GRAPH = 64,
  /* PACKED_OUT (se_inference only): composed_out points at ONE (B,4,H,W) buffer -- planes 0-2 the composite, plane 3
   * the soft mask (mask_out is ignored and may be NULL): the unit a batch-sharded caller all-gathers. */
  SE_FLAG_PACKED_OUT = 128,
  /* BF16 (BASELINE config 5): activations and conv weights are stored as bf16 and multiplied on the bf16 matrix
   * pipe (v_mfma_f32_16x16x32_bf16) with fp32 accumulation; bias, activations, gate, softmax and composites stay
   * fp32; the external tensors stay fp32 NCHW.  The comparator is the oracle's bf16 mode (oracle/sketchedit_oracle.py);
   * the 1e-3 fp32 bound of the north star does not apply (stated tolerances: tests/test_gpu_bf16.py). */
  SE_FLAG_BF16 = 256,
  /* CONSERVATIVE (fp32 mode; no reference counterpart): the precision choice for netM, whose soft mask feeds the hard 0.5
   * threshold (editline2_model.py:346-347).  By default the 96->192 3x3 layers of BOTH nets run the hybrid Winograd
   * F(2,3)xF(4,3) form; with this flag netM's run F(2x2,3x3) (dyadic transforms, error like the direct form) and only netG
   * keeps the hybrid.  Measured over 72 images / 4.7 M mask pixels of the three procedural weight sets
   * (profiles/r05_f43_flips.json): hard-mask pixels that differ from the fp32 CPU reference 4 (default) vs 1 (this flag;
   * the direct form also has 1), soft-mask max-abs 2.6e-5 vs 1.6e-5, for +1.7 % per step (11.10 -> 11.29 ms at 256x256
   * batch 32).  A caller with a real checkpoint whose logits cluster at the threshold sets it; honoured by se_inference,
   * se_inference_u8, se_netM_forward_ex.  INTEGRATION.md "Precision choice". */
  SE_FLAG_CONSERVATIVE = 512,
  /* RAW_FINE (the window fill of sketchedit_fill.h only; every other entry clears the bit): the uint8 rgb result is the
   * quantisation of netG's `fine` at every pixel instead of the composite's -- the same rule, the same last kernel in a
   * compile-time form of its epilogue, no extra launch.  What a seamless paste of a fill reads on the hole's rim. */
  SE_FLAG_RAW_FINE = 1024
};

/* replaces networks.create_network's .cuda() (models/networks/__init__.py:30-38) */
int se_create(int device_id, se_ctx** out);
void se_destroy(se_ctx* ctx);
const char* se_last_error(se_ctx* ctx);
const char* se_version(void);

/* replaces util.load_network / load_state_dict (util/util.py:214-225).  `name` is a state_dict key
 * ("conv1.weight", "conv1.bias", a leading "module." is stripped); `host` points at shape[0..ndim)
 * fp32 values in the checkpoint's own layout (weight OIHW, bias O).  Unknown keys or wrong shapes
 * are errors (strict load).  se_weights_ready() reports 1 when every tensor of both nets is set. */
int se_load_weights(se_ctx* ctx, int net_id, const char* name, const float* host, const int* shape, int ndim);
int se_weights_ready(se_ctx* ctx);

size_t se_workspace_bytes(se_ctx* ctx, int B, int H, int W);

/* MDGenerator.forward (editline2_g.py:59-94).  image (B,3,H,W), sketch (B,1,H,W) ->
 * mask_out (B,1,H,W); maskim_out (B,3,H,W) may be NULL (its decoder is then skipped, as in
 * mode='inference' where the value is unused). */
int se_netM_forward(se_ctx* ctx, void* stream, const float* image, const float* sketch, float* mask_out,
                    float* maskim_out, void* workspace, size_t workspace_bytes, int B, int H, int W);

/* the same with execution options (SE_FLAG_LOW_LATENCY, SE_FLAG_BF16, SE_FLAG_CONSERVATIVE) */
int se_netM_forward_ex(se_ctx* ctx, void* stream, const float* image, const float* sketch, float* mask_out,
                       float* maskim_out, void* workspace, size_t workspace_bytes, int B, int H, int W, int exec_flags);

/* DeepFillC2Generator.forward (editline_g.py:119-221).  x,x2 (B,3,H,W); mask,mask2,guide (B,1,H,W);
 * coarse_out / fine_out (B,3,H,W), coarse_out may be NULL. */
int se_netG_forward(se_ctx* ctx, void* stream, const float* x, const float* x2, const float* mask,
                    const float* mask2, const float* guide, float* coarse_out, float* fine_out, void* workspace,
                    size_t workspace_bytes, int B, int H, int W, int flags);

/* netG with optional intermediate outputs ("taps"; test support -- the reference's counterparts are forward hooks on
 * netG.pmconv6 / netG.cam_2 / netG.conv11, tests/golden/make_golden.py).  Any pointer may be NULL; taps == NULL is
 * se_netG_forward.  The tensors are written by the SAME launches that feed the next layer of the production plan (the
 * attention runs in whatever form the forward would use), so a test sees what the forward computed, in the reference's
 * NCHW fp32 layout.  One pass only: B must fit the 32-bit offset range (341 images at 256x256). */
typedef struct se_netG_taps {
  float* pmconv6;   /* (B,96,H/4,W/4)  output of pmconv6 = input of the attention   editline_g.py:202 */
  float* attn_out;  /* (B,96,H/4,W/4)  output of cam_2                              editline_g.py:203-207 */
  float* style_vec; /* (B,96)          pooled style vector fed to conv11            editline_g.py:159-167 */
} se_netG_taps;
int se_netG_forward_taps(se_ctx* ctx, void* stream, const float* x, const float* x2, const float* mask,
                         const float* mask2, const float* guide, float* coarse_out, float* fine_out, void* workspace,
                         size_t workspace_bytes, int B, int H, int W, int flags, const se_netG_taps* taps);

/* EditLine2Model.forward(mode='inference') (editline2_model.py:128-133 + generate_fake :338-370):
 * netM -> (mask > 0.5) -> netG -> composed = fine*mask + image*(1-mask) with the SOFT mask.
 * Optional outputs (may be NULL): hard_out (B,1,H,W), maskim_out, coarse_out, fine_out (B,3,H,W)
 * -- the extra tensors of mode='visualize' (:134-145). */
int se_inference(se_ctx* ctx, void* stream, const float* image, const float* sketch, float* composed_out,
                 float* mask_out, float* hard_out, float* maskim_out, float* coarse_out, float* fine_out,
                 void* workspace, size_t workspace_bytes, int B, int H, int W, int flags);

/* se_inference with the output quantisation of test.py:25-27 fused into its last kernel: rgb_out (B,H,W,3) uint8 =
 * trunc((composed + 1) / 2 * 255) in the HWC order test.py:35 transposes to, mask_u8_out (B,H,W) uint8 = trunc(mask * 255)
 * (may be NULL); same fp32 operation order as the reference's tensor expressions, no clamp.  No fp32 output tensor is
 * written at all.  flags as se_inference (GRAPH and PACKED_OUT are ignored). */
int se_inference_u8(se_ctx* ctx, void* stream, const float* image, const float* sketch, unsigned char* rgb_out,
                    unsigned char* mask_u8_out, void* workspace, size_t workspace_bytes, int B, int H, int W, int flags);

/* The INPUT side of test.py's loop on the device (data/testimage_dataset.py:89-111 = ToTensor + Normalize(0.5, 0.5) and
 * `sketch > 0`): image_u8 (B,H,W,3) uint8 RGB as the PNG decoder delivers it -> image_out (B,3,H,W) fp32 = (v/255 - 0.5)/0.5;
 * sketch_u8 (B,H,W) uint8 ('L') -> sketch_out (B,1,H,W) fp32 in {0,1}.  The 256 possible image values are tabulated on the
 * host in IEEE fp32 in that operation order and looked up on the device: bit-identical to the tensors the dataset builds on
 * the CPU.  Either pair may be NULL.  A 4x smaller host-to-device copy for the caller. */
int se_dequantize_u8(se_ctx* ctx, void* stream, const unsigned char* image_u8, const unsigned char* sketch_u8, float* image_out,
                     float* sketch_out, int B, int H, int W);

/* se_inference_u8 fed with the uint8 arrays above: uint8 in, uint8 out -- the whole body of test.py:20-37 between the PNG
 * decoder and the PNG encoder as one call; the fp32 inputs live in the workspace (se_workspace_bytes includes them). */
int se_inference_u8io(se_ctx* ctx, void* stream, const unsigned char* image_u8, const unsigned char* sketch_u8,
                      unsigned char* rgb_out, unsigned char* mask_u8_out, void* workspace, size_t workspace_bytes, int B, int H,
                      int W, int flags);

/* Output quantisation of test.py:25-27 on the device: rgb_out (B,H,W,3) uint8 = trunc((composed + 1) / 2 * 255)
 * in the HWC order test.py:35 transposes to, mask_u8_out (B,H,W) uint8 = trunc(mask * 255); same fp32 operation
 * order as the reference's tensor expressions, no clamp (as test.py; demo.py:62 clamps -- a [-1,1] input cannot
 * leave [0,255] either way).  Either output may be NULL.  A 4x smaller device-to-host copy for the caller. */
int se_quantize_u8(se_ctx* ctx, void* stream, const float* composed, const float* mask, unsigned char* rgb_out,
                   unsigned char* mask_u8_out, int B, int H, int W);

/* ---- the demo's per-request steps on the device (demo.py:39-73, process_image) --------------------------------------
 * Pillow's `Image.resize` of an 'L' or 'RGB' uint8 image, bit for bit: the resampling filters below (values as
 * PIL.Image.Resampling; demo.py uses the default, BICUBIC).  NEAREST, a box and reducing_gap are not provided.  Per axis
 * the host computes Pillow's fixed-point coefficient table in double precision (cached in the ctx per (in, out, filter),
 * the 64 most recently used); the device runs a horizontal pass into a uint8 intermediate and a vertical pass, int32
 * accumulation, each pass skipped where its axis keeps its size (both unchanged: a copy).  The intermediate and the
 * tables live in the ctx (device memory it grows as needed); a call that uses them on another stream than the previous
 * one is ordered after it through an event. */
enum { SE_RESAMPLE_LANCZOS = 1, SE_RESAMPLE_BILINEAR = 2, SE_RESAMPLE_BICUBIC = 3 };

/* in (B,Hin,Win,C) uint8 -> out (B,Hout,Wout,C) uint8, C in {1, 3}: Image.resize((Wout, Hout), filter) of every image.  A
 * filter longer than the kernels take (a bicubic downscale by more than ~2000x) is refused. */
int se_resize_u8(se_ctx* ctx, void* stream, const unsigned char* in, int B, int Hin, int Win, int C, unsigned char* out,
                 int Hout, int Wout, int filter);

/* demo.py:40-56 for ONE request: image_u8 (Hi,Wi,3) RGB and sketch_u8 (Hs,Ws) 'L' uint8, raw sizes (the sketch's may differ
 * from the image's) -> the forward's fp32 inputs at the working size H x W (multiples of 8, >= 16):
 * image_out (3,H,W) = (v/255 - 0.5)/0.5 of the BICUBIC resize (the table se_dequantize_u8 uses), sketch_out (1,H,W) =
 * (resized v > 0).  The last resize pass writes these directly.  The outputs may point into a batch (a request's slot of a
 * (B,3,H,W) / (B,1,H,W) pair).  Either pair may be NULL.  Bit-identical to the host steps with Pillow and torch. */
int se_prepare_u8(se_ctx* ctx, void* stream, const unsigned char* image_u8, int Hi, int Wi, const unsigned char* sketch_u8, int Hs,
                  int Ws, float* image_out, float* sketch_out, int H, int W);

/* The whole of demo.py's process_image for B requests of one raw size as one call: se_prepare_u8 at the working size
 * (Hi/8*8, Wi/8*8), the forward with the fused output quantisation of se_inference_u8 (the demo's clamp cannot change a
 * value: see se_quantize_u8), and the BICUBIC resize of the uint8 result back to Hi x Wi.  image_u8 (B,Hi,Wi,3),
 * sketch_u8 (B,Hs,Ws), rgb_out (B,Hi,Wi,3), all uint8 device arrays.  A working size under 16 is refused, as the demo's
 * host path refuses it.  flags as se_inference_u8; workspace: se_edit_u8_workspace_bytes(ctx, B, Hi, Wi). */
int se_edit_u8(se_ctx* ctx, void* stream, const unsigned char* image_u8, const unsigned char* sketch_u8, unsigned char* rgb_out,
               void* workspace, size_t workspace_bytes, int B, int Hi, int Wi, int Hs, int Ws, int flags);
size_t se_edit_u8_workspace_bytes(se_ctx* ctx, int B, int Hi, int Wi);

/* ---- editing sessions: a frame that stays on the device, edited in place through a window ----------------
 * The forward runs on an H x W window of a larger uint8 frame and the result is pasted back in place; only the window is
 * touched, read or moved.  A window edit is DEFINED as the inference above on the contiguous crop, pasted by the rule of
 * se_window_paste_u8 -- the network sees the window only.  B requests per call, each with its own frame; every step is one
 * launch for the whole group (the records travel through a small table the ctx owns).  wins is a HOST array of B records.
 * H, W multiples of 8, >= 16; every window inside its frame (0 <= y0, y0 + H <= Hi, likewise x); violations return non-zero
 * before anything is enqueued and se_last_error names the argument. */
typedef struct se_window {
  unsigned char* frame_u8;        /* (Hi,Wi,3) RGB uint8, device, contiguous: read by gather, written by paste */
  const unsigned char* sketch_u8; /* the sketch OF THE WINDOW: (H,W) uint8, device (used by gather only) */
  int Hi, Wi, y0, x0;             /* frame size and the window's top-left corner; y0, x0 need NOT be multiples of 8 */
} se_window;

/* the window of each frame -> image_out (B,3,H,W) fp32 through the table se_dequantize_u8 uses, sketch_u8 > 0 -> sketch_out
 * (B,1,H,W): bit-identical to se_dequantize_u8 on a contiguous crop.  Either output may be NULL; outputs 16-byte aligned. */
int se_window_gather_u8(se_ctx* ctx, void* stream, const se_window* wins, int B, int H, int W, float* image_out, float* sketch_out);
/* mask_u8 (B,H,W) (the forward's quantised soft mask) -> hits_out (B,4) int32, DEVICE: pixels with mask_u8 >= 128 on the
 * window's top / bottom / left / right one-pixel edge; a side that lies on the frame's own edge reports 0.  (>= 128 on the
 * quantised mask rather than > 0.5 on the float: the statistic is computable from what the uint8 path produces.) */
int se_window_border_u8(se_ctx* ctx, void* stream, const se_window* wins, int B, int H, int W, const unsigned char* mask_u8,
                        int* hits_out);
/* frame[y0 + y, x0 + x, :] = rgb[b, y, x, :] WHERE mask_u8[b, y, x] > 0; every other byte of the frame is untouched, so pixels
 * the edit did not select stay byte-identical, inside the window too.  rgb (B,H,W,3), mask_u8 (B,H,W), 4-byte aligned.  Two
 * requests of one call must not name overlapping windows of one frame (or frames that overlap in memory): refused. */
int se_window_paste_u8(se_ctx* ctx, void* stream, const se_window* wins, int B, int H, int W, const unsigned char* rgb,
                       const unsigned char* mask_u8);
/* gather -> the forward of se_inference_u8 (fused quantisation) -> border -> paste if commit != 0, as one call without a host
 * synchronisation.  rgb_out (B,H,W,3), mask_u8_out (B,H,W), hits_out (B,4) int32: device, each may be NULL (the workspace then
 * holds it).  flags as se_inference_u8; workspace: se_edit_window_u8_workspace_bytes(ctx, B, H, W).  With commit != 0 the
 * aliasing rule of se_window_paste_u8 applies. */
int se_edit_window_u8(se_ctx* ctx, void* stream, const se_window* wins, int B, int H, int W, unsigned char* rgb_out,
                      unsigned char* mask_u8_out, int* hits_out, int commit, void* workspace, size_t workspace_bytes, int flags);
size_t se_edit_window_u8_workspace_bytes(se_ctx* ctx, int B, int H, int W);

/* ---- window edits at a working size ------------------------------------------------------------------------
 * The hs x ws window of the frame (any sizes >= 16, inside the frame) is resampled into the forward's inputs at the working
 * size H x W (multiples of 8, >= 16), the forward runs there, and its result AND its mask are resampled back to hs x ws and
 * pasted where the resampled mask byte is > 0.  Every resample is Pillow's BICUBIC `Image.resize` bit for bit (se_resize_u8),
 * so a scaled window edit is DEFINED as: se_prepare_u8 of the contiguous crop and of the window's sketch -> the forward of
 * se_inference_u8 -> se_resize_u8 of rgb and of mask_u8 to hs x ws -> the paste rule of se_window_paste_u8; the border counts
 * are taken on the working-size mask, a side counting 0 where the hs x ws window lies on the frame's own edge.  The working
 * size is the caller's policy (serve.choose_working_size); no claim about visual quality is attached to it.  All requests of
 * a call share (hs, ws, H, W); se_window.sketch_u8 is the window's sketch at frame scale, (hs, ws).  With (H, W) == (hs, ws)
 * every entry below is its unscaled counterpart above, byte for byte.  Violations (a window outside its frame, hs / ws < 16,
 * H / W not multiples of 8 or < 16, a resize the kernels' tap limit refuses, overlapping windows where the call writes)
 * return non-zero before anything is enqueued; se_last_error names the argument and the frame is untouched. */
/* the gather end: no contiguous crop is made, and no byte outside a window's own rows is read */
int se_window_gather_resize_u8(se_ctx* ctx, void* stream, const se_window* wins, int B, int hs, int ws, int H, int W,
                               float* image_out, float* sketch_out);
/* the paste end: rgb (B,H,W,3), mask_u8 (B,H,W) at the working size, 4-byte aligned */
int se_window_paste_resize_u8(se_ctx* ctx, void* stream, const se_window* wins, int B, int hs, int ws, int H, int W,
                              const unsigned char* rgb, const unsigned char* mask_u8);
/* gather -> forward -> border -> paste if commit != 0, as one call without a host synchronisation, as se_edit_window_u8.
 * rgb_out (B,H,W,3), mask_u8_out (B,H,W): the forward's outputs AT THE WORKING SIZE; hits_out (B,4); each may be NULL. */
int se_edit_window_scaled_u8(se_ctx* ctx, void* stream, const se_window* wins, int B, int hs, int ws, int H, int W,
                             unsigned char* rgb_out, unsigned char* mask_u8_out, int* hits_out, int commit, void* workspace,
                             size_t workspace_bytes, int flags);
size_t se_edit_window_scaled_u8_workspace_bytes(se_ctx* ctx, int B, int hs, int ws, int H, int W);

/* ---- the undo journal of an editing session ---------------------------------------------------------------
 * A paste changes only bytes inside its window's hs x ws rectangle of the frame, so the rectangle's bytes before the paste
 * are all it takes to undo it.  se_window_save_u8 copies the rectangle of every request into that request's SLOT; enqueued in
 * front of a committing se_edit_window_u8 / se_edit_window_scaled_u8 (or of the paste of an uncommitted run) on the same
 * stream, the slot holds the pre-image.  se_window_swap_u8 EXCHANGES rectangle and slot: after the paste it restores the
 * frame byte for byte (undo) and leaves the edit's result in the slot; the same call again puts it back (redo).
 * A slot is hs rows of round_up(3 ws, 16) bytes in device memory, 16-byte aligned: se_window_saved_bytes(hs, ws) bytes (host
 * only, no ctx, no HIP call; 0 if hs or ws < 16).  A row's padding bytes are unspecified.  slots is a HOST array of B device
 * pointers; se_window.sketch_u8 is not used.  hs, ws >= 16, any values; every window inside its frame.  No byte outside a
 * window's rows is read and none outside the rectangle is written.  Violations (a window outside its frame, hs / ws < 16, a
 * NULL or misaligned slot, slots that overlap each other or a frame, for swap overlapping windows as se_window_paste_u8
 * refuses them) return non-zero before anything is enqueued; se_last_error names the argument, frames and slots untouched. */
size_t se_window_saved_bytes(int hs, int ws);
int se_window_save_u8(se_ctx* ctx, void* stream, const se_window* wins, int B, int hs, int ws, unsigned char* const* slots);
int se_window_swap_u8(se_ctx* ctx, void* stream, const se_window* wins, int B, int hs, int ws, unsigned char* const* slots);

/* ---- locked regions of an editing session ------------------------------------------------------------------
 * A LOCK PLANE is a (Hi,Wi) uint8 plane in device memory that belongs to a frame; a non-zero byte means "no edit may change
 * this pixel".  The lock enters the forward where the mask is made, so that a locked pixel is known context for netG and not
 * a hole it fills: with lock in {0,1} at the forward's size,
 *     mask = where(lock, 0, netM(image, sketch));  hard = mask > 0.5;  netG(image, image, hard, hard, sketch);
 *     composed = fine * mask + image * (1 - mask)          -- composed == image, bit for bit, where locked
 * (generate_fake, models/editline2_model.py:338-370, with the mask netG is given taken from elsewhere than the threshold of
 * netM alone).  lock_u8 (B,H,W) uint8, device: NULL, or all zero, gives se_inference / se_inference_u8 bit for bit.
 * se_inference_locked has every optional output of se_inference; flags as there, GRAPH is ignored. */
int se_inference_locked(se_ctx* ctx, void* stream, const float* image, const float* sketch, const unsigned char* lock_u8,
                        float* composed_out, float* mask_out, float* hard_out, float* maskim_out, float* coarse_out,
                        float* fine_out, void* workspace, size_t workspace_bytes, int B, int H, int W, int flags);
int se_inference_u8_locked(se_ctx* ctx, void* stream, const float* image, const float* sketch, const unsigned char* lock_u8,
                           unsigned char* rgb_out, unsigned char* mask_u8_out, void* workspace, size_t workspace_bytes, int B,
                           int H, int W, int flags);
/* The window entries with locks.  `locks` is a HOST array of B device pointers: locks[b] = the (Hi,Wi) plane of request b's
 * frame, or NULL (that request has no lock).  Sizes as in the scaled entries; (H, W) == (hs, ws) is the unscaled edit.
 * the lock at the working size: lock_out (B,H,W) uint8 in {0,1}, 8-byte aligned.  Unscaled: lock_crop > 0.  Scaled:
 * Image.resize(lock_crop as 'L', (W, H), BICUBIC) > 0 -- the sketch's filter and test, the image's axis tables; bicubic
 * ringing can only add locked pixels.  A row starts at byte (y0 + r) Wi + x0 of the plane, any alignment; no byte outside a
 * window's own rows is read.  A NULL plane gives zeros. */
int se_window_gather_lock_u8(se_ctx* ctx, void* stream, const se_window* wins, const unsigned char* const* locks, int B, int hs,
                             int ws, int H, int W, unsigned char* lock_out);
/* se_window_paste_resize_u8 with the rule  frame[y0 + y, x0 + x, :] = RGB[y, x, :]  WHERE  M[y, x] > 0  AND
 * locks[b][y0 + y, x0 + x] == 0  (RGB, M: rgb and mask_u8 resampled to hs x ws; the arrays themselves when unscaled).  The
 * second condition is tested in frame space, so the ringing of a resampled mask cannot reach a locked pixel: a locked pixel's
 * three bytes never change, at any scale. */
int se_window_paste_locked_u8(se_ctx* ctx, void* stream, const se_window* wins, const unsigned char* const* locks, int B, int hs,
                              int ws, int H, int W, const unsigned char* rgb, const unsigned char* mask_u8);
/* se_edit_window_scaled_u8 with locks: gather, lock gather, the forward of se_inference_u8_locked, border, and the locked
 * paste if commit != 0.  The border counts are taken on the working-size mask, where locked pixels are 0.  With every entry of
 * locks NULL, or every plane zero: the frame, rgb_out, mask_u8_out and the counts of se_edit_window_scaled_u8 / _u8, byte for
 * byte.  Refused before anything is enqueued (frames untouched, se_last_error names the argument): everything the scaled
 * entries refuse, and -- where the call writes frames -- a lock plane that shares a byte with a frame of the call.
 * Setting a lock is not an edit: the journal (6f) neither sees nor restores lock planes. */
int se_edit_window_locked_u8(se_ctx* ctx, void* stream, const se_window* wins, const unsigned char* const* locks, int B, int hs,
                             int ws, int H, int W, unsigned char* rgb_out, unsigned char* mask_u8_out, int* hits_out, int commit,
                             void* workspace, size_t workspace_bytes, int flags);
size_t se_edit_window_locked_u8_workspace_bytes(se_ctx* ctx, int B, int hs, int ws, int H, int W);

/* ---- region edits of an editing session ---------------------------------------------------------------------
 * Where a full-size sketch is drawn: sketch_u8 is an (Hi,Wi) uint8 plane in device memory (its base may have any alignment),
 * cut into tile x tile squares, tile in {16, 32, 64}; the last row / column of squares is ragged where tile does not divide
 * Hi / Wi.  tiles_out (ceil(Hi / tile), ceil(Wi / tile), 5) int32, device, 4-byte aligned: one record [count, y0, x0, y1, x1]
 * per square -- the number of its pixels > 0 and their tight half-open box in FRAME coordinates; five zeros for an empty
 * square.  EVERY record is written (the buffer need not be zeroed) and no byte outside the plane's Hi Wi bytes is read, even
 * inside the same allocation.  Deterministic: one wave per square, shuffle reductions, plain stores, no atomics.  One launch,
 * no workspace (SE_TEST_POISON has nothing to fill).  Refused before anything is enqueued (non-zero return, se_last_error
 * names the argument, tiles_out untouched): Hi or Wi < 16, another tile, a NULL pointer, a misaligned tiles_out. */
int se_sketch_tiles_u8(se_ctx* ctx, void* stream, const unsigned char* sketch_u8, int Hi, int Wi, int tile, int* tiles_out);

/* ---- strokes as polylines ------------------------------------------------------------------------------------
 * The windows' sketches rasterised on the device from a few segments, so that no full-size sketch plane exists anywhere.  A new
 * operation with an integer-only definition, in quarter pixels: the centre of frame pixel (y, x) is P = (4 x + 2, 4 y + 2); a
 * SEGMENT is five int32 [ax, ay, bx, by, r] with 0 <= ax, bx <= 4 Wi, 0 <= ay, by <= 4 Hi, 3 <= r <= 512 and Hi, Wi <= 8192.
 * With d = B - A, e = P - A, f = P - B, t = e.d, dd = d.d, cr = ex dy - ey dx, the segment COVERS the pixel iff, in this order,
 *     t <= 0: e.e <= r r        (a zero-length segment, a dot, always lands here)
 *     t >= dd: f.f <= r r
 *     otherwise: cr cr <= r r dd
 * -- every intermediate fits int64 (cr cr <= 2^62).  sketch_out[b, y, x] = 255 if any segment first .. first + count - 1 of
 * request b covers frame pixel (y0 + y, x0 + x), else 0.
 * wins: a HOST array of B records of which only Hi, Wi, y0, x0 are used; segs: (N,5) int32 in DEVICE memory, 4-byte aligned;
 * ranges: a HOST array (B,2) of [first, count] (ranges may overlap: requests share segments; count 0 gives zeros); sketch_out
 * (B,hs,ws) uint8, device, ANY alignment, hs, ws >= 16 of any value -- slice b has the shape se_window.sketch_u8 takes.  EVERY
 * byte of sketch_out is written on every call (it need not be zeroed) and none outside it; one launch, plain stores, no atomics,
 * no workspace (SE_TEST_POISON has nothing to fill).  The limits on a segment's values are the caller's to keep, the segments
 * being on the device: the kernel clamps what it loads to them, so other values give other pixels, never an access outside
 * segs or sketch_out.  Refused before anything is enqueued (non-zero return, se_last_error names the argument, sketch_out
 * untouched): a NULL pointer, B < 1, hs or ws < 16, a window outside its frame, Hi or Wi > 8192, N < 0 or a range outside
 * [0, N], a misaligned segs, segs overlapping sketch_out. */
int se_sketch_strokes_u8(se_ctx* ctx, void* stream, const se_window* wins, int B, int hs, int ws, const int* segs, int N,
                         const int* ranges, unsigned char* sketch_out);

/* Host only (no HIP call, no ctx): the coefficient table the resize uses for one axis.  Returns ksize, the taps per output
 * (-1: bad arguments); when bounds (2*out ints: first input index, tap count) and k (cap >= out*ksize ints, fixed point
 * with 22 fractional bits, rows zero padded to ksize) are given, fills them.  Lets a test compare the tables with Pillow's. */
int se_resample_coeffs(int in, int out, int filter, int* bounds, int* k, size_t cap);

/* ---- measurement support (no reference counterpart; used by bench.py) ----------------------------
 * se_profile_enable(ctx, 1): wrap every kernel launch of subsequent forwards in a pair of HIP events
 * recorded on the launch stream; se_profile_report synchronises the device and writes a JSON array
 *   [{"kernel": name, "launches": n, "total_ms": t, "flops": algorithmic FLOPs, "bytes": ...}, ...]
 * aggregated per kernel ("kernels"), the same per layer ("layers"), and every launch on its own in launch order
 * ("launches": [{"form": the kernel form the dispatcher chose, "kernel", "layer", "workgroups"}, ...] -- what the tests
 * read to know which kernel ran).  se_profile_enable(ctx, 0) switches it off and drops the records. */
int se_profile_enable(se_ctx* ctx, int on);
int se_profile_report(se_ctx* ctx, char* buf, size_t cap);

/* ---- developer switches (no reference counterpart; used by the tests and the A/B tools) -----------
 * The library's kernel-form switches ("SE_WINOGRAD_F43", "SE_ATT_FUSED", ...) live in ONE process-wide
 * table that is filled from the environment once, at first use; no forward ever calls getenv.  se_debug_set_option
 * changes an entry for every later call of the process (name with or without the "SE_" prefix; returns 0, or 1 for an
 * unknown name), se_debug_get_option reads one, se_debug_reset_options restores the environment / built-in values.
 * "SE_TEST_OFFSET_LIMIT" (settable only here) lowers the byte range the 32-bit-offset kernels may address, so that a
 * test reaches the large-batch passes of the forwards with a few small images.
 * "SE_TEST_POISON" (settable only here; 0, the default: off, nothing is added to any call) with a value v in 1..255 (any other value is off) fills every
 * scratch region with the byte v when it is handed out and before its first producer is enqueued, on that producer's stream:
 * every block of the workspace arenas of the forwards, the scratch the per-op entry points allocate, every region a call
 * carves out of the workspace outside the arenas (the hard / soft masks, the fp32 inputs of the uint8 entries, the rgb /
 * mask / counts / lock regions of the window entries where the caller passed NULL, the resample intermediates) and the
 * ctx-owned resize intermediate at each use -- not the weight images, not the window record ring.  A result that changes
 * with v depends on a byte nobody wrote (tests/test_gpu_poison.py).  While it is set, a call with SE_FLAG_GRAPH runs
 * uncaptured and enters nothing into the graph cache.
 * "SE_PAIR_MIN_PIXELS" (DESIGN.md section 6): in the default mode se_inference, se_inference_locked and the uint8 forwards run a
 * pass of B >= 2 images with B H W >= this value as two half-batch chains on the caller's stream and the ctx's side stream (0:
 * never; never while the profiler is on); results do not depend on it, bit for bit.  se_debug_get_option also answers one
 * derived, read-only name, "SE_PAIR_RULE:B,H,W,exec_flags" (decimal integers): 1 if such a pass is paired, 0 if not -- host
 * arithmetic on the arguments and the switch, no ctx, no device; a malformed query or B, H, W < 1 returns 1.
 * "SE_S2_POLY" (DESIGN.md 3.1g): the polyphase F(2,2) form of the 3x3 stride-2 layers with 48 input channels ("s2poly48"): 0 off,
 * 1 (default) everywhere, 2 netG only.  Two more derived, read-only names answer what that form is built from, on the host:
 * "SE_S2POLY_TABLE:q,j" -- entry j of 1-D position q = 0..4: [source +, source - (or -1), coefficient of w0, w1, w2, fold into
 * o0, o1], the sources indexing the patch in[4t-1 .. 4t+3] of the output pair o0 = out[2t], o1 = out[2t+1]; and
 * "SE_S2POLY_PACK:cout,i" -- the bits of float i of [weight image (cout/96, 38, 96, 32), bias (cout)] as the library's packer
 * (csrc/se_s2poly.h) builds them for the probe layer w.flat[n] = p(n), b[n] = p(10007 + n), p(n) = ((7919 n) % 2053 - 1026) / 1024,
 * w (cout,48,3,3), cout 96 or 192. */
int se_debug_set_option(const char* name, int value);
int se_debug_get_option(const char* name, int* value);
void se_debug_reset_options(void);
/* Which kernel form(s) se_gated_conv2d_ex would launch for this call, without running it: the comma-separated
 * form names of its conv launches as se_profile_report records them, e.g. "wino24", "vecbias,rconv16", "small_conv".  cin1 = 0:
 * one source.  exec_flags: SE_FLAG_LOW_LATENCY | SE_FLAG_BF16 | SE_FLAG_CONSERVATIVE; net_id: the network whose layer it is taken
 * to be (SE_NET_G for the per-op entries).  Needs no ctx and no device: host arithmetic on the arguments and the developer
 * switches.  Returns 1 for a layer se_gated_conv2d_ex refuses or a buffer that is too small. */
int se_debug_gconv_form(int cin, int cin1, int src1_is_vector, int cout, int k, int stride, int rate, int act, int upsample,
                        int B, int H, int W, int exec_flags, int net_id, char* out, size_t cap);

/* ---- per-op entry points (unit tests; same kernels as the forwards) ----------------------------
 * gen_conv / gen_deconv (models/networks/utils.py:9-51): x (B,Cin,H,W) device, w (Cout,Cin,k,k) and
 * b (Cout) HOST, y device (B, Cout/2 or Cout, Ho, Wo).  act: 0 ELU, 1 ReLU, 2 None (raw conv).
 * Supported: gated Cout%8==0 (any Cin, k in {3,5}); raw only for k=3, Cin=12, Cout in {1,3}. */
int se_gated_conv2d(se_ctx* ctx, void* stream, const float* x, const float* w_host, const float* b_host, float* y,
                    int B, int Cin, int H, int W, int Cout, int k, int stride, int rate, int act, int upsample);
/* The same with the options the forwards use: a second source x1 of the virtual channel concat in front of conv11 /
 * allconv11 (editline_g.py:166-167,211) -- a tensor (B,Cin1,H,W), or with x1_is_vector a spatially constant per-image
 * vector (B,Cin1), still zero padded at the borders; w is (Cout, Cin+Cin1, k, k) -- and exec_flags: SE_FLAG_LOW_LATENCY
 * runs the layer in its small-grid launch shape, SE_FLAG_BF16 on the bf16 path (x, x1 and w are rounded to bf16 on the
 * way in, y is the bf16 result widened to fp32).  x1 may be NULL. */
int se_gated_conv2d_ex(se_ctx* ctx, void* stream, const float* x, const float* x1, int x1_is_vector, const float* w_host,
                       const float* b_host, float* y, int B, int Cin, int Cin1, int H, int W, int Cout, int k, int stride,
                       int rate, int act, int upsample, int exec_flags);
/* cam_1 + cam_2 (models/networks/splitcam.py:57-108,147-174 as configured at editline_g.py:35-42,
 * 203-207): x (B,96,h,w), mask_full (B,1,4h,4w) -> out (B,96,h,w); similar_out (B,L,hs,ws) may be NULL.
 * similar_out is the materialised score matrix: where R Rp 4 >= 2^31 (R = h/2 * w/2, Rp = R rounded up to 32 keys, 64 in
 * bf16; from h x w = 153 x 153 on, i.e. 1224 x 1224 inputs) the attention runs in the streaming form, which never forms
 * it, and a non-NULL similar_out is refused (non-zero return, se_last_error); out alone works at every size. */
int se_attention(se_ctx* ctx, void* stream, const float* x, const float* mask_full, float* out, float* similar_out,
                 int B, int h, int w);
/* the same with exec_flags (SE_FLAG_BF16: x is rounded to bf16 on the way in, out is the bf16 result widened to fp32) */
int se_attention_ex(se_ctx* ctx, void* stream, const float* x, const float* mask_full, float* out, float* similar_out,
                    int B, int h, int w, int exec_flags);

/* The kernels between the convolutions, through the launchers the forwards call (tests/test_gpu_glue.py).  Any B, H, W >= 1.
 *
 * Input packing, the first kernel of netM / netG.  net_id SE_NET_M (editline2_g.py:62): x = image (B,3,H,W), guide = sketch
 * (B,1,H,W), the others ignored; packed_out (B,H,W,4) fp32 = [image(3), sketch].  net_id SE_NET_G (editline_g.py:120-135):
 * x, x2 (B,3,H,W), mask, mask2, guide (B,1,H,W); packed_out (B,H,W,8) fp32 = [x (1 - mask) (3), guide, mask, 0, 0, 0], the
 * coarse encoder's input; style_out (B,H,W,8) fp32 = [x2 mask2 (3), guide, mask2, 0, 0, 0], or with SE_FLAG_JOINT_TRAIN_INP
 * in `flags` (B,H,W,4) fp32 = [x2 mask2 (3), mask2]; with SE_FLAG_NO_MASK_CC the three colour channels are x2 itself.
 * With SE_FLAG_BF16 in exec_flags every buffer is instead ONE 16-byte granule per pixel, (B,H,W,8) bf16, the fp32 values
 * above rounded to nearest even in the same channel order, the remaining half-words zero.  The kernels write the caller's
 * buffers directly (device memory, 16-byte aligned): the layout is the contract with the first conv. */
int se_pack_inputs(se_ctx* ctx, void* stream, int net_id, const float* x, const float* x2, const float* mask, const float* mask2,
                   const float* guide, void* packed_out, void* style_out, int B, int H, int W, int flags, int exec_flags);
/* The column reduce over pixels (the pooled style vector, editline_g.py:159-165, and the key norm of the attention): x
 * (B,C,H,W) fp32 -> out (B,C) fp32; op 0: max, 1: mean, 2: 1 / sqrt(sum x^2 + 1e-8).  Deterministic: the same input gives the
 * same bits.  SE_FLAG_BF16: x is rounded to bf16 on the way in (the sums stay fp32).  out_bf16 (B,C) bf16, may be NULL: the
 * result rounded to nearest even, as conv11 reads the style vector in bf16 mode.  Refused (non-zero return, nothing enqueued):
 * C > 256, C % 4 != 0, with SE_FLAG_BF16 C % 8 != 0. */
int se_column_reduce(se_ctx* ctx, void* stream, const float* x, float* out, unsigned short* out_bf16, int B, int C, int H, int W,
                     int op, int exec_flags);
/* The last kernel of every decoder: the 3x3 conv 12 -> cout with its fused epilogue.  x (B,12,H,W) device, w (cout,12,3,3)
 * and b (cout) HOST; with SE_FLAG_BF16 x and w are rounded to bf16 on the way in.  With a = conv(x) + b:
 *   mode 0 (cout 1)  m = lock ? 0 : sigmoid(a) -> out (B,1,H,W);  hard (B,1,H,W) = (m > 0.5);  lock (B,H,W) uint8, non-zero =
 *                    locked (editline2_g.py:94, editline2_model.py:346-347)
 *   mode 1 (cout 3)  tanh(a) -> out (B,3,H,W)
 *   mode 2 (cout 3)  t = tanh(a) -> out;  xnow = t mask + (img (1 - mask)) (1 - mask), or t with no_mask_coarse
 *                    (editline_g.py:124,179-180): (B,H,W,4) fp32 with a zero fourth channel, or with SE_FLAG_BF16 one
 *                    16-byte granule per pixel, (B,H,W,8) bf16, channels 3-7 zero
 *   mode 3 (cout 3)  t = tanh(a) -> out;  v = t mask + img (1 - mask) -> composed (B,3,H,W) (editline2_model.py:132);
 *                    rgb8 (B,H,W,3) uint8 = trunc((v + 1) * 0.5 * 255), m8 (B,H,W) uint8 = trunc(mask * 255) (test.py:25-27)
 * img (B,3,H,W), mask (B,1,H,W).  Every pointer but those a mode needs (0: out; 2: img, mask, xnow; 3: img and mask where
 * composed, rgb8 or m8 is given) may be NULL.  packed != 0 gives the strides of SE_FLAG_PACKED_OUT: one (B,4,H,W) buffer, the
 * composite in planes 0-2 and the soft mask in plane 3 -- mode 0 then takes `out`, mode 3 `mask` and `composed`, with a batch
 * stride of 4 H W floats, each pointing at its plane of image 0. */
typedef struct se_output_conv_io {
  float* out;
  float* hard;
  const unsigned char* lock;
  const float* img;
  const float* mask;
  void* xnow;
  float* composed;
  unsigned char* rgb8;
  unsigned char* m8;
} se_output_conv_io;
int se_output_conv(se_ctx* ctx, void* stream, const float* x, const float* w_host, const float* b_host, int B, int H, int W,
                   int cout, int mode, const se_output_conv_io* io, int no_mask_coarse, int packed, int exec_flags);

#ifdef __cplusplus
}
#endif
#endif
