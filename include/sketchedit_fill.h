/* libsketchedit_hip.so -- fills of a painted region: the caller says where the network MUST change the frame, and
 * netG alone fills it; netM never runs.  Conventions as in sketchedit_hip.h (device pointers owned by the caller, calls only
 * enqueue work, 0 = ok, se_last_error describes a failure).
 *
 * THE DEFINITION, with hole, lock in {0,1} at the forward's size H x W:
 *     hole         = fill & ~lock                       (a locked pixel is never a hole: 6g's promise holds)
 *     coarse, fine = netG(image, image, hole, hole, sketch)          (sketch: the caller's, or all zeros)
 *     composed     = fine * hole + image * (1 - hole)   (== where(hole, fine, image), bit for bit)
 *     rgb, m8      = the uint8 quantisation of se_inference_u8 (m8 is 255 in the hole, 0 elsewhere)
 * A byte plane sets a pixel where its byte is non-zero.  There is no threshold and no grow loop: the hole is known before the
 * forward; the sketch is used as given, not masked by the hole.  No quality is claimed: no trained checkpoint exists here.
 *
 * A FILL PLANE is an (Hi,Wi) uint8 plane on the device that belongs to a frame, as a lock plane does.  A window's planes at the
 * working size: unscaled `crop > 0`; scaled, each plane separately by 6g's rule (Pillow's BICUBIC resize of the crop, `> 0`) --
 * what se_window_gather_lock_u8 computes.  Both planes dilate and the lock wins where they meet.
 *
 * THE PASTE RULE: frame[y0 + y, x0 + x] = RGB[y, x] where M[y, x] > 0 (RGB, M as in 6d / 6e: at a working size the bicubic
 * upsamples of rgb, m8) and fill_plane[y0 + y, x0 + x] != 0 and lock_plane[y0 + y, x0 + x] == 0 -- the last two tested in frame
 * space, so at any scale only painted, unlocked pixels can change, however the upsampled M rings.  It is
 * se_window_paste_locked_u8 (or se_window_paste_feather_u8) given a KEEP plane in place of the lock:
 * keep = 255 where fill == 0 or lock != 0, else 0, which se_fill_keep_u8 writes over the window's rectangle of a frame-sized
 * plane (the pastes read nothing outside the window). */
#ifndef SKETCHEDIT_FILL_H
#define SKETCHEDIT_FILL_H
#include "sketchedit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The definition on fp32 tensors.  image (B,3,H,W); sketch (B,1,H,W) or NULL (zeros); hole_u8 (B,H,W) and lock_u8 (B,H,W) or
 * NULL, uint8, 16-byte aligned; composed_out (B,3,H,W); coarse_out, fine_out (B,3,H,W) and hard_out (B,1,H,W: the hole plane,
 * 16-byte aligned) may be NULL.  workspace: se_workspace_bytes(B, H, W) bytes, 256-byte aligned, a multiple of 16 bytes.
 * flags as se_inference_locked (GRAPH and PACKED_OUT are ignored).  A batch that runs as several passes advances the planes
 * with the images. */
int se_fill(se_ctx* ctx, void* stream, const float* image, const float* sketch, const unsigned char* hole_u8, const unsigned char* lock_u8,
            float* composed_out, float* coarse_out, float* fine_out, float* hard_out, void* workspace, size_t workspace_bytes, int B,
            int H, int W, int flags);

/* The fill of B windows of resident frames, ONE call without a host synchronisation: wins as in se_edit_window_locked_u8 except
 * that wins[i].sketch_u8 may be NULL (a fill without a sketch); holes a HOST array of B device pointers, request i's (Hi,Wi)
 * fill plane (required, every entry); locks the same for the lock planes, an entry or the whole array may be NULL.  hs x ws is
 * the window in the frame, H x W the size of the forward (equal: the frame's own resolution).  rgb_out (B,H,W,3) and
 * mask_u8_out (B,H,W), 4-byte aligned, either may be NULL (the result then stays in the workspace).  The entry NEVER commits:
 * it leaves rgb and m8 where se_edit_window_locked_u8(commit = 0) leaves them and every paste takes them unchanged.
 * With SE_FLAG_RAW_FINE in flags rgb (rgb_out, or its place in the workspace) holds at EVERY pixel the quantisation of netG's
 * `fine` itself, (unsigned char)(int)(((f + 1) * 0.5f) * 255.f), not of the composite where(hole, fine, image): equal to the
 * unflagged result on every hole pixel, the generator's own prediction on every other -- the lift a seamless paste needs on
 * the hole's rim (sketchedit_blend.h).  mask_u8_out is as without the flag, and this is the one entry that honours it. */
size_t se_fill_window_u8_workspace_bytes(se_ctx* ctx, int B, int hs, int ws, int H, int W);
int se_fill_window_u8(se_ctx* ctx, void* stream, const se_window* wins, const unsigned char* const* holes, const unsigned char* const* locks,
                      int B, int hs, int ws, int H, int W, unsigned char* rgb_out, unsigned char* mask_u8_out, void* workspace,
                      size_t workspace_bytes, int flags);

/* The keep planes of B windows, ONE launch: keeps a HOST array of B device pointers to (Hi,Wi) uint8 planes; the hs x ws
 * rectangle at (y0, x0) of keeps[i] becomes 255 where holes[i] is 0 or locks[i] is non-zero there, else 0.  Any hs, ws >= 16 and
 * any alignment of x0, Wi and the planes; no byte outside the rectangle is read or written.  locks, or an entry, may be NULL.
 * Refused: a keep plane that shares a byte with a frame, hole or lock plane of the call, or whose rectangle meets another
 * request's rectangle of the same keep plane. */
int se_fill_keep_u8(se_ctx* ctx, void* stream, const se_window* wins, const unsigned char* const* holes, const unsigned char* const* locks,
                    unsigned char* const* keeps, int B, int hs, int ws);

/* Every refusal happens on the host before anything is enqueued (non-zero return, se_last_error names the argument): what the
 * locked entries refuse, and a NULL holes or holes[i]. */

#ifdef __cplusplus
}
#endif
#endif
