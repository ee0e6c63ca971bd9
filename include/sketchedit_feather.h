/* libsketchedit_hip.so -- the feathered paste of the editing sessions: a window's result enters the resident frame
 * with a soft edge instead of the one-pixel cut of se_window_paste_u8.  Conventions as in sketchedit_hip.h (device pointers owned
 * by the caller, calls only enqueue work, 0 = ok, se_last_error describes a failure).
 *
 * THE RULE is a definition, restated in plain numpy in tests/feather_util.py, and the kernel produces it byte for byte.  Per
 * request: the window is hs x ws at (y0, x0) of an (Hi, Wi, 3) frame, the radius r is 0 .. 16, RGB (hs, ws, 3) and M (hs, ws) are
 * the edit's result and mask at the window's size.
 *  1. sel(y, x) = M[y, x] > 0 and lock[y0 + y, x0 + x] == 0 (no lock plane: the second term is dropped) -- the set the locked paste
 *     writes.
 *  2. Outside the window sel is defined per axis.  On a side of the window that lies on the frame's own edge (y0 == 0,
 *     y0 + hs == Hi, x0 == 0, x0 + ws == Wi: se_window_border_u8's test) the coordinate is clamped into the window; on any other
 *     side the sample is 0.  A sample out of range on both axes is 0 if either axis says 0, else both coordinates are clamped.
 *  3. n = (2r + 1)^2 and c(y, x) = the sum of sel(y + dy, x + dx) over |dy| <= r, |dx| <= r: 1 <= c <= n wherever sel holds.
 *  4. For every sel pixel and channel: frame' = (c RGB + (n - c) frame + (n - 1) / 2) / n, in integers, floor division.
 *  5. Every other byte of the frame is untouched: unselected pixels of the window, locked pixels, everything outside the window.
 * Hence r = 0 is se_window_paste_locked_u8 at (H, W) = (hs, ws) byte for byte, c == n gives RGB exactly, an edit that touches the
 * frame's edge does not fade towards it, and a mask that reaches a side of the window inside the frame fades out there.  No
 * quality is claimed: like max_side, feathering is a policy. */
#ifndef SKETCHEDIT_FEATHER_H
#define SKETCHEDIT_FEATHER_H
#include "sketchedit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SE_FEATHER_MAX_RADIUS 16

/* In place, ONE launch for the B requests: wins is a HOST array of B records (sketch_u8 is not used), locks a HOST array of B
 * device pointers -- request b's (Hi,Wi) uint8 lock plane or NULL -- or NULL for none at all; rgb (B,hs,ws,3) and mask_u8
 * (B,hs,ws) uint8 on the device AT THE WINDOW'S SIZE (a result at a working size is resized first: se_resize_u8, BICUBIC), any
 * alignment; hs, ws >= 16 with no other constraint.  No byte outside a window's own rows of the frame, the lock plane, rgb or
 * mask_u8 is read, and only bytes of sel pixels are written.  No workspace, no host synchronisation.
 * Refused before anything is enqueued (non-zero return, se_last_error names the argument, the frames untouched): everything
 * se_window_paste_locked_u8 refuses -- a window outside its frame, hs or ws < 16, overlapping windows of one frame, a lock plane
 * that shares bytes with a frame of the call -- a radius outside 0 .. 16, NULL rgb / mask_u8. */
int se_window_paste_feather_u8(se_ctx* ctx, void* stream, const se_window* wins, const unsigned char* const* locks, int B, int hs, int ws,
                               int radius, const unsigned char* rgb, const unsigned char* mask_u8);

#ifdef __cplusplus
}
#endif
#endif
