/* libsketchedit_hip.so -- move or clone a selection: "drag this over there" -- the selected pixels of a frame,
 * as they were when they were LIFTED, dropped somewhere else in the frame, optionally mirrored and with a soft edge, and the
 * selection's plane shifted the same way.  Conventions as in sketchedit_hip.h (device pointers owned by the caller, calls only
 * enqueue work, 0 = ok, the ctx's last error describes a failure).
 *
 * THE ARGUMENTS.  F: an (Hi,Wi,3) uint8 frame, Hi, Wi >= 16.  P: a LIFT, one journal slot in the layout of DESIGN.md 6f -- lh
 * rows of round_up(3 lw, 16) bytes, 16-byte aligned -- that holds the rectangle (ly0, lx0, lh, lw) of the frame as it was before
 * the move (the journal's save entry on that rectangle makes it; lh, lw >= 16).  S: an (Hi,Wi) uint8 selection plane, non-zero
 * = selected.  A BOX (by0, bx0, by1, bx1), half open, non-empty, inside the lift rectangle.  L: an optional (Hi,Wi) lock plane.
 * An OFFSET (dy, dx), |dy|, |dx| <= SE_MOVE_MAX_OFFSET.  flip in 0 .. 3: bit 0 (SE_MOVE_FLIP_X) mirrors x about the box, bit 1
 * (SE_MOVE_FLIP_Y) mirrors y.  A radius r in 0 .. SE_MOVE_MAX_RADIUS.
 *
 * THE RULE, for a destination pixel p = (y, x) -- any integer pair, in the frame or not:
 *   1. source   qy = y - dy, or by0 + by1 - 1 - (y - dy) with flip bit 1; qx likewise with dx, bx0, bx1 and bit 0.
 *               moved(p) = q lies in the box and S[q] != 0.
 *   2. target   target(p) = p lies in the frame, moved(p), and there is no lock plane or L[p] == 0.
 *   3. count    n = (2r + 1)^2; c(p) = the number of e, |ey| <= r, |ex| <= r, with moved(p + e): 1 <= c <= n on targets.  The count
 *               is taken on the moved selection alone: neither the frame's edge nor the lock enters it, so an object pushed
 *               partly over the edge does not fade towards the edge and one next to a locked pixel keeps its own alpha.
 *   4. blend    for every target and channel, in integers with floor division (the rounding of DESIGN.md 6m):
 *                   F'[p] = (c P[q] + (n - c) F[p] + (n - 1) / 2) / n
 *               r = 0 is a plain copy, and c == n gives P[q] exactly.
 *   5. the rest every other byte of the frame is untouched; P, S and L are only read.  F[p] is read and written by the one thread
 *               that owns p, and the object's pixels come from P, never from F: source and destination may overlap freely.
 *   6. SHIFT    out[p] = 255 if moved(p) else 0 for every p in the frame: every byte of out is written; out is another buffer
 *               than S.
 * c 255 <= 1089 * 255 stays in int32.
 *
 * A KNOWN ANSWER.  Frame 16 x 16, every byte 10; the lift is the whole frame when every byte was 200; S selects rows 2 .. 3,
 * columns 2 .. 4; box (2, 2, 4, 5); offset (1, 3); flip 0; no lock.  moved is rows 3 .. 4, columns 5 .. 7.  With r = 0 those 18
 * bytes become 200.  With r = 1 (n = 9): the four corners have c = 4 and become (4 * 200 + 5 * 10 + 4) / 9 = 94, the two middle
 * pixels have c = 6 and become (6 * 200 + 3 * 10 + 4) / 9 = 137; no other byte changes.  With S[2, 2] = 0 instead and flip 1 the
 * unselected corner lands at row 3, column 7. */
#ifndef SKETCHEDIT_MOVE_H
#define SKETCHEDIT_MOVE_H
#include "sketchedit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SE_MOVE_MAX_OFFSET 16384
#define SE_MOVE_MAX_RADIUS 16
#define SE_MOVE_FLIP_X 1
#define SE_MOVE_FLIP_Y 2

/* The DROP: rule 1 .. 5 on frame_u8, in place.  Only the tiles of the shifted box clipped to the frame are visited; an offset
 * that puts the whole box outside the frame is valid and enqueues nothing.  Any alignment of the frame, the planes and Wi; no
 * byte outside the frame's 3 Hi Wi, the planes' Hi Wi or the slot's rows is touched.  ONE launch, no workspace, no host
 * synchronisation. */
int se_move_drop_u8(se_ctx* ctx, void* stream, unsigned char* frame_u8, int Hi, int Wi, const unsigned char* lift, int ly0, int lx0,
                    int lh, int lw, const unsigned char* sel_u8, const unsigned char* lock_u8_or_NULL, int by0, int bx0, int by1,
                    int bx1, int dy, int dx, int flip, int radius);

/* The SHIFT: rule 6.  plane_out (Hi,Wi) at any alignment; EVERY byte is written (zeros when the whole box lands outside the
 * frame), none outside its Hi Wi.  The box lies inside the frame.  ONE launch, no workspace, no host synchronisation. */
int se_plane_shift_u8(se_ctx* ctx, void* stream, const unsigned char* sel_u8, int Hi, int Wi, int by0, int bx0, int by1, int bx1,
                      int dy, int dx, int flip, unsigned char* plane_out);

/* Every refusal happens on the host before anything is enqueued (non-zero return, the ctx's last error names the argument, the
 * frame and the planes are untouched): a NULL pointer (but the lock), Hi or Wi < 16, a frame of more than one launch takes (Hi >
 * 16 * 65 535 or Hi Wi >= 2^41), a lift rectangle outside the frame or with a side < 16, a lift that is not 16-byte aligned, an
 * empty box or one outside the lift rectangle (the frame, for the shift), |dy| or |dx| > SE_MOVE_MAX_OFFSET, flip outside
 * 0 .. 3, a radius outside 0 .. 16, a plane or slot that shares bytes with the frame, plane_out sharing bytes with sel_u8. */

#ifdef __cplusplus
}
#endif
#endif
