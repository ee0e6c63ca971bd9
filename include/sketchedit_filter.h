/* libsketchedit_hip.so -- blur, sharpen or pixelate a selection: "blur that face", "pixelate that number plate",
 * "sharpen what I just scaled up" -- the selected pixels of a frame replaced by a filter of the frame as it was when it was
 * LIFTED.  Conventions as in sketchedit_hip.h (device pointers owned by the caller, calls only enqueue work, 0 = ok, the ctx's
 * last error describes a failure).  Integer only: the same bytes on every machine.
 *
 * THE ARGUMENTS, as in sketchedit_move.h.  F: an (Hi,Wi,3) uint8 frame, Hi, Wi >= 16.  P: a LIFT, one journal slot in the layout of
 * DESIGN.md 6f -- lh rows of round_up(3 lw, 16) bytes, 16-byte aligned -- that holds the rectangle (ly0, lx0, lh, lw) of the frame
 * as it was before (lh, lw >= 16); below, P[y][x] is the lift's pixel of FRAME row y and column x.  S: an (Hi,Wi) uint8 selection
 * plane, non-zero = selected.  A BOX (by0, bx0, by1, bx1), half open, non-empty, inside the lift rectangle.  L: an optional (Hi,Wi)
 * lock plane.
 *
 * BLUR takes a radius R in 1 .. SE_FILTER_MAX_RADIUS and `taps`, a host pointer to R + 1 ints t[0 .. R], each >= 0, with
 * t[0] + 2 (t[1] + .. + t[R]) == SE_FILTER_ONE.  The lift rectangle must contain the box grown by R and clipped to the frame, so
 * every tap below lies in the lift.  Two passes, per channel:
 *   H[y'][x] = sum over k = -R .. R of t[|k|] P[y'][clamp(x + k, 0, Wi - 1)]                      exact, <= 255 * 4096
 *   B[y][x]  = (sum over k of t[|k|] H[clamp(y + k, 0, Hi - 1)][x] + 2^23) >> 24                  in UNSIGNED 32 bits:
 *              the largest value is 255 * 2^24 + 2^23 = 4 286 578 688 < 2^32; a signed accumulator overflows.
 * MOSAIC takes a cell b in 2 .. SE_FILTER_MAX_CELL.  Cells are anchored at the box's origin (by0, bx0) and clipped to the box
 * (the last row and column of cells may be narrower).  B of every pixel of a cell is (sum + cnt / 2) / cnt per channel, floor
 * division, the sum over ALL cnt pixels of the clipped cell as P holds them, selected or not.  The lift must only contain the box.
 *
 * COMMON.  amount a in SE_FILTER_MIN_AMOUNT .. SE_FILTER_MAX_AMOUNT (Q8), feather f in 0 .. SE_FILTER_MAX_FEATHER.
 *   O         = clamp(P + ((a (P - B) + 128) >> 8), 0, 255), an arithmetic shift.  a = -256 gives B exactly (the blur), a = 0
 *               gives P, a > 0 is an unsharp mask.
 *   target(p) = p lies in the box, S[p] != 0, and there is no lock or L[p] == 0.
 *   c(p)      = the number of e with |ey|, |ex| <= f, p + e in the box and S[p + e] != 0;  n = (2 f + 1)^2.  Neither the frame's
 *               edge nor the lock enters the count.
 *   F'[p]     = (c O + (n - c) P[p] + (n - 1) / 2) / n on targets, floor division; f = 0 stores O.  The blend is against P, not
 *               F: the frame is NEVER read, and there is one writer per byte.
 *   the rest    no other byte changes; P, S, L and taps are only read.
 *
 * KNOWN ANSWERS.  P 16 x 16, every byte 10 in columns 0 .. 7 and 200 in columns 8 .. 15; taps (2048, 1024), R = 1.  Columns 6 .. 9
 * of any row:  B = 10, 58, 153, 200;  a = -128: 10, 34, 177, 200;  a = 256: 10, 0, 247, 200;  a = 1024: 10, 0, 255, 200.
 * Mosaic, b = 3, the box the whole frame: the cell of columns 6 .. 8 is (660 + 4) / 9 = 73, the one-column cell of column 15 is 200. */
#ifndef SKETCHEDIT_FILTER_H
#define SKETCHEDIT_FILTER_H
#include "sketchedit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SE_FILTER_MAX_RADIUS 32
#define SE_FILTER_ONE 4096
#define SE_FILTER_MAX_CELL 64
#define SE_FILTER_MIN_AMOUNT (-256)
#define SE_FILTER_MAX_AMOUNT 1024
#define SE_FILTER_MAX_FEATHER 16

/* The BLUR (and, with amount > 0, the unsharp mask) on frame_u8, in place.  taps: a HOST pointer to radius + 1 ints, read before
 * the call returns.  Only the 64 x 16 tiles of the box are visited, and a tile without a selected pixel loads nothing but its
 * part of S.  Any alignment of the frame, the planes and Wi; no byte outside the frame's 3 Hi Wi, the planes' Hi Wi or the first
 * 3 lw bytes of the slot's rows is touched.  ONE launch, no workspace, no host synchronisation. */
int se_filter_blur_u8(se_ctx* ctx, void* stream, unsigned char* frame_u8, int Hi, int Wi, const unsigned char* lift, int ly0, int lx0,
                      int lh, int lw, const unsigned char* sel_u8, const unsigned char* lock_u8_or_NULL, int by0, int bx0, int by1,
                      int bx1, const int* taps, int radius, int amount, int feather);

/* The MOSAIC on frame_u8, in place: one wave per cell.  As above: ONE launch, no workspace, no host synchronisation. */
int se_filter_mosaic_u8(se_ctx* ctx, void* stream, unsigned char* frame_u8, int Hi, int Wi, const unsigned char* lift, int ly0, int lx0,
                        int lh, int lw, const unsigned char* sel_u8, const unsigned char* lock_u8_or_NULL, int by0, int bx0, int by1,
                        int bx1, int cell, int amount, int feather);

/* Every refusal happens on the host before anything is enqueued (non-zero return, the ctx's last error names the argument, the
 * frame and the planes are untouched): those of DESIGN.md 6r -- a NULL pointer (but the lock), Hi or Wi < 16, a frame of more
 * than one launch takes, a lift rectangle outside the frame or with a side < 16, a lift that is not 16-byte aligned, an empty
 * box or one outside the lift rectangle, a plane or slot that shares bytes with the frame -- and NULL taps, a negative tap, a
 * tap sum other than SE_FILTER_ONE, a radius, cell, amount or feather out of range, a lift rectangle that does not contain the
 * box grown by the radius and clipped to the frame. */

#ifdef __cplusplus
}
#endif
#endif
