/* libsketchedit_hip.so -- scale and rotate a selection: "make this bigger and turn it" -- the selected pixels of
 * a frame, as they were when they were LIFTED, dropped through an affine map with bilinear interpolation, and the selection's
 * plane warped the same way.  It is the drop of DESIGN.md 6r with a resampling gather in place of the integer offset.
 * Conventions as in sketchedit_hip.h (device pointers owned by the caller, calls only enqueue work, 0 = ok, the ctx's last
 * error describes a failure).  Integer only: the same bytes on every machine.
 *
 * THE ARGUMENTS.  F: an (Hi,Wi,3) uint8 frame, Hi, Wi >= 16.  P: a LIFT, one journal slot in the layout of DESIGN.md 6f / 6r -- lh
 * rows of round_up(3 lw, 16) bytes, 16-byte aligned -- that holds the rectangle (ly0, lx0, lh, lw) of the frame as it was before
 * (lh, lw >= 16).  S: an (Hi,Wi) uint8 selection plane, non-zero = selected.  A BOX (by0, bx0, by1, bx1), half open, non-empty,
 * inside the lift rectangle.  L: an optional (Hi,Wi) lock plane.  A destination rectangle R = (ry0, rx0, rh, rw), non-empty and
 * inside the frame.  The INVERSE map m = (ayy, ayx, ay0, axy, axx, ax0), six signed 64-bit integers in Q16 (65 536 = 1.0) that
 * take a destination pixel to its source position: |ayy|, |ayx|, |axy|, |axx| <= SE_WARP_MAX_COEF, |ay0|, |ax0| <=
 * SE_WARP_MAX_TRANSLATION.
 *
 * THE RULE, for a destination pixel p = (y, x), in int64 with arithmetic shifts:
 *   1. source   sy = ayy y + ayx x + ay0, sx = axy y + axx x + ax0.  An integer value k << 16 is the CENTRE of source row or
 *               column k.  iy = sy >> 16, fy = (sy >> 8) & 255; ix, fx likewise.
 *   2. taps     four: (iy, ix) with weight (256 - fy)(256 - fx), (iy, ix + 1) with (256 - fy) fx, (iy + 1, ix) with fy (256 - fx),
 *               (iy + 1, ix + 1) with fy fx: the weights sum to 65 536.  A tap COUNTS (s = 1) when it lies in the box and S
 *               there is non-zero.  A tap outside the box, or with weight 0, is never read.
 *   3. coverage a(p) = sum of w s, in 0 .. 65 536.
 *   4. target   target(p) = p lies in R, a(p) > 0, and there is no lock plane or L[p] == 0.
 *   5. blend    for every target and channel:  F'[p] = (sum of w s P[tap] + (65 536 - a) F[p] + 32 768) >> 16.
 *               Premultiplied: the object's rim fades into the frame by its coverage, and an unselected neighbour's colour
 *               never bleeds in.  a = 65 536 with integer source positions gives P[q] exactly.  Every term fits int32
 *               (65 536 * 255 + 32 768 < 2^31).
 *   6. the rest every other byte of the frame is untouched; P, S and L are only read.  F[p] is read and written by the one thread
 *               that owns p, and the object's pixels come from P, never from F: source and destination may overlap freely.
 *   7. WARP     out[p] = 255 if a(p) >= 32 768 else 0 for every p of the frame (half coverage): every byte of out is written;
 *               out is another buffer than S.
 * Bilinear taps undersample below a scale of 1/2: there is no prefilter.
 *
 * KNOWN ANSWERS.  Frame 16 x 16, every byte 10; the lift is the whole frame when every byte was 200; S selects rows 2 .. 3,
 * columns 2 .. 3; box (2, 2, 4, 4); R the frame; no lock.
 *   m = (65536, 0, 0, 0, 65536, -32768), half a pixel to the right: rows 2 .. 3, columns 2, 3, 4 become 105, 200, 105 --
 *     (32 768 * 200 + 32 768 * 10 + 32 768) >> 16 = 105 -- and the warped plane is rows 2 .. 3, columns 2 .. 4.
 *   m = (65536, 0, -32768, 0, 65536, -32768), half a pixel down too: rows 2 .. 4, columns 2 .. 4 become
 *     58 105 58 / 105 200 105 / 58 105 58 -- a corner has a = 16 384: (16 384 * 200 + 49 152 * 10 + 32 768) >> 16 = 58 -- and the
 *     warped plane is the plus shape of the five pixels with a >= 32 768. */
#ifndef SKETCHEDIT_WARP_H
#define SKETCHEDIT_WARP_H
#include "sketchedit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SE_WARP_MAX_COEF (1 << 20)
#define SE_WARP_MAX_TRANSLATION (1ll << 40)

/* The DROP: rule 1 .. 6 on frame_u8, in place.  m: a HOST pointer to the six values, read before the call returns.  Only the
 * 64 x 16 tiles of R are visited, and a tile whose source positions all miss the box loads nothing; a map that lands nothing in
 * R is valid.  Any alignment of the frame, the planes and Wi; no byte outside the frame's 3 Hi Wi, the planes' Hi Wi or the
 * slot's rows is touched.  ONE launch, no workspace, no host synchronisation. */
int se_warp_drop_u8(se_ctx* ctx, void* stream, unsigned char* frame_u8, int Hi, int Wi, const unsigned char* lift, int ly0, int lx0,
                    int lh, int lw, const unsigned char* sel_u8, const unsigned char* lock_u8_or_NULL, int by0, int bx0, int by1,
                    int bx1, int ry0, int rx0, int rh, int rw, const long long* m);

/* The WARP: rule 7.  plane_out (Hi,Wi) at any alignment; EVERY byte is written, none outside its Hi Wi.  The box lies inside
 * the frame.  m as above.  ONE launch, no workspace, no host synchronisation. */
int se_plane_warp_u8(se_ctx* ctx, void* stream, const unsigned char* sel_u8, int Hi, int Wi, int by0, int bx0, int by1, int bx1,
                     const long long* m, unsigned char* plane_out);

/* Every refusal happens on the host before anything is enqueued (non-zero return, the ctx's last error names the argument, the
 * frame and the planes are untouched): those of DESIGN.md 6r -- a NULL pointer (but the lock), Hi or Wi < 16, a frame of more
 * than one launch takes, a lift rectangle outside the frame or with a side < 16, a lift that is not 16-byte aligned, an empty
 * box or one outside the lift rectangle (the frame, for the warp), a plane or slot that shares bytes with the frame -- and a
 * NULL m, a coefficient above SE_WARP_MAX_COEF or a translation above SE_WARP_MAX_TRANSLATION in magnitude, an R that is empty
 * or outside the frame, plane_out sharing bytes with sel_u8. */

#ifdef __cplusplus
}
#endif
#endif
