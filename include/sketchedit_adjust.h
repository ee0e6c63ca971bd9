/* libsketchedit_hip.so -- adjust a selection's tone and colour: "brighten that face", "desaturate the background",
 * "stretch the contrast of this region", "make what I just dropped match the place it landed in" -- the selected pixels of a
 * frame replaced by a pointwise function of the frame as it was when it was LIFTED, the function given as a table and a matrix,
 * the table made on the device from histograms of the frame.  Conventions as in sketchedit_hip.h (device pointers owned by the
 * caller, calls only enqueue work, 0 = ok, the ctx's last error describes a failure).  Integer only: the same bytes on every
 * machine.
 *
 * THE ARGUMENTS, as in DESIGN.md 6t.  F: an (Hi,Wi,3) uint8 frame, Hi, Wi >= 16.  P: a LIFT, one journal slot in the layout of
 * DESIGN.md 6f -- lh rows of round_up(3 lw, 16) bytes, 16-byte aligned -- that holds the rectangle (ly0, lx0, lh, lw) of the frame
 * as it was before (lh, lw >= 16); below, P[y][x] is the lift's pixel of FRAME row y and column x.  S: an (Hi,Wi) uint8 selection
 * plane, non-zero = selected.  A BOX (by0, bx0, by1, bx1), half open, non-empty, inside the lift rectangle.  L: an optional (Hi,Wi)
 * lock plane.
 *
 * ADJUST takes `lut`, 3 x 256 bytes on the device, a row per channel (NULL: the identity); `matrix`, a HOST pointer to 12 ints
 * (NULL: none) -- m[c][j] = matrix[3 c + j] in Q12 with |m| <= SE_ADJUST_MAX_COEF, then o[c] = matrix[9 + c] with
 * |o| <= SE_ADJUST_MAX_OFFSET; an amount a in 0 .. SE_ADJUST_ONE_AMOUNT (Q8) and a feather f in 0 .. SE_ADJUST_MAX_FEATHER.  Per
 * target pixel, the table FIRST, then the matrix:
 *   Q[c]      = lut[c][P[c]]
 *   M[c]      = clamp((m[c][0] Q[0] + m[c][1] Q[1] + m[c][2] Q[2] + o[c] + 2048) >> 12, 0, 255), an arithmetic shift, in int32:
 *               the largest magnitude is 3 * 255 * 32768 + 2^20 + 2048 = 26 118 144 < 2^31.  Without a matrix M = Q.
 *   O         = P + ((a (M - P) + 128) >> 8), an arithmetic shift.  a = 256 gives M exactly, a = 0 gives P.
 *   target(p) = p lies in the box, S[p] != 0, and there is no lock or L[p] == 0.
 *   c(p)      = the number of e with |ey|, |ex| <= f, p + e in the box and S[p + e] != 0;  n = (2 f + 1)^2.  Neither the frame's
 *               edge nor the lock enters the count.
 *   F'[p]     = (c O + (n - c) P[p] + (n - 1) / 2) / n on targets, floor division; f = 0 stores O.  The blend is against P, not
 *               F: the frame is NEVER read, and there is one writer per byte.
 *   the rest    no other byte changes; P, S, L, lut and matrix are only read.
 *
 * HIST reads the FRAME, not a lift: for every p of a box with S[p] != 0 (S NULL: every pixel of the box; the lock plays no part)
 * it counts F[p][0], F[p][1], F[p][2] and Y = (77 R + 150 G + 29 B + 128) >> 8 into hist[4][256], uint32, on the device.  All
 * 1024 words are written, zeros included.
 *
 * LUT makes the 768 bytes of a table on the device from one hist record (two for MATCH).  `which` SE_ADJUST_PER_CHANNEL: row c
 * comes from hist[c]; SE_ADJUST_LUMA: all three rows come from hist[3].  With h the row used, N = sum of h and
 * cdf[v] = h[0] + .. + h[v], in unsigned 64 bits, cdf[-1] = 0:
 *   N == 0 (for MATCH also N_ref == 0): the identity row.
 *   SE_ADJUST_STRETCH, clip k in 0 .. SE_ADJUST_MAX_CLIP per mille: t = (N k) / 1000; lo the smallest v with cdf[v] > t; hi the
 *               largest v with N - cdf[v - 1] > t (lo <= hi because 2 t < N); hi == lo: the identity row; otherwise
 *               lut[v] = 0 for v < lo, else min(((v - lo) 255 + (hi - lo) / 2) / (hi - lo), 255).
 *   SE_ADJUST_EQUALIZE: m the smallest v with h[v] > 0, c0 = cdf[m]; N == c0: the identity row; otherwise lut[v] = 0 for v < m,
 *               else ((cdf[v] - c0) 255 + (N - c0) / 2) / (N - c0).
 *   SE_ADJUST_MATCH: lut[v] = the smallest u with cdf_ref[u] N_src >= cdf_src[v] N_ref (u = 255 always qualifies; the products
 *               stay below 2^50 for frames of up to 2^25 pixels).
 *
 * KNOWN ANSWERS.  The grey matrix, rows (1225, 2404, 467), o = 0, the identity table, P = (200, 100, 50): M = 124 in every channel,
 * and a = 128 gives O[0] = 162.  Y(200, 100, 50) = 124.  STRETCH, k = 0, 10 pixels at 50 and 10 at 150: lut[50] = 0, lut[100] = 128,
 * lut[150] = lut[200] = 255.  EQUALIZE, one pixel at 10, one at 20, two at 30: lut[10] = lut[15] = 0, lut[20] = 85, lut[30] = 255.
 * MATCH, source two pixels at 10 and two at 20, reference one at 100 and three at 200: lut[5] = 0, lut[10] = lut[20] = 200. */
#ifndef SKETCHEDIT_ADJUST_H
#define SKETCHEDIT_ADJUST_H
#include "sketchedit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SE_ADJUST_MAX_COEF 32768
#define SE_ADJUST_MAX_OFFSET 1048576
#define SE_ADJUST_ONE_AMOUNT 256
#define SE_ADJUST_MAX_FEATHER 16
#define SE_ADJUST_MAX_CLIP 200
#define SE_ADJUST_STRETCH 0
#define SE_ADJUST_EQUALIZE 1
#define SE_ADJUST_MATCH 2
#define SE_ADJUST_PER_CHANNEL 0
#define SE_ADJUST_LUMA 1

/* ADJUST on frame_u8, in place.  lut_dev_or_NULL: 768 bytes on the device, any alignment; matrix_host_or_NULL: 12 ints on the HOST,
 * read before the call returns.  Only the 64 x 16 tiles of the box are visited, and a tile without a selected pixel loads nothing
 * but its part of S.  Any alignment of the frame, the planes, the table and Wi; no byte outside the frame's 3 Hi Wi, the planes'
 * Hi Wi, the table's 768 or the first 3 lw bytes of the slot's rows is touched.  ONE launch, no workspace, no host
 * synchronisation. */
int se_adjust_u8(se_ctx* ctx, void* stream, unsigned char* frame_u8, int Hi, int Wi, const unsigned char* lift, int ly0, int lx0, int lh,
                 int lw, const unsigned char* sel_u8, const unsigned char* lock_u8_or_NULL, int by0, int bx0, int by1, int bx1,
                 const unsigned char* lut_dev_or_NULL, const int* matrix_host_or_NULL, int amount, int feather);

/* The bytes of workspace HIST needs for a frame of this size (host only): a record of 4096 bytes per workgroup, at most
 * SE_ADJUST_HIST_GROUPS of them.  0 if Hi or Wi < 16. */
#define SE_ADJUST_HIST_GROUPS 256
size_t se_adjust_hist_u8_workspace_bytes(int Hi, int Wi);

/* HIST of the box (by0, bx0, by1, bx1) of the frame, half open, non-empty, inside the frame, into hist_dev: 1024 uint32 on the
 * device, 4-byte aligned.  workspace: 256-byte aligned, every word of it that is read is written first.  The result does not
 * depend on timing or on the grid.  TWO launches, no host synchronisation. */
int se_adjust_hist_u8(se_ctx* ctx, void* stream, const unsigned char* frame_u8, int Hi, int Wi, const unsigned char* sel_u8_or_NULL,
                      int by0, int bx0, int by1, int bx1, unsigned int* hist_dev, void* workspace, size_t workspace_bytes);

/* LUT: hist_src_dev (and, for SE_ADJUST_MATCH only, hist_ref_dev) -> the 768 bytes of lut_dev, any alignment.  ONE launch of one
 * workgroup, no host synchronisation. */
int se_adjust_lut_u8(se_ctx* ctx, void* stream, const unsigned int* hist_src_dev, const unsigned int* hist_ref_dev_or_NULL, int mode,
                     int which, int clip, unsigned char* lut_dev);

/* Every refusal happens on the host before anything is enqueued (non-zero return, the ctx's last error names the argument, the
 * frame and the planes are untouched): those of DESIGN.md 6t for the frame, the lift, the box and the overlaps -- a NULL pointer
 * (but the lock, the table, the matrix, HIST's plane), Hi or Wi < 16, a frame of more than one launch takes, a lift rectangle
 * outside the frame or with a side < 16, a lift that is not 16-byte aligned, an empty box or one outside the lift rectangle (for
 * HIST: the frame), a plane or slot that shares bytes with the frame -- and a matrix entry, amount, feather, mode, which or clip
 * out of range, SE_ADJUST_MATCH without a reference or a reference with another mode, a hist that is not 4-byte aligned, a
 * workspace that is too small or not 256-byte aligned, a table, hist or workspace that shares bytes with the frame or with each
 * other. */

#ifdef __cplusplus
}
#endif
#endif
