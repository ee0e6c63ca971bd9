/* libsketchedit_hip.so -- the canvas of an editing session: crop it, extend it, rotate it by quarter turns and
 * mirror it, all as ONE out-of-place gather with integer indices.  Conventions as in sketchedit_hip.h (device pointers owned by
 * the caller, calls only enqueue work, 0 = ok, the ctx's last error describes a failure).
 *
 * THE ARGUMENTS.  I: an (Hi,Wi,C) uint8 array, C = 1 (a plane) or 3 (a frame).  An ORIENTATION o in 0 .. 7.  An output (Hn,Wn,C)
 * with an ORIGIN (oy, ox).  A PAD MODE and, for SE_CANVAS_CONSTANT, a colour of C bytes.
 *
 * THE RULE.
 *   1. orient   bit 0 of o (SE_CANVAS_MIRROR_X) mirrors x, bit 1 (SE_CANVAS_MIRROR_Y) mirrors y, bit 2
 *               (SE_CANVAS_TRANSPOSE) transposes AFTER the mirrors.  (Ho, Wo) = (Hi, Wi) without bit 2 and (Wi, Hi) with it.
 *               With a = y, b = x without bit 2 and a = x, b = y with it, the oriented image is
 *                   O[y, x] = I[(o & 2) ? Hi - 1 - a : a, (o & 1) ? Wi - 1 - b : b]       for 0 <= y < Ho, 0 <= x < Wo.
 *               The named orientations: 0 identity, 1 flip horizontal, 2 flip vertical, 3 rotate by 180 degrees, 4 transpose,
 *               5 a quarter turn counter-clockwise, 6 a quarter turn clockwise, 7 transverse.
 *   2. rect     out[y, x] = O[fold(y + oy, Ho), fold(x + ox, Wo)] for 0 <= y < Hn, 0 <= x < Wn.  Either origin may be negative and
 *               the rectangle may reach past Ho, Wo: a crop, an extension and any mixture of the two are this one rule.
 *   3. fold     fold(i, n) = i for 0 <= i < n.  Outside, by pad mode:
 *                 SE_CANVAS_EDGE      min(max(i, 0), n - 1);
 *                 SE_CANVAS_REFLECT   with the period p = 2 n - 2 and j = i mod p (the floor modulus, 0 <= j < p): j where
 *                                         j < n, else p - j; n = 1 gives 0.  The edge pixel is not repeated.
 *                 SE_CANVAS_CONSTANT  no index: a pixel with y + oy outside [0, Ho) or x + ox outside [0, Wo) takes the
 *                                         colour, byte c of the pixel = (pad_rgb >> 8 c) & 255.
 *   4. NULL     with C = 1 the input may be NULL and is then taken as all zeros.  With SE_CANVAS_CONSTANT and the colour 255 the
 *               output is the plane of the NEW area: 255 where the rectangle lies outside O, 0 inside.
 *   5. the rest the operation is out of place: every byte of out's C Hn Wn is written exactly once, I is only read, and no byte
 *               outside the two arrays is touched.
 *
 * WHAT FOLLOWS.  Orientation 6 followed by orientation 5 is the identity, and so is each of 0, 1, 2, 3, 4 and 7 applied twice.
 * A crop of an extension by the extension's margins gives I back.  The x mirror reverses PIXELS: a pixel's C bytes keep their order.
 *
 * KNOWN ANSWERS.  I = [[1, 2, 3], [4, 5, 6]] (Hi = 2, Wi = 3, C = 1).
 *   o = 6, the 3 x 2 rectangle at (0, 0):                       [[4, 1], [5, 2], [6, 3]]
 *   o = 5, the same rectangle:                                  [[3, 6], [2, 5], [1, 4]]
 *   o = 1, (Hn, Wn) = (2, 5), (oy, ox) = (0, -1), EDGE:          [[3, 3, 2, 1, 1], [6, 6, 5, 4, 4]]
 *   o = 0, (Hn, Wn) = (1, 9), (oy, ox) = (1, -4), REFLECT:       [[4, 5, 6, 5, 4, 5, 6, 5, 4]]
 *   o = 0, (Hn, Wn) = (3, 4), (oy, ox) = (-1, 1), CONSTANT 9:    [[9, 9, 9, 9], [2, 3, 9, 9], [5, 6, 9, 9]]
 *   NULL input, (Hn, Wn) = (3, 4), (oy, ox) = (-1, 1), CONSTANT 255: [[255, 255, 255, 255], [0, 0, 255, 255], [0, 0, 255, 255]] */
#ifndef SKETCHEDIT_CANVAS_H
#define SKETCHEDIT_CANVAS_H
#include "sketchedit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SE_CANVAS_MIRROR_X 1
#define SE_CANVAS_MIRROR_Y 2
#define SE_CANVAS_TRANSPOSE 4
#define SE_CANVAS_EDGE 0
#define SE_CANVAS_REFLECT 1
#define SE_CANVAS_CONSTANT 2
#define SE_CANVAS_MAX_SIDE 32768
#define SE_CANVAS_MAX_OFFSET 1048576

/* The canvas, rule 1 .. 5.  Limits: 1 <= Hi, Wi, Hn, Wn <= SE_CANVAS_MAX_SIDE, C Hi Wi < 2^31, C Hn Wn < 2^31, |oy|, |ox| <=
 * SE_CANVAS_MAX_OFFSET.  Any alignment of in, out, Wi and Wn.  ONE launch -- an orientation without bit 2 walks the output's
 * flat bytes, one with it turns 64 x 32 tiles through the LDS -- no workspace, no atomics, nothing polled, no host
 * synchronisation. */
int se_canvas_u8(se_ctx* ctx, void* stream, const unsigned char* in_or_NULL, int Hi, int Wi, int C, unsigned char* out, int Hn, int Wn,
                     int oy, int ox, int orient, int pad_mode, unsigned pad_rgb);

/* Every refusal happens on the host before anything is enqueued (non-zero return, the ctx's last error names the argument, no
 * buffer is touched): a NULL out, a NULL in with C = 3, C other than 1 or 3, orient outside 0 .. 7, pad_mode outside 0 .. 2, a
 * size or an offset outside the limits above, in and out sharing a byte. */

#ifdef __cplusplus
}
#endif
#endif
