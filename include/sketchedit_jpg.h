/* libsketchedit_hip.so -- the JPEG entries of the editing sessions: a window of a resident frame leaves the device
 * as the entropy-coded segment of a baseline JPEG, a lossy preview several times smaller than the PNG of 6j.  The resident frame
 * stays byte-exact; only what is sent is lossy.  Conventions as in sketchedit_hip.h (device pointers owned by the caller, calls
 * only enqueue work, 0 = ok, se_last_error describes a failure).
 *
 * THE STREAM is a definition, restated in plain Python in tests/jpg_stream_util.py, and the kernels produce it byte for byte.
 * The source is the hs x ws RGB rectangle at (y0, x0) of a frame, 16 <= hs, ws <= 8192, and a quality 1 .. 100.  Everything is
 * integer arithmetic; every intermediate fits a signed 32-bit int.
 *  1. Colour (JFIF, 16-bit fixed point).  Y = (19595 R + 38470 G + 7471 B + 32768) >> 16,
 *     Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16, Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16
 *     (arithmetic shifts; all three lie in 0 .. 255).  4:4:4 sampling; one MCU is one 8 x 8 block of each, in the order Y, Cb, Cr.
 *  2. Edges.  A side that is no multiple of 8 is extended by repeating the rectangle's last column and last row: the repeated
 *     pixels come from the rectangle, never from the frame behind it.
 *  3. DCT.  A[u][x] = round(8192 * 1/2 * c(u) * cos((2 x + 1) u pi / 16)), c(0) = 1/sqrt 2, else 1 -- the 64 integers
 *       2896  2896  2896  2896  2896  2896  2896  2896      4017  3406  2276   799  -799 -2276 -3406 -4017
 *       3784  1567 -1567 -3784 -3784 -1567  1567  3784      3406  -799 -4017 -2276  2276  4017   799 -3406
 *       2896 -2896 -2896  2896  2896 -2896 -2896  2896      2276 -4017   799  3406 -3406  -799  4017 -2276
 *       1567 -3784  3784 -1567 -1567  3784 -3784  1567       799 -2276  3406 -4017  4017 -3406  2276  -799     (u = 0, 1 / 2, 3 / ...)
 *     Rows: t = sum_x A[u][x] (p[y][x] - 128), |t| <= 128 * 8 * 2896 < 2^22; t1[y][u] = (t + 512) >> 10, |t1| <= 2896.
 *     Columns: s[v][u] = sum_y A[v][y] t1[y][u], |s| < 2^27, the coefficient with 16 fraction bits.
 *  4. Quantise.  c = sign(s) ((|s| + (q << 15)) / (q << 16)), floor division.  q = clamp((base scale + 50) / 100, 1, 255) with
 *     scale = 5000 / Q for Q < 50, else 200 - 2 Q (libjpeg's quality scaling) and base = Annex K's luminance table for Y, its
 *     chrominance table for Cb and Cr.  The 64 coefficients of a block are taken in zigzag order.
 *  5. Entropy code.  Baseline Huffman with the four tables of Annex K (K.3 - K.6), bits packed MSB first.  The DC difference is
 *     taken against the previous block of the same component and is 0 at the start of each restart interval.  A non-zero AC
 *     coefficient with r zeros in front of it is r >> 4 times ZRL (F0), the code of ((r & 15) << 4 | size) and `size` magnitude
 *     bits (v for v > 0, v - 1 in `size` bits for v < 0); EOB (00) when coefficient 63 is zero.
 *  6. Restart intervals.  One interval is one row of MCUs, ceil(ws / 8).  At its end the bits are padded with 1-bits to a byte;
 *     every FF byte of the interval's data (the padded byte included) is followed by 00; then FF D0+(row mod 8) after every row
 *     but the last.
 *  7. The segment is the rows and their markers, no headers.  The file around it (SOI, a JFIF APP0, two DQT, SOF0, four DHT, DRI,
 *     SOS, the segment, EOI) is the host's: serve.jpg_from_scan.
 * Ranges (DESIGN.md 6k has the proofs): |AC| <= 1021 and -1024 <= DC <= 1016 at q = 1, so an AC size is at most 10 and a DC
 * difference's at most 11 -- what the Annex K tables have codes for.  Not claimed: chroma subsampling, optimised tables,
 * progressive mode. */
#ifndef SKETCHEDIT_JPG_H
#define SKETCHEDIT_JPG_H
#include "sketchedit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The most bytes the segment of an hs x ws rectangle can take (host only, no ctx, no HIP call; 0 for a side outside [16, 8192]):
 * ceil(hs / 8) rows of 2 ceil((1660 n + 7) / 8) + 2 bytes, n = 3 ceil(ws / 8) blocks a row -- a block is at most 22 bits of DC
 * and 26 bits per AC coefficient (a token that covers a coefficient and the r zeros in front of it costs at most
 * 11 (r >> 4) + 16 + 10 <= 26 (r + 1) bits, EOB's 4 bits stand for at least one zero), every byte may be followed by a stuffed
 * 00, and a row ends in a marker.  DESIGN.md 6k has the proof. */
size_t se_jpg_bound(int hs, int ws);

/* Image b = the hs x ws rectangle at (y0, x0) of wins[b].frame_u8, as se_window_save_u8 reads it (sketch_u8 is not used; wins is
 * a HOST array of B records).  Its segment goes to out + b cap (device, any alignment) and its length to sizes_out[b] (device,
 * 8-byte aligned).  Every byte of out[b cap, b cap + sizes_out[b]) is written and none beyond it; frames are only read, and no
 * byte outside a rectangle's rows.  No address depends on a pixel's value except through the sizes, which the bound covers.
 * workspace: se_jpg_encode_u8_workspace_bytes(ctx, B, hs, ws) bytes, 256-byte aligned (the int16 coefficients, the rows' sizes,
 * one slot of the row bound's size per row); SE_TEST_POISON fills it.  Three launches, no host synchronisation.  Refused before
 * anything is enqueued (non-zero return, se_last_error names the argument, out untouched): a NULL pointer, B < 1 (or > 65535), a
 * side outside [16, 8192], a quality outside [1, 100], a window outside its frame, cap < se_jpg_bound(hs, ws), a short or
 * misaligned workspace, a misaligned sizes_out, out overlapping a frame, the workspace or sizes_out.  The call is
 * se_jpg2_encode_u8 (sketchedit_jpg2.h) with flags = 0 and no tables_out: the same checks, workspace and launches. */
int se_jpg_encode_u8(se_ctx* ctx, void* stream, const se_window* wins, int B, int hs, int ws, int quality, unsigned char* out,
                     size_t cap, unsigned long long* sizes_out, void* workspace, size_t workspace_bytes);
size_t se_jpg_encode_u8_workspace_bytes(se_ctx* ctx, int B, int hs, int ws);

#ifdef __cplusplus
}
#endif
#endif
