/* libsketchedit_hip.so -- the PNG entries of the editing sessions: a window of a resident frame leaves the device
 * as the zlib stream of a PNG, so that a front end which shows patches in a browser needs no pixel loop on the host and only the
 * compressed bytes cross the bus.  Conventions as in sketchedit_hip.h (device pointers owned by the caller, calls only enqueue
 * work, 0 = ok, se_last_error describes a failure).
 *
 * THE STREAM is a definition, restated in plain Python in tests/png_stream_util.py, and the kernels produce it byte for byte.
 * The source is the hs x ws RGB rectangle at (y0, x0) of a frame, 16 <= hs, ws <= 8192.
 *  1. Filter.  Each row becomes 1 + 3 ws bytes: the filter type, then the residuals.  Two candidates: SUB (type 1) subtracts the
 *     byte 3 to the left, or 0; UP (type 2) the byte above, or 0 on the rectangle's first row.  The row takes the candidate with
 *     the smaller sum of |residual read as int8|; a tie goes to SUB.
 *  2. Stripes.  32 filtered rows form a stripe, the last may be shorter.  Stripes are compressed independently.
 *  3. Tokens.  Each maximal run of n equal bytes inside a stripe: the first byte is a literal; for the remaining r = n - 1, while
 *     r >= 3 a match of length m = min(r, 258) at distance 1 and r -= m; then r literals.  End-of-block after the last token.
 *  4. Code.  The counts of the 286 literal/length symbols, end-of-block counted once.  Huffman lengths by repeatedly removing the
 *     two nodes with the smallest (weight, id): a leaf's id is its symbol, internal nodes take 286, 287, ... as they are made; a
 *     symbol's length is its leaf's depth.  If a length exceeds 15 every non-zero count c becomes (c + 1) >> 1 and the tree is
 *     built again.  Canonical codes (RFC 1951 3.2.2).  The distance alphabet is the single code 0 of length 1.
 *  5. Block.  BFINAL 0, BTYPE 2, HLIT 29, HDIST 0, HCLEN 15; the code-length code is constant: symbols 0-15 have length 4 (the
 *     codeword is the symbol's value), 16-18 length 0; the 287 lengths follow at 4 bits each, no run symbols.  After end-of-block
 *     an empty stored block (000, pad to a byte, 00 00 FF FF): every stripe ends on a byte boundary.
 *  6. Stream.  78 01, the stripes, 01 00 00 FF FF, Adler-32 of all filtered bytes, big-endian.
 * The PNG file around it (signature, IHDR for 8-bit RGB, ONE IDAT, IEND) is the host's: serve.png_from_zlib.  Not claimed: the
 * ratio of an encoder that searches for matches, and filters beyond these two. */
#ifndef SKETCHEDIT_PNG_H
#define SKETCHEDIT_PNG_H
#include "sketchedit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The most bytes the stream of an hs x ws rectangle can take (host only, no ctx, no HIP call; 0 for a side outside [16, 8192]):
 * 2 + sum over stripes of (159 + ceil(15 n / 8)) + 9, n = the stripe's filtered bytes -- a stripe is 1222 header bits, at most 15
 * bits per filtered byte (a literal is one code of at most 15 bits; a match, at most 15 + 5 + 1 bits, stands for 3 bytes or
 * more), at most 15 for end-of-block, 3 + at most 7 of padding, and 4 bytes.  DESIGN.md 6j has the proof. */
size_t se_png_bound(int hs, int ws);

/* Image b = the hs x ws rectangle at (y0, x0) of wins[b].frame_u8, as se_window_save_u8 reads it (sketch_u8 is not used; wins is
 * a HOST array of B records).  Its stream goes to out + b cap (device, any alignment) and its length to sizes_out[b] (device,
 * 8-byte aligned).  Every byte of out[b cap, b cap + sizes_out[b]) is written and none beyond it; frames are only read, and no
 * byte outside a rectangle's rows.  No address depends on a pixel's value except through the sizes, which the bound covers.
 * workspace: se_png_encode_u8_workspace_bytes(ctx, B, hs, ws) bytes, 256-byte aligned (the rows' filter types, the stripes'
 * sizes and checksum parts, one slot of the bound's size per stripe); SE_TEST_POISON fills it.  Three launches, no host
 * synchronisation.  Refused before anything is enqueued (non-zero return, se_last_error names the argument, out untouched): a
 * NULL pointer, B < 1 (or > 65535), a side outside [16, 8192], a window outside its frame, cap < se_png_bound(hs, ws), a short or
 * misaligned workspace, a misaligned sizes_out, out overlapping a frame, the workspace or sizes_out. */
int se_png_encode_u8(se_ctx* ctx, void* stream, const se_window* wins, int B, int hs, int ws, unsigned char* out, size_t cap,
                     unsigned long long* sizes_out, void* workspace, size_t workspace_bytes);
size_t se_png_encode_u8_workspace_bytes(se_ctx* ctx, int B, int hs, int ws);

#ifdef __cplusplus
}
#endif
#endif
