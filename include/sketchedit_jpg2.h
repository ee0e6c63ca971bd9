/* libsketchedit_hip.so -- the JPEG entries of the editing sessions with 4:2:0 sampling and per-image Huffman tables.
 * Conventions as in sketchedit_jpg.h; its entries stay what they are.
 *
 * THE STREAM is sketchedit_jpg.h's rules 1 - 7 with two independent options, restated in plain Python in
 * tests/jpg2_stream_util.py; the kernels produce it byte for byte.  flags = 0 is sketchedit_jpg.h's stream exactly.
 *
 * SE_JPG_420: chroma at half resolution.
 *  2'.  Edges.  A side that is no multiple of 16 is extended by repeating the rectangle's last column and last row (from the
 *       rectangle, never from the frame behind it), before rule 1'': a repeated column enters the averages.
 *  1''. Downsampling.  Y stays at full resolution.  Each Cb and Cr sample is (a + b + c + d + bias) >> 2 over its 2 x 2 pixels of
 *       the extended rectangle, bias = 1 + (x & 1) with x the chroma sample's column in the whole image: 1, 2, 1, 2, ... from 1 in
 *       every row (libjpeg's h2v2 rule).  The result lies in 0 .. 255 as every input does, so rule 3's ranges and 6k's proofs of
 *       |AC| <= 1021 and -1024 <= DC <= 1016 carry over unchanged.
 *  MCU. 16 x 16 pixels, six blocks in the order Y(0,0), Y(0,1), Y(1,0), Y(1,1), Cb, Cr (the Y blocks row-major inside the MCU); Y
 *       with the luminance quantiser and Huffman tables, Cb and Cr with the chrominance ones.  The DC difference is against the
 *       previous block of the same component in this order (for Y(0,0): Y(1,1) of the MCU to the left), 0 at the start of a
 *       restart interval.
 *  6'.  One restart interval is one row of MCUs: ceil(ws / 16) MCUs, 16 pixel rows; the marker after row r is FF D0+(r mod 8).
 *  7'.  The host's file has Y's sampling factors 0x22 in SOF0 and ceil(w / 16) in DRI (serve.jpg_from_scan).
 *
 * SE_JPG_OPTIMIZE: four Huffman tables made for this image.
 *  5a.  Counts.  Four alphabets of 256 symbols: DC luminance, AC luminance, DC chrominance, AC chrominance.  A symbol is counted
 *       once for every time rule 5 emits its code over the whole image, every ZRL and every EOB included.  Every block emits a DC
 *       symbol and either an EOB or a coefficient 63, so no alphabet is empty.
 *  5b.  Lengths.  A 257th symbol, number 256, is added with count 1; it is never emitted.  Lengths by sketchedit_png.h's rule 4:
 *       repeatedly remove the two nodes with the smallest (weight, id), a leaf's id is its symbol, internal nodes take 257, 258,
 *       ... as they are made, a symbol's length is its leaf's depth.  If any length (symbol 256's included) exceeds 16, every
 *       non-zero count c of the 256 real symbols becomes (c + 1) >> 1, symbol 256 keeps count 1, and the tree is built again.
 *  5c.  Codes.  The real symbols with a non-zero count, sorted by (length, symbol), get the canonical codes of Annex C; symbol 256
 *       gets none.  Its leaf keeps the real symbols' Kraft sum strictly below 1, so no code consists of 1-bits only.  With a
 *       single real symbol the table is one code 0 of length 1.
 *  5d.  Every code may be 16 bits long: a coefficient's token (up to three ZRLs, its code, its magnitude bits) up to 74 bits.
 *  5e.  The tables leave the device as one record of 4 x 272 bytes per image, in the order DC lum, AC lum, DC chr, AC chr: per
 *       table the 16 counts of codes per length, then the symbols in code order, zero-padded to 256 -- the payload of a DHT segment
 *       after its class/id byte.  The host writes the four DHT segments with the true symbol counts, not the padding.
 *
 * Clamp.  se_jpg2_code_i16 takes any int16: an AC coefficient is clamped to -1023 .. 1023 and a DC DIFFERENCE to -2047 .. 2047
 * before its size is taken (sizes at most 10 and 11); the predecessor of a DC is the neighbour's coefficient as given.  Inside the
 * ranges above, which se_jpg2_encode_u8's own coefficients keep, neither does anything. */
#ifndef SKETCHEDIT_JPG2_H
#define SKETCHEDIT_JPG2_H
#include "sketchedit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SE_JPG_420 1
#define SE_JPG_OPTIMIZE 2
#define SE_JPG_TABLE_RECORD_BYTES 1088

/* The most bytes the segment of an hs x ws rectangle can take (host only, no ctx, no HIP call; 0 for a side outside [16, 8192] or
 * flags outside 0 .. 3): rows (2 ceil((bits n + 7) / 8) + 2) with rows = ceil(hs / m), m = 16 under SE_JPG_420 and 8 otherwise, n =
 * 6 ceil(ws / 16) resp. 3 ceil(ws / 8) blocks a row, bits = 1665 under SE_JPG_OPTIMIZE and 1660 otherwise: a block is at most
 * 16 + 11 bits of DC and 26 bits per AC coefficient (a token over r zeros and a coefficient costs 16 (r >> 4) + 16 + 10 <=
 * 26 (r + 1) bits, an EOB of at most 16 bits covers at least one zero).  se_jpg_bound(hs, ws) at flags = 0.  DESIGN.md 6l. */
size_t se_jpg2_bound(int hs, int ws, int flags);

/* se_jpg_encode_u8 with `flags`: image b's segment to out + b cap (device, any alignment), its length to sizes_out[b] (device,
 * 8-byte aligned) and, under SE_JPG_OPTIMIZE, its table record to tables_out + 1088 b (device, 16-byte aligned).  Without
 * SE_JPG_OPTIMIZE tables_out is ignored, may be NULL and is not written.  Every byte of out[b cap, b cap + sizes_out[b]) and of
 * the B records is written and nothing else; frames are only read, and no byte outside a rectangle's rows.  workspace:
 * se_jpg2_encode_u8_workspace_bytes(ctx, B, hs, ws, flags) bytes, 256-byte aligned; SE_TEST_POISON fills it.  Five launches with
 * SE_JPG_OPTIMIZE, three without; no host synchronisation.  Refused before anything is enqueued (non-zero return, se_last_error
 * names the argument, nothing written): what se_jpg_encode_u8 refuses, with cap < se_jpg2_bound(hs, ws, flags); flags outside
 * 0 .. 3; under SE_JPG_OPTIMIZE a NULL or misaligned tables_out, or one that overlaps a frame, out, sizes_out or the workspace. */
int se_jpg2_encode_u8(se_ctx* ctx, void* stream, const se_window* wins, int B, int hs, int ws, int quality, int flags,
                      unsigned char* out, size_t cap, unsigned long long* sizes_out, unsigned char* tables_out, void* workspace,
                      size_t workspace_bytes);
size_t se_jpg2_encode_u8_workspace_bytes(se_ctx* ctx, int B, int hs, int ws, int flags);

/* The stages behind the DCT on their own.  coef (device, 2-byte aligned, only read): B images of R rows of nblk blocks of 64 int16
 * in zigzag order, as the blocks kernels leave them; 1 <= R <= 1024; nblk a multiple of 6 under SE_JPG_420, otherwise of 3, at
 * most 3072.  Any int16 is taken: see Clamp above.  cap >= R (2 ceil((bits nblk + 7) / 8) + 2), bits as in se_jpg2_bound.  out,
 * sizes_out, tables_out, the workspace (se_jpg2_code_i16_workspace_bytes(ctx, B, R, nblk, flags), 256-byte aligned) and the
 * refusals as above, coef in the place of the frames.  Four launches with SE_JPG_OPTIMIZE, two without. */
int se_jpg2_code_i16(se_ctx* ctx, void* stream, const short* coef, int B, int R, int nblk, int flags, unsigned char* out, size_t cap,
                     unsigned long long* sizes_out, unsigned char* tables_out, void* workspace, size_t workspace_bytes);
size_t se_jpg2_code_i16_workspace_bytes(se_ctx* ctx, int B, int R, int nblk, int flags);

#ifdef __cplusplus
}
#endif
#endif
