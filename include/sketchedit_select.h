/* libsketchedit_hip.so -- selection by colour: "click on it": the region of a resident frame whose colour is
 * similar to a seed pixel's, contiguous with the seed or not, grown by a few pixels -- made where the frame is, as a fill plane
 * in the sense of sketchedit_fill.h.  Conventions as in sketchedit_hip.h (device pointers owned by the caller, calls only
 * enqueue work, 0 = ok, se_last_error describes a failure).
 *
 * THE DEFINITION, for a frame F (Hi,Wi,3) uint8, a seed (sy, sx) inside it, a tolerance t in 0 .. 255, `contiguous` and a
 * grow r in 0 .. SE_SELECT_MAX_GROW:
 *     similar[y, x]  = max over c of |F[y, x, c] - F[sy, sx, c]| <= t          (Chebyshev over the channels; the seed is similar)
 *     reached        = contiguous ? the 4-connected component of `similar` that holds the seed : similar
 *                      (diagonal neighbours do not connect)
 *     selected[y, x] = 255 if a reached pixel lies within Chebyshev distance r of (y, x) inside the frame, else 0
 * The frame's border does not wrap and adds nothing; r = 0 gives selected = 255 reached.
 *
 * A STATE PLANE is an (Hi,Wi) uint8 plane on the device that the caller owns: 0 not similar, 1 similar and not (yet) reached,
 * 255 reached.  se_select_similar_u8 writes every byte of it, se_select_flood_u8 turns 1 into 255 and nothing else,
 * se_select_grow_u8 reads it and writes every byte of another plane.  Any Hi, Wi >= 16 and any alignment of the planes and of
 * Wi; no byte outside a plane's Hi Wi bytes, or outside the frame's 3 Hi Wi, is read or written.
 *
 * THE LOOP is the caller's: se_select_similar_u8; if contiguous, se_select_flood_u8 until a pass stored nothing (its word of
 * changed_out is 0 -- the one download); se_select_grow_u8.  A pass that stored nothing is a fixed point and every pass after
 * it is a no-op, so the state is the same whatever `passes` is.  At most Hi Wi productive passes exist (each reaches a pixel
 * at least).  How many passes a frame takes may vary with timing -- a pass may see a byte its neighbour stores in the same
 * launch, and bytes only go 1 -> 255 -- the fixed point may not: it is unique. */
#ifndef SKETCHEDIT_SELECT_H
#define SKETCHEDIT_SELECT_H
#include "sketchedit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SE_SELECT_MAX_GROW 16
#define SE_SELECT_MAX_PASSES 64

/* state_u8 <- 255 at the seed; elsewhere, for a similar pixel, 1 when `contiguous` is non-zero and 255 when it is 0; 0 for every
 * other pixel.  The seed's colour is read on the device.  ONE launch. */
int se_select_similar_u8(se_ctx* ctx, void* stream, const unsigned char* frame_u8, int Hi, int Wi, int seed_y, int seed_x, int tolerance,
                         int contiguous, unsigned char* state_u8);

/* `passes` (1 .. SE_SELECT_MAX_PASSES) launches of one pass each: a byte of 1 with a reached 4-neighbour becomes 255, closed
 * over every 64 x 64 tile with its one-pixel halo.  changed_out: `passes` device words, 4-byte aligned, EVERY word written: 1 if
 * that pass stored a byte, else 0 (zeroed by the call, then the kernels). */
int se_select_flood_u8(se_ctx* ctx, void* stream, unsigned char* state_u8, int Hi, int Wi, int passes, unsigned* changed_out);

/* plane_out (Hi,Wi), another buffer <- 255 where a byte of 255 of state_u8 lies within Chebyshev distance `grow` (0 ..
 * SE_SELECT_MAX_GROW), else 0; every byte is written.  ONE launch.  The box and the count of the result are
 * se_sketch_tiles_u8's of plane_out. */
int se_select_grow_u8(se_ctx* ctx, void* stream, const unsigned char* state_u8, int Hi, int Wi, int grow, unsigned char* plane_out);

/* Every refusal happens on the host before anything is enqueued (non-zero return, se_last_error names the argument): a NULL
 * pointer, Hi or Wi < 16 (or a plane of more than 2^40 bytes), a seed outside the frame, tolerance outside 0 .. 255, passes
 * outside 1 .. 64, grow outside 0 .. 16, a misaligned changed_out, changed_out or plane_out sharing a byte with state_u8, a
 * state or output plane sharing a byte with the frame. */

#ifdef __cplusplus
}
#endif
#endif
