/* libsketchedit_hip.so -- lasso selections and the algebra of selections: "draw an outline around it", and
 * "this selection minus that one" -- both made where the frame is, as fill planes in the sense of sketchedit_fill.h.
 * Conventions as in sketchedit_hip.h (device pointers owned by the caller, calls only enqueue work, 0 = ok, se_last_error
 * describes a failure).  Units as in se_sketch_strokes_u8: coordinates are int32 in QUARTER PIXELS of the frame; the centre of
 * frame pixel (y, x) is P = (px, py) = (4 x + 2, 4 y + 2).  16 <= Hi, Wi <= 8192.
 *
 * THE LASSO.  An EDGE is four int32 [ax, ay, bx, by], 0 <= ax, bx <= 4 Wi, 0 <= ay, by <= 4 Hi.  A lasso is N edges, 0 <= N <=
 * SE_LASSO_MAX_EDGES: the edges of one or more closed rings, each ring's closing edge included; nothing in the rule knows which
 * ring an edge belongs to, or in what order the edges come.  For pixel (y, x):
 *     the edge SPANS the pixel's scanline  iff  (ay <= py) != (by <= py)
 *                                          (half open: a horizontal edge never spans, a vertex on a scanline counts once)
 *     s = (px - ax) (by - ay) - (py - ay) (bx - ax)
 *     a spanning edge COUNTS               iff  by > ay ? s > 0 : s < 0       (its crossing lies strictly left of the centre)
 *     selected[y, x] = 255 if an odd number of edges count, else 0            (even-odd: a ring inside a ring is a hole, and so
 *                                                                              is the middle of a self-crossing outline)
 * Every intermediate is held in int64: the factors are below 2^15 + 64 in magnitude, so |s| < 2^31.1.
 * A centre on a top or right boundary is in, one on a left or bottom boundary is out.  On a 6 x 8 frame the ring (6,6) (26,6)
 * (26,18) (6,18) selects exactly rows 1 .. 3, columns 2 .. 6; the ring (0,0) (4 Wi,0) (4 Wi,4 Hi) (0,4 Hi) selects every pixel.
 * The selected pixels lie in rows [ceil((min_y - 2) / 4), floor((max_y - 3) / 4) + 1) and columns [floor((min_x - 2) / 4) + 1,
 * floor((max_x - 2) / 4) + 1) of the edges' end points (a bound, not the tight box).
 * What the kernel loads is clamped to [0, 4 * 8192] -- a no-op on valid edges -- so a buffer of other contents gives the rule's
 * result on the clamped values and never an access outside the buffers.
 *
 * COMBINE.  Planes are (Hi,Wi) uint8, non-zero = selected; the output is always 0 / 255:
 *     SE_COMBINE_ADD a | b    SE_COMBINE_SUBTRACT a & ~b    SE_COMBINE_INTERSECT a & b    SE_COMBINE_XOR a ^ b
 *     SE_COMBINE_INVERT ~a  (b must be NULL)
 *
 * GROW.  A lasso's plane is a valid state plane of sketchedit_select.h (0 / 255): se_select_grow_u8 grows it as it is. */
#ifndef SKETCHEDIT_LASSO_H
#define SKETCHEDIT_LASSO_H
#include "sketchedit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SE_LASSO_MAX_EDGES 65536
#define SE_LASSO_MAX_EXTENT 8192

#define SE_COMBINE_ADD 0
#define SE_COMBINE_SUBTRACT 1
#define SE_COMBINE_INTERSECT 2
#define SE_COMBINE_XOR 3
#define SE_COMBINE_INVERT 4

/* plane_out (Hi,Wi) <- the lasso of `edges` ((N,4) int32 on the device, 4-byte aligned; may be NULL when N == 0): EVERY byte is
 * written (N == 0: zeros), none outside its Hi Wi; any alignment of plane_out.  ONE launch, no workspace. */
int se_lasso_fill_u8(se_ctx* ctx, void* stream, const int* edges, int N, int Hi, int Wi, unsigned char* plane_out);

/* out (Hi,Wi) <- a `op` b, every byte written as 0 / 255; a, b and out at any alignment, each its own.  out may be exactly a,
 * exactly b, or share no byte with either.  ONE launch, no workspace. */
int se_plane_combine_u8(se_ctx* ctx, void* stream, const unsigned char* a, const unsigned char* b, int Hi, int Wi, int op,
                        unsigned char* out);

/* Every refusal happens on the host before anything is enqueued (non-zero return, se_last_error names the argument, the outputs
 * are untouched): a NULL pointer (except edges when N == 0, and b for SE_COMBINE_INVERT), a non-NULL b for SE_COMBINE_INVERT,
 * Hi or Wi < 16 or > 8192, N outside 0 .. 65536, a misaligned edges, edges sharing a byte with plane_out, an op outside 0 .. 4,
 * out overlapping a or b other than being identical to it. */

#ifdef __cplusplus
}
#endif
#endif
