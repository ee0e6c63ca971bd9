/* libsketchedit_hip.so -- the outline of a selection: the boundary of the pixels a plane selects, extracted where
 * the plane is, as records in the lasso's edge format -- 16 bytes per boundary run come down, not the plane.
 * Conventions as in sketchedit_hip.h (device pointers owned by the caller, calls only enqueue work, 0 = ok, se_last_error
 * describes a failure).  Units as in sketchedit_lasso.h: int32 QUARTER PIXELS of the frame; the corner (X, Y) of the pixel lattice
 * is (4 X, 4 Y), the centre of pixel (y, x) is (4 x + 2, 4 y + 2).  A plane is (Hi,Wi) uint8, 16 <= Hi, Wi <= 8192; a pixel is
 * SELECTED iff its byte is non-zero, and everything outside the frame is unselected (a lock plane is a valid input as it is).
 *
 * SIDES.  A selected pixel (y, x) has a boundary side N / S / E / W iff its neighbour above / below / right / left is unselected.
 * Every boundary side of the set belongs to exactly one selected pixel: the frame's border needs no special case.
 * RUNS.  The frame is cut into SE_OUTLINE_TILE x SE_OUTLINE_TILE tiles, ragged at the right and bottom.  A run is a maximal
 * sequence of pixels of ONE tile, consecutive along x (N, S) or along y (E, W), that all have that side.  Runs are split at tile
 * boundaries and nowhere else.
 * RECORDS.  One run is one record [ax, ay, bx, by] -- an edge of sketchedit_lasso.h, so the output is a valid `edges` argument of
 * se_lasso_fill_u8 -- oriented clockwise on the screen (y down), the interior on the right of the direction of travel.  For a run
 * over the pixels x0 .. x1 - 1 of row y, or y0 .. y1 - 1 of column x:
 *     N  [4 x0, 4 y, 4 x1, 4 y]              S  [4 x1, 4 y + 4, 4 x0, 4 y + 4]
 *     E  [4 x + 4, 4 y0, 4 x + 4, 4 y1]      W  [4 x, 4 y1, 4 x, 4 y0]
 * ORDER.  Tiles in row-major order.  Within a tile all N runs, then all S runs, both sorted by (y, x) of the run's first pixel;
 * then all E runs, then all W runs, both sorted by (x, y).
 * CAPACITY.  With `total` records and the caller's `cap`, exactly the first written = min(total, cap) records in that order are
 * written.  A run holds at least one side and a unit edge of the corner lattice carries at most one, so total <= 2 Hi Wi + Hi + Wi
 * < 2^28 -- which may exceed SE_OUTLINE_MAX_CAP: such an outline (noise over a frame of thousands of pixels on a side) is counted,
 * and no single call returns all of it.
 *
 * Known answers: one selected pixel (y, x) gives [4x,4y,4x+4,4y] [4x+4,4y+4,4x,4y+4] [4x+4,4y,4x+4,4y+4] [4x,4y+4,4x,4y]; a fully
 * selected 64 x 64 frame gives 4 records, 100 x 90 gives 8, 65 x 129 gives 10; the checkerboard gives 8192 records at 64 x 64 and
 * 18 200 at 130 x 70.
 *
 * PROPERTY.  se_lasso_fill_u8 of all the records of a plane is 255 (plane != 0), bit for bit: corners lie at multiples of 4 and
 * centres at 4 k + 2, so no centre lies on an edge; only the vertical records count for the lasso's rule. */
#ifndef SKETCHEDIT_OUTLINE_H
#define SKETCHEDIT_OUTLINE_H
#include "sketchedit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SE_OUTLINE_TILE 64
#define SE_OUTLINE_MAX_CAP (1 << 24)

/* the bytes se_outline_u8 needs for an (Hi,Wi) plane (a multiple of 256); 0, and se_last_error, for a side outside 16 .. 8192 */
size_t se_outline_u8_workspace_bytes(se_ctx* ctx, int Hi, int Wi);

/* edges_out ((cap,4) int32, 4-byte aligned; may be NULL when cap == 0) <- the first min(total, cap) records of `plane` ((Hi,Wi)
 * uint8 on the device, any alignment; no byte outside its Hi Wi is read); info_out (2 int32, 4-byte aligned) <- {total, written}.
 * No other byte of edges_out is written, and none outside the buffers.  THREE launches on `stream` (count, scan, emit; two when cap == 0), the
 * launch boundary their only synchronisation.  `workspace`: se_outline_u8_workspace_bytes(ctx, Hi, Wi) bytes, 256-byte aligned
 * (the tiles' run counts, scanned in place); its contents on entry play no part. */
int se_outline_u8(se_ctx* ctx, void* stream, const unsigned char* plane, int Hi, int Wi, int* edges_out, int cap, int* info_out,
                  void* workspace, size_t workspace_bytes);

/* Every refusal happens on the host before anything is enqueued (non-zero return, se_last_error names the argument, the outputs
 * are untouched): a NULL pointer (except edges_out when cap == 0), Hi or Wi < 16 or > 8192, cap outside 0 .. SE_OUTLINE_MAX_CAP,
 * edges_out or info_out not 4-byte aligned, a workspace that is NULL, too small or not 256-byte aligned, any two of plane,
 * edges_out, info_out and workspace sharing a byte. */

#ifdef __cplusplus
}
#endif
#endif
