/* libsketchedit_hip.so -- seamless move and clone: the drop of sketchedit_move.h with the object's colour matched
 * to the place it lands in.  The object keeps its own detail and takes the local colour of its new surroundings: F' = P + m, where
 * m is a smooth MEMBRANE that equals F - P on the object's rim.  The membrane is not the solution of a system solved to a
 * tolerance: it is the result of a FIXED SCHEDULE of integer steps, stated below, so it is a definition with the same bytes on
 * every machine.  Conventions as in sketchedit_hip.h (device pointers owned by the caller, calls only enqueue work, 0 = ok, the
 * ctx's last error describes a failure).
 *
 * THE ARGUMENTS are the plain drop's (sketchedit_move.h) without the radius: the frame F (Hi,Wi,3), a lift P with its rectangle (ly0, lx0, lh, lw),
 * the plane S and the box, the optional lock L, an offset within SE_MOVE_MAX_OFFSET, flip in 0 .. 3.  src(p), moved(p) and
 * target(p) are rules 1 and 2 of sketchedit_move.h for any integer p; the mirror formula is applied as written to pixels outside
 * the box too.  OMEGA is the set of targets.
 *
 * LEVEL 0.
 *   1. rectangles  D = the shifted box clipped to the frame; E = D grown by one pixel on each side and clipped to the frame.  An
 *                  empty D is valid and enqueues nothing.  A side of the box is at most SE_BLEND_MAX_SIDE.  Level 0 is the grid
 *                  of E's pixels, its origin at E's corner.
 *   2. states      UNKNOWN: p is in OMEGA.  KNOWN: p is in the frame, not in OMEGA, src(p) lies in the lift rectangle, and one of
 *                  p's four neighbours is in OMEGA.  OUT: everything else.  A locked destination pixel next to the object is
 *                  therefore KNOWN.  A neighbour outside the frame, or one whose source the lift does not hold, is OUT, and OUT
 *                  neighbours are left out of every sum (a Neumann edge): an object pushed over the frame's edge does not blend
 *                  towards the edge (rule 3 of sketchedit_move.h, for the same reason).
 *   3. values      per channel, independently: on KNOWN cells u = 16 (F[p] - P[src(p)]) + 4096, in 16 .. 8176 (a uint16).  The
 *                  offset keeps every intermediate non-negative: floor division and C's division agree.
 *
 * PULL, levels 1 .. T.  Level l has ceil(h / 2) x ceil(w / 2) cells of level l - 1's h x w; T is the first level of 1 x 1.  A cell's
 * children are the up to four cells (2y + a, 2x + b), a, b in {0, 1}, that exist.  If cnt >= 1 of them are KNOWN the cell is KNOWN
 * with u = (2 SUM u + cnt) / (2 cnt) over those; otherwise, if a child is UNKNOWN, the cell is UNKNOWN; otherwise OUT.
 *
 * PUSH, levels T .. 0, for each level in order:
 *   1. initialise  every UNKNOWN cell takes its parent's u -- cell (y >> 1, x >> 1) of level l + 1 after that level's sweeps; at
 *                  level T it takes 4096.
 *   2. sweep       J_l = min(4 << l, 64) red-black Gauss-Seidel sweeps.  A sweep is the half-sweep over the UNKNOWN cells with
 *                  (y + x) & 1 == 0, then the one over those with == 1.  Each cell computes u = (2 SUM u_n + k) / (2 k) over the k
 *                  neighbours (up, down, left, right) that are inside the grid and not OUT; a cell with k == 0 keeps its value;
 *                  KNOWN cells never change.
 *   3. parity      a half-sweep reads only cells of the other parity, so the result does not depend on the order or the grouping
 *                  of the work.
 *
 * RESULT.  For every target and channel F'[p] = clamp(((16 P[src(p)] + u0[p] + 8) >> 4) - 256, 0, 255).  No other byte of the
 * frame changes; P, S and L are only read.
 *
 * WHAT FOLLOWS.  A constant rim difference c gives exactly P + c, clamped (the average of equal values is that value under this
 * rounding).  With no KNOWN cell anywhere the result is the plain drop at r = 0, byte for byte.  Every u lies between the least
 * and the greatest KNOWN value.
 *
 * KNOWN ANSWERS.  Frame 16 x 16, every byte 10; the lift is the whole frame when every byte was 180, except rows 2 .. 3 of columns
 * 2 .. 4, which were 200; S selects those six pixels; box (2, 2, 4, 5); offset (1, 3); flip 0; no lock.  The eighteen bytes of rows
 * 3 .. 4, columns 5 .. 7 become 30 (the rim's difference is 10 - 180 everywhere), and no other byte changes.  With 100 for the
 * object and 250 around it they become 0 (the clamp). */
#ifndef SKETCHEDIT_BLEND_H
#define SKETCHEDIT_BLEND_H
#include "sketchedit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SE_BLEND_MAX_SIDE 2048

/* The workspace of one call for a box of box_h x box_w: two buffers of 8 bytes a cell for every level of the largest E, (box_h +
 * 2) x (box_w + 2).  0 for a side outside 1 .. SE_BLEND_MAX_SIDE. */
size_t se_move_blend_u8_workspace_bytes(int box_h, int box_w);

/* The seamless drop, in place on frame_u8.  Launches: one that classifies E and reads F and P, one per level of the pull, at most
 * 16 per level of the push, one that writes D's targets.  Their number and every loop's trip count depend on E's size alone, never
 * on data in memory; there is no synchronisation between workgroups but the launch boundaries, no atomics, nothing polled, and no
 * host synchronisation.  Any alignment of the frame, the planes and Wi; no byte outside the frame's 3 Hi Wi, the planes' Hi Wi,
 * the slot's rows or the workspace is touched, and every workspace byte the kernels read was written by them. */
int se_move_blend_u8(se_ctx* ctx, void* stream, unsigned char* frame_u8, int Hi, int Wi, const unsigned char* lift, int ly0, int lx0,
                     int lh, int lw, const unsigned char* sel_u8, const unsigned char* lock_u8_or_NULL, int by0, int bx0, int by1,
                     int bx1, int dy, int dx, int flip, void* workspace, size_t workspace_bytes);

/* Every refusal happens on the host before anything is enqueued (non-zero return, the ctx's last error names the argument, the
 * frame, the planes and the workspace are untouched): the refusals of the plain drop (sketchedit_move.h) but the radius', a side of
 * the box above SE_BLEND_MAX_SIDE, a NULL workspace or one smaller than the bytes above, one that is not 16-byte aligned, one that
 * shares bytes with the frame, the lift or a plane. */

#ifdef __cplusplus
}
#endif
#endif
