/* libsketchedit_hip.so -- modify a selection's shape: "Select > Modify" -- expand or contract a selection by a
 * round brush, or smooth it by a majority vote in a disc -- made where the selection is, as fill planes in the sense of
 * sketchedit_fill.h.  Conventions as in sketchedit_hip.h (device pointers owned by the caller, calls only enqueue work, 0 = ok,
 * se_last_error describes a failure).  Integers only: the same bytes on every machine.
 *
 * Planes are (Hi,Wi) uint8, non-zero = selected, as for the algebra of selections; the output is always 0 / 255.
 * 16 <= Hi, Wi <= 8192.  A radius r is an int in 1 .. SE_MODIFY_MAX_RADIUS.
 *
 * THE DISC.  D(r) is the set of offsets (dy, dx) with dy^2 + dx^2 <= r^2.  It holds
 *     5, 13, 29, 49, 81, 197, 797, 3001 and 3209 offsets for r = 1, 2, 3, 4, 5, 8, 16, 31 and 32
 * -- known answers: a single selected pixel at least r pixels away from every border expands to exactly that many pixels.
 *
 * THE DEFINITION, for pixels p and q of the frame:
 *     SE_MODIFY_EXPAND    out[p] = 255 iff some selected q inside the frame has q - p in D(r).  Outside the frame adds nothing.
 *     SE_MODIFY_CONTRACT  out[p] = 255 iff p is selected and no unselected q inside the frame has q - p in D(r).  Outside the
 *                         frame removes nothing: a selection that touches the frame's edge does not shrink away from it, and a
 *                         full plane contracts to a full plane (DESIGN.md 6m's rule: an edit at the image border does not fade
 *                         towards it).  So contract(S, r) = invert(expand(invert(S), r)) exactly.
 *     SE_MODIFY_SMOOTH    a majority vote in the disc: c[p] = the number of selected pixels among the in-frame pixels of
 *                         p + D(r), n[p] = the number of those in-frame pixels (c, n <= 3209);
 *                         out[p] = 255 iff 2 c > n, or 2 c == n and p is selected.  It removes specks and pinholes smaller than
 *                         half a disc and rounds corners.
 * A BORDER is not an entry of its own; it is composed with the subtraction of DESIGN.md 6p:
 *     inside = S - contract(S, r)      outside = expand(S, r) - S      both = expand(S, r) - contract(S, r) */
#ifndef SKETCHEDIT_MODIFY_H
#define SKETCHEDIT_MODIFY_H
#include "sketchedit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SE_MODIFY_MAX_RADIUS 32

#define SE_MODIFY_EXPAND 0
#define SE_MODIFY_CONTRACT 1
#define SE_MODIFY_SMOOTH 2

/* out (Hi,Wi), another buffer <- `plane` modified by `op` (SE_MODIFY_*) at `radius`: EVERY byte of out is written, as 0 / 255,
 * and none outside its Hi Wi; both planes and Wi at any alignment.  ONE launch, no workspace, no download. */
int se_plane_modify_u8(se_ctx* ctx, void* stream, const unsigned char* plane, int Hi, int Wi, int op, int radius, unsigned char* out);

/* Every refusal happens on the host before anything is enqueued (non-zero return, se_last_error names the argument, out is
 * untouched): a NULL pointer, Hi or Wi outside 16 .. 8192, an op outside 0 .. 2, a radius outside 1 .. 32, out sharing a byte with
 * plane (a workgroup reads a halo that another one stores: in place would be a race, so it is refused, not allowed). */

#ifdef __cplusplus
}
#endif
#endif
