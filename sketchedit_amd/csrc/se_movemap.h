// The offset / flip map of a move and the box it gathers from (rule 1 of include/sketchedit_move.h): what the drop,
// the shift of the plane (se_move.hip) and the seamless drop (se_blend.hip, 6x) share.
//
//  moved(y, x) = S[q] != 0 with q = (y - dy, x - dx), mirrored about the box by the flip bits, where q lies in the box; else 0.
//                q is a function of the DESTINATION pixel: the kernels gather.  Four neighbouring x have four neighbouring qx,
//                ascending without the x flip and descending with it, so they are one load4_within bounded by the box's row of S
//                (bytes outside the box read as 0 without a load), byte-swapped under the flip.
#pragma once
#include "../../include/sketchedit_move.h"
#include "se_device.h"

namespace se {

struct MoveMap {
  const unsigned char* sel;
  int Wi, by0, bx0, by1, bx1, dy, dx, flip;
  __device__ __forceinline__ int qy(int y) const { return (flip & SE_MOVE_FLIP_Y) ? by0 + by1 - 1 - (y - dy) : y - dy; }
  // the source column of destination column x; the columns x + 1 .. follow it ascending, descending with the x flip
  __device__ __forceinline__ int qx(int x) const { return (flip & SE_MOVE_FLIP_X) ? bx0 + bx1 - 1 - (x - dx) : x - dx; }
  // moved of the destination pixels (y, x .. x + 3): a byte of {0, 1} each
  __device__ __forceinline__ unsigned moved4(int y, int x) const {
    const int sy = qy(y);
    if (sy < by0 || sy >= by1) return 0u;
    const unsigned char* row = sel + (size_t)sy * Wi;                     // the box's row of S: [row + bx0, row + bx1)
    const int sx = qx(x);
    if (flip & SE_MOVE_FLIP_X) {
      if (sx < bx0 || sx - 3 >= bx1) return 0u;
      return bytes_nonzero(__builtin_bswap32(load4_within(row + (sx - 3), row + bx0, row + bx1)));
    }
    if (sx + 3 < bx0 || sx >= bx1) return 0u;
    return bytes_nonzero(load4_within(row + sx, row + bx0, row + bx1));
  }
};

}  // namespace se
