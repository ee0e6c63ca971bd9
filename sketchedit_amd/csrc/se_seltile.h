// The selection tile: what the operators on a selection share on the device -- the feathered paste (se_feather.hip),
// move (se_move.hip, 6r), scale / rotate (se_warp.hip, 6s: the lift only), the filters (se_filter.hip, 6t) and adjust (se_adjust.hip,
// 6u).  One workgroup = one SEL_W x SEL_H tile, 256 lanes; lane tid owns the 4 consecutive pixels 4 (tid & 15) .. of row tid >> 4.
//
//  c(y, x) = the number of selected pixels in the (2r + 1) x (2r + 1) box around (y, x); n = (2r + 1)^2.  Over LDS in three steps:
//   stage: the kernel's own: sel of the tile and its r-wide halo, (16 + 2r) x (64 + 2r) bytes of {0, 1}, row pitch SEL_PITCH, four
//          pixels (one dword) per lane and step; stage_sel_in_box is the plain one, S != 0 inside a box of the frame.
//   rows:  count_rows: for every staged row the 64 horizontal sums over 2r + 1 columns, a byte each (<= 33): a lane forms four
//          neighbouring sums from the 2r + 4 bytes under them, the first by adding up, the next three by sliding.
//   sum:   count4: a lane adds the 2r + 1 dwords of row sums above and below its pixels, two 16-bit fields per register
//          (33 x 33 < 2^16).
//  blend   BoxDiv: (c v + (n - c) old + (n - 1) / 2) / n, and v itself where c == n.  The division is exact: q = mulhi(u, floor(2^32
//          / n) + 1) equals u / n while u (m n - 2^32) < 2^32 with m n - 2^32 <= n, and u <= 255 n + (n - 1) / 2 < 2^19, n <= 1089.
//  store   store_targets: se_window.hip's ownership rule: three dwords where all four pixels are targets and the address is
//          aligned, single bytes of targets otherwise; each byte has one writer.  No atomics.
#pragma once
#include "../../include/sketchedit_adjust.h"
#include "../../include/sketchedit_feather.h"
#include "../../include/sketchedit_filter.h"
#include "../../include/sketchedit_move.h"
#include "se_device.h"

namespace se {

constexpr int SEL_W = 64, SEL_H = 16, SEL_RMAX = 16;
constexpr int SEL_PITCH = 192;                        // bytes: 48 dwords = 16 mod 32, two rows of 16 dword reads share no bank
constexpr int SEL_ROWS = SEL_H + 2 * SEL_RMAX;        // staged rows at the largest radius
constexpr int SEL_LDS_BYTES = SEL_ROWS * SEL_PITCH + SEL_ROWS * SEL_W;      // staged sel, then its row sums (row pitch SEL_W bytes)
static_assert(SE_FEATHER_MAX_RADIUS == SEL_RMAX && SE_MOVE_MAX_RADIUS == SEL_RMAX && SE_FILTER_MAX_FEATHER == SEL_RMAX &&
                  SE_ADJUST_MAX_FEATHER == SEL_RMAX, "one tile serves every operator: the four limits are its largest radius");

// the lift: the slot's row of frame row y is [row(y), row(y) + 3 lw), its pixel x at 3 (x - lx0)
struct Lift {
  const unsigned char* p;
  int ly0, lx0, lw, lpitch;
  DEVFN const unsigned char* row(int y) const { return p + (size_t)(y - ly0) * lpitch; }
};

// S != 0 of the pixels (y, x .. x + 3) that lie in the box, a byte of {0, 1} each; nothing outside the box's row of S is read
DEVFN unsigned sel4_in_box(const unsigned char* sel, int Wi, int by0, int bx0, int by1, int bx1, int y, int x) {
  if (y < by0 || y >= by1 || x + 3 < bx0 || x >= bx1) return 0u;
  const unsigned char* row = sel + (size_t)y * Wi;
  return bytes_nonzero(load4_within(row + x, row + bx0, row + bx1));
}

// S != 0 of the lane's pixels (y, x .. x + 3) inside a tile that ends at (ty1, tx1): a byte of {0, 1} each, and their number
DEVFN unsigned select_targets(const unsigned char* sel, int Wi, int y, int x, int ty1, int tx1, int& npx) {
  npx = 0;
  if (y >= ty1 || x >= tx1) return 0u;
  npx = min(4, tx1 - x);
  const unsigned char* srow = sel + (size_t)y * Wi + x;                     // the lane's bytes of S: [srow, srow + npx)
  return bytes_nonzero(load4_within(srow, srow, srow + npx));
}
// ... and the locked ones cleared: the lock's bytes of the lane's npx pixels are read where some pixel is still set.  Two calls,
// since the callers' __syncthreads_or and early return lie between them: a helper must not hide a barrier behind a return.
DEVFN unsigned unlocked_targets(unsigned tg, const unsigned char* lock, int Wi, int y, int x, int npx) {
  if (!lock || !tg) return tg;
  const unsigned char* lrow = lock + (size_t)y * Wi + x;                    // the lane's bytes of the lock: [lrow, lrow + npx)
  return tg & ~bytes_nonzero(load4_within(lrow, lrow, lrow + npx));
}

// stage: staged (i, j) = S != 0 in the box at (ty0 - r + i, tx0 - r + j): neither the frame's edge nor the lock enters the count
DEVFN void stage_sel_in_box(unsigned* s_sel, const unsigned char* sel, int Wi, int by0, int bx0, int by1, int bx1, int ty0, int tx0, int r,
                            int tid) {
  const int rows = SEL_H + 2 * r, cols4 = (SEL_W + 2 * r + 3) >> 2;         // the staged rows, and dwords per staged row
  for (int t = tid; t < rows * cols4; t += 256) {
    const int i = t / cols4, j4 = t % cols4;
    s_sel[i * (SEL_PITCH / 4) + j4] = sel4_in_box(sel, Wi, by0, bx0, by1, bx1, ty0 - r + i, tx0 - r + 4 * j4);
  }
}

// rows: s_row (i, x) = sum of staged (i, x .. x + 2r), four neighbouring x per lane and step
DEVFN void count_rows(const unsigned* s_sel, unsigned* s_row, int rows, int r, int tid) {
  for (int t = tid; t < rows * (SEL_W / 4); t += 256) {
    const int i = t >> 4, k = t & 15;
    const unsigned* s = s_sel + i * (SEL_PITCH / 4) + k;                    // staged columns 4k ..
    const int nb = 2 * r + 4, nd = (nb + 3) >> 2;                           // bytes under the four sums, and their dwords
    unsigned char e[2 * SEL_RMAX + 4];
#pragma unroll
    for (int q = 0; q < (2 * SEL_RMAX + 4) / 4; ++q) {
      const unsigned d = q < nd ? s[q] : 0u;
#pragma unroll
      for (int z = 0; z < 4; ++z) e[4 * q + z] = (unsigned char)((d >> (8 * z)) & 255u);
    }
    unsigned s0 = 0;
#pragma unroll
    for (int z = 0; z < 2 * SEL_RMAX + 1; ++z) s0 += z <= 2 * r ? e[z] : 0u;
    // e[2r + 1 ..]: a compile-time walk with a run-time pick, so that e stays in registers
    unsigned in1 = 0, in2 = 0, in3 = 0;
#pragma unroll
    for (int z = 1; z < 2 * SEL_RMAX + 4; ++z) {
      in1 = z == 2 * r + 1 ? e[z] : in1;
      in2 = z == 2 * r + 2 ? e[z] : in2;
      in3 = z == 2 * r + 3 ? e[z] : in3;
    }
    const unsigned s1 = s0 - e[0] + in1, s2 = s1 - e[1] + in2, s3 = s2 - e[2] + in3;
    s_row[i * (SEL_W / 4) + k] = s0 | (s1 << 8) | (s2 << 16) | (s3 << 24);
  }
}

// sum: c[p] = the count of the lane's pixel p: the 2r + 1 rows of sums from staged row ly on, dword k = tid & 15 of each
DEVFN void count4(const unsigned* s_row, int ly, int k, int r, unsigned c[4]) {
  unsigned lo = 0, hi = 0;                                                  // pixels 0, 2 and 1, 3 in 16-bit fields
  for (int d = 0; d <= 2 * r; ++d) {
    const unsigned v = s_row[(ly + d) * (SEL_W / 4) + k];
    lo += v & 0x00ff00ffu;
    hi += (v >> 8) & 0x00ff00ffu;
  }
  c[0] = lo & 0xffffu; c[1] = hi & 0xffffu; c[2] = lo >> 16; c[3] = hi >> 16;
}

// the blend by the count: n = (2r + 1)^2 and the division by it
struct BoxDiv {
  unsigned n, magic, half;
  DEVFN explicit BoxDiv(unsigned n_) : n(n_), magic((unsigned)((1ull << 32) / n_) + 1u), half((n_ - 1u) >> 1) {}
  DEVFN unsigned blend(unsigned cp, unsigned v, unsigned old) const { return cp == n ? v : __umulhi(cp * v + (n - cp) * old + half, magic); }
};
DEVFN unsigned box_area(int r) { return (unsigned)((2 * r + 1) * (2 * r + 1)); }

// store: the 12 bytes o of the lane's 4 pixels at dst, of which the pixels with a set byte in tg are written
DEVFN void store_targets(unsigned char* dst, const unsigned o[3], unsigned tg) {
  if (tg == 0x01010101u && ((size_t)dst & 3) == 0) {
    unsigned* d = (unsigned*)dst;
    d[0] = o[0]; d[1] = o[1]; d[2] = o[2];
    return;
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    if ((tg >> (8 * p)) & 1u) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const int j = 3 * p + ch;
        dst[j] = (unsigned char)((o[j >> 2] >> (8 * (j & 3))) & 255u);
      }
    }
  }
}

}  // namespace se
