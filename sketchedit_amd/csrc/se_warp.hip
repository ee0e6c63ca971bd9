// Scale and rotate a selection (the rule is stated in include/sketchedit_warp.h and in plain numpy in
// tests/warp_util.py).  Two integer-only kernels, plain vector loads and stores, no atomics, nothing polled, any alignment of the
// frame, the planes and Wi, no byte outside the frame, a plane or the slot's rows read or written.
//
//  taps:        a destination pixel's source position (sy, sx) in Q16 gives the rows iy, iy + 1 and the columns ix, ix + 1.  The
//               two x-taps of a row are neighbours, so a row of taps is ONE span: S[row][ix .. ix + 1] through load4_within and
//               the slot row's six bytes through two, bounded by the pixels xlo .. xhi - 1 = the taps' columns that lie in the
//               box and have weight (ix + 1 has none where fx == 0); a row outside the box or with weight 0 is skipped.
//               BOUNDS: a tap outside the box is never loaded, the box lies inside the lift rectangle and the lift rectangle
//               inside the frame (the host checks all three), so every S address lies in the plane's Hi Wi bytes and every P
//               address in the first 3 lw bytes of a slot row; load4_within reads aligned dwords only where they lie wholly in
//               the span and single bytes of the span otherwise.
//  warp_drop:   the grid covers the 64 x 16 tiles of R, never the frame; 256 lanes, lane tid owns the pixels (tid >> 6) + 4 k,
//               k = 0 .. 3, of column tid & 63, so a wavefront's stores are 192 consecutive bytes of a row.  Lane 0's position of
//               the tile's first pixel is taken in int64 once; the lanes add int32 deltas (|coef| <= 2^20, 15 rows and 63
//               columns: < 2^27).  An affine map takes its extremes at the tile's corners: where their source bounding box misses
//               the box the workgroup returns before any load.  A pixel with a > 0 that is not locked reads its taps of P, its
//               own three frame bytes where a < 65 536, and stores three bytes: one writer per byte.
//  plane_warp:  plane_combine's walk (se_lasso.hip; store_plane_dword): one lane per aligned dword of the output's Hi Wi flat bytes.
#include "../../include/sketchedit_hip.h"
#include "../../include/sketchedit_warp.h"
#include "se_kernels.h"
#include "se_seltile.h"

#include <cstdint>

namespace se {

namespace {

constexpr int WP_W = SEL_W, WP_H = SEL_H;

struct WarpMap {
  long long ayy, ayx, ay0, axy, axx, ax0;
};

// the plane and the box it gathers from
struct WarpSel {
  const unsigned char* sel;
  int Wi, by0, bx0, by1, bx1;
};

// the four taps of one source position: their weights times s (rule 2), the rows and the span of columns they may read
struct Taps {
  int iy, ix, xlo, xhi;
  unsigned w[4];            // (iy, ix), (iy, ix + 1), (iy + 1, ix), (iy + 1, ix + 1)
};

// a(p) of rule 3, and the taps; 0 without a load where no tap can count
__device__ __forceinline__ unsigned warp_taps(const WarpSel& ws, long long sy, long long sx, Taps& t) {
  const long long liy = sy >> 16, lix = sx >> 16;
  if (liy + 1 < ws.by0 || liy >= ws.by1 || lix + 1 < ws.bx0 || lix >= ws.bx1) return 0u;
  const int iy = (int)liy, ix = (int)lix;
  const unsigned fy = (unsigned)(sy >> 8) & 255u, fx = (unsigned)(sx >> 8) & 255u;
  const int xlo = max(ix, ws.bx0), xhi = min(ix + (fx ? 2 : 1), ws.bx1);
  if (xlo >= xhi) return 0u;
  t.iy = iy; t.ix = ix; t.xlo = xlo; t.xhi = xhi;
  unsigned a = 0;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int yy = iy + r;
    const unsigned wy = r ? fy : 256u - fy;
    t.w[2 * r] = t.w[2 * r + 1] = 0u;
    if (wy == 0u || yy < ws.by0 || yy >= ws.by1) continue;
    const unsigned char* row = ws.sel + (size_t)yy * ws.Wi;               // the span: [row + xlo, row + xhi), inside the box's row
    const unsigned u = load4_within(row + ix, row + xlo, row + xhi);
    t.w[2 * r] = (u & 255u) ? wy * (256u - fx) : 0u;
    t.w[2 * r + 1] = ((u >> 8) & 255u) ? wy * fx : 0u;
    a += t.w[2 * r] + t.w[2 * r + 1];
  }
  return a;
}

__global__ void __launch_bounds__(256) warp_drop_kernel(unsigned char* __restrict__ frame, int Wi, Lift lift, WarpSel ws, WarpMap m,
                                                        const unsigned char* __restrict__ lock, int ry0, int rx0, int ry1, int rx1) {
  const int tid = threadIdx.x;
  const int tx0 = rx0 + blockIdx.x * WP_W, ty0 = ry0 + blockIdx.y * WP_H;   // the tile, in frame pixels
  // the tile's first pixel in int64, its corners by int32 deltas
  const long long by = m.ayy * ty0 + m.ayx * tx0 + m.ay0, bx = m.axy * ty0 + m.axx * tx0 + m.ax0;
  const int ayy = (int)m.ayy, ayx = (int)m.ayx, axy = (int)m.axy, axx = (int)m.axx;
  {
    const int dyr = ayy * (WP_H - 1), dyc = ayx * (WP_W - 1), dxr = axy * (WP_H - 1), dxc = axx * (WP_W - 1);
    const long long ymin = by + min(min(0, dyr), min(dyc, dyr + dyc)), ymax = by + max(max(0, dyr), max(dyc, dyr + dyc));
    const long long xmin = bx + min(min(0, dxr), min(dxc, dxr + dxc)), xmax = bx + max(max(0, dxr), max(dxc, dxr + dxc));
    // no tap of the tile lies in the box: nothing to load or store (uniform over the workgroup)
    if ((ymax >> 16) + 1 < ws.by0 || (ymin >> 16) >= ws.by1 || (xmax >> 16) + 1 < ws.bx0 || (xmin >> 16) >= ws.bx1) return;
  }
  const int lx = tid & (WP_W - 1), x = tx0 + lx;
  if (x >= rx1) return;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ly = (tid >> 6) + 4 * k, y = ty0 + ly;
    if (y >= ry1) continue;
    Taps t;
    const unsigned a = warp_taps(ws, by + (long long)(ayy * ly + ayx * lx), bx + (long long)(axy * ly + axx * lx), t);
    if (a == 0u) continue;
    if (lock && lock[(size_t)y * Wi + x]) continue;
    unsigned acc[3] = {0u, 0u, 0u};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const unsigned w0 = t.w[2 * r], w1 = t.w[2 * r + 1];
      if (!(w0 | w1)) continue;
      // the row's taps: six consecutive bytes of the slot row, of which those of the pixels xlo .. xhi - 1 are read
      const unsigned char* prow = lift.row(t.iy + r);
      const unsigned char* at = prow + 3 * (ptrdiff_t)(t.ix - lift.lx0);
      const unsigned char *lo = prow + 3 * (ptrdiff_t)(t.xlo - lift.lx0), *hi = prow + 3 * (ptrdiff_t)(t.xhi - lift.lx0);
      const unsigned u0 = load4_within(at, lo, hi), u1 = load4_within(at + 4, lo, hi);
      acc[0] += w0 * (u0 & 255u) + w1 * (u0 >> 24);
      acc[1] += w0 * ((u0 >> 8) & 255u) + w1 * (u1 & 255u);
      acc[2] += w0 * ((u0 >> 16) & 255u) + w1 * ((u1 >> 8) & 255u);
    }
    unsigned char* dst = frame + ((size_t)y * Wi + x) * 3;                  // the lane's own pixel: inside R, inside the frame
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      unsigned v = acc[ch] + 32768u;
      if (a < 65536u) v += (65536u - a) * (unsigned)dst[ch];
      dst[ch] = (unsigned char)(v >> 16);
    }
  }
}

// n = Hi Wi pixels; lane q owns the aligned dword at (out - mis) + 4 q, mis = out & 3: the pixels 4 q - mis .. + 3
__global__ void __launch_bounds__(256) plane_warp_kernel(WarpSel ws, WarpMap m, unsigned char* __restrict__ out, long n, long ndw) {
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= ndw) return;
  const int mis = (int)((uintptr_t)out & 3);
  const long p0 = 4 * q - mis;                                       // the dword's first pixel (may lie outside [0, n))
  unsigned v = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const long p = p0 + e;
    if (p < 0 || p >= n) continue;
    const int y = (int)(p / ws.Wi), x = (int)(p - (long)y * ws.Wi);
    Taps t;
    if (warp_taps(ws, m.ayy * y + m.ayx * x + m.ay0, m.axy * y + m.axx * x + m.ax0, t) >= 32768u) v |= 255u << (8 * e);
  }
  store_plane_dword(out, p0, n, v);
}

}  // namespace

hipError_t launch_warp_drop(unsigned char* frame, int Hi, int Wi, const unsigned char* lift, int ly0, int lx0, int lw, int lpitch,
                            const unsigned char* sel, const unsigned char* lock, int by0, int bx0, int by1, int bx1, int ry0, int rx0,
                            int rh, int rw, const long long* m, hipStream_t st) {
  (void)Hi;
  const dim3 grid((unsigned)((rw + WP_W - 1) / WP_W), (unsigned)((rh + WP_H - 1) / WP_H));
  const Lift lf{lift, ly0, lx0, lw, lpitch};
  const WarpSel ws{sel, Wi, by0, bx0, by1, bx1};
  const WarpMap wm{m[0], m[1], m[2], m[3], m[4], m[5]};
  // bytes: an upper bound (every pixel of R a target with four taps of its own and a < 65 536): the plane's taps, the lock,
  // the lift's taps, the frame's pixel read and written
  set_launch_cost(0.0, (double)rh * rw * (4.0 + (lock ? 1.0 : 0.0) + 12.0 + 6.0), "warp_drop");
  set_launch_grid((long)grid.x * grid.y);
  ProfScope ps_(st, PL_WARP_DROP);
  hipLaunchKernelGGL(warp_drop_kernel, grid, dim3(256), 0, st, frame, Wi, lf, ws, wm, lock, ry0, rx0, ry0 + rh, rx0 + rw);
  return hipGetLastError();
}

hipError_t launch_plane_warp(const unsigned char* sel, int Hi, int Wi, int by0, int bx0, int by1, int bx1, const long long* m,
                             unsigned char* out, hipStream_t st) {
  const long n = (long)Hi * Wi;
  const long ndw = (n + (long)((uintptr_t)out & 3) + 3) / 4;         // the aligned dwords that hold the output's bytes
  const WarpSel ws{sel, Wi, by0, bx0, by1, bx1};
  const WarpMap wm{m[0], m[1], m[2], m[3], m[4], m[5]};
  // bytes: the output written once; of the plane at most four taps per pixel that lands near the box (bounded by the output)
  set_launch_cost(0.0, (double)n + 4.0 * (double)n, "plane_warp");
  set_launch_grid((ndw + 255) / 256);
  ProfScope ps_(st, PL_PLANE_WARP);
  hipLaunchKernelGGL(plane_warp_kernel, dim3((unsigned)((ndw + 255) / 256)), dim3(256), 0, st, ws, wm, out, n, ndw);
  return hipGetLastError();
}

}  // namespace se
