// Lasso selections and the algebra of selections (the rules are stated in include/sketchedit_lasso.h and in
// plain Python integers in tests/lasso_util.py).  Two integer-only kernels, plain vector loads and stores, no atomics, nothing
// polled, any alignment of the planes and of Wi, no byte outside a plane (or the edge buffer) read or written:
//
//  lasso_fill:    polygon scan conversion by the even-odd rule on pixel centres, in quarter pixels.  sketch_strokes' shape: one
//                 workgroup = one 64 x 16 tile of the frame, one lane = 4 consecutive pixels of a row.  The edges are walked in
//                 chunks of 256, one per lane; a lane keeps its edge if the edge's half-open y-span holds the py of one of the
//                 tile's rows and min(ax, bx) lies below the tile's largest px (an edge wholly to the right never counts).  Kept
//                 edges are compacted into LDS (a ballot and a prefix count per wave, the waves' totals through LDS), ORIENTED
//                 UPWARDS (ay < by): swapping an edge's ends negates s and swaps the rule's two cases, so "spans and counts"
//                 becomes ay <= py < ay + dy and (px - ax) dy - (py - ay) dx > 0, the rule's value bit for bit.  Every lane
//                 toggles four parity bits over the kept edges; the span test and (py - ay) dx are shared by its four pixels.
//                 An edge wholly LEFT of a tile is tested per pixel like every other: there is no per-row parity fold.
//  plane_combine: out = a op b as 0 / 255.  The output's Hi Wi flat bytes are walked in the ALIGNED dwords that hold them (a lane
//                 owns one: four consecutive pixels; single bytes at the plane's two ends); a and b are read at their own
//                 alignments through aligned dwords bounded by their own bytes.  One writer per byte.  out may be exactly a or
//                 exactly b: a lane's four input pixels are then the very dword (or end bytes) it stores, read before it is
//                 written, and nobody else reads them -- an aligned address needs no second dword and a bounded one reads only
//                 bytes inside the plane.
#include "../../include/sketchedit_hip.h"
#include "../../include/sketchedit_lasso.h"
#include "se_device.h"
#include "se_kernels.h"

#include <cstdint>

namespace se {

namespace {

// What is loaded is clamped to [0, 4 * 8192] -- a no-op on valid edges -- so that every intermediate fits int64 whatever the
// buffer holds: |dx|, |dy| <= 2^15 and |px - ax|, |py - ay| < 2^15 + 2^8 (a lane's pixels may lie up to 63 columns / 15 rows
// past the frame; they are not stored), hence |s| < 2^31.1.
__global__ void __launch_bounds__(256) lasso_fill_kernel(const int* __restrict__ edges, int N, int Hi, int Wi, unsigned char* __restrict__ out) {
  constexpr int CHUNK = 256, LIM = 4 * SE_LASSO_MAX_EXTENT;
  __shared__ int s_ax[CHUNK], s_ay[CHUNK], s_dx[CHUNK], s_dy[CHUNK];
  __shared__ int s_wave_n[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tx0 = blockIdx.x * 64, ty0 = blockIdx.y * 16;                       // the tile, in frame pixels
  const int tx1 = min(tx0 + 64, Wi), ty1 = min(ty0 + 16, Hi);
  const int cx1 = 4 * (tx1 - 1) + 2;                                            // the tile's largest px
  const int x = tx0 + 4 * (tid & 15), y = ty0 + (tid >> 4);
  const int n = y < Hi ? max(0, min(4, Wi - x)) : 0;                           // the lane's pixels inside the frame
  const long long px = 4 * x + 2, py = 4 * y + 2;
  unsigned par = 0;                                                             // bit p: an odd number of edges count at pixel x + p
  for (int base = 0; base < N; base += CHUNK) {                                // (block-uniform: every lane meets the barriers)
    bool keep = false;
    int ax = 0, ay = 0, bx = 0, by = 0;
    if (base + tid < N) {
      const int* e = edges + 4 * ((size_t)base + tid);
      ax = min(max(e[0], 0), LIM); ay = min(max(e[1], 0), LIM);
      bx = min(max(e[2], 0), LIM); by = min(max(e[3], 0), LIM);
      // the first row of the tile whose py is >= min(ay, by) (ceil((lo - 2) / 4) = (lo + 1) >> 2 for lo >= 0): the span
      // [lo, hi) holds a py of the tile iff that row is one of the tile's and its py is < hi
      const int lo = min(ay, by), hi = max(ay, by);
      const int r = max(ty0, (lo + 1) >> 2);
      keep = r < ty1 && 4 * r + 2 < hi && min(ax, bx) < cx1;
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) s_wave_n[wave] = __popcll(m);
    __syncthreads();                              // the totals are there, and the previous chunk's tests are over
    int at = __popcll(m & ((1ull << lane) - 1ull)), kept = 0;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      at += v < wave ? s_wave_n[v] : 0;
      kept += s_wave_n[v];
    }
    if (keep) {                                   // oriented upwards: (ay < by); a kept edge is never horizontal
      const bool up = by > ay;
      s_ax[at] = up ? ax : bx; s_ay[at] = up ? ay : by;
      s_dx[at] = up ? bx - ax : ax - bx; s_dy[at] = up ? by - ay : ay - by;
    }
    __syncthreads();
    if (n > 0) {
      for (int i = 0; i < kept; ++i) {
        const long long ey = py - s_ay[i], dy = s_dy[i];
        if (ey < 0 || ey >= dy) continue;                                      // the edge does not span this scanline
        const long long t = ey * s_dx[i], ex0 = px - s_ax[i];
#pragma unroll
        for (int p = 0; p < 4; ++p) par ^= (ex0 + 4 * p) * dy - t > 0 ? 1u << p : 0u;
      }
    }
  }
  if (n > 0) {
    unsigned char* a = out + (size_t)y * Wi + x;
    const unsigned v = ((par & 1u) ? 0xffu : 0u) | ((par & 2u) ? 0xff00u : 0u) | ((par & 4u) ? 0xff0000u : 0u) | ((par & 8u) ? 0xff000000u : 0u);
    if (n == 4 && ((uintptr_t)a & 3) == 0) {
      *(unsigned*)a = v;
    } else {
      for (int e = 0; e < n; ++e) a[e] = (unsigned char)((v >> (8 * e)) & 255u);
    }
  }
}

// n = Hi Wi pixels; lane q owns the aligned dword at (out - mis) + 4 q, mis = out & 3: the pixels 4 q - mis .. + 3.  (No
// __restrict__: out may be a or b.)
__global__ void __launch_bounds__(256) plane_combine_kernel(const unsigned char* a, const unsigned char* b, unsigned char* out, long n, int op,
                                                            long ndw) {
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= ndw) return;
  const int mis = (int)((uintptr_t)out & 3);
  const long p0 = 4 * q - mis;                                       // the dword's first pixel (may lie outside [0, n))
  const unsigned ua = load4_within(a + p0, a, a + n);
  const unsigned ub = b ? load4_within(b + p0, b, b + n) : 0u;
  unsigned v = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const bool sa = ((ua >> (8 * e)) & 255u) != 0, sb = ((ub >> (8 * e)) & 255u) != 0;
    const bool s = op == SE_COMBINE_ADD ? sa || sb : op == SE_COMBINE_SUBTRACT ? sa && !sb : op == SE_COMBINE_INTERSECT ? sa && sb :
                   op == SE_COMBINE_XOR ? sa != sb : !sa;
    v |= s ? 255u << (8 * e) : 0u;
  }
  store_plane_dword(out, p0, n, v);
}

}  // namespace

hipError_t launch_lasso_fill(const int* edges, int N, int Hi, int Wi, unsigned char* plane_out, hipStream_t st) {
  const dim3 grid((unsigned)((Wi + 63) / 64), (unsigned)((Hi + 15) / 16));
  // bytes: every tile reads the edges (an upper bound: the L2 serves most of it), the plane written once
  set_launch_cost(0.0, (double)Hi * Wi + 16.0 * (double)N * grid.x * grid.y, "lasso_fill");
  set_launch_grid((long)grid.x * grid.y);
  ProfScope ps_(st, PL_LASSO_FILL);
  hipLaunchKernelGGL(lasso_fill_kernel, grid, dim3(256), 0, st, edges, N, Hi, Wi, plane_out);
  return hipGetLastError();
}

hipError_t launch_plane_combine(const unsigned char* a, const unsigned char* b, int Hi, int Wi, int op, unsigned char* out, hipStream_t st) {
  const long n = (long)Hi * Wi;
  const long ndw = (n + (long)((uintptr_t)out & 3) + 3) / 4;         // the aligned dwords that hold the output's bytes
  // bytes: a (and b) read once, the output written once
  set_launch_cost(0.0, (b ? 3.0 : 2.0) * (double)n, "plane_combine");
  set_launch_grid((ndw + 255) / 256);
  ProfScope ps_(st, PL_PLANE_COMBINE);
  hipLaunchKernelGGL(plane_combine_kernel, dim3((unsigned)((ndw + 255) / 256)), dim3(256), 0, st, a, b, out, n, op, ndw);
  return hipGetLastError();
}

}  // namespace se
