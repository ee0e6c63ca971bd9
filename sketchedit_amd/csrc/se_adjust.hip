// Adjust a selection's tone and colour (the rule is stated in include/sketchedit_adjust.h and in plain numpy
// in tests/adjust_util.py).  Four integer-only kernels, plain vector loads and stores, no global atomics (the histogram adds in
// LDS), nothing polled, any alignment of the frame, the planes, the table and Wi, no byte outside the frame, a plane, the table's
// 768 or the first 3 lw bytes of the slot's rows read or written.
//
//  adjust:      the grid covers se_seltile.h's tiles of the BOX, never the frame.  The frame is only WRITTEN: every input pixel
//               comes from the lift.
//                select: select_targets; no selected pixel in the tile: return before any other load.  Then unlocked_targets; no
//                        target left: return.
//                stage:  the table's 768 bytes -> LDS, a dword per lane of the first 192 (load4_within: any alignment); with f > 0
//                        stage_sel_in_box and count_rows.
//                point:  a target's lane reads its 12 bytes of the lift (three bounded dwords), looks each byte up, applies the
//                        matrix in int32, mixes by the amount, blends by the count (count4, BoxDiv).  Stores: store_targets.
//  hist_tiles:  at most SE_ADJUST_HIST_GROUPS workgroups stride over the box's 64 x 16 tiles; 4 x 4 x 256 counters in LDS, a
//               sub-histogram per WAVE.  A flat selection (what select_similar makes) puts every lane on one counter: a wave whose
//               active lanes all hold one value adds their number once, from one lane; otherwise each lane adds 1.  At the end
//               the four sub-histograms are added and the workgroup writes its 1024 words to its own slab of the workspace.
//  hist_sum:    1024 lanes, one per word: the slabs added in slab order into the caller's record.  Integer sums of values that
//               do not depend on which workgroup took which tile: the same words for every grid and timing.
//  adjust_lut:  one workgroup, a lane per value v: the rows' prefix sums in LDS in unsigned 64 bits, then the mode's rule; MATCH
//               by a binary search over cdf_ref.  768 byte stores, one writer each.
#include "../../include/sketchedit_hip.h"
#include "../../include/sketchedit_adjust.h"
#include "se_kernels.h"
#include "se_seltile.h"

namespace se {

namespace {

typedef unsigned long long u64;

constexpr int AJ_LUT_BYTES = 768;

// the matrix by value: m[3 c + j], then o[c]; on = 0: none
struct AdjustMatrix {
  int m[12];
  int on;
};

__global__ void __launch_bounds__(256) adjust_kernel(unsigned char* __restrict__ frame, int Wi, Lift lift, const unsigned char* __restrict__ sel,
                                                     const unsigned char* __restrict__ lock, int by0, int bx0, int by1, int bx1,
                                                     const unsigned char* __restrict__ lut, AdjustMatrix mx, int amount, int f) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_mem[];
  unsigned* s_lut = (unsigned*)s_mem;                                       // the table: 192 dwords
  unsigned* s_sel = (unsigned*)(s_mem + AJ_LUT_BYTES);                      // f > 0: {0, 1} per pixel; row pitch SEL_PITCH bytes
  unsigned* s_row = s_sel + SEL_ROWS * SEL_PITCH / 4;                       // f > 0: horizontal counts, a byte per pixel; pitch SEL_W
  const int tid = threadIdx.x;
  const int tx0 = bx0 + blockIdx.x * SEL_W, ty0 = by0 + blockIdx.y * SEL_H; // the tile, in frame pixels, clipped to the box
  const int tx1 = min(tx0 + SEL_W, bx1), ty1 = min(ty0 + SEL_H, by1);
  const int lx = 4 * (tid & 15), ly = tid >> 4;
  const int x = tx0 + lx, y = ty0 + ly;                                     // the lane's 4 pixels (y, x .. x + 3)

  // ---- select: S of the lane's pixels, then the lock of the selected ones
  int npx;
  unsigned tg = select_targets(sel, Wi, y, x, ty1, tx1, npx);               // a byte per pixel, {0, 1}: selected, then target
  if (!__syncthreads_or((int)tg)) return;                                   // nothing selected under the tile: nothing else is loaded
  tg = unlocked_targets(tg, lock, Wi, y, x, npx);
  if (!__syncthreads_or((int)tg)) return;

  // ---- stage: the table, and with a feather S around the tile
  if (lut && tid < AJ_LUT_BYTES / 4) s_lut[tid] = load4_within(lut + 4 * tid, lut, lut + AJ_LUT_BYTES);
  if (f > 0) {
    stage_sel_in_box(s_sel, sel, Wi, by0, bx0, by1, bx1, ty0, tx0, f, tid);
    __syncthreads();
    count_rows(s_sel, s_row, SEL_H + 2 * f, f, tid);
  }
  __syncthreads();

  // ---- point: the lane's targets
  if (!tg) return;
  const BoxDiv bd(box_area(f));
  unsigned c[4] = {bd.n, bd.n, bd.n, bd.n};
  if (f > 0) count4(s_row, ly, tid & 15, f, c);
  const unsigned char* src = lift.row(y) + 3 * (x - lift.lx0);              // the lane's bytes of P: [src, src + 3 npx)
  unsigned pw[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) pw[q] = load4_within(src + 4 * q, src, src + 3 * npx);
  const unsigned char* tb = (const unsigned char*)s_lut;
  unsigned o[3] = {0u, 0u, 0u};
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    int P[3], M[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const int j = 3 * p + ch;
      P[ch] = (int)((pw[j >> 2] >> (8 * (j & 3))) & 255u);
      M[ch] = lut ? (int)tb[256 * ch + P[ch]] : P[ch];
    }
    if (mx.on) {
      const int q0 = M[0], q1 = M[1], q2 = M[2];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
        M[ch] = min(max((mx.m[3 * ch] * q0 + mx.m[3 * ch + 1] * q1 + mx.m[3 * ch + 2] * q2 + mx.m[9 + ch] + 2048) >> 12, 0), 255);
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const int j = 3 * p + ch;
      const unsigned v = (unsigned)(P[ch] + ((amount * (M[ch] - P[ch]) + 128) >> 8));
      o[j >> 2] |= bd.blend(c[p], v, (unsigned)P[ch]) << (8 * (j & 3));
    }
  }
  unsigned char* dst = frame + ((size_t)y * Wi + x) * 3;
  store_targets(dst, o, tg);
}

// one counter of a wave's sub-histogram: every lane of the wave calls this (`on`: the lane has a value).  All active lanes on one
// value: their number is added once, by the first of them; otherwise every active lane adds 1.
__device__ __forceinline__ void wave_add(unsigned* h, bool on, unsigned v, int lane) {
  const u64 act = __ballot(on);
  if (!act) return;
  const int first = __ffsll((long long)act) - 1;
  const unsigned v0 = (unsigned)__shfl((int)v, first);
  if (__all(!on || v == v0)) {
    if (lane == first) atomicAdd(&h[v0], (unsigned)__popcll(act));
  } else if (on) {
    atomicAdd(&h[v], 1u);
  }
}

__global__ void __launch_bounds__(256) hist_tiles_kernel(const unsigned char* __restrict__ frame, int Wi, const unsigned char* __restrict__ sel,
                                                         int by0, int bx0, int by1, int bx1, int ntx, int ntiles, unsigned* __restrict__ slabs) {
  __shared__ unsigned s_h[4][1024];                                         // a sub-histogram per wave: [R, G, B, Y][256]
  const int tid = threadIdx.x, lane = tid & 63;
  unsigned* mine = s_h[tid >> 6];
  for (int w = tid; w < 4096; w += 256) (&s_h[0][0])[w] = 0u;
  __syncthreads();
  const int lx = 4 * (tid & 15), ly = tid >> 4;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {           // the same trips for every lane of the workgroup
    const int tx0 = bx0 + (tile % ntx) * SEL_W, ty0 = by0 + (tile / ntx) * SEL_H;
    const int tx1 = min(tx0 + SEL_W, bx1), ty1 = min(ty0 + SEL_H, by1);
    const int x = tx0 + lx, y = ty0 + ly;
    unsigned on = 0;                                                        // a byte per pixel, {0, 1}: counted
    unsigned pw[3] = {0u, 0u, 0u};
    if (y < ty1 && x < tx1) {
      const int npx = min(4, tx1 - x);
      if (sel) {
        const unsigned char* srow = sel + (size_t)y * Wi + x;               // the lane's bytes of S: [srow, srow + npx)
        on = bytes_nonzero(load4_within(srow, srow, srow + npx));
      } else {
        on = 0x01010101u >> (8 * (4 - npx));
      }
      if (on) {
        const unsigned char* src = frame + ((size_t)y * Wi + x) * 3;        // the lane's bytes of F: [src, src + 3 npx)
#pragma unroll
        for (int q = 0; q < 3; ++q) pw[q] = load4_within(src + 4 * q, src, src + 3 * npx);
      }
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const bool a = ((on >> (8 * p)) & 1u) != 0;
      unsigned v[3];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const int j = 3 * p + ch;
        v[ch] = (pw[j >> 2] >> (8 * (j & 3))) & 255u;
        wave_add(mine + 256 * ch, a, v[ch], lane);
      }
      wave_add(mine + 768, a, (77u * v[0] + 150u * v[1] + 29u * v[2] + 128u) >> 8, lane);
    }
  }
  __syncthreads();
  unsigned* out = slabs + (size_t)blockIdx.x * 1024;
  for (int w = tid; w < 1024; w += 256) out[w] = s_h[0][w] + s_h[1][w] + s_h[2][w] + s_h[3][w];
}

__global__ void __launch_bounds__(256) hist_sum_kernel(const unsigned* __restrict__ slabs, int groups, unsigned* __restrict__ hist) {
  const int w = blockIdx.x * 256 + threadIdx.x;                             // 4 workgroups: the record's 1024 words
  unsigned s = 0;
  for (int g = 0; g < groups; ++g) s += slabs[(size_t)g * 1024 + w];
  hist[w] = s;
}

// the inclusive prefix sums of x over the 256 lanes, left in s[0 .. 255]
__device__ __forceinline__ u64 scan256(u64* s, u64 x, int v) {
  s[v] = x;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const u64 t = v >= d ? s[v - d] : 0ull;
    __syncthreads();
    x += t;
    s[v] = x;
    __syncthreads();
  }
  return x;
}

__global__ void __launch_bounds__(256) adjust_lut_kernel(const unsigned* __restrict__ hs, const unsigned* __restrict__ hr, int mode, int which,
                                                         int clip, unsigned char* __restrict__ lut) {
  __shared__ u64 s_a[256], s_b[256];                                        // cdf_src, cdf_ref
  __shared__ int s_lo, s_hi;
  const int v = threadIdx.x;
  const int rows = which == SE_ADJUST_LUMA ? 1 : 3;
  for (int r = 0; r < rows; ++r) {
    const int row = which == SE_ADJUST_LUMA ? 3 : r;
    const u64 cur = scan256(s_a, hs[256 * row + v], v);
    const u64 prev = v ? s_a[v - 1] : 0ull, N = s_a[255];
    unsigned o = (unsigned)v;                                               // the identity row
    if (mode == SE_ADJUST_MATCH) {
      scan256(s_b, hr[256 * row + v], v);
      const u64 Nr = s_b[255];
      if (N && Nr) {
        const u64 want = cur * Nr;                                          // < 2^50 for frames of up to 2^25 pixels
        int lo = 0, hi = 255;                                               // the smallest u with cdf_ref[u] N >= want; 255 qualifies
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (s_b[mid] * N >= want) hi = mid; else lo = mid + 1;
        }
        o = (unsigned)lo;
      }
    } else {
      const u64 t = mode == SE_ADJUST_STRETCH ? N * (u64)clip / 1000ull : 0ull;
      if (N) {                                                              // cdf is monotone: exactly one lane writes each
        if (cur > t && prev <= t) s_lo = v;                                 // the smallest v with cdf[v] > t
        if (N - prev > t && (v == 255 || !(N - cur > t))) s_hi = v;         // the largest v with N - cdf[v - 1] > t
      }
      __syncthreads();
      if (N && mode == SE_ADJUST_STRETCH) {
        const int lo = s_lo, hi = s_hi;
        if (hi != lo) o = v < lo ? 0u : min((unsigned)(((v - lo) * 255 + (hi - lo) / 2) / (hi - lo)), 255u);
      } else if (N) {
        const u64 c0 = s_a[s_lo];
        if (N != c0) o = v < s_lo ? 0u : (unsigned)(((cur - c0) * 255ull + (N - c0) / 2ull) / (N - c0));
      }
    }
    if (which == SE_ADJUST_LUMA) {
      lut[v] = (unsigned char)o; lut[256 + v] = (unsigned char)o; lut[512 + v] = (unsigned char)o;
    } else {
      lut[256 * r + v] = (unsigned char)o;
    }
    __syncthreads();                                                        // s_a, s_lo and s_hi are the next row's
  }
}

}  // namespace

int adjust_hist_groups(int bh, int bw) {
  const long tiles = (long)((bw + SEL_W - 1) / SEL_W) * ((bh + SEL_H - 1) / SEL_H);
  return (int)(tiles < SE_ADJUST_HIST_GROUPS ? tiles : SE_ADJUST_HIST_GROUPS);
}

hipError_t launch_adjust(unsigned char* frame, int Hi, int Wi, const unsigned char* lift, int ly0, int lx0, int lw, int lpitch,
                         const unsigned char* sel, const unsigned char* lock, int by0, int bx0, int by1, int bx1, const unsigned char* lut,
                         const int* matrix, int amount, int feather, hipStream_t st) {
  (void)Hi;
  const dim3 grid((unsigned)((bx1 - bx0 + SEL_W - 1) / SEL_W), (unsigned)((by1 - by0 + SEL_H - 1) / SEL_H));
  const Lift lf{lift, ly0, lx0, lw, lpitch};
  AdjustMatrix mx;
  for (int k = 0; k < 12; ++k) mx.m[k] = matrix ? matrix[k] : 0;
  mx.on = matrix ? 1 : 0;
  // bytes: an upper bound (every pixel a target): S with the feather's halo, the lock, the lift, the box written
  const double fhalo = feather ? (double)(SEL_W + 2 * feather) * (SEL_H + 2 * feather) / (double)(SEL_W * SEL_H) : 0.0;
  set_launch_cost(0.0, (double)(by1 - by0) * (bx1 - bx0) * (1.0 + fhalo + (lock ? 1.0 : 0.0) + 6.0), "adjust");
  set_launch_grid((long)grid.x * grid.y);
  ProfScope ps_(st, PL_ADJUST);
  hipLaunchKernelGGL(adjust_kernel, grid, dim3(256), AJ_LUT_BYTES + (feather > 0 ? SEL_LDS_BYTES : 0), st, frame, Wi, lf, sel, lock, by0, bx0, by1,
                     bx1, lut, mx, amount, feather);
  return hipGetLastError();
}

hipError_t launch_hist_tiles(const unsigned char* frame, int Wi, const unsigned char* sel, int by0, int bx0, int by1, int bx1, unsigned* slabs,
                             hipStream_t st) {
  const int ntx = (bx1 - bx0 + SEL_W - 1) / SEL_W, nty = (by1 - by0 + SEL_H - 1) / SEL_H;
  const int groups = adjust_hist_groups(by1 - by0, bx1 - bx0);
  set_launch_cost(0.0, (double)(by1 - by0) * (bx1 - bx0) * (sel ? 4.0 : 3.0) + 4096.0 * groups, "hist_tiles");
  set_launch_grid(groups);
  ProfScope ps_(st, PL_HIST_TILES);
  hipLaunchKernelGGL(hist_tiles_kernel, dim3((unsigned)groups), dim3(256), 0, st, frame, Wi, sel, by0, bx0, by1, bx1, ntx, ntx * nty, slabs);
  return hipGetLastError();
}

hipError_t launch_hist_sum(const unsigned* slabs, int groups, unsigned* hist, hipStream_t st) {
  set_launch_cost(0.0, 4096.0 * (groups + 1), "hist_sum");
  set_launch_grid(4);
  ProfScope ps_(st, PL_HIST_SUM);
  hipLaunchKernelGGL(hist_sum_kernel, dim3(4), dim3(256), 0, st, slabs, groups, hist);
  return hipGetLastError();
}

hipError_t launch_adjust_lut(const unsigned* hist_src, const unsigned* hist_ref, int mode, int which, int clip, unsigned char* lut, hipStream_t st) {
  set_launch_cost(0.0, 4096.0 * (hist_ref ? 2 : 1) + 768.0, "adjust_lut");
  set_launch_grid(1);
  ProfScope ps_(st, PL_ADJUST_LUT);
  hipLaunchKernelGGL(adjust_lut_kernel, dim3(1), dim3(256), 0, st, hist_src, hist_ref, mode, which, clip, lut);
  return hipGetLastError();
}

}  // namespace se
