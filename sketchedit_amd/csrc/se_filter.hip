// Blur, sharpen or pixelate a selection (the rule is stated in include/sketchedit_filter.h and in plain numpy
// in tests/filter_util.py).  Two integer-only kernels, plain vector loads and stores, no atomics, nothing polled, any alignment of
// the frame, the planes and Wi, no byte outside the frame, a plane or the first 3 lw bytes of the slot's rows read or written.  The
// frame is only WRITTEN: every input pixel comes from the lift.
//
//  filter_blur<RC>: the grid covers the 64 x 16 tiles of the BOX, never the frame; one workgroup = one tile, 256 lanes, a lane
//                owns 4 consecutive pixels of a row.  RC = 8 / 16 / 32 is the radius class: it sets the pitches and the bytes of
//                LDS (all dynamic; BlurTile), nothing else.
//                 select: the lane's 4 bytes of S, bounded by the tile's row; no selected pixel in the tile: return before any
//                         other load.  Then the lock's bytes of the selected pixels; no target left: return.
//                 stage:  the tile's rows ty0 - R .. and columns tx0 - R .., clamped to the frame, as BYTES of the lift: per
//                         staged row the run of columns that need no clamp is one span of the slot's row, read through
//                         load4_within in dwords; the columns left of column 0 and right of column Wi - 1 (a tile at the frame's
//                         edge only) repeat that column's three bytes.  With f > 0 the box's S around the tile as move_drop<true>
//                         stages the moved selection: {0, 1} bytes, neither the frame's edge nor the lock.
//                 rows:   H of every staged row: per byte of the tile's 3 tw the 2R + 1 taps, folded by their symmetry, a dword
//                         each (<= 255 * 4096); with f > 0 the horizontal counts of S.
//                 blend:  a target's lane adds the 2R + 1 row sums of its 12 bytes in UNSIGNED 32 bits (<= 255 * 2^24 + 2^23),
//                         makes B, O, the separable count and the blend against the staged P.  Stores follow se_window.hip's
//                         ownership rule: three dwords where all four pixels are targets and the address is aligned, single
//                         bytes of targets otherwise.
//                The division is se_feather.hip's: mulhi(v, floor(2^32 / n) + 1) == v / n for v < 2^19, n <= 1089.
//  filter_mosaic: one wave per cell of the box, four cells per workgroup, the cells along grid.x.  The wave's lanes stride over the
//                cell's pixels: S (and the lock where S is set) -> a bit per step and lane; no target: the wave returns.  The
//                lift's bytes -> three sums, reduced across the wave (<= 4096 * 255); the same lanes then write the targets they
//                found, the feather count taken straight from S inside the box, at most 33^2 byte loads per target.
#include "../../include/sketchedit_hip.h"
#include "../../include/sketchedit_filter.h"
#include "se_device.h"
#include "se_kernels.h"

#include <cstdint>

namespace se {

namespace {

constexpr int FL_W = 64, FL_H = 16, FL_FMAX = SE_FILTER_MAX_FEATHER;
constexpr int FL_SEL_PITCH = 192;                     // bytes: 48 dwords = 16 mod 32 (se_feather.hip)
constexpr int FL_SEL_ROWS = FL_H + 2 * FL_FMAX;       // staged rows of S at the largest feather
constexpr int FL_H_PITCH = 3 * FL_W;                  // dwords: a row of horizontal sums

// the LDS of one tile at radius class RC: the sums, the staged bytes of P and, with a feather, S and its row counts
template <int RC>
struct BlurTile {
  static constexpr int ROWS = FL_H + 2 * RC;
  static constexpr int P_PITCH = (3 * (FL_W + 2 * RC) + 3) & ~3;       // bytes
  static constexpr int H_BYTES = ROWS * FL_H_PITCH * 4;
  static constexpr int P_BYTES = ROWS * P_PITCH;                      // a multiple of 16 for RC = 8, 16, 32
  static constexpr int F_BYTES = FL_SEL_ROWS * FL_SEL_PITCH + FL_SEL_ROWS * FL_W;
  static constexpr int bytes(bool feather) { return H_BYTES + P_BYTES + (feather ? F_BYTES : 0); }
};
static_assert(BlurTile<8>::P_BYTES % 16 == 0 && BlurTile<16>::P_BYTES % 16 == 0 && BlurTile<32>::P_BYTES % 16 == 0, "s_sel is dword aligned");

struct FilterTaps {
  int t[SE_FILTER_MAX_RADIUS + 1];
};

// the lift: the slot's row of frame row y is [p + (y - ly0) lpitch, + 3 lw), its pixel x at 3 (x - lx0)
struct Lift {
  const unsigned char* p;
  int ly0, lx0, lw, lpitch;
};

// each non-zero byte of u -> 1
__device__ __forceinline__ unsigned bytes_nonzero(unsigned u) {
  return ((u & 0xffu) ? 1u : 0u) | ((u & 0xff00u) ? 0x100u : 0u) | ((u & 0xff0000u) ? 0x10000u : 0u) | ((u & 0xff000000u) ? 0x1000000u : 0u);
}

// S != 0 of the pixels (y, x .. x + 3) that lie in the box, a byte of {0, 1} each; nothing outside the box's row of S is read
__device__ __forceinline__ unsigned sel4_in_box(const unsigned char* sel, int Wi, int by0, int bx0, int by1, int bx1, int y, int x) {
  if (y < by0 || y >= by1 || x + 3 < bx0 || x >= bx1) return 0u;
  const unsigned char* row = sel + (size_t)y * Wi;
  return bytes_nonzero(load4_within(row + x, row + bx0, row + bx1));
}

// O of the rule: P, B in 0 .. 255, a in -256 .. 1024
__device__ __forceinline__ unsigned filter_mix(unsigned P, unsigned B, int a) {
  const int o = (int)P + ((a * ((int)P - (int)B) + 128) >> 8);
  return (unsigned)min(max(o, 0), 255);
}

template <int RC>
__global__ void __launch_bounds__(256) filter_blur_kernel(unsigned char* __restrict__ frame, int Hi, int Wi, Lift lift,
                                                          const unsigned char* __restrict__ sel, const unsigned char* __restrict__ lock,
                                                          int by0, int bx0, int by1, int bx1, FilterTaps taps, int R, int amount, int f) {
  using T = BlurTile<RC>;
  extern __shared__ __attribute__((aligned(16))) unsigned char s_mem[];
  unsigned* s_h = (unsigned*)s_mem;                                         // H: row pitch FL_H_PITCH dwords
  unsigned char* s_p = s_mem + T::H_BYTES;                                  // P: row pitch P_PITCH bytes
  unsigned* s_sel = (unsigned*)(s_mem + T::H_BYTES + T::P_BYTES);           // f > 0: {0, 1} per pixel; row pitch FL_SEL_PITCH bytes
  unsigned* s_row = s_sel + FL_SEL_ROWS * FL_SEL_PITCH / 4;                 // f > 0: horizontal counts, a byte per pixel; pitch FL_W
  const int tid = threadIdx.x;
  const int tx0 = bx0 + blockIdx.x * FL_W, ty0 = by0 + blockIdx.y * FL_H;   // the tile, in frame pixels, clipped to the box
  const int tx1 = min(tx0 + FL_W, bx1), ty1 = min(ty0 + FL_H, by1);
  const int tw = tx1 - tx0, th = ty1 - ty0;
  const int lx = 4 * (tid & 15), ly = tid >> 4;
  const int x = tx0 + lx, y = ty0 + ly;                                     // the lane's 4 pixels (y, x .. x + 3)

  // ---- select: S of the lane's pixels, then the lock of the selected ones
  unsigned tg = 0;                                                          // a byte per pixel, {0, 1}: selected, then target
  int npx = 0;
  if (y < ty1 && x < tx1) {
    npx = min(4, tx1 - x);
    const unsigned char* srow = sel + (size_t)y * Wi + x;                   // the lane's bytes of S: [srow, srow + npx)
    tg = bytes_nonzero(load4_within(srow, srow, srow + npx));
  }
  if (!__syncthreads_or((int)tg)) return;                                   // nothing selected under the tile: nothing else is loaded
  if (lock && tg) {
    const unsigned char* lrow = lock + (size_t)y * Wi + x;
    tg &= ~bytes_nonzero(load4_within(lrow, lrow, lrow + npx));
  }
  if (!__syncthreads_or((int)tg)) return;

  // ---- stage: staged (i, j) = P[clamp(ty0 - R + i, 0, Hi - 1)][clamp(tx0 - R + j, 0, Wi - 1)], i < th + 2R, j < tw + 2R
  const int rows = th + 2 * R;
  {
    const int xa = max(tx0 - R, 0), xb = min(tx1 + R, Wi);                  // the frame columns that need no clamp: one span of a slot row
    const int run = 3 * (xb - xa), rdw = (run + 3) >> 2;
    const int nl = xa - (tx0 - R), jr = xb - (tx0 - R);                     // staged columns [0, nl) repeat column 0, [jr, tw + 2R) column Wi - 1
    for (int t = tid; t < rows * rdw; t += 256) {
      const int i = t / rdw, q = t % rdw;
      const int fy = min(max(ty0 - R + i, 0), Hi - 1);
      const unsigned char* src = lift.p + (size_t)(fy - lift.ly0) * lift.lpitch + 3 * (xa - lift.lx0);
      const unsigned v = load4_within(src + 4 * q, src, src + run);
      unsigned char* d = s_p + i * T::P_PITCH + 3 * nl + 4 * q;
      const int nb = min(4, run - 4 * q);
      for (int e = 0; e < nb; ++e) d[e] = (unsigned char)((v >> (8 * e)) & 255u);
    }
    const int nc = nl + (tw + 2 * R - jr);                                  // clamped columns: a tile near the frame's left or right edge
    for (int t = tid; t < rows * nc * 3; t += 256) {
      const int i = t / (nc * 3), jc = (t % (nc * 3)) / 3, ch = t % 3;
      const int fy = min(max(ty0 - R + i, 0), Hi - 1);
      const int j = jc < nl ? jc : jr + (jc - nl), cx = jc < nl ? 0 : Wi - 1;
      s_p[i * T::P_PITCH + 3 * j + ch] = lift.p[(size_t)(fy - lift.ly0) * lift.lpitch + 3 * (cx - lift.lx0) + ch];
    }
  }
  const int frows = FL_H + 2 * f;
  if (f > 0) {                                                              // staged S (i, j) = S != 0 in the box at (ty0 - f + i, tx0 - f + j)
    const int cols4 = (FL_W + 2 * f + 3) >> 2;
    for (int t = tid; t < frows * cols4; t += 256) {
      const int i = t / cols4, j4 = t % cols4;
      s_sel[i * (FL_SEL_PITCH / 4) + j4] = sel4_in_box(sel, Wi, by0, bx0, by1, bx1, ty0 - f + i, tx0 - f + 4 * j4);
    }
  }
  __syncthreads();

  // ---- rows: s_h (i, b) = sum over k of t[|k|] staged (i, b + 3 (R + k)), b a byte of the tile's 3 tw
  {
    const int nb3 = 3 * tw;
    for (int t = tid; t < rows * nb3; t += 256) {
      const int i = t / nb3, b = t % nb3;
      const unsigned char* p = s_p + i * T::P_PITCH + b + 3 * R;
      unsigned acc = (unsigned)taps.t[0] * p[0];
      for (int k = 1; k <= R; ++k) acc += (unsigned)taps.t[k] * ((unsigned)p[-3 * k] + (unsigned)p[3 * k]);
      s_h[i * FL_H_PITCH + b] = acc;
    }
  }
  if (f > 0) {                                                              // s_row (i, x) = sum of staged S (i, x .. x + 2f): se_move.hip's rows
    for (int t = tid; t < frows * (FL_W / 4); t += 256) {
      const int i = t >> 4, k = t & 15;
      const unsigned* s = s_sel + i * (FL_SEL_PITCH / 4) + k;
      const int nd = (2 * f + 4 + 3) >> 2;
      unsigned char e[2 * FL_FMAX + 4];
#pragma unroll
      for (int q = 0; q < (2 * FL_FMAX + 4) / 4; ++q) {
        const unsigned d = q < nd ? s[q] : 0u;
#pragma unroll
        for (int z = 0; z < 4; ++z) e[4 * q + z] = (unsigned char)((d >> (8 * z)) & 255u);
      }
      unsigned s0 = 0;
#pragma unroll
      for (int z = 0; z < 2 * FL_FMAX + 1; ++z) s0 += z <= 2 * f ? e[z] : 0u;
      unsigned in1 = 0, in2 = 0, in3 = 0;
#pragma unroll
      for (int z = 1; z < 2 * FL_FMAX + 4; ++z) {
        in1 = z == 2 * f + 1 ? e[z] : in1;
        in2 = z == 2 * f + 2 ? e[z] : in2;
        in3 = z == 2 * f + 3 ? e[z] : in3;
      }
      const unsigned s1 = s0 - e[0] + in1, s2 = s1 - e[1] + in2, s3 = s2 - e[2] + in3;
      s_row[i * (FL_W / 4) + k] = s0 | (s1 << 8) | (s2 << 16) | (s3 << 24);
    }
  }
  __syncthreads();

  // ---- blend: the lane's targets
  if (!tg) return;
  const unsigned n = (unsigned)((2 * f + 1) * (2 * f + 1));
  unsigned c[4] = {n, n, n, n};
  if (f > 0) {
    unsigned lo = 0, hi = 0;                                                // pixels 0, 2 and 1, 3 in 16-bit fields
    for (int d = 0; d <= 2 * f; ++d) {
      const unsigned v = s_row[(ly + d) * (FL_W / 4) + (tid & 15)];
      lo += v & 0x00ff00ffu;
      hi += (v >> 8) & 0x00ff00ffu;
    }
    c[0] = lo & 0xffffu; c[1] = hi & 0xffffu; c[2] = lo >> 16; c[3] = hi >> 16;
  }
  unsigned acc[12];
  const unsigned* hp = s_h + (ly + R) * FL_H_PITCH + 3 * lx;               // the lane's 12 sums of its own row; row k away at k FL_H_PITCH
#pragma unroll
  for (int j = 0; j < 12; ++j) acc[j] = (unsigned)taps.t[0] * hp[j];
  for (int k = 1; k <= R; ++k) {
    const unsigned tk = (unsigned)taps.t[k];
    const unsigned* up = hp - k * FL_H_PITCH;
    const unsigned* dn = hp + k * FL_H_PITCH;
#pragma unroll
    for (int j = 0; j < 12; ++j) acc[j] += tk * (up[j] + dn[j]);           // unsigned: the whole sum is at most 255 * 2^24
  }
  const unsigned char* pp = s_p + (ly + R) * T::P_PITCH + 3 * (lx + R);     // the lane's 12 bytes of P
  const unsigned magic = (unsigned)((1ull << 32) / n) + 1u, half = (n - 1u) >> 1;
  unsigned o[3] = {0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < 12; ++j) {
    const unsigned P = pp[j], B = (acc[j] + (1u << 23)) >> 24;
    unsigned v = filter_mix(P, B, amount);
    const unsigned cp = c[j / 3];
    if (cp != n) v = __umulhi(cp * v + (n - cp) * P + half, magic);
    o[j >> 2] |= v << (8 * (j & 3));
  }
  unsigned char* dst = frame + ((size_t)y * Wi + x) * 3;
  if (tg == 0x01010101u && ((uintptr_t)dst & 3) == 0) {
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

// cell q of the box's ncx columns of cells: wave q & 3 of workgroup q >> 2
__global__ void __launch_bounds__(256) filter_mosaic_kernel(unsigned char* __restrict__ frame, int Wi, Lift lift, const unsigned char* __restrict__ sel,
                                                            const unsigned char* __restrict__ lock, int by0, int bx0, int by1, int bx1, int b,
                                                            int ncx, long ncells, int amount, int f) {
  const int lane = threadIdx.x & 63;
  const long cell = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (cell >= ncells) return;
  const int y0 = by0 + (int)(cell / ncx) * b, x0 = bx0 + (int)(cell % ncx) * b;
  const int cw = min(b, bx1 - x0), cnt = min(b, by1 - y0) * cw;             // the cell clipped to the box: cnt <= 4096 pixels

  // ---- select: bit `it` of mine = the pixel lane + 64 it of the cell is a target
  unsigned long long mine = 0;
  for (int idx = lane, it = 0; idx < cnt; idx += 64, ++it) {
    const size_t at = (size_t)(y0 + idx / cw) * Wi + (x0 + idx % cw);
    if (sel[at] != 0 && !(lock && lock[at] != 0)) mine |= 1ull << it;
  }
  if (!__any(mine != 0)) return;                                            // the whole wave: no target in the cell

  // ---- the cell's mean of the lift, selected or not
  unsigned s[3] = {0u, 0u, 0u};
  for (int idx = lane; idx < cnt; idx += 64) {
    const unsigned char* p = lift.p + (size_t)(y0 + idx / cw - lift.ly0) * lift.lpitch + 3 * (x0 + idx % cw - lift.lx0);
    s[0] += p[0]; s[1] += p[1]; s[2] += p[2];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) s[ch] += (unsigned)__shfl_xor((int)s[ch], off);
  }
  unsigned B[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) B[ch] = (s[ch] + (unsigned)cnt / 2u) / (unsigned)cnt;

  // ---- the targets this lane found
  const unsigned n = (unsigned)((2 * f + 1) * (2 * f + 1));
  const unsigned magic = (unsigned)((1ull << 32) / n) + 1u, half = (n - 1u) >> 1;
  for (int idx = lane, it = 0; idx < cnt; idx += 64, ++it) {
    if (!((mine >> it) & 1ull)) continue;
    const int py = y0 + idx / cw, px = x0 + idx % cw;
    unsigned cp = n;
    if (f > 0) {                                                            // S of the box within f of the pixel
      cp = 0;
      const int ya = max(py - f, by0), yb = min(py + f + 1, by1), xa = max(px - f, bx0), xb = min(px + f + 1, bx1);
      for (int yy = ya; yy < yb; ++yy) {
        const unsigned char* row = sel + (size_t)yy * Wi;
        for (int xx = xa; xx < xb; ++xx) cp += row[xx] != 0 ? 1u : 0u;
      }
    }
    const unsigned char* p = lift.p + (size_t)(py - lift.ly0) * lift.lpitch + 3 * (px - lift.lx0);
    unsigned char* dst = frame + ((size_t)py * Wi + px) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const unsigned P = p[ch];
      unsigned v = filter_mix(P, B[ch], amount);
      if (cp != n) v = __umulhi(cp * v + (n - cp) * P + half, magic);
      dst[ch] = (unsigned char)v;
    }
  }
}

template <int RC>
hipError_t blur_launch(dim3 grid, bool feather, hipStream_t st, unsigned char* frame, int Hi, int Wi, Lift lf, const unsigned char* sel,
                       const unsigned char* lock, int by0, int bx0, int by1, int bx1, const FilterTaps& tp, int R, int amount, int f) {
  const int lds = BlurTile<RC>::bytes(feather);
  hipError_t e = ensure_max_lds((const void*)filter_blur_kernel<RC>, BlurTile<RC>::bytes(true));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(filter_blur_kernel<RC>, grid, dim3(256), lds, st, frame, Hi, Wi, lf, sel, lock, by0, bx0, by1, bx1, tp, R, amount, f);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_filter_blur(unsigned char* frame, int Hi, int Wi, const unsigned char* lift, int ly0, int lx0, int lw, int lpitch,
                              const unsigned char* sel, const unsigned char* lock, int by0, int bx0, int by1, int bx1, const int* taps,
                              int radius, int amount, int feather, hipStream_t st) {
  const dim3 grid((unsigned)((bx1 - bx0 + FL_W - 1) / FL_W), (unsigned)((by1 - by0 + FL_H - 1) / FL_H));
  const Lift lf{lift, ly0, lx0, lw, lpitch};
  FilterTaps tp;
  for (int k = 0; k <= SE_FILTER_MAX_RADIUS; ++k) tp.t[k] = k <= radius ? taps[k] : 0;
  // bytes: an upper bound (every pixel a target): S with the feather's halo, the lock, the lift with the radius' halo, the box written
  const double halo = (double)(FL_W + 2 * radius) * (FL_H + 2 * radius) / (double)(FL_W * FL_H);
  const double fhalo = feather ? (double)(FL_W + 2 * feather) * (FL_H + 2 * feather) / (double)(FL_W * FL_H) : 0.0;
  set_launch_cost(0.0, (double)(by1 - by0) * (bx1 - bx0) * (1.0 + fhalo + (lock ? 1.0 : 0.0) + 3.0 * halo + 3.0), "filter_blur");
  set_launch_grid((long)grid.x * grid.y);
  ProfScope ps_(st, PL_FILTER_BLUR);
  if (radius <= 8) return blur_launch<8>(grid, feather > 0, st, frame, Hi, Wi, lf, sel, lock, by0, bx0, by1, bx1, tp, radius, amount, feather);
  if (radius <= 16) return blur_launch<16>(grid, feather > 0, st, frame, Hi, Wi, lf, sel, lock, by0, bx0, by1, bx1, tp, radius, amount, feather);
  return blur_launch<32>(grid, feather > 0, st, frame, Hi, Wi, lf, sel, lock, by0, bx0, by1, bx1, tp, radius, amount, feather);
}

hipError_t launch_filter_mosaic(unsigned char* frame, int Hi, int Wi, const unsigned char* lift, int ly0, int lx0, int lw, int lpitch,
                                const unsigned char* sel, const unsigned char* lock, int by0, int bx0, int by1, int bx1, int cell, int amount,
                                int feather, hipStream_t st) {
  (void)Hi;
  const int ncx = (bx1 - bx0 + cell - 1) / cell, ncy = (by1 - by0 + cell - 1) / cell;
  const long ncells = (long)ncx * ncy, groups = (ncells + 3) / 4;
  const Lift lf{lift, ly0, lx0, lw, lpitch};
  // bytes: an upper bound (every pixel a target): S, the lock, the lift read twice, the box written; the feather's loads hit the cache
  set_launch_cost(0.0, (double)(by1 - by0) * (bx1 - bx0) * (1.0 + (lock ? 1.0 : 0.0) + 9.0), "filter_mosaic");
  set_launch_grid(groups);
  ProfScope ps_(st, PL_FILTER_MOSAIC);
  hipLaunchKernelGGL(filter_mosaic_kernel, dim3((unsigned)groups), dim3(256), 0, st, frame, Wi, lf, sel, lock, by0, bx0, by1, bx1, cell, ncx,
                     ncells, amount, feather);
  return hipGetLastError();
}

}  // namespace se
