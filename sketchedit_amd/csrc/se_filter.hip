// Blur, sharpen or pixelate a selection (the rule is stated in include/sketchedit_filter.h and in plain numpy
// in tests/filter_util.py).  Two integer-only kernels, plain vector loads and stores, no atomics, nothing polled, any alignment of
// the frame, the planes and Wi, no byte outside the frame, a plane or the first 3 lw bytes of the slot's rows read or written.  The
// frame is only WRITTEN: every input pixel comes from the lift.
//
//  filter_blur<RC>: the grid covers se_seltile.h's tiles of the BOX, never the frame.  RC = 8 / 16 / 32 is the radius class: it sets
//                the pitches and the bytes of LDS (all dynamic; BlurTile), nothing else.
//                 select: select_targets; no selected pixel in the tile: return before any other load.  Then unlocked_targets; no
//                         target left: return.
//                 stage:  the tile's rows ty0 - R .. and columns tx0 - R .., clamped to the frame, as BYTES of the lift: per
//                         staged row the run of columns that need no clamp is one span of the slot's row, read through
//                         load4_within in dwords; the columns left of column 0 and right of column Wi - 1 (a tile at the frame's
//                         edge only) repeat that column's three bytes.  With f > 0 stage_sel_in_box.
//                 rows:   H of every staged row: per byte of the tile's 3 tw the 2R + 1 taps, folded by their symmetry, a dword
//                         each (<= 255 * 4096); with f > 0 count_rows.
//                 blend:  a target's lane adds the 2R + 1 row sums of its 12 bytes in UNSIGNED 32 bits (<= 255 * 2^24 + 2^23),
//                         makes B, O, the separable count (count4) and the blend against the staged P (BoxDiv).  Stores:
//                         store_targets.
//  filter_mosaic: one wave per cell of the box, four cells per workgroup, the cells along grid.x.  The wave's lanes stride over the
//                cell's pixels: S (and the lock where S is set) -> a bit per step and lane; no target: the wave returns.  The
//                lift's bytes -> three sums, reduced across the wave (<= 4096 * 255); the same lanes then write the targets they
//                found, the feather count taken straight from S inside the box, at most 33^2 byte loads per target.
#include "../../include/sketchedit_hip.h"
#include "../../include/sketchedit_filter.h"
#include "se_kernels.h"
#include "se_seltile.h"

namespace se {

namespace {

constexpr int FL_H_PITCH = 3 * SEL_W;                 // dwords: a row of horizontal sums

// the LDS of one tile at radius class RC: the sums, the staged bytes of P and, with a feather, S and its row counts
template <int RC>
struct BlurTile {
  static constexpr int ROWS = SEL_H + 2 * RC;
  static constexpr int P_PITCH = (3 * (SEL_W + 2 * RC) + 3) & ~3;       // bytes
  static constexpr int H_BYTES = ROWS * FL_H_PITCH * 4;
  static constexpr int P_BYTES = ROWS * P_PITCH;                      // a multiple of 16 for RC = 8, 16, 32
  static constexpr int bytes(bool feather) { return H_BYTES + P_BYTES + (feather ? SEL_LDS_BYTES : 0); }
};
static_assert(BlurTile<8>::P_BYTES % 16 == 0 && BlurTile<16>::P_BYTES % 16 == 0 && BlurTile<32>::P_BYTES % 16 == 0, "s_sel is dword aligned");

struct FilterTaps {
  int t[SE_FILTER_MAX_RADIUS + 1];
};

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
  unsigned* s_sel = (unsigned*)(s_mem + T::H_BYTES + T::P_BYTES);           // f > 0: {0, 1} per pixel; row pitch SEL_PITCH bytes
  unsigned* s_row = s_sel + SEL_ROWS * SEL_PITCH / 4;                       // f > 0: horizontal counts, a byte per pixel; pitch SEL_W
  const int tid = threadIdx.x;
  const int tx0 = bx0 + blockIdx.x * SEL_W, ty0 = by0 + blockIdx.y * SEL_H; // the tile, in frame pixels, clipped to the box
  const int tx1 = min(tx0 + SEL_W, bx1), ty1 = min(ty0 + SEL_H, by1);
  const int tw = tx1 - tx0, th = ty1 - ty0;
  const int lx = 4 * (tid & 15), ly = tid >> 4;
  const int x = tx0 + lx, y = ty0 + ly;                                     // the lane's 4 pixels (y, x .. x + 3)

  // ---- select: S of the lane's pixels, then the lock of the selected ones
  int npx;
  unsigned tg = select_targets(sel, Wi, y, x, ty1, tx1, npx);               // a byte per pixel, {0, 1}: selected, then target
  if (!__syncthreads_or((int)tg)) return;                                   // nothing selected under the tile: nothing else is loaded
  tg = unlocked_targets(tg, lock, Wi, y, x, npx);
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
      const unsigned char* src = lift.row(fy) + 3 * (xa - lift.lx0);
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
      s_p[i * T::P_PITCH + 3 * j + ch] = lift.row(fy)[3 * (cx - lift.lx0) + ch];
    }
  }
  if (f > 0) stage_sel_in_box(s_sel, sel, Wi, by0, bx0, by1, bx1, ty0, tx0, f, tid);
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
  if (f > 0) count_rows(s_sel, s_row, SEL_H + 2 * f, f, tid);
  __syncthreads();

  // ---- blend: the lane's targets
  if (!tg) return;
  const BoxDiv bd(box_area(f));
  unsigned c[4] = {bd.n, bd.n, bd.n, bd.n};
  if (f > 0) count4(s_row, ly, tid & 15, f, c);
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
  unsigned o[3] = {0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < 12; ++j) {
    const unsigned P = pp[j], B = (acc[j] + (1u << 23)) >> 24;
    o[j >> 2] |= bd.blend(c[j / 3], filter_mix(P, B, amount), P) << (8 * (j & 3));
  }
  unsigned char* dst = frame + ((size_t)y * Wi + x) * 3;
  store_targets(dst, o, tg);
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
    const unsigned char* p = lift.row(y0 + idx / cw) + 3 * (x0 + idx % cw - lift.lx0);
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
  const BoxDiv bd(box_area(f));
  for (int idx = lane, it = 0; idx < cnt; idx += 64, ++it) {
    if (!((mine >> it) & 1ull)) continue;
    const int py = y0 + idx / cw, px = x0 + idx % cw;
    unsigned cp = bd.n;
    if (f > 0) {                                                            // S of the box within f of the pixel
      cp = 0;
      const int ya = max(py - f, by0), yb = min(py + f + 1, by1), xa = max(px - f, bx0), xb = min(px + f + 1, bx1);
      for (int yy = ya; yy < yb; ++yy) {
        const unsigned char* row = sel + (size_t)yy * Wi;
        for (int xx = xa; xx < xb; ++xx) cp += row[xx] != 0 ? 1u : 0u;
      }
    }
    const unsigned char* p = lift.row(py) + 3 * (px - lift.lx0);
    unsigned char* dst = frame + ((size_t)py * Wi + px) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const unsigned P = p[ch];
      dst[ch] = (unsigned char)bd.blend(cp, filter_mix(P, B[ch], amount), P);
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
  const dim3 grid((unsigned)((bx1 - bx0 + SEL_W - 1) / SEL_W), (unsigned)((by1 - by0 + SEL_H - 1) / SEL_H));
  const Lift lf{lift, ly0, lx0, lw, lpitch};
  FilterTaps tp;
  for (int k = 0; k <= SE_FILTER_MAX_RADIUS; ++k) tp.t[k] = k <= radius ? taps[k] : 0;
  // bytes: an upper bound (every pixel a target): S with the feather's halo, the lock, the lift with the radius' halo, the box written
  const double halo = (double)(SEL_W + 2 * radius) * (SEL_H + 2 * radius) / (double)(SEL_W * SEL_H);
  const double fhalo = feather ? (double)(SEL_W + 2 * feather) * (SEL_H + 2 * feather) / (double)(SEL_W * SEL_H) : 0.0;
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
