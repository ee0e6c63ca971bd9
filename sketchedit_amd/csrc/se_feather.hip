// Feathered paste of a window edit (the rule is stated in include/sketchedit_feather.h and in plain
// numpy in tests/feather_util.py): the paste of se_window.hip with a soft edge.  B requests per launch, each one se_window
// record of the ctx's device table; wins holds 2 B records and wins[B + b].frame_u8 is request b's lock plane or null, as for
// the locked paste.
//
//  sel(y, x) = m8[b, y, x] > 0 and lock[y0 + y, x0 + x] == 0 inside the hs x ws window.  Outside it, per axis: on a side of the
//              window that is the frame's own edge the coordinate is clamped into the window, on any other side the sample is 0.
//  c(y, x)   = the number of sel pixels in the (2r + 1) x (2r + 1) box around (y, x); n = (2r + 1)^2.
//  frame'    = (c rgb + (n - c) frame + (n - 1) / 2) / n for every byte of a sel pixel; no other byte is written.
//
// One workgroup = one 64 x 16 pixel tile of one request's window, 256 lanes, in three steps over LDS:
//  stage: sel of the tile and its r-wide halo, (16 + 2r) x (64 + 2r) bytes of {0, 1}, four pixels (one dword) per lane and
//         step.  Four columns that lie inside the window are read with load4_within bounded by the window row's own bytes (mask
//         and lock alike); a group that crosses a side of the window goes pixel by pixel through the edge rule.
//  rows:  for every staged row the 64 horizontal sums over 2r + 1 columns, a byte each (<= 33): a lane forms four neighbouring
//         sums from the 2r + 4 bytes under them, the first by adding up, the next three by sliding.
//  blend: a lane owns 4 consecutive pixels of one row, as in window_paste.  It adds the 2r + 1 dwords of row sums above and
//         below its pixels (two 16-bit fields per register: 33 x 33 < 2^16), reads the rgb bytes of its pixels and -- only
//         where some c < n -- the frame's old bytes, and writes by the ownership rule of se_window.hip: three dwords where all
//         four pixels are selected and the address is aligned, single bytes of selected pixels otherwise.  c == n gives rgb
//         itself, so r = 0 is window_paste_locked byte for byte.
// The division is exact: q = mulhi(v, floor(2^32 / n) + 1) equals v / n while v (m n - 2^32) < 2^32 with m n - 2^32 <= n, and
// v <= 255 n + (n - 1) / 2 < 2^19, n <= 1089.
// A lane reads a frame byte only of pixels it may write, through aligned dwords that stay inside the window row's bytes; a
// dword may hold bytes another lane writes, but the lane uses its own bytes only, and each byte has one writer.  No atomics.
#include "../../include/sketchedit_hip.h"
#include "se_device.h"
#include "se_kernels.h"

#include <cstdint>

namespace se {

namespace {

constexpr int FT_W = 64, FT_H = 16, FT_RMAX = 16;
constexpr int FT_SEL_PITCH = 192;                     // bytes: 48 dwords = 16 mod 32, two rows of 16 dword reads share no bank
constexpr int FT_ROWS = FT_H + 2 * FT_RMAX;           // staged rows at the largest radius

// the 12 bytes at `a` (any alignment), of which only those inside [lo, hi) are read (the others are 0)
__device__ __forceinline__ void load12_within(const unsigned char* a, const unsigned char* lo, const unsigned char* hi, unsigned u[3]) {
  const unsigned char* a0 = (const unsigned char*)((uintptr_t)a & ~(uintptr_t)3);
  const int sh = (int)((uintptr_t)a & 3) * 8;
  unsigned d[4];
#pragma unroll
  for (int i = 0; i < 3; ++i) d[i] = load_dword_within(a0 + 4 * i, lo, hi);
  d[3] = sh ? load_dword_within(a0 + 12, lo, hi) : 0u;
#pragma unroll
  for (int i = 0; i < 3; ++i) u[i] = sh ? (d[i] >> sh) | (d[i + 1] << (32 - sh)) : d[i];
}

// each non-zero byte of u -> 1
__device__ __forceinline__ unsigned bytes_nonzero(unsigned u) {
  return ((u & 0xffu) ? 1u : 0u) | ((u & 0xff00u) ? 0x100u : 0u) | ((u & 0xff0000u) ? 0x10000u : 0u) | ((u & 0xff000000u) ? 0x1000000u : 0u);
}

__global__ void __launch_bounds__(256) window_paste_feather_kernel(const se_window* __restrict__ wins, const unsigned char* __restrict__ rgb,
                                                                   const unsigned char* __restrict__ m8, int B, int hs, int ws, int r) {
  __shared__ unsigned s_sel[FT_ROWS * FT_SEL_PITCH / 4];          // {0, 1} per pixel; row pitch FT_SEL_PITCH bytes
  __shared__ unsigned s_row[FT_ROWS * FT_W / 4];                  // horizontal sums, a byte per pixel; row pitch FT_W bytes
  const int tid = threadIdx.x, b = blockIdx.z;
  const se_window w = wins[b];
  const unsigned char* plane = wins[B + b].frame_u8;
  const int tx0 = blockIdx.x * FT_W, ty0 = blockIdx.y * FT_H;     // the tile, in window pixels
  const int rows = FT_H + 2 * r, cols4 = (FT_W + 2 * r + 3) >> 2; // the staged rows, and dwords per staged row
  const bool edge_t = w.y0 == 0, edge_b = w.y0 + hs == w.Hi, edge_l = w.x0 == 0, edge_r = w.x0 + ws == w.Wi;
  const unsigned char* mb = m8 + (size_t)b * hs * ws;

  // ---- stage: staged (i, j) = sel(ty0 - r + i, tx0 - r + j)
  unsigned any = 0;
  for (int t = tid; t < rows * cols4; t += 256) {
    const int i = t / cols4, j4 = t % cols4;
    int y = ty0 - r + i;
    const int xs = tx0 - r + 4 * j4;
    unsigned v = 0;
    const bool row_in = y >= 0 ? (y < hs || edge_b) : edge_t;
    if (row_in) {
      y = min(max(y, 0), hs - 1);
      const unsigned char* mrow = mb + (size_t)y * ws;                               // the mask row's bytes: [mrow, mrow + ws)
      const unsigned char* lrow = plane ? plane + (size_t)(w.y0 + y) * w.Wi + w.x0 : nullptr;       // the lock row's: [lrow, lrow + ws)
      if (xs >= 0 && xs + 4 <= ws) {
        v = bytes_nonzero(load4_within(mrow + xs, mrow, mrow + ws));
        if (v && lrow) v &= ~bytes_nonzero(load4_within(lrow + xs, lrow, lrow + ws));
      } else {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          int x = xs + p;
          if (x >= 0 ? (x < ws || edge_r) : edge_l) {
            x = min(max(x, 0), ws - 1);
            if (mrow[x] && !(lrow && lrow[x])) v |= 1u << (8 * p);
          }
        }
      }
    }
    s_sel[i * (FT_SEL_PITCH / 4) + j4] = v;
    any |= v;
  }
  // (also the barrier between stage and rows.)  Nothing selected under the tile or its halo: nothing to write
  if (!__syncthreads_or((int)any)) return;

  // ---- rows: s_row (i, x) = sum of staged (i, x .. x + 2r), four neighbouring x per lane and step
  for (int t = tid; t < rows * (FT_W / 4); t += 256) {
    const int i = t >> 4, k = t & 15;
    const unsigned* s = s_sel + i * (FT_SEL_PITCH / 4) + k;        // staged columns 4k ..
    const int nb = 2 * r + 4, nd = (nb + 3) >> 2;                  // bytes under the four sums, and their dwords
    unsigned char e[2 * FT_RMAX + 4];
#pragma unroll
    for (int q = 0; q < (2 * FT_RMAX + 4) / 4; ++q) {
      const unsigned d = q < nd ? s[q] : 0u;
#pragma unroll
      for (int z = 0; z < 4; ++z) e[4 * q + z] = (unsigned char)((d >> (8 * z)) & 255u);
    }
    unsigned s0 = 0;
#pragma unroll
    for (int z = 0; z < 2 * FT_RMAX + 1; ++z) s0 += z <= 2 * r ? e[z] : 0u;
    // e[2r + 1 ..]: a compile-time walk with a run-time pick, so that e stays in registers
    unsigned in1 = 0, in2 = 0, in3 = 0;
#pragma unroll
    for (int z = 1; z < 2 * FT_RMAX + 4; ++z) {
      in1 = z == 2 * r + 1 ? e[z] : in1;
      in2 = z == 2 * r + 2 ? e[z] : in2;
      in3 = z == 2 * r + 3 ? e[z] : in3;
    }
    const unsigned s1 = s0 - e[0] + in1, s2 = s1 - e[1] + in2, s3 = s2 - e[2] + in3;
    s_row[i * (FT_W / 4) + k] = s0 | (s1 << 8) | (s2 << 16) | (s3 << 24);
  }
  __syncthreads();

  // ---- blend: the lane's 4 pixels (y, x .. x + 3) of the window
  const int lx = 4 * (tid & 15), ly = tid >> 4;
  const int x = tx0 + lx, y = ty0 + ly;
  if (y >= hs || x >= ws) return;
  const int npx = min(4, ws - x);                                 // the lane's pixels inside the window
  unsigned sel = 0;                                               // a byte per pixel, {0, 1}
  {
    const unsigned char* c8 = (const unsigned char*)s_sel + (ly + r) * FT_SEL_PITCH + lx + r;
    for (int p = 0; p < npx; ++p) sel |= (unsigned)c8[p] << (8 * p);
  }
  if (!sel) return;
  unsigned lo = 0, hi = 0;                                        // pixels 0, 2 and 1, 3 in 16-bit fields
  for (int dy = 0; dy <= 2 * r; ++dy) {
    const unsigned d = s_row[(ly + dy) * (FT_W / 4) + (tid & 15)];
    lo += d & 0x00ff00ffu;
    hi += (d >> 8) & 0x00ff00ffu;
  }
  const unsigned n = (unsigned)((2 * r + 1) * (2 * r + 1));
  const unsigned c[4] = {lo & 0xffffu, hi & 0xffffu, lo >> 16, hi >> 16};
  const size_t pix = ((size_t)b * hs + y) * ws;                   // the first pixel of the lane's row of rgb
  const unsigned char* srow = rgb + pix * 3;                      // that row's bytes: [srow, srow + 3 ws)
  unsigned char* frow = w.frame_u8 + ((size_t)(w.y0 + y) * w.Wi + w.x0) * 3;       // the window row's bytes: [frow, frow + 3 ws)
  unsigned char* dst = frow + 3 * x;
  unsigned s[3], o[3] = {0u, 0u, 0u};
  load12_within(srow + 3 * x, srow, srow + 3 * (size_t)ws, s);
  bool full = true;                                               // every selected pixel of the lane has c == n
#pragma unroll
  for (int p = 0; p < 4; ++p) full = full && (!((sel >> (8 * p)) & 1u) || c[p] == n);
  if (!full) {
    unsigned f[3];
    load12_within(dst, frow, frow + 3 * (size_t)ws, f);
    const unsigned magic = (unsigned)((1ull << 32) / n) + 1u, half = (n - 1u) >> 1;      // (n > 1 here: n == 1 has c == n)
#pragma unroll
    for (int j = 0; j < 12; ++j) {
      const unsigned cp = c[j / 3], a = (s[j >> 2] >> (8 * (j & 3))) & 255u, old = (f[j >> 2] >> (8 * (j & 3))) & 255u;
      const unsigned v = cp * a + (n - cp) * old + half;
      o[j >> 2] |= (cp == n ? a : __umulhi(v, magic)) << (8 * (j & 3));
    }
  } else {
    o[0] = s[0]; o[1] = s[1]; o[2] = s[2];
  }
  if (sel == 0x01010101u && ((uintptr_t)dst & 3) == 0) {
    unsigned* d = (unsigned*)dst;
    d[0] = o[0]; d[1] = o[1]; d[2] = o[2];
    return;
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    if ((sel >> (8 * p)) & 1u) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const int j = 3 * p + ch;
        dst[j] = (unsigned char)((o[j >> 2] >> (8 * (j & 3))) & 255u);
      }
    }
  }
}

}  // namespace

hipError_t launch_window_paste_feather(const se_window* d_wins, const unsigned char* rgb, const unsigned char* m8, int B, int hs, int ws,
                                       int radius, hipStream_t st) {
  const dim3 grid((unsigned)((ws + FT_W - 1) / FT_W), (unsigned)((hs + FT_H - 1) / FT_H), (unsigned)B);
  // bytes: an upper bound (every pixel selected, every count below n): mask and lock with the halo's share, rgb and the frame's
  // window read, the window written
  const double halo = (double)(FT_W + 2 * radius) * (FT_H + 2 * radius) / (double)(FT_W * FT_H);
  set_launch_cost(0.0, (double)B * hs * ws * (2.0 * halo + 9.0), "window_paste_feather");
  set_launch_grid((long)grid.x * grid.y * grid.z);
  ProfScope ps_(st, PL_WINDOW_PASTE_FEATHER);
  hipLaunchKernelGGL(window_paste_feather_kernel, grid, dim3(256), 0, st, d_wins, rgb, m8, B, hs, ws, radius);
  return hipGetLastError();
}

}  // namespace se
