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
// One workgroup = one tile of one request's window (se_seltile.h: the tile, the count, the division, the store), in three steps:
//  stage: sel of the tile and its r-wide halo.  Four columns that lie inside the window are read with load4_within bounded by the
//         window row's own bytes (mask and lock alike); a group that crosses a side of the window goes pixel by pixel through the
//         edge rule.
//  rows:  count_rows.
//  blend: a lane owns 4 consecutive pixels of one row, as in window_paste.  It counts (count4), reads the rgb bytes of its pixels
//         and -- only where some c < n -- the frame's old bytes, and writes by store_targets.  c == n gives rgb itself, so r = 0 is
//         window_paste_locked byte for byte.
// A lane reads a frame byte only of pixels it may write, through aligned dwords that stay inside the window row's bytes; a
// dword may hold bytes another lane writes, but the lane uses its own bytes only, and each byte has one writer.  No atomics.
#include "../../include/sketchedit_hip.h"
#include "se_kernels.h"
#include "se_seltile.h"

namespace se {

namespace {

__global__ void __launch_bounds__(256) window_paste_feather_kernel(const se_window* __restrict__ wins, const unsigned char* __restrict__ rgb,
                                                                   const unsigned char* __restrict__ m8, int B, int hs, int ws, int r) {
  __shared__ unsigned s_sel[SEL_ROWS * SEL_PITCH / 4];            // {0, 1} per pixel; row pitch SEL_PITCH bytes
  __shared__ unsigned s_row[SEL_ROWS * SEL_W / 4];                // horizontal sums, a byte per pixel; row pitch SEL_W bytes
  const int tid = threadIdx.x, b = blockIdx.z;
  const se_window w = wins[b];
  const unsigned char* plane = wins[B + b].frame_u8;
  const int tx0 = blockIdx.x * SEL_W, ty0 = blockIdx.y * SEL_H;   // the tile, in window pixels
  const int rows = SEL_H + 2 * r, cols4 = (SEL_W + 2 * r + 3) >> 2;       // the staged rows, and dwords per staged row
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
    s_sel[i * (SEL_PITCH / 4) + j4] = v;
    any |= v;
  }
  // (also the barrier between stage and rows.)  Nothing selected under the tile or its halo: nothing to write
  if (!__syncthreads_or((int)any)) return;

  // ---- rows
  count_rows(s_sel, s_row, rows, r, tid);
  __syncthreads();

  // ---- blend: the lane's 4 pixels (y, x .. x + 3) of the window
  const int lx = 4 * (tid & 15), ly = tid >> 4;
  const int x = tx0 + lx, y = ty0 + ly;
  if (y >= hs || x >= ws) return;
  const int npx = min(4, ws - x);                                 // the lane's pixels inside the window
  unsigned sel = 0;                                               // a byte per pixel, {0, 1}
  {
    const unsigned char* c8 = (const unsigned char*)s_sel + (ly + r) * SEL_PITCH + lx + r;
    for (int p = 0; p < npx; ++p) sel |= (unsigned)c8[p] << (8 * p);
  }
  if (!sel) return;
  const unsigned n = box_area(r);
  unsigned c[4];
  count4(s_row, ly, tid & 15, r, c);
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
    const BoxDiv bd(n);                                           // (n > 1 here: n == 1 has c == n)
#pragma unroll
    for (int j = 0; j < 12; ++j) {
      const unsigned a = (s[j >> 2] >> (8 * (j & 3))) & 255u, old = (f[j >> 2] >> (8 * (j & 3))) & 255u;
      o[j >> 2] |= bd.blend(c[j / 3], a, old) << (8 * (j & 3));
    }
  } else {
    o[0] = s[0]; o[1] = s[1]; o[2] = s[2];
  }
  store_targets(dst, o, sel);
}

}  // namespace

hipError_t launch_window_paste_feather(const se_window* d_wins, const unsigned char* rgb, const unsigned char* m8, int B, int hs, int ws,
                                       int radius, hipStream_t st) {
  const dim3 grid((unsigned)((ws + SEL_W - 1) / SEL_W), (unsigned)((hs + SEL_H - 1) / SEL_H), (unsigned)B);
  // bytes: an upper bound (every pixel selected, every count below n): mask and lock with the halo's share, rgb and the frame's
  // window read, the window written
  const double halo = (double)(SEL_W + 2 * radius) * (SEL_H + 2 * radius) / (double)(SEL_W * SEL_H);
  set_launch_cost(0.0, (double)B * hs * ws * (2.0 * halo + 9.0), "window_paste_feather");
  set_launch_grid((long)grid.x * grid.y * grid.z);
  ProfScope ps_(st, PL_WINDOW_PASTE_FEATHER);
  hipLaunchKernelGGL(window_paste_feather_kernel, grid, dim3(256), 0, st, d_wins, rgb, m8, B, hs, ws, radius);
  return hipGetLastError();
}

}  // namespace se
