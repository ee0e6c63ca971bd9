// Move or clone a selection (the rule is stated in include/sketchedit_move.h and in plain numpy in
// tests/move_util.py).  Two integer-only kernels, plain vector loads and stores, no atomics, nothing polled, any alignment of the
// frame, the planes and Wi, no byte outside the frame, a plane or the slot's rows read or written.
//
//  moved(y, x): MoveMap (se_movemap.h), the gather that the seamless drop (se_blend.hip) shares.
//
//  move_drop<FEATHER>: window_paste_feather's shape (se_feather.hip) on se_seltile.h's tile.  The grid covers the tiles of the shifted box
//                clipped to the frame, never the frame.  FEATHER (r > 0), three steps over LDS:
//                 stage: moved of the tile and its r-wide halo, a dword of four {0, 1} bytes per lane and step -- taken as the
//                        rule takes it, on the moved selection alone: neither the frame's edge nor the lock enters the count;
//                 rows:  count_rows;
//                 blend: a lane owns 4 consecutive pixels of a row, counts (count4), clears the locked ones, reads the lift's
//                        bytes of its pixels and -- only where some c < n -- the frame's old bytes.
//                A tile whose halo holds no selected pixel stores nothing.  !FEATHER (r = 0) takes neither LDS nor the count: a
//                lane's four moved bytes come straight from S.  Stores: store_targets.  A lane reads frame bytes only through
//                aligned dwords that stay inside the destination row's bytes and uses its own pixels' only.
//                The object's bytes come from the lift, so where source and destination overlap nobody reads what another wrote.
//  plane_shift:  plane_combine's walk (se_lasso.hip; store_plane_dword): one lane per aligned dword of the output's Hi Wi flat
//                bytes.  A dword's pixels that share a row take the gather above; a dword across a row's end goes pixel by pixel.
#include "../../include/sketchedit_hip.h"
#include "../../include/sketchedit_move.h"
#include "se_kernels.h"
#include "se_movemap.h"
#include "se_seltile.h"

#include <cstdint>

namespace se {

namespace {

template <bool FEATHER>
__global__ void __launch_bounds__(256) move_drop_kernel(unsigned char* __restrict__ frame, int Wi, Lift lift, MoveMap mm,
                                                        const unsigned char* __restrict__ lock, int ry0, int rx0, int ry1, int rx1, int r) {
  __shared__ unsigned s_sel[FEATHER ? SEL_ROWS * SEL_PITCH / 4 : 1];        // {0, 1} per pixel; row pitch SEL_PITCH bytes
  __shared__ unsigned s_row[FEATHER ? SEL_ROWS * SEL_W / 4 : 1];            // horizontal sums, a byte per pixel; row pitch SEL_W bytes
  const int tid = threadIdx.x;
  const int tx0 = rx0 + blockIdx.x * SEL_W, ty0 = ry0 + blockIdx.y * SEL_H; // the tile, in frame pixels
  const int lx = 4 * (tid & 15), ly = tid >> 4;
  const int x = tx0 + lx, y = ty0 + ly;                                     // the lane's 4 pixels (y, x .. x + 3)

  unsigned sel = 0;                                                         // a byte per pixel, {0, 1}: moved, then target
  unsigned c[4] = {1u, 1u, 1u, 1u};
  const BoxDiv bd(box_area(r));
  if (FEATHER) {
    const int rows = SEL_H + 2 * r, cols4 = (SEL_W + 2 * r + 3) >> 2;       // the staged rows, and dwords per staged row
    // ---- stage: staged (i, j) = moved(ty0 - r + i, tx0 - r + j)
    unsigned any = 0;
    for (int t = tid; t < rows * cols4; t += 256) {
      const int i = t / cols4, j4 = t % cols4;
      const unsigned v = mm.moved4(ty0 - r + i, tx0 - r + 4 * j4);
      s_sel[i * (SEL_PITCH / 4) + j4] = v;
      any |= v;
    }
    // (also the barrier between stage and rows.)  Nothing selected under the tile or its halo: nothing to write
    if (!__syncthreads_or((int)any)) return;

    // ---- rows
    count_rows(s_sel, s_row, rows, r, tid);
    __syncthreads();
  }

  // ---- blend: the lane's pixels inside the destination rectangle
  if (y >= ry1 || x >= rx1) return;
  const int npx = min(4, rx1 - x);
  if (FEATHER) {
    const unsigned char* c8 = (const unsigned char*)s_sel + (ly + r) * SEL_PITCH + lx + r;
    for (int p = 0; p < npx; ++p) sel |= (unsigned)c8[p] << (8 * p);
  } else {
    sel = mm.moved4(y, x) & (0xffffffffu >> (8 * (4 - npx)));
  }
  if (!sel) return;
  sel = unlocked_targets(sel, lock, Wi, y, x, npx);
  if (!sel) return;
  if (FEATHER) count4(s_row, ly, tid & 15, r, c);
  // the lift's bytes of the lane's pixels: 12 consecutive bytes of one slot row, from the lowest source column
  const bool fx = (mm.flip & SE_MOVE_FLIP_X) != 0;
  const int sy = mm.qy(y), sx = mm.qx(x);                                   // sy lies in the box: y is a row of the shifted box
  const unsigned char* prow = lift.row(sy);
  unsigned s[3], o[3] = {0u, 0u, 0u};
  load12_within(prow + 3 * (ptrdiff_t)((fx ? sx - 3 : sx) - lift.lx0), prow, prow + 3 * (size_t)lift.lw, s);
  unsigned char* frow = frame + ((size_t)y * Wi + rx0) * 3;                 // the destination row's bytes: [frow, frow + 3 (rx1 - rx0))
  unsigned char* dst = frame + ((size_t)y * Wi + x) * 3;
  bool full = true;                                                         // every target of the lane has c == n
  if (FEATHER) {
#pragma unroll
    for (int p = 0; p < 4; ++p) full = full && (!((sel >> (8 * p)) & 1u) || c[p] == bd.n);
  }
  unsigned f[3] = {0u, 0u, 0u};
  if (!full) load12_within(dst, frow, frow + 3 * (size_t)(rx1 - rx0), f);
#pragma unroll
  for (int j = 0; j < 12; ++j) {
    const int js = 3 * (3 - j / 3) + j % 3;                                 // the byte of pixel j / 3 under the x flip
    const unsigned a = ((fx ? s[js >> 2] >> (8 * (js & 3)) : s[j >> 2] >> (8 * (j & 3)))) & 255u;
    const unsigned v = FEATHER ? bd.blend(c[j / 3], a, (f[j >> 2] >> (8 * (j & 3))) & 255u) : a;
    o[j >> 2] |= v << (8 * (j & 3));
  }
  store_targets(dst, o, sel);
}

// n = Hi Wi pixels; lane q owns the aligned dword at (out - mis) + 4 q, mis = out & 3: the pixels 4 q - mis .. + 3
__global__ void __launch_bounds__(256) plane_shift_kernel(MoveMap mm, unsigned char* __restrict__ out, long n, long ndw) {
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= ndw) return;
  const int mis = (int)((uintptr_t)out & 3);
  const long p0 = 4 * q - mis;                                       // the dword's first pixel (may lie outside [0, n))
  const long first = p0 < 0 ? 0 : p0, last = p0 + 3 < n ? p0 + 3 : n - 1;      // the lane's pixels of the plane
  const int y = (int)(first / mm.Wi), x = (int)(first - (long)y * mm.Wi);
  unsigned v = 0;
  if (x + (int)(last - first) < mm.Wi) {                             // one row: (y, x ..) are the dword's bytes from first - p0 on
    v = (mm.moved4(y, x) * 255u) << (8 * (int)(first - p0));         // (bytes past `last` are never stored)
  } else {
    for (long p = first; p <= last; ++p) {
      const int py = (int)(p / mm.Wi), px = (int)(p - (long)py * mm.Wi);
      v |= ((mm.moved4(py, px) & 1u) * 255u) << (8 * (int)(p - p0));
    }
  }
  store_plane_dword(out, p0, n, v);
}

}  // namespace

hipError_t launch_move_drop(unsigned char* frame, int Hi, int Wi, const unsigned char* lift, int ly0, int lx0, int lw, int lpitch,
                            const unsigned char* sel, const unsigned char* lock, int by0, int bx0, int by1, int bx1, int dy, int dx, int flip,
                            int radius, hipStream_t st) {
  // the destination rectangle: the shifted box clipped to the frame
  const int ry0 = max(by0 + dy, 0), rx0 = max(bx0 + dx, 0), ry1 = min(by1 + dy, Hi), rx1 = min(bx1 + dx, Wi);
  if (ry0 >= ry1 || rx0 >= rx1) return hipSuccess;                   // the whole box lands outside: nothing to do
  const dim3 grid((unsigned)((rx1 - rx0 + SEL_W - 1) / SEL_W), (unsigned)((ry1 - ry0 + SEL_H - 1) / SEL_H));
  const Lift lf{lift, ly0, lx0, lw, lpitch};
  const MoveMap mm{sel, Wi, by0, bx0, by1, bx1, dy, dx, flip};
  // bytes: an upper bound (every pixel a target, every count below n): the plane with the halo's share, the lock, the lift and
  // the frame's rectangle read, the rectangle written
  const double halo = radius ? (double)(SEL_W + 2 * radius) * (SEL_H + 2 * radius) / (double)(SEL_W * SEL_H) : 1.0;
  set_launch_cost(0.0, (double)(ry1 - ry0) * (rx1 - rx0) * (halo + (lock ? 1.0 : 0.0) + (radius ? 9.0 : 6.0)), "move_drop");
  set_launch_grid((long)grid.x * grid.y);
  ProfScope ps_(st, PL_MOVE_DROP);
  if (radius > 0)
    hipLaunchKernelGGL(move_drop_kernel<true>, grid, dim3(256), 0, st, frame, Wi, lf, mm, lock, ry0, rx0, ry1, rx1, radius);
  else
    hipLaunchKernelGGL(move_drop_kernel<false>, grid, dim3(256), 0, st, frame, Wi, lf, mm, lock, ry0, rx0, ry1, rx1, 0);
  return hipGetLastError();
}

hipError_t launch_plane_shift(const unsigned char* sel, int Hi, int Wi, int by0, int bx0, int by1, int bx1, int dy, int dx, int flip,
                              unsigned char* out, hipStream_t st) {
  const long n = (long)Hi * Wi;
  const long ndw = (n + (long)((uintptr_t)out & 3) + 3) / 4;         // the aligned dwords that hold the output's bytes
  const MoveMap mm{sel, Wi, by0, bx0, by1, bx1, dy, dx, flip};
  // bytes: the output written once, the box read once
  set_launch_cost(0.0, (double)n + (double)(by1 - by0) * (bx1 - bx0), "plane_shift");
  set_launch_grid((ndw + 255) / 256);
  ProfScope ps_(st, PL_PLANE_SHIFT);
  hipLaunchKernelGGL(plane_shift_kernel, dim3((unsigned)((ndw + 255) / 256)), dim3(256), 0, st, mm, out, n, ndw);
  return hipGetLastError();
}

}  // namespace se
