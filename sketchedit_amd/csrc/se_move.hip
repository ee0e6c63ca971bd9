// Move or clone a selection (the rule is stated in include/sketchedit_move.h and in plain numpy in
// tests/move_util.py).  Two integer-only kernels, plain vector loads and stores, no atomics, nothing polled, any alignment of the
// frame, the planes and Wi, no byte outside the frame, a plane or the slot's rows read or written.
//
//  moved(y, x) = S[q] != 0 with q = (y - dy, x - dx), mirrored about the box by the flip bits, where q lies in the box; else 0.
//                q is a function of the DESTINATION pixel: the kernels gather.  Four neighbouring x have four neighbouring qx,
//                ascending without the x flip and descending with it, so they are one load4_within bounded by the box's row of S
//                (bytes outside the box read as 0 without a load), byte-swapped under the flip.
//
//  move_drop<FEATHER>: window_paste_feather's shape (se_feather.hip).  The grid covers the tiles of the shifted box clipped to the
//                frame, never the frame.  One workgroup = one 64 x 16 tile, 256 lanes.  FEATHER (r > 0), three steps over LDS:
//                 stage: moved of the tile and its r-wide halo, a dword of four {0, 1} bytes per lane and step -- taken as the
//                        rule takes it, on the moved selection alone: neither the frame's edge nor the lock enters the count;
//                 rows:  per staged row the 64 horizontal sums over 2r + 1 columns, a byte each (<= 33);
//                 blend: a lane owns 4 consecutive pixels of a row, adds the 2r + 1 row sums above and below them, clears the
//                        locked ones, reads the lift's bytes of its pixels and -- only where some c < n -- the frame's old bytes.
//                A tile whose halo holds no selected pixel stores nothing.  !FEATHER (r = 0) takes neither LDS nor the count: a
//                lane's four moved bytes come straight from S.  Stores follow se_window.hip's ownership rule: three dwords where
//                all four pixels are targets and the address is aligned, single bytes of targets otherwise.  A lane reads frame
//                bytes only through aligned dwords that stay inside the destination row's bytes and uses its own pixels' only.
//                The object's bytes come from the lift, so where source and destination overlap nobody reads what another wrote.
//                The division is se_feather.hip's: mulhi(v, floor(2^32 / n) + 1) == v / n for v < 2^19, n <= 1089.
//  plane_shift:  plane_combine's walk (se_lasso.hip): the output's Hi Wi flat bytes in the ALIGNED dwords that hold them, one lane
//                per dword, single bytes at the plane's two ends; every byte written, one writer per byte.  A dword's pixels that
//                share a row take the gather above; a dword across a row's end goes pixel by pixel.
#include "../../include/sketchedit_hip.h"
#include "../../include/sketchedit_move.h"
#include "se_device.h"
#include "se_kernels.h"

#include <cstdint>

namespace se {

namespace {

constexpr int MV_W = 64, MV_H = 16, MV_RMAX = SE_MOVE_MAX_RADIUS;
constexpr int MV_SEL_PITCH = 192;                     // bytes: 48 dwords = 16 mod 32 (se_feather.hip)
constexpr int MV_ROWS = MV_H + 2 * MV_RMAX;           // staged rows at the largest radius

// each non-zero byte of u -> 1
__device__ __forceinline__ unsigned bytes_nonzero(unsigned u) {
  return ((u & 0xffu) ? 1u : 0u) | ((u & 0xff00u) ? 0x100u : 0u) | ((u & 0xff0000u) ? 0x10000u : 0u) | ((u & 0xff000000u) ? 0x1000000u : 0u);
}

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

// the offset / flip map and the box it gathers from
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

// the lift: the slot's row of source row sy is [lift + (sy - ly0) lpitch, + 3 lw), its pixel sx at 3 (sx - lx0)
struct Lift {
  const unsigned char* p;
  int ly0, lx0, lw, lpitch;
};

template <bool FEATHER>
__global__ void __launch_bounds__(256) move_drop_kernel(unsigned char* __restrict__ frame, int Wi, Lift lift, MoveMap mm,
                                                        const unsigned char* __restrict__ lock, int ry0, int rx0, int ry1, int rx1, int r) {
  __shared__ unsigned s_sel[FEATHER ? MV_ROWS * MV_SEL_PITCH / 4 : 1];      // {0, 1} per pixel; row pitch MV_SEL_PITCH bytes
  __shared__ unsigned s_row[FEATHER ? MV_ROWS * MV_W / 4 : 1];              // horizontal sums, a byte per pixel; row pitch MV_W bytes
  const int tid = threadIdx.x;
  const int tx0 = rx0 + blockIdx.x * MV_W, ty0 = ry0 + blockIdx.y * MV_H;   // the tile, in frame pixels
  const int lx = 4 * (tid & 15), ly = tid >> 4;
  const int x = tx0 + lx, y = ty0 + ly;                                     // the lane's 4 pixels (y, x .. x + 3)

  unsigned sel = 0;                                                         // a byte per pixel, {0, 1}: moved, then target
  unsigned c[4] = {1u, 1u, 1u, 1u};
  const unsigned n = (unsigned)((2 * r + 1) * (2 * r + 1));
  if (FEATHER) {
    const int rows = MV_H + 2 * r, cols4 = (MV_W + 2 * r + 3) >> 2;         // the staged rows, and dwords per staged row
    // ---- stage: staged (i, j) = moved(ty0 - r + i, tx0 - r + j)
    unsigned any = 0;
    for (int t = tid; t < rows * cols4; t += 256) {
      const int i = t / cols4, j4 = t % cols4;
      const unsigned v = mm.moved4(ty0 - r + i, tx0 - r + 4 * j4);
      s_sel[i * (MV_SEL_PITCH / 4) + j4] = v;
      any |= v;
    }
    // (also the barrier between stage and rows.)  Nothing selected under the tile or its halo: nothing to write
    if (!__syncthreads_or((int)any)) return;

    // ---- rows: s_row (i, x) = sum of staged (i, x .. x + 2r), four neighbouring x per lane and step
    for (int t = tid; t < rows * (MV_W / 4); t += 256) {
      const int i = t >> 4, k = t & 15;
      const unsigned* s = s_sel + i * (MV_SEL_PITCH / 4) + k;               // staged columns 4k ..
      const int nb = 2 * r + 4, nd = (nb + 3) >> 2;                         // bytes under the four sums, and their dwords
      unsigned char e[2 * MV_RMAX + 4];
#pragma unroll
      for (int q = 0; q < (2 * MV_RMAX + 4) / 4; ++q) {
        const unsigned d = q < nd ? s[q] : 0u;
#pragma unroll
        for (int z = 0; z < 4; ++z) e[4 * q + z] = (unsigned char)((d >> (8 * z)) & 255u);
      }
      unsigned s0 = 0;
#pragma unroll
      for (int z = 0; z < 2 * MV_RMAX + 1; ++z) s0 += z <= 2 * r ? e[z] : 0u;
      // e[2r + 1 ..]: a compile-time walk with a run-time pick, so that e stays in registers
      unsigned in1 = 0, in2 = 0, in3 = 0;
#pragma unroll
      for (int z = 1; z < 2 * MV_RMAX + 4; ++z) {
        in1 = z == 2 * r + 1 ? e[z] : in1;
        in2 = z == 2 * r + 2 ? e[z] : in2;
        in3 = z == 2 * r + 3 ? e[z] : in3;
      }
      const unsigned s1 = s0 - e[0] + in1, s2 = s1 - e[1] + in2, s3 = s2 - e[2] + in3;
      s_row[i * (MV_W / 4) + k] = s0 | (s1 << 8) | (s2 << 16) | (s3 << 24);
    }
    __syncthreads();
  }

  // ---- blend: the lane's pixels inside the destination rectangle
  if (y >= ry1 || x >= rx1) return;
  const int npx = min(4, rx1 - x);
  if (FEATHER) {
    const unsigned char* c8 = (const unsigned char*)s_sel + (ly + r) * MV_SEL_PITCH + lx + r;
    for (int p = 0; p < npx; ++p) sel |= (unsigned)c8[p] << (8 * p);
  } else {
    sel = mm.moved4(y, x) & (0xffffffffu >> (8 * (4 - npx)));
  }
  if (!sel) return;
  if (lock) {
    const unsigned char* lrow = lock + (size_t)y * Wi;                      // the lane's bytes of the lock: [lrow + x, lrow + x + npx)
    sel &= ~bytes_nonzero(load4_within(lrow + x, lrow + x, lrow + x + npx));
    if (!sel) return;
  }
  if (FEATHER) {
    unsigned lo = 0, hi = 0;                                                // pixels 0, 2 and 1, 3 in 16-bit fields
    for (int d = 0; d <= 2 * r; ++d) {
      const unsigned v = s_row[(ly + d) * (MV_W / 4) + (tid & 15)];
      lo += v & 0x00ff00ffu;
      hi += (v >> 8) & 0x00ff00ffu;
    }
    c[0] = lo & 0xffffu; c[1] = hi & 0xffffu; c[2] = lo >> 16; c[3] = hi >> 16;
  }
  // the lift's bytes of the lane's pixels: 12 consecutive bytes of one slot row, from the lowest source column
  const bool fx = (mm.flip & SE_MOVE_FLIP_X) != 0;
  const int sy = mm.qy(y), sx = mm.qx(x);                                   // sy lies in the box: y is a row of the shifted box
  const unsigned char* prow = lift.p + (size_t)(sy - lift.ly0) * lift.lpitch;
  unsigned s[3], o[3] = {0u, 0u, 0u};
  load12_within(prow + 3 * (ptrdiff_t)((fx ? sx - 3 : sx) - lift.lx0), prow, prow + 3 * (size_t)lift.lw, s);
  unsigned char* frow = frame + ((size_t)y * Wi + rx0) * 3;                 // the destination row's bytes: [frow, frow + 3 (rx1 - rx0))
  unsigned char* dst = frame + ((size_t)y * Wi + x) * 3;
  bool full = true;                                                         // every target of the lane has c == n
  if (FEATHER) {
#pragma unroll
    for (int p = 0; p < 4; ++p) full = full && (!((sel >> (8 * p)) & 1u) || c[p] == n);
  }
  unsigned f[3] = {0u, 0u, 0u};
  if (!full) load12_within(dst, frow, frow + 3 * (size_t)(rx1 - rx0), f);
  const unsigned magic = (unsigned)((1ull << 32) / n) + 1u, half = (n - 1u) >> 1;
#pragma unroll
  for (int j = 0; j < 12; ++j) {
    const int js = 3 * (3 - j / 3) + j % 3;                                 // the byte of pixel j / 3 under the x flip
    const unsigned a = ((fx ? s[js >> 2] >> (8 * (js & 3)) : s[j >> 2] >> (8 * (j & 3)))) & 255u;
    unsigned v = a;
    if (FEATHER) {
      const unsigned cp = c[j / 3], old = (f[j >> 2] >> (8 * (j & 3))) & 255u;
      v = cp == n ? a : __umulhi(cp * a + (n - cp) * old + half, magic);
    }
    o[j >> 2] |= v << (8 * (j & 3));
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
  unsigned char* dst = out + p0;                                     // 4-byte aligned
  if (p0 >= 0 && p0 + 4 <= n) {
    *(unsigned*)dst = v;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (p0 + e >= 0 && p0 + e < n) dst[e] = (unsigned char)((v >> (8 * e)) & 255u);
  }
}

}  // namespace

hipError_t launch_move_drop(unsigned char* frame, int Hi, int Wi, const unsigned char* lift, int ly0, int lx0, int lw, int lpitch,
                            const unsigned char* sel, const unsigned char* lock, int by0, int bx0, int by1, int bx1, int dy, int dx, int flip,
                            int radius, hipStream_t st) {
  // the destination rectangle: the shifted box clipped to the frame
  const int ry0 = max(by0 + dy, 0), rx0 = max(bx0 + dx, 0), ry1 = min(by1 + dy, Hi), rx1 = min(bx1 + dx, Wi);
  if (ry0 >= ry1 || rx0 >= rx1) return hipSuccess;                   // the whole box lands outside: nothing to do
  const dim3 grid((unsigned)((rx1 - rx0 + MV_W - 1) / MV_W), (unsigned)((ry1 - ry0 + MV_H - 1) / MV_H));
  const Lift lf{lift, ly0, lx0, lw, lpitch};
  const MoveMap mm{sel, Wi, by0, bx0, by1, bx1, dy, dx, flip};
  // bytes: an upper bound (every pixel a target, every count below n): the plane with the halo's share, the lock, the lift and
  // the frame's rectangle read, the rectangle written
  const double halo = radius ? (double)(MV_W + 2 * radius) * (MV_H + 2 * radius) / (double)(MV_W * MV_H) : 1.0;
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
