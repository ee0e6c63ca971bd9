// Seamless move and clone (the definition is stated in include/sketchedit_blend.h and in plain numpy in
// tests/blend_util.py).  Four integer-only kernels, plain vector loads and stores, no atomics, nothing polled; every loop bound is
// a launch argument or a constant, so the schedule depends on the rectangle's size alone.  Workgroups meet at launch boundaries only.
//
//  A CELL of a level is one 8-byte record {u0 | u1 << 16, u2 | state << 16}: the three channels' values (uint16 each) and the state.
//  A level of h x w cells has two buffers of h w records; a launch reads one and writes the other, or reads a finer / coarser level.
//
//  blend_init:   E's 64 x 16 tiles on se_seltile.h's tile.  stage: target of the tile and its halo of 1, a dword of four {0, 1}
//                bytes per lane and step (MoveMap's gather, the frame's edge and the lock cleared).  Then a lane owns 4 cells of a
//                row: UNKNOWN where its own byte is set; KNOWN where it is not, a neighbour's is and the lift holds src(p) -- there it
//                reads F[p] and P[src(p)]; OUT otherwise.  Every record of level 0's first buffer is written.
//  blend_pull:   one lane per cell of level l: its up to four children of level l - 1's first buffer -> level l's first buffer.
//  blend_relax:  a workgroup stages the cells of its RX_H x RX_W = 32 x 80 rectangle that lie inside the grid in LDS (the others are
//                OUT and are neither written nor read); UNKNOWN cells take the parent's value in a level's first launch.  It runs `sweeps` red-black sweeps there and writes the cells `halo`
//                inside the staged rectangle.  Two forms, one kernel: halo 8, 4 sweeps, the grid the level's 64 x 16 tiles (a
//                half-sweep lets a wrong value travel one cell, so after 8 half-sweeps the cells 8 inside the staged edge are
//                what global sweeps give them: DESIGN.md 6x); halo 0, all J_l sweeps, ONE workgroup, where the level is at most
//                32 x 80 cells.  A half-sweep reads cells of the other parity only, so its lanes race on nothing.  A block whose
//                half-sweep has at most 64 candidates runs its sweeps in one wave, without a workgroup barrier.
//  blend_apply:  move_drop_kernel<false>'s walk over D's tiles and its store (store_targets: one writer per byte): the lift's bytes
//                plus the membrane of level 0.
#include "../../include/sketchedit_blend.h"
#include "../../include/sketchedit_hip.h"
#include "se_kernels.h"
#include "se_movemap.h"
#include "se_seltile.h"

#include <cstdint>

namespace se {

namespace {

constexpr unsigned ST_OUT = 0u, ST_KNOWN = 1u, ST_UNKNOWN = 2u;
constexpr unsigned U_ZERO = 4096u;                       // the value of a difference of 0
constexpr int RX_H = 32, RX_W = 80, RX_HALO = 8;         // the staged cells of blend_relax, and the halo of its tiled form
static_assert(RX_H - 2 * RX_HALO == SEL_H && RX_W - 2 * RX_HALO == SEL_W, "the tiled form writes one selection tile");

DEVFN unsigned cell_state(uint2 r) { return r.y >> 16; }
DEVFN uint2 make_cell(unsigned u0, unsigned u1, unsigned u2, unsigned st) { return make_uint2(u0 | (u1 << 16), u2 | (st << 16)); }

// (2 sum + n) / (2 n), n in 1 .. 4: the mean of n values, halves rounded up
DEVFN unsigned mean_round(unsigned sum, int n) {
  switch (n) {
    case 1: return sum;
    case 2: return (sum + 1u) >> 1;
    case 3: return (2u * sum + 3u) / 6u;
    default: return (sum + 2u) >> 2;
  }
}

// the three channels' sums of up to four cells
struct Sum3 {
  unsigned a = 0, b = 0, c = 0;
  int n = 0;
  DEVFN void add(uint2 r) { a += r.x & 0xffffu; b += r.x >> 16; c += r.y & 0xffffu; ++n; }
  DEVFN uint2 mean(unsigned st) const { return make_cell(mean_round(a, n), mean_round(b, n), mean_round(c, n), st); }
};

// target of the pixels (y, x .. x + 3), any integers: a byte of {0, 1} each
DEVFN unsigned targets4(const MoveMap& mm, const unsigned char* lock, int Hi, int y, int x) {
  const int Wi = mm.Wi;
  if (y < 0 || y >= Hi || x + 3 < 0 || x >= Wi) return 0u;
  unsigned m = mm.moved4(y, x);
  if (!m) return 0u;
  const int lo = max(x, 0), hi = min(x + 4, Wi);         // the pixels of the four that lie in the frame
#pragma unroll
  for (int p = 0; p < 4; ++p)
    if (x + p < lo || x + p >= hi) m &= ~(255u << (8 * p));
  if (lock && m) {
    const unsigned char* lrow = lock + (size_t)y * Wi;   // the lock's bytes of those pixels: [lrow + lo, lrow + hi)
    m &= ~bytes_nonzero(load4_within(lrow + x, lrow + lo, lrow + hi));
  }
  return m;
}

constexpr int INIT_PITCH = 68;                            // bytes of a staged row: 64 + 2 pixels in 17 dwords

__global__ void __launch_bounds__(256) blend_init_kernel(const unsigned char* __restrict__ frame, int Hi, Lift lift, int lh, MoveMap mm,
                                                         const unsigned char* __restrict__ lock, int ey0, int ex0, int eh, int ew,
                                                         uint2* __restrict__ out) {
  __shared__ unsigned s_t[(SEL_H + 2) * INIT_PITCH / 4];
  const int tid = threadIdx.x;
  const int tx0 = ex0 + blockIdx.x * SEL_W, ty0 = ey0 + blockIdx.y * SEL_H;
  // ---- stage: staged (i, j) = target(ty0 - 1 + i, tx0 - 1 + j)
  for (int t = tid; t < (SEL_H + 2) * (INIT_PITCH / 4); t += 256) {
    const int i = t / (INIT_PITCH / 4), j4 = t % (INIT_PITCH / 4);
    s_t[t] = targets4(mm, lock, Hi, ty0 - 1 + i, tx0 - 1 + 4 * j4);
  }
  __syncthreads();
  const int lx = 4 * (tid & 15), ly = tid >> 4;
  const int x = tx0 + lx, y = ty0 + ly;
  if (y >= ey0 + eh) return;
  const unsigned char* s8 = (const unsigned char*)s_t;
  const int sy = mm.qy(y);
  const bool rowin = sy >= lift.ly0 && sy < lift.ly0 + lh;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int xp = x + p;
    if (xp >= ex0 + ew) break;
    const int c = (ly + 1) * INIT_PITCH + lx + 1 + p;
    uint2 r = make_cell(0u, 0u, 0u, ST_OUT);
    if (s8[c]) {
      r = make_cell(0u, 0u, 0u, ST_UNKNOWN);
    } else if (s8[c - INIT_PITCH] | s8[c + INIT_PITCH] | s8[c - 1] | s8[c + 1]) {
      const int sx = mm.qx(xp);
      if (rowin && sx >= lift.lx0 && sx < lift.lx0 + lift.lw) {
        const unsigned char* f = frame + ((size_t)y * mm.Wi + xp) * 3;
        const unsigned char* q = lift.row(sy) + 3 * (size_t)(sx - lift.lx0);
        r = make_cell(16u * f[0] + U_ZERO - 16u * q[0], 16u * f[1] + U_ZERO - 16u * q[1], 16u * f[2] + U_ZERO - 16u * q[2], ST_KNOWN);
      }
    }
    out[(size_t)(y - ey0) * ew + (xp - ex0)] = r;
  }
}

// level l (ph x pw) from level l - 1 (ch x cw)
__global__ void __launch_bounds__(256) blend_pull_kernel(const uint2* __restrict__ child, int ch, int cw, uint2* __restrict__ out, int ph, int pw) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= ph * pw) return;
  const int y = t / pw, x = t - y * pw;
  Sum3 s;
  bool unknown = false;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int cy = 2 * y + a, cx = 2 * x + b;
      if (cy < ch && cx < cw) {
        const uint2 r = child[(size_t)cy * cw + cx];
        if (cell_state(r) == ST_KNOWN) s.add(r);
        else if (cell_state(r) == ST_UNKNOWN) unknown = true;
      }
    }
  out[t] = s.n ? s.mean(ST_KNOWN) : make_cell(0u, 0u, 0u, unknown ? ST_UNKNOWN : ST_OUT);
}

// One red-black sweep's half of parity `par` over the staged cells [i0, i1) x [j0, j1): `cells` = (i1 - i0) ceil((j1 - j0) / 2)
// candidates, `stride` lanes.  A neighbour outside that rectangle is outside the grid, OUT by definition, and is never read.
DEVFN void relax_half(uint2* s, int tid, int stride, int cells, int half_w, int i0, int i1, int j0, int j1, int phase) {
  for (int t = tid; t < cells; t += stride) {
    const int ii = t / half_w, jj = t - ii * half_w;
    const int i = i0 + ii;
    const int j = j0 + 2 * jj + ((phase + i) & 1);
    if (j >= j1) continue;
    const int c = i * RX_W + j;
    const uint2 r = s[c];
    if (cell_state(r) != ST_UNKNOWN) continue;
    Sum3 n;
    if (i > i0) { const uint2 v = s[c - RX_W]; if (cell_state(v) != ST_OUT) n.add(v); }
    if (i < i1 - 1) { const uint2 v = s[c + RX_W]; if (cell_state(v) != ST_OUT) n.add(v); }
    if (j > j0) { const uint2 v = s[c - 1]; if (cell_state(v) != ST_OUT) n.add(v); }
    if (j < j1 - 1) { const uint2 v = s[c + 1]; if (cell_state(v) != ST_OUT) n.add(v); }
    if (n.n) s[c] = n.mean(ST_UNKNOWN);
  }
}

// `sweeps` sweeps of the h x w level on the staged rectangle whose corner is the tile's less `halo`; first: UNKNOWN cells start
// from the parent's value (parent == nullptr: from U_ZERO) instead of their own.
// Only the staged cells INSIDE the grid are walked -- rows [i0, i1), columns [j0, j1) of the staged rectangle -- by the stage, the
// half-sweeps and the write-out alike.  The cells outside are OUT in the statement and never change; here they are NEVER READ (a
// neighbour test stops at the rectangle's own edge) and so are not initialised either.  Where a half-sweep has at most 64
// candidates (the coarse levels: the whole form, one workgroup) wave 0 alone sweeps, the other waves leave behind the stage's
// barrier, and the half-sweeps are ordered by the wave's own program order on the LDS: a wavefront-scope fence pair keeps the
// compiler from moving an LDS access across it, and no workgroup barrier is executed.  Every trip count is a function of h, w and
// the block's index.
__global__ void __launch_bounds__(256) blend_relax_kernel(const uint2* __restrict__ src, uint2* __restrict__ dst, const uint2* __restrict__ parent,
                                                          int h, int w, int pw, int halo, int sweeps, int first) {
  __shared__ uint2 s[RX_H * RX_W];
  const int tid = threadIdx.x;
  const int gy0 = blockIdx.y * (RX_H - 2 * halo) - halo, gx0 = blockIdx.x * (RX_W - 2 * halo) - halo;      // the staged corner
  const int i0 = max(0, -gy0), i1 = min(RX_H, h - gy0), j0 = max(0, -gx0), j1 = min(RX_W, w - gx0);      // ... and the grid's part of it
  const int nh = i1 - i0, nw = j1 - j0;
  if (nh <= 0 || nw <= 0) return;                          // (no block of either form: its tile holds a cell of the grid)
  // ---- stage
  for (int t = tid; t < nh * nw; t += 256) {
    const int ii = t / nw, i = i0 + ii, j = j0 + (t - ii * nw);
    const int gy = gy0 + i, gx = gx0 + j;
    uint2 r = src[(size_t)gy * w + gx];
    if (first && cell_state(r) == ST_UNKNOWN) {
      if (parent) {
        const uint2 q = parent[(size_t)(gy >> 1) * pw + (gx >> 1)];
        r = make_uint2(q.x, (q.y & 0xffffu) | (ST_UNKNOWN << 16));
      } else {
        r = make_cell(U_ZERO, U_ZERO, U_ZERO, ST_UNKNOWN);
      }
    }
    s[i * RX_W + j] = r;
  }
  __syncthreads();
  // ---- sweep: the half-sweep of parity 0, then of parity 1, of the GRID's coordinates: staged (i, j) has parity (gy0 + i + gx0 + j) & 1
  const int half_w = (nw + 1) / 2, cells = nh * half_w;
  const int phase0 = gy0 + gx0 + j0;
  const bool one_wave = cells <= 64;                       // block-uniform: one wave covers a half-sweep
  if (one_wave && tid >= 64) return;                       // (behind the stage's barrier; wave 0 executes no other)
  const int stride = one_wave ? 64 : 256;
  for (int sw = 0; sw < sweeps; ++sw) {
    for (int par = 0; par < 2; ++par) {
      relax_half(s, tid, stride, cells, half_w, i0, i1, j0, j1, phase0 + par);
      if (one_wave) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      } else {
        __syncthreads();
      }
    }
  }
  // ---- the cells `halo` inside, by the lanes that swept them
  const int a0 = max(i0, halo), a1 = min(i1, RX_H - halo), b0 = max(j0, halo), b1 = min(j1, RX_W - halo);
  const int ah = a1 - a0, aw = b1 - b0;
  if (ah <= 0 || aw <= 0) return;
  for (int t = tid; t < ah * aw; t += stride) {
    const int ii = t / aw, i = a0 + ii, j = b0 + (t - ii * aw);
    dst[(size_t)(gy0 + i) * w + (gx0 + j)] = s[i * RX_W + j];
  }
}

__global__ void __launch_bounds__(256) blend_apply_kernel(unsigned char* __restrict__ frame, int Wi, Lift lift, MoveMap mm,
                                                          const unsigned char* __restrict__ lock, int ry0, int rx0, int ry1, int rx1,
                                                          const uint2* __restrict__ u0, int ey0, int ex0, int ew) {
  const int tid = threadIdx.x;
  const int x = rx0 + blockIdx.x * SEL_W + 4 * (tid & 15), y = ry0 + blockIdx.y * SEL_H + (tid >> 4);
  if (y >= ry1 || x >= rx1) return;
  const int npx = min(4, rx1 - x);
  unsigned sel = mm.moved4(y, x) & (0xffffffffu >> (8 * (4 - npx)));
  if (!sel) return;
  sel = unlocked_targets(sel, lock, Wi, y, x, npx);
  if (!sel) return;
  // the lift's bytes of the lane's pixels: 12 consecutive bytes of one slot row, from the lowest source column
  const bool fx = (mm.flip & SE_MOVE_FLIP_X) != 0;
  const int sy = mm.qy(y), sx = mm.qx(x);
  const unsigned char* prow = lift.row(sy);
  unsigned s[3], o[3] = {0u, 0u, 0u};
  load12_within(prow + 3 * (ptrdiff_t)((fx ? sx - 3 : sx) - lift.lx0), prow, prow + 3 * (size_t)lift.lw, s);
  const uint2* urow = u0 + (size_t)(y - ey0) * ew + (x - ex0);
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    if (!((sel >> (8 * p)) & 1u)) continue;
    const uint2 r = urow[p];
    const unsigned u[3] = {r.x & 0xffffu, r.x >> 16, r.y & 0xffffu};
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const int j = 3 * p + ch, js = 3 * (3 - p) + ch;                     // the byte of pixel p under the x flip
      const unsigned a = ((fx ? s[js >> 2] >> (8 * (js & 3)) : s[j >> 2] >> (8 * (j & 3)))) & 255u;
      const int v = (int)((16u * a + u[ch] + 8u) >> 4) - 256;
      o[j >> 2] |= (unsigned)min(max(v, 0), 255) << (8 * (j & 3));
    }
  }
  unsigned char* dst = frame + ((size_t)y * Wi + x) * 3;
  store_targets(dst, o, sel);
}

// the levels of an eh x ew grid: their sizes and where their two buffers begin, in records
struct Levels {
  int n = 0, h[16], w[16];
  size_t off[16], total = 0;
  Levels(int eh, int ew) {
    for (;;) {
      h[n] = eh; w[n] = ew; off[n] = total;
      total += 2 * (size_t)eh * ew;
      ++n;
      if (eh == 1 && ew == 1) break;
      eh = (eh + 1) / 2; ew = (ew + 1) / 2;
    }
  }
  uint2* buf(void* ws, int l, int k) const { return (uint2*)ws + off[l] + (size_t)k * h[l] * w[l]; }
};

}  // namespace

size_t blend_workspace_bytes(int eh, int ew) { return Levels(eh, ew).total * sizeof(uint2); }

hipError_t launch_move_blend(unsigned char* frame, int Hi, int Wi, const unsigned char* lift, int ly0, int lx0, int lh, int lw, int lpitch,
                             const unsigned char* sel, const unsigned char* lock, int by0, int bx0, int by1, int bx1, int dy, int dx, int flip,
                             void* ws, hipStream_t st) {
  // D: the shifted box clipped to the frame; E: D grown by one pixel and clipped to the frame
  const int ry0 = max(by0 + dy, 0), rx0 = max(bx0 + dx, 0), ry1 = min(by1 + dy, Hi), rx1 = min(bx1 + dx, Wi);
  if (ry0 >= ry1 || rx0 >= rx1) return hipSuccess;                   // the whole box lands outside: nothing to do
  const int ey0 = max(ry0 - 1, 0), ex0 = max(rx0 - 1, 0), eh = min(ry1 + 1, Hi) - ey0, ew = min(rx1 + 1, Wi) - ex0;
  const Lift lf{lift, ly0, lx0, lw, lpitch};
  const MoveMap mm{sel, Wi, by0, bx0, by1, bx1, dy, dx, flip};
  const Levels lv(eh, ew);
  const int T = lv.n - 1;
  hipError_t e;
  {
    const dim3 grid((unsigned)((ew + SEL_W - 1) / SEL_W), (unsigned)((eh + SEL_H - 1) / SEL_H));
    set_launch_cost(0.0, (double)eh * ew * (1.0 + (lock ? 1.0 : 0.0) + 8.0), "blend_init");
    set_launch_grid((long)grid.x * grid.y);
    ProfScope ps_(st, PL_BLEND_INIT);
    hipLaunchKernelGGL(blend_init_kernel, grid, dim3(256), 0, st, frame, Hi, lf, lh, mm, lock, ey0, ex0, eh, ew, lv.buf(ws, 0, 0));
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  for (int l = 1; l <= T; ++l) {
    const int cells = lv.h[l] * lv.w[l];
    set_launch_cost(0.0, 8.0 * ((double)lv.h[l - 1] * lv.w[l - 1] + cells), "blend_pull");
    set_launch_grid((cells + 255) / 256);
    ProfScope ps_(st, PL_BLEND_PULL);
    hipLaunchKernelGGL(blend_pull_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, lv.buf(ws, l - 1, 0), lv.h[l - 1], lv.w[l - 1],
                       lv.buf(ws, l, 0), lv.h[l], lv.w[l]);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  const uint2* parent = nullptr;                                     // the level above after its sweeps
  for (int l = T; l >= 0; --l) {
    const int h = lv.h[l], w = lv.w[l], sweeps = min(4 << min(l, 4), 64), pw = l < T ? lv.w[l + 1] : 0;
    const bool whole = h <= RX_H && w <= RX_W;
    const int launches = whole ? 1 : sweeps / 4, halo = whole ? 0 : RX_HALO;
    const dim3 grid(whole ? 1u : (unsigned)((w + SEL_W - 1) / SEL_W), whole ? 1u : (unsigned)((h + SEL_H - 1) / SEL_H));
    for (int k = 0; k < launches; ++k) {
      set_launch_cost(0.0, 8.0 * (double)grid.x * grid.y * (RX_H * RX_W + SEL_H * SEL_W), "blend_relax");
      set_launch_grid((long)grid.x * grid.y);
      ProfScope ps_(st, PL_BLEND_RELAX);
      hipLaunchKernelGGL(blend_relax_kernel, grid, dim3(256), 0, st, lv.buf(ws, l, k & 1), lv.buf(ws, l, (k + 1) & 1), parent, h, w, pw, halo,
                         whole ? sweeps : 4, k == 0 ? 1 : 0);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    parent = lv.buf(ws, l, launches & 1);
  }
  {
    const dim3 grid((unsigned)((rx1 - rx0 + SEL_W - 1) / SEL_W), (unsigned)((ry1 - ry0 + SEL_H - 1) / SEL_H));
    set_launch_cost(0.0, (double)(ry1 - ry0) * (rx1 - rx0) * (1.0 + (lock ? 1.0 : 0.0) + 6.0 + 8.0), "blend_apply");
    set_launch_grid((long)grid.x * grid.y);
    ProfScope ps_(st, PL_BLEND_APPLY);
    hipLaunchKernelGGL(blend_apply_kernel, grid, dim3(256), 0, st, frame, Wi, lf, mm, lock, ry0, rx0, ry1, rx1, parent, ey0, ex0, ew);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace se
