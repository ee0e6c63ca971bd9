// Window edits of a resident frame: the three memory-bound helpers around the forward when it runs on an
// H x W window of a larger uint8 frame that stays on the device.  B requests per launch, each with its own frame; a request
// is one se_window record (include/sketchedit_hip.h) of a device table the ctx owns (se_api_window.hip win_put).
//
//  gather: the window of each frame -> that request's slot of the forward's fp32 NCHW inputs, through the ctx's
//          dequantisation table (bit-identical to se_dequantize_u8 on a contiguous crop), and the window's sketch as (v > 0);
//  border: from the forward's uint8 mask, the pixels >= 128 on each one-pixel edge of the window (4 counts per request; an
//          edge that is the frame's own edge counts 0) -- "did the edit reach the window's border";
//  paste:  frame[y0 + y, x0 + x, :] = rgb[b, y, x, :] where mask_u8[b, y, x] > 0; every other byte of the frame is untouched.
//
// A window row starts at byte 3 (y Wi + x0) of the frame: any alignment.  gather reads it with aligned dword loads and a
// byte shift; a dword that would reach outside the row's own bytes (the first and the last of a row) is assembled from byte
// loads of the row's bytes only, so nothing outside the window is ever read.  paste writes whole dwords only where four
// neighbouring pixels are all selected and the address allows it, single bytes otherwise: it never rewrites a byte it does
// not own, so concurrent lanes (and windows of other requests on the same frame, which the host requires to be disjoint)
// do not race.
//
// The undo journal of a session adds two copies between a window and a journal slot -- hs rows of
// pitch = round_up(3 ws, 16) bytes, 16-byte aligned, so the slot side moves as aligned 16-byte vectors:
//
//  save: the window's hs x ws rectangle of each frame -> that request's slot (the bytes before a paste);
//  swap: the rectangle <-> the slot (undo, and redo: the same exchange again).
//
// One lane owns one 16-byte chunk of a slot row and the (up to) 16 frame bytes that belong in it.  It reads them as gather
// does and, in swap, writes them back by the ownership rule above: aligned dwords that lie inside its own bytes, single bytes
// in front of and behind them.  No lane writes a byte another lane owns, and none outside the rectangle.
//
// Locked regions: a frame may own a (Hi, Wi) uint8 LOCK PLANE, non-zero = locked.  Its pointers travel
// like the journal's slots: wins holds 2 B records and wins[B + b].frame_u8 is request b's plane, or null.
//
//  lock gather:  the window of each plane -> that request's slot of a contiguous (B,H,W) plane of {0, 1} (null: zeros), which
//                the mask predictor's last kernel takes; a row starts at byte (y0 + r) Wi + x0 and is read as gather reads;
//  locked paste: paste, with `and lock[y0 + y, x0 + x] == 0` added to the rule -- the four lock bytes of a lane's pixels are
//                read the same way and those pixels leave the selection before it decides between dwords and bytes.
//
// Region edits: one more helper, in front of the forwards, that finds where a full-size sketch is drawn.
//
//  sketch tiles: the (Hi, Wi) sketch plane cut into tile x tile squares (the last row / column of squares ragged) -> one record
//                [count, y0, x0, y1, x1] per square: the pixels > 0 in it and their tight half-open box in frame coordinates,
//                five zeros for an empty square.  The plane's base and pitch have any alignment: a row's part of a square is
//                read as gather reads a window row, so no byte outside the plane is read.
//
// Strokes as polylines: the windows' sketches need not come from a full-size plane at all.
//
//  sketch strokes: (N,5) int32 segments [ax, ay, bx, by, r] in quarter pixels of the frame -> the (hs, ws) sketch of each
//                  request's window, 255 where a segment of the request's range covers the pixel's centre and 0 elsewhere, by
//                  the integer rule of 6i.  wins holds 2 B records: wins[B + b].Hi / .Wi are request b's first segment and
//                  its segment count.  Every byte of the output is written, by the paste's ownership rule; none outside it.
#include "../../include/sketchedit_hip.h"
#include "se_device.h"
#include "se_kernels.h"

#include <cstdint>

namespace se {

namespace {

// the 16 bytes at `a` (any alignment), of which only those inside [lo, hi) are read (the others are 0): aligned dwords and a
// byte shift
__device__ __forceinline__ uint4 load16_within(const unsigned char* a, const unsigned char* lo, const unsigned char* hi) {
  const unsigned char* a0 = (const unsigned char*)((uintptr_t)a & ~(uintptr_t)3);
  const int sh = (int)((uintptr_t)a & 3) * 8;
  unsigned d[5], u[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) d[i] = load_dword_within(a0 + 4 * i, lo, hi);
  d[4] = sh ? load_dword_within(a0 + 16, lo, hi) : 0u;
#pragma unroll
  for (int i = 0; i < 4; ++i) u[i] = sh ? (d[i] >> sh) | (d[i + 1] << (32 - sh)) : d[i];
  return make_uint4(u[0], u[1], u[2], u[3]);
}

// the first n (1..16) bytes of s -> [a, a + n), any alignment, and not one byte more: the aligned dwords that lie inside the
// span whole, single bytes at its head and tail
__device__ __forceinline__ void store_owned(unsigned char* a, int n, uint4 s) {
  const int mis = (int)((uintptr_t)a & 3);
  if (n == 16 && ((uintptr_t)a & 15) == 0) {
    *(uint4*)a = s;
    return;
  }
  unsigned char* a0 = a - mis;
  const unsigned v[5] = {s.x, s.y, s.z, s.w, 0u};
  const int sl = mis * 8;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    // the dword at a0 + 4 k holds the bytes 4 k - mis .. 4 k - mis + 3 of s
    const unsigned f = sl ? (v[k] << sl) | (k > 0 ? v[k - 1] >> (32 - sl) : 0u) : v[k];
    const int off = 4 * k - mis;
    if (off >= 0 && off + 4 <= n) {
      *(unsigned*)(a0 + 4 * k) = f;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (off + e >= 0 && off + e < n) a0[4 * k + e] = (unsigned char)((f >> (8 * e)) & 255u);
    }
  }
}

// One lane = one 16-byte chunk of one slot row.  wins holds 2 B records: wins[B + b].frame_u8 is request b's slot.
template <bool SWAP>
__device__ __forceinline__ void window_journal(const se_window* __restrict__ wins, int B, int hs, int ws) {
  const int pitch = (3 * ws + 15) & ~15, chunks = pitch >> 4;
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= (long)B * hs * chunks) return;
  const int j = (int)(q % chunks);
  const long by = q / chunks;
  const int y = (int)(by % hs), b = (int)(by / hs);
  const se_window w = wins[b];
  unsigned char* row = w.frame_u8 + ((size_t)(w.y0 + y) * w.Wi + w.x0) * 3;       // the window row's bytes: [row, row + 3 ws)
  unsigned char* a = row + 16 * j;
  uint4* s = (uint4*)(wins[B + b].frame_u8 + (size_t)y * pitch) + j;
  const uint4 f = load16_within(a, row, row + 3 * ws);
  if (SWAP) {
    const uint4 old = *s;
    store_owned(a, min(16, 3 * ws - 16 * j), old);
  }
  *s = f;
}

__global__ void __launch_bounds__(256) window_save_kernel(const se_window* __restrict__ wins, int B, int hs, int ws) {
  window_journal<false>(wins, B, hs, ws);
}

__global__ void __launch_bounds__(256) window_swap_kernel(const se_window* __restrict__ wins, int B, int hs, int ws) {
  window_journal<true>(wins, B, hs, ws);
}

// One lane = 4 consecutive pixels of one window row: 12 frame bytes + 4 sketch bytes in, four float4 stores out.
__global__ void __launch_bounds__(256) window_gather_kernel(const se_window* __restrict__ wins, const float* __restrict__ lut,
                                                            float* __restrict__ image, float* __restrict__ sketch, int B, int H,
                                                            int W) {
  __shared__ float T[256];
  T[threadIdx.x] = lut[threadIdx.x];
  __syncthreads();
  const int W4 = W >> 2;
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= (long)B * H * W4) return;
  const int x = (int)(q % W4) * 4;
  const long by = q / W4;
  const int y = (int)(by % H), b = (int)(by / H);
  const se_window w = wins[b];
  const size_t HW = (size_t)H * W, in = (size_t)y * W + x;
  if (image) {
    const unsigned char* row = w.frame_u8 + ((size_t)(w.y0 + y) * w.Wi + w.x0) * 3;       // the window row's bytes: [row, row + 3 W)
    const unsigned char* a = row + 3 * x;
    const unsigned char* a0 = (const unsigned char*)((uintptr_t)a & ~(uintptr_t)3);
    const int sh = (int)((uintptr_t)a & 3) * 8;
    unsigned d[4];
#pragma unroll
    for (int i = 0; i < 3; ++i) d[i] = load_dword_within(a0 + 4 * i, row, row + 3 * W);
    d[3] = sh ? load_dword_within(a0 + 12, row, row + 3 * W) : 0u;
    unsigned char v[12];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const unsigned u = sh ? (d[i] >> sh) | (d[i + 1] << (32 - sh)) : d[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[4 * i + e] = (u >> (8 * e)) & 255u;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
      *(float4*)(image + ((size_t)b * 3 + c) * HW + in) = make_float4(T[v[c]], T[v[3 + c]], T[v[6 + c]], T[v[9 + c]]);
  }
  if (sketch) {
    const unsigned char* s = w.sketch_u8 + in;
    unsigned u;
    if (((uintptr_t)w.sketch_u8 & 3) == 0) u = *(const unsigned*)s;       // (W % 4 == 0: every group of a 4-aligned sketch is)
    else u = (unsigned)s[0] | ((unsigned)s[1] << 8) | ((unsigned)s[2] << 16) | ((unsigned)s[3] << 24);
    *(float4*)(sketch + (size_t)b * HW + in) =
        make_float4((u & 0xffu) ? 1.f : 0.f, (u & 0xff00u) ? 1.f : 0.f, (u & 0xff0000u) ? 1.f : 0.f, (u & 0xff000000u) ? 1.f : 0.f);
  }
}

// One wave per (side, request): the lanes walk the edge 64 pixels at a time, a shuffle reduction adds their counts and lane 0
// stores the total (a plain vector store: every count is written on every call, nothing to zero beforehand).
// side 0 top, 1 bottom, 2 left, 3 right.  The mask is H x W; the window it stands for covers hs x ws frame pixels (the same
// unless the edit ran at a working size), and that extent decides which sides lie on the frame's own edge.
__global__ void __launch_bounds__(64) window_border_kernel(const se_window* __restrict__ wins, const unsigned char* __restrict__ m8,
                                                           int* __restrict__ hits, int H, int W, int hs, int ws) {
  const int side = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const se_window w = wins[b];
  const bool on_frame_edge = side == 0 ? w.y0 == 0 : side == 1 ? w.y0 + hs == w.Hi : side == 2 ? w.x0 == 0 : w.x0 + ws == w.Wi;
  int n = 0;
  if (!on_frame_edge) {
    const unsigned char* m = m8 + (size_t)b * H * W;
    const int len = side < 2 ? W : H;
    const size_t first = side == 1 ? (size_t)(H - 1) * W : side == 3 ? (size_t)(W - 1) : 0;
    const size_t step = side < 2 ? 1 : (size_t)W;
    for (int i = lane; i < len; i += 64) n += m[first + i * step] >= 128 ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o, 64);
  if (lane == 0) hits[b * 4 + side] = n;
}

// One lane = 16 consecutive bytes of one window row of a lock plane (W % 8 == 0: the last lane of a row may hold 8), written
// as two 8-byte stores (out is 8-byte aligned and so is every chunk).  wins holds 2 B records (see above).
__global__ void __launch_bounds__(256) window_lock_gather_kernel(const se_window* __restrict__ wins, unsigned char* __restrict__ out,
                                                                 int B, int H, int W) {
  const int chunks = (W + 15) >> 4;
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= (long)B * H * chunks) return;
  const int j = (int)(q % chunks);
  const long by = q / chunks;
  const int y = (int)(by % H), b = (int)(by / H);
  const se_window w = wins[b];
  const unsigned char* plane = wins[B + b].frame_u8;
  uint4 f = make_uint4(0u, 0u, 0u, 0u);
  if (plane) {
    const unsigned char* row = plane + (size_t)(w.y0 + y) * w.Wi + w.x0;       // the window row's bytes: [row, row + W)
    f = load16_within(row + 16 * j, row, row + W);
  }
  unsigned d[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    unsigned u = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) u |= ((d[i] >> (8 * e)) & 255u) ? 1u << (8 * e) : 0u;
    d[i] = u;
  }
  uint2* o = (uint2*)(out + ((size_t)b * H + y) * W + 16 * j);
  o[0] = make_uint2(d[0], d[1]);
  if (16 * j + 8 < W) o[1] = make_uint2(d[2], d[3]);
}

// One lane = 4 consecutive pixels of one window row.  LOCKED: wins holds 2 B records (see above).
template <bool LOCKED>
__device__ __forceinline__ void window_paste(const se_window* __restrict__ wins, const unsigned char* __restrict__ rgb,
                                             const unsigned char* __restrict__ m8, int B, int H, int W) {
  const int W4 = W >> 2;
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= (long)B * H * W4) return;
  const int x = (int)(q % W4) * 4;
  const long by = q / W4;
  const int y = (int)(by % H), b = (int)(by / H);
  const size_t pix = ((size_t)b * H + y) * W + x;
  unsigned mk = *(const unsigned*)(m8 + pix);
  if (!mk) return;
  const se_window w = wins[b];
  if (LOCKED) {
    const unsigned char* plane = wins[B + b].frame_u8;
    if (plane) {
      const unsigned char* row = plane + (size_t)(w.y0 + y) * w.Wi + w.x0;     // the window row's lock bytes: [row, row + W)
      mk = clear_locked(mk, load4_within(row + x, row, row + W));
      if (!mk) return;
    }
  }
  unsigned char* dst = w.frame_u8 + ((size_t)(w.y0 + y) * w.Wi + w.x0 + x) * 3;
  const unsigned* src = (const unsigned*)(rgb + pix * 3);
  const unsigned s0 = src[0], s1 = src[1], s2 = src[2];
  const bool all4 = (mk & 0xffu) && (mk & 0xff00u) && (mk & 0xff0000u) && (mk & 0xff000000u);
  if (all4 && ((uintptr_t)dst & 3) == 0) {
    unsigned* d = (unsigned*)dst;
    d[0] = s0; d[1] = s1; d[2] = s2;
    return;
  }
  const unsigned s[3] = {s0, s1, s2};
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    if ((mk >> (8 * p)) & 255u) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int j = 3 * p + c;
        dst[j] = (unsigned char)((s[j >> 2] >> (8 * (j & 3))) & 255u);
      }
    }
  }
}

__global__ void __launch_bounds__(256) window_paste_kernel(const se_window* __restrict__ wins, const unsigned char* __restrict__ rgb,
                                                           const unsigned char* __restrict__ m8, int B, int H, int W) {
  window_paste<false>(wins, rgb, m8, B, H, W);
}

__global__ void __launch_bounds__(256) window_paste_locked_kernel(const se_window* __restrict__ wins, const unsigned char* __restrict__ rgb,
                                                                  const unsigned char* __restrict__ m8, int B, int H, int W) {
  window_paste<true>(wins, rgb, m8, B, H, W);
}

// One wave per tile x tile square (TILE 16 / 32 / 64), four squares per workgroup.  A lane owns 4 consecutive bytes of a row of
// the square, TILE / 4 lanes a row, and the wave walks the square 256 bytes at a time; the bytes come from load4_within bounded
// by the square's own part of the row, so a byte past the row's end (or the plane's) is never read and counts as 0.  Five
// shuffle reductions (a sum, two minima, two maxima) and lane 0 stores the record with plain vector stores: every record is
// written on every call, the empty ones as zeros, and the same plane gives the same bits.
template <int TILE>
__global__ void __launch_bounds__(256) sketch_tiles_kernel(const unsigned char* __restrict__ plane, int Hi, int Wi, int ntx, long ntiles,
                                                           int* __restrict__ out) {
  constexpr int C = TILE / 4, R = 64 / C;       // lanes per row, rows per step
  const int lane = threadIdx.x & 63;
  const long t = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= ntiles) return;                      // (wave-uniform; the kernel has no barrier)
  const int ty = (int)(t / ntx), tx = (int)(t % ntx);
  const int xt = tx * TILE, xe = min(xt + TILE, Wi);
  const int x = xt + 4 * (lane % C);
  int n = 0, y0 = 0x7fffffff, x0 = 0x7fffffff, y1 = -1, x1 = -1;
  if (x < xe) {
#pragma unroll 4
    for (int r = lane / C; r < TILE; r += R) {
      const int y = ty * TILE + r;
      if (y >= Hi) break;
      const unsigned char* row = plane + (size_t)y * Wi;
      const unsigned u = load4_within(row + x, row + xt, row + xe);
      if (!u) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if ((u >> (8 * e)) & 255u) {
          ++n;
          x0 = min(x0, x + e);
          x1 = max(x1, x + e);
        }
      }
      y0 = min(y0, y);
      y1 = max(y1, y);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    n += __shfl_down(n, o, 64);
    y0 = min(y0, __shfl_down(y0, o, 64));
    x0 = min(x0, __shfl_down(x0, o, 64));
    y1 = max(y1, __shfl_down(y1, o, 64));
    x1 = max(x1, __shfl_down(x1, o, 64));
  }
  if (lane == 0) {
    int* rec = out + t * 5;
    rec[0] = n;
    rec[1] = n ? y0 : 0;
    rec[2] = n ? x0 : 0;
    rec[3] = n ? y1 + 1 : 0;
    rec[4] = n ? x1 + 1 : 0;
  }
}

// One workgroup = one 64 x 16 pixel tile of one request's window; one lane = 4 consecutive pixels of one row.  The request's
// segments are walked in chunks of 256, one per lane: a lane keeps its segment if the segment's box grown by r meets the box
// of the tile's pixel centres, the kept ones are compacted into LDS (a ballot and a prefix count per wave, the waves' totals
// through LDS) together with what the test needs of them, and every lane tests its pixels against those only.  A range of
// any length is so many chunks; an empty one writes zeros.
// What is loaded is clamped to the limits the rule is stated for (coordinates to [0, 4 * 8192], r to [0, 512]) -- a no-op on
// valid segments -- so that every intermediate fits int64 whatever the buffer holds: |e|, |d| <= 2^15 + 62 per axis (a lane's
// pixels may lie up to 3 columns / 15 rows past the window), hence |t|, |cr| < 2^31.01, cr^2 < 2^62.02, r^2 dd <= 2^49.
// The store is window_paste's: a dword where all four bytes are the lane's and the address is aligned, single bytes otherwise.
__global__ void __launch_bounds__(256) sketch_strokes_kernel(const se_window* __restrict__ wins, int B, int hs, int ws,
                                                             const int* __restrict__ segs, unsigned char* __restrict__ out) {
  constexpr int CHUNK = 256, LIM = 4 * 8192, RMAX = 512;
  __shared__ int s_ax[CHUNK], s_ay[CHUNK], s_dx[CHUNK], s_dy[CHUNK], s_r2[CHUNK];
  __shared__ long long s_dd[CHUNK], s_r2dd[CHUNK];
  __shared__ int s_wave_n[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.z;
  const se_window w = wins[b];
  const int first = wins[B + b].Hi, count = wins[B + b].Wi;
  const int tx0 = blockIdx.x * 64, ty0 = blockIdx.y * 16;                       // the tile, in window pixels
  const int tx1 = min(tx0 + 64, ws), ty1 = min(ty0 + 16, hs);
  // the box of the tile's pixel centres, in quarter pixels of the frame
  const int cx0 = 4 * (w.x0 + tx0) + 2, cx1 = 4 * (w.x0 + tx1 - 1) + 2, cy0 = 4 * (w.y0 + ty0) + 2, cy1 = 4 * (w.y0 + ty1 - 1) + 2;
  const int x = tx0 + 4 * (tid & 15), y = ty0 + (tid >> 4);
  const int n = y < hs ? max(0, min(4, ws - x)) : 0;                           // the lane's pixels inside the window
  const long long px = 4 * (w.x0 + x) + 2, py = 4 * (w.y0 + y) + 2;
  unsigned cov = 0;                                                             // bit p: pixel x + p is covered
  for (int base = 0; base < count; base += CHUNK) {                            // (block-uniform: every lane meets the barriers)
    bool keep = false;
    int ax = 0, ay = 0, bx = 0, by = 0, r = 0;
    if (base + tid < count) {
      const int* s = segs + 5 * ((size_t)first + base + tid);
      ax = min(max(s[0], 0), LIM); ay = min(max(s[1], 0), LIM);
      bx = min(max(s[2], 0), LIM); by = min(max(s[3], 0), LIM);
      r = min(max(s[4], 0), RMAX);
      keep = min(ax, bx) - r <= cx1 && max(ax, bx) + r >= cx0 && min(ay, by) - r <= cy1 && max(ay, by) + r >= cy0;
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
    if (keep) {
      const int dx = bx - ax, dy = by - ay;
      const long long dd = (long long)dx * dx + (long long)dy * dy;
      s_ax[at] = ax; s_ay[at] = ay; s_dx[at] = dx; s_dy[at] = dy; s_r2[at] = r * r;
      s_dd[at] = dd; s_r2dd[at] = (long long)(r * r) * dd;
    }
    __syncthreads();
    if (n > 0) {
      for (int i = 0; i < kept && cov != 15u; ++i) {
        const long long dx = s_dx[i], dy = s_dy[i], r2 = s_r2[i], dd = s_dd[i], r2dd = s_r2dd[i];
        const long long ex0 = px - s_ax[i], ey = py - s_ay[i], fy = ey - dy;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const long long ex = ex0 + 4 * p, fx = ex - dx;
          const long long t = ex * dx + ey * dy, cr = ex * dy - ey * dx;
          const bool c = t <= 0 ? ex * ex + ey * ey <= r2 : t >= dd ? fx * fx + fy * fy <= r2 : cr * cr <= r2dd;
          cov |= c ? 1u << p : 0u;
        }
      }
    }
  }
  if (n > 0) {
    unsigned char* a = out + ((size_t)b * hs + y) * ws + x;
    const unsigned v = ((cov & 1u) ? 0xffu : 0u) | ((cov & 2u) ? 0xff00u : 0u) | ((cov & 4u) ? 0xff0000u : 0u) | ((cov & 8u) ? 0xff000000u : 0u);
    if (n == 4 && ((uintptr_t)a & 3) == 0) {
      *(unsigned*)a = v;
    } else {
      for (int e = 0; e < n; ++e) a[e] = (unsigned char)((v >> (8 * e)) & 255u);
    }
  }
}

}  // namespace

hipError_t launch_sketch_strokes(const se_window* d_wins, int B, int hs, int ws, const int* segs, long nseg_sum, unsigned char* sketch_out,
                                 hipStream_t st) {
  const dim3 grid((unsigned)((ws + 63) / 64), (unsigned)((hs + 15) / 16), (unsigned)B);
  // bytes: every tile reads its request's segments (an upper bound: the L2 serves most of it), the sketches written once
  set_launch_cost(0.0, (double)B * hs * ws + 20.0 * (double)nseg_sum * grid.x * grid.y, "sketch_strokes");
  set_launch_grid((long)grid.x * grid.y * grid.z);
  ProfScope ps_(st, PL_SKETCH_STROKES);
  hipLaunchKernelGGL(sketch_strokes_kernel, grid, dim3(256), 0, st, d_wins, B, hs, ws, segs, sketch_out);
  return hipGetLastError();
}

hipError_t launch_sketch_tiles(const unsigned char* plane, int Hi, int Wi, int tile, int* tiles_out, hipStream_t st) {
  const int ntx = (Wi + tile - 1) / tile;
  const long ntiles = (long)((Hi + tile - 1) / tile) * ntx;
  const dim3 grid((unsigned)((ntiles + 3) / 4));
  // bytes: the plane read once, the records written once
  set_launch_cost(0.0, (double)Hi * Wi + 20.0 * ntiles, "sketch_tiles");
  set_launch_grid((ntiles + 3) / 4);
  ProfScope ps_(st, PL_SKETCH_TILES);
  if (tile == 16) hipLaunchKernelGGL(sketch_tiles_kernel<16>, grid, dim3(256), 0, st, plane, Hi, Wi, ntx, ntiles, tiles_out);
  else if (tile == 32) hipLaunchKernelGGL(sketch_tiles_kernel<32>, grid, dim3(256), 0, st, plane, Hi, Wi, ntx, ntiles, tiles_out);
  else hipLaunchKernelGGL(sketch_tiles_kernel<64>, grid, dim3(256), 0, st, plane, Hi, Wi, ntx, ntiles, tiles_out);
  return hipGetLastError();
}

hipError_t launch_window_gather(const se_window* d_wins, const float* lut, float* image, float* sketch, int B, int H, int W,
                                hipStream_t st) {
  const long nq = (long)B * H * W / 4;
  // bytes: the window's uint8 image and sketch read once, the fp32 planes written once
  set_launch_cost(0.0, (double)B * H * W * ((image ? 3.0 + 12.0 : 0.0) + (sketch ? 1.0 + 4.0 : 0.0)), "window_gather");
  set_launch_grid((nq + 255) / 256);
  ProfScope ps_(st, PL_WINDOW_GATHER);
  hipLaunchKernelGGL(window_gather_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, d_wins, lut, image, sketch, B, H, W);
  return hipGetLastError();
}

hipError_t launch_window_border(const se_window* d_wins, const unsigned char* m8, int* hits, int B, int H, int W, int hs, int ws,
                                hipStream_t st) {
  set_launch_cost(0.0, (double)B * (2.0 * W + 2.0 * H + 16.0), "window_border");
  set_launch_grid(4L * B);
  ProfScope ps_(st, PL_WINDOW_BORDER);
  hipLaunchKernelGGL(window_border_kernel, dim3(4, (unsigned)B), dim3(64), 0, st, d_wins, m8, hits, H, W, hs, ws);
  return hipGetLastError();
}

hipError_t launch_window_paste(const se_window* d_wins, const unsigned char* rgb, const unsigned char* m8, int B, int H, int W,
                               hipStream_t st, bool locked) {
  const long nq = (long)B * H * W / 4;
  // bytes: an upper bound (every pixel selected): mask (and lock) and rgb read, the frame's window written
  set_launch_cost(0.0, (double)B * H * W * (locked ? 8.0 : 7.0), locked ? "window_paste_locked" : "window_paste");
  set_launch_grid((nq + 255) / 256);
  ProfScope ps_(st, locked ? PL_WINDOW_PASTE_LOCKED : PL_WINDOW_PASTE);
  if (locked) hipLaunchKernelGGL(window_paste_locked_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, d_wins, rgb, m8, B, H, W);
  else hipLaunchKernelGGL(window_paste_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, d_wins, rgb, m8, B, H, W);
  return hipGetLastError();
}

hipError_t launch_window_lock_gather(const se_window* d_wins, unsigned char* out, int B, int H, int W, hipStream_t st) {
  const long nq = (long)B * H * ((W + 15) / 16);
  set_launch_cost(0.0, (double)B * H * W * 2.0, "window_lock_gather");
  set_launch_grid((nq + 255) / 256);
  ProfScope ps_(st, PL_WINDOW_LOCK_GATHER);
  hipLaunchKernelGGL(window_lock_gather_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, d_wins, out, B, H, W);
  return hipGetLastError();
}

hipError_t launch_window_journal(const se_window* d_wins, int B, int hs, int ws, bool swap, hipStream_t st) {
  const long nq = (long)B * hs * ((3 * ws + 15) / 16);
  // bytes: save reads the rectangle and writes the slot's rows; swap reads and writes both
  set_launch_cost(0.0, (double)B * hs * (3.0 * ws + (double)((3 * ws + 15) & ~15)) * (swap ? 2.0 : 1.0), swap ? "window_swap" : "window_save");
  set_launch_grid((nq + 255) / 256);
  ProfScope ps_(st, swap ? PL_WINDOW_SWAP : PL_WINDOW_SAVE);
  if (swap) hipLaunchKernelGGL(window_swap_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, d_wins, B, hs, ws);
  else hipLaunchKernelGGL(window_save_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, d_wins, B, hs, ws);
  return hipGetLastError();
}

}  // namespace se
