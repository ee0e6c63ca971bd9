// Fills of a painted region (include/sketchedit_fill.h): the two elementwise kernels a fill adds around
// netG.  Everything else a fill runs -- the gathers at either scale, the forward, the pastes -- exists already.
//
//  fill masks: the working-size byte planes fill (B,H,W) and lock (B,H,W) or null, non-zero = set -> the fp32 hole plane
//              hole = fill & ~lock in {0, 1} that netG reads as its mask AND as the composite's soft mask, the same values into
//              `hard` where the caller wants them, and zeros into `zero`, the sketch of a call without one.  One lane = 16
//              consecutive bytes in, four float4 stores per output plane; H and W are multiples of 8, so B H W is a multiple of
//              16 and every float of every output plane is written.
//  fill keep:  per request the hs x ws rectangle at (y0, x0) of a frame-sized KEEP plane: 255 where fill == 0 or lock != 0,
//              else 0 -- the plane the locked and the feathered paste take in place of a lock, which makes `painted and not
//              locked` a condition tested in frame space.  wins holds 4 B records: wins[B + b].frame_u8 is request b's fill
//              plane, wins[2 B + b] its lock plane or null, wins[3 B + b] its keep plane.  One lane = 16 consecutive bytes of a
//              rectangle row, at any alignment of x0, Wi and the planes: the row's bytes are read with aligned dwords that lie
//              inside [row, row + ws) and single bytes at its ends, and written by the same rule, so no byte outside the
//              rectangle is read or written and no lane writes a byte another lane owns.
#include "../../include/sketchedit_hip.h"
#include "se_device.h"
#include "se_kernels.h"

#include <cstdint>

namespace se {

namespace {

// per byte of u: 0xff where it is non-zero, else 0
__device__ __forceinline__ unsigned nonzero_bytes(unsigned u) {
  unsigned r = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) r |= ((u >> (8 * e)) & 255u) ? 255u << (8 * e) : 0u;
  return r;
}

__device__ __forceinline__ float4 bytes_to_01(unsigned u) {
  return make_float4((u & 0xffu) ? 1.f : 0.f, (u & 0xff00u) ? 1.f : 0.f, (u & 0xff0000u) ? 1.f : 0.f, (u & 0xff000000u) ? 1.f : 0.f);
}

// n16 = B H W / 16 lanes.  fill, lock, hole, hard, zero: 16-byte aligned; lock, hard, zero may be null.
__global__ void __launch_bounds__(256) fill_masks_kernel(const unsigned char* __restrict__ fill, const unsigned char* __restrict__ lock,
                                                         float* __restrict__ hole, float* __restrict__ hard, float* __restrict__ zero,
                                                         long n16) {
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= n16) return;
  const uint4 f = *(const uint4*)(fill + 16 * q);
  uint4 l = make_uint4(0u, 0u, 0u, 0u);
  if (lock) l = *(const uint4*)(lock + 16 * q);
  const unsigned h[4] = {nonzero_bytes(f.x) & ~nonzero_bytes(l.x), nonzero_bytes(f.y) & ~nonzero_bytes(l.y),
                         nonzero_bytes(f.z) & ~nonzero_bytes(l.z), nonzero_bytes(f.w) & ~nonzero_bytes(l.w)};
  float4* o = (float4*)(hole + 16 * q);
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = bytes_to_01(h[i]);
  if (hard) {
    float4* o2 = (float4*)(hard + 16 * q);
#pragma unroll
    for (int i = 0; i < 4; ++i) o2[i] = bytes_to_01(h[i]);
  }
  if (zero) {
    float4* z = (float4*)(zero + 16 * q);
#pragma unroll
    for (int i = 0; i < 4; ++i) z[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// the 16 bytes at `a` (any alignment), of which only those inside [lo, hi) are read (the others are 0)
__device__ __forceinline__ uint4 row16_within(const unsigned char* a, const unsigned char* lo, const unsigned char* hi) {
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
__device__ __forceinline__ void row16_store(unsigned char* a, int n, uint4 s) {
  const int mis = (int)((uintptr_t)a & 3);
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

__global__ void __launch_bounds__(256) fill_keep_kernel(const se_window* __restrict__ wins, int B, int hs, int ws) {
  const int chunks = (ws + 15) >> 4;
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= (long)B * hs * chunks) return;
  const int j = (int)(q % chunks);
  const long by = q / chunks;
  const int y = (int)(by % hs), b = (int)(by / hs);
  const se_window w = wins[b];
  const size_t at = (size_t)(w.y0 + y) * w.Wi + w.x0;                 // the rectangle row's bytes of every plane: [at, at + ws)
  const unsigned char* fill = wins[B + b].frame_u8 + at;
  const unsigned char* lock = wins[2 * B + b].frame_u8;
  unsigned char* keep = wins[3 * B + b].frame_u8 + at;
  const uint4 f = row16_within(fill + 16 * j, fill, fill + ws);
  uint4 l = make_uint4(0u, 0u, 0u, 0u);
  if (lock) l = row16_within(lock + at + 16 * j, lock + at, lock + at + ws);
  const uint4 k = make_uint4(~nonzero_bytes(f.x) | nonzero_bytes(l.x), ~nonzero_bytes(f.y) | nonzero_bytes(l.y),
                             ~nonzero_bytes(f.z) | nonzero_bytes(l.z), ~nonzero_bytes(f.w) | nonzero_bytes(l.w));
  row16_store(keep + 16 * j, min(16, ws - 16 * j), k);
}

}  // namespace

hipError_t launch_fill_masks(const unsigned char* fill, const unsigned char* lock, float* hole, float* hard, float* zero, int B, int H,
                             int W, hipStream_t st) {
  const long n16 = (long)B * H * W / 16;
  // bytes: the byte planes read once, every fp32 plane written once
  set_launch_cost(0.0, (double)B * H * W * ((lock ? 2.0 : 1.0) + 4.0 * (1.0 + (hard ? 1.0 : 0.0) + (zero ? 1.0 : 0.0))), "fill_masks");
  set_launch_grid((n16 + 255) / 256);
  ProfScope ps_(st, PL_FILL_MASKS);
  hipLaunchKernelGGL(fill_masks_kernel, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, st, fill, lock, hole, hard, zero, n16);
  return hipGetLastError();
}

hipError_t launch_fill_keep(const se_window* d_wins, int B, int hs, int ws, hipStream_t st) {
  const long nq = (long)B * hs * ((ws + 15) / 16);
  // bytes: the fill and lock rectangles read, the keep rectangle written
  set_launch_cost(0.0, (double)B * hs * ws * 3.0, "fill_keep");
  set_launch_grid((nq + 255) / 256);
  ProfScope ps_(st, PL_FILL_KEEP);
  hipLaunchKernelGGL(fill_keep_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, d_wins, B, hs, ws);
  return hipGetLastError();
}

}  // namespace se
