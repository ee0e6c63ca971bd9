// Pillow-exact separable resampling of uint8 images (the resize steps of the reference's demo.py:39-73, process_image):
// `Image.resize` of an 'L' or 'RGB' image with BILINEAR, BICUBIC (Pillow's default) or LANCZOS, no box, no reducing gap.
//
// Pillow's uint8 resampler is fixed-point arithmetic, so it is reproduced bit for bit:
//  - per axis the host computes the coefficients in double precision, one IEEE operation at a time (this file is
//    compiled without floating-point contraction, see the pragma below), normalises them by their sum and converts them
//    to int with 22 fractional bits, rounding away from zero (resample_coeffs);
//  - a pass accumulates tap * weight in int32 from 1 << 21 and clips (acc >> 22) to [0, 255];
//  - the horizontal pass runs first and writes a uint8 intermediate, the vertical pass reads it; the pass of an axis whose
//    size does not change is skipped (the caller decides that, se_api.hip resize_locked).
// tests/pil_resample_util.py restates the same in Python and is checked against Pillow itself.
//
// The last pass can write the forward's fp32 NCHW inputs instead of uint8 (ResizeOut::mode): the image through the
// ctx's dequantisation table (the one se_dequantize_u8 uses, bit-identical to (v/255 - 0.5)/0.5) and the sketch as
// (v > 0) in {0, 1}.
//
// A window edit at a working size uses the same passes with two fused ends: window_resample_h_kernel is the
// horizontal pass with its rows taken from the frames' windows (no crop copy), window_paste_v_kernel the vertical pass of the
// way back whose epilogue is the paste rule of se_window.hip (no full-size result is ever written).  A session's lock plane
//  takes the same two ends: window_lock_resample_h_kernel reads its rows from the planes' windows and the last
// pass writes (v > 0) as bytes (RESIZE_OUT_LOCK_U8); window_paste_v_locked_kernel tests the plane in frame space.
//
// The kernels are memory-bound (a few int multiply-adds per byte).  The coefficients of a block's outputs are staged
// in LDS; the vertical pass treats an output row as a flat byte string (every channel of a row shares the row's weights)
// and moves 16 bytes per lane with the widest loads the alignment allows; the horizontal pass stages the input span of
// its rows in LDS with dword loads where its LDS budget allows it, and reads global memory directly otherwise.
#include "../../include/sketchedit_hip.h"
#include "se_device.h"
#include "se_kernels.h"

#include <algorithm>
#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

namespace se {

namespace {

double bilinear_filter(double x) {
  if (x < 0.0) x = -x;
  if (x < 1.0) return 1.0 - x;
  return 0.0;
}
double bicubic_filter(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}
double sinc_filter(double x) {
  if (x == 0.0) return 1.0;
  x = x * M_PI;
  return sin(x) / x;
}
double lanczos_filter(double x) {
  if (-3.0 <= x && x < 3.0) return sinc_filter(x) * sinc_filter(x / 3);
  return 0.0;
}

}  // namespace

int resample_ksize(int in, int out, int filter) {
  double support;
  switch (filter) {
    case SE_RESAMPLE_BILINEAR: support = 1.0; break;
    case SE_RESAMPLE_BICUBIC: support = 2.0; break;
    case SE_RESAMPLE_LANCZOS: support = 3.0; break;
    default: return -1;
  }
  if (in < 1 || out < 1) return -1;
  const double scale = (double)in / out;
  const double fs = scale > 1.0 ? scale : 1.0;
  return (int)ceil(support * fs) * 2 + 1;
}

int resample_coeffs(int in, int out, int filter, int* bounds, int* kk) {
  const int ksize = resample_ksize(in, out, filter);
  if (ksize < 0) return -1;
  double (*f)(double) = filter == SE_RESAMPLE_BILINEAR ? bilinear_filter : filter == SE_RESAMPLE_BICUBIC ? bicubic_filter : lanczos_filter;
  const double fsupport = filter == SE_RESAMPLE_BILINEAR ? 1.0 : filter == SE_RESAMPLE_BICUBIC ? 2.0 : 3.0;
  const double scale = (double)in / out;
  const double filterscale = scale > 1.0 ? scale : 1.0;
  const double support = fsupport * filterscale;
  const double ss = 1.0 / filterscale;
  std::vector<double> w(ksize);
  for (int xx = 0; xx < out; ++xx) {
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
      w[x] = f((x + xmin - center + 0.5) * ss);
      ww += w[x];
    }
    int* k = kk + (size_t)xx * ksize;
    for (int x = 0; x < ksize; ++x) {
      double v = x < xmax ? w[x] : 0.0;
      if (x < xmax && ww != 0.0) v /= ww;
      k[x] = v < 0 ? (int)(-0.5 + v * (1 << 22)) : (int)(0.5 + v * (1 << 22));
    }
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = xmax;
  }
  return ksize;
}

namespace {

constexpr int kLdsBudget = 48 * 1024;   // per workgroup: well inside the default dynamic-LDS limit, several blocks per CU
constexpr int kRoundOne = 1 << 21;

__device__ __forceinline__ unsigned char clip8(int acc) {
  const int v = acc >> 22;
  return (unsigned char)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// four clipped bytes in one dword.  Packed through v_perm_b32: written as shifts and ORs, the clip-and-pack of two
// neighbours is selected into v_ashr_pk_u8_i32, which writes only the low 16 bits of its register, and the stale upper half
// then ends up in bytes 2 and 3 (hipcc 6.x / gfx950)
__device__ __forceinline__ unsigned pack4(int a0, int a1, int a2, int a3) {
  const unsigned lo = __builtin_amdgcn_perm((unsigned)clip8(a1), (unsigned)clip8(a0), 0x0c0c0400u);   // bytes: a0, a1, 0, 0
  const unsigned hi = __builtin_amdgcn_perm((unsigned)clip8(a3), (unsigned)clip8(a2), 0x04000c0cu);   // bytes: 0, 0, a2, a3
  return lo | hi;
}

// the epilogue of the last pass: byte value v of channel c of pixel (b, y, x)
__device__ __forceinline__ void store_px(const ResizeOut& o, int b, int y, int x, int c, int C, unsigned char v) {
  if (o.mode == RESIZE_OUT_U8)
    o.u8[(((size_t)b * o.H + y) * o.W + x) * C + c] = v;
  else if (o.mode == RESIZE_OUT_IMAGE_F32)
    o.f32[(((size_t)b * C + c) * o.H + y) * o.W + x] = o.lut[v];
  else if (o.mode == RESIZE_OUT_LOCK_U8)
    o.u8[((size_t)b * o.H + y) * o.W + x] = v ? 1 : 0;
  else
    o.f32[(((size_t)b * C + c) * o.H + y) * o.W + x] = v ? 1.f : 0.f;
}

// Where the horizontal pass finds its input rows.  Contiguous: the (B, Hrows, Win, C) array.  Window: row r of
// request b is a row of that request's WINDOW -- C == 3: the frame's bytes from 3 ((y0 + r) Wi + x0), any alignment, pitch
// 3 Wi; C == 1: the window's own contiguous (hs, ws) sketch.  The pass touches a row's bytes [first tap, last tap] only
// (columns of the window), so nothing outside the window is read.
struct ContiguousRows {
  const unsigned char* in;
  size_t plane, pitch;
  __device__ __forceinline__ const unsigned char* row(int b, int y) const { return in + b * plane + (size_t)y * pitch; }
};
template <int C>
struct WindowRows {
  const se_window* wins;
  int ws;
  __device__ __forceinline__ const unsigned char* row(int b, int y) const {
    const se_window w = wins[b];
    if (C == 3) return w.frame_u8 + ((size_t)(w.y0 + y) * w.Wi + w.x0) * 3;
    return w.sketch_u8 + (size_t)y * ws;
  }
};

// Lock plane (C == 1): wins holds 2 B records, wins[B + b].frame_u8 = request b's (Hi, Wi) plane; row r of the
// window starts at byte (y0 + r) Wi + x0, any alignment, pitch Wi.
struct LockRows {
  const se_window* wins;
  int B;
  __device__ __forceinline__ const unsigned char* row(int b, int y) const {
    const se_window w = wins[b];
    return wins[B + b].frame_u8 + (size_t)(w.y0 + y) * w.Wi + w.x0;
  }
};

// Horizontal pass: Hrows rows of Win pixels per request -> (B, Hrows, Wout, C).  A block = TX output columns x TY rows, one
// output pixel per thread.  LDS: [TX * ksize] weights, [TX] (first tap, tap count), then (staged) TY rows of `span` input bytes.
template <int C, class Rows>
__device__ __forceinline__ void resample_h_body(const Rows in, const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                                                int Hrows, int Wout, int TX, int TY, int span, const ResizeOut& o) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int* coef = (int*)smem;
  int2* bnd = (int2*)(smem + ((TX * ksize * 4 + 15) & ~15));
  unsigned char* rows = (unsigned char*)bnd + ((TX * 8 + 15) & ~15);
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int x0 = blockIdx.x * TX, nx = min(TX, Wout - x0);
  const int y0 = blockIdx.y * TY, b = blockIdx.z;
  for (int i = tid; i < nx * ksize; i += nthr) coef[i] = kk[(size_t)x0 * ksize + i];
  for (int i = tid; i < nx; i += nthr) bnd[i] = make_int2(bounds[2 * (x0 + i)], bounds[2 * (x0 + i) + 1]);
  // the block's input columns [p0, p1): first tap of its first output to the last tap of its last (both monotone in x)
  const int p0 = bounds[2 * x0], p1 = bounds[2 * (x0 + nx - 1)] + bounds[2 * (x0 + nx - 1) + 1];
  if (span) {
    // row r's bytes [p0 C, p1 C) land at rows[r * span + lead + j], lead = the address's offset within its dword (per row:
    // rows of a window differ), so that the dwords wholly inside the range are copied with dword loads and LDS writes; the
    // partial ones byte by byte
    const int nb = (p1 - p0) * C;
    for (int r = 0; r < TY && y0 + r < Hrows; ++r) {
      const unsigned char* g = in.row(b, y0 + r) + (size_t)p0 * C;
      const int lead = (int)((uintptr_t)g & 3);
      unsigned char* l = rows + r * span;
      const int head = lead ? min(4 - lead, nb) : 0;      // bytes before the first whole dword
      const int nw = (nb - head) >> 2;                     // whole dwords
      const unsigned* gw = (const unsigned*)(g + head);
      unsigned* lw = (unsigned*)(l + lead + head);
      for (int i = tid; i < nw; i += nthr) lw[i] = gw[i];
      const int tail0 = head + 4 * nw;
      for (int i = tid; i < head + (nb - tail0); i += nthr) {
        const int j = i < head ? i : tail0 + (i - head);
        l[lead + j] = g[j];
      }
    }
  }
  __syncthreads();
  const int tx = tid % TX, ty = tid / TX;
  const int xx = x0 + tx, y = y0 + ty;
  if (tx >= nx || y >= Hrows) return;
  const int2 bd = bnd[tx];
  const unsigned char* src;
  if (span) {
    const unsigned char* g = in.row(b, y) + (size_t)p0 * C;
    src = rows + ty * span + (int)((uintptr_t)g & 3) + (bd.x - p0) * C;
  } else {
    src = in.row(b, y) + (size_t)bd.x * C;
  }
  const int* k = coef + tx * ksize;
  int acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = kRoundOne;
  for (int t = 0; t < bd.y; ++t) {
    const int w = k[t];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] += (int)src[t * C + c] * w;
  }
#pragma unroll
  for (int c = 0; c < C; ++c) store_px(o, b, y, xx, c, C, clip8(acc[c]));
}

template <int C>
__global__ void __launch_bounds__(256) resample_h_kernel(const unsigned char* __restrict__ in, const int* __restrict__ bounds,
                                                         const int* __restrict__ kk, int ksize, int Hrows, int Win, int Wout,
                                                         int TX, int TY, int span, ResizeOut o) {
  resample_h_body<C>(ContiguousRows{in, (size_t)Hrows * Win * C, (size_t)Win * C}, bounds, kk, ksize, Hrows, Wout, TX, TY, span, o);
}

// The gather end of a scaled window edit: the same pass with its rows taken straight from the frames (C == 3) or from the
// requests' window sketches (C == 1) -- no contiguous crop is ever made.
template <int C>
__global__ void __launch_bounds__(256) window_resample_h_kernel(const se_window* __restrict__ wins, const int* __restrict__ bounds,
                                                                const int* __restrict__ kk, int ksize, int hs, int ws, int Wout,
                                                                int TX, int TY, int span, ResizeOut o) {
  resample_h_body<C>(WindowRows<C>{wins, ws}, bounds, kk, ksize, hs, Wout, TX, TY, span, o);
}

// The gather end for the lock planes: the same pass over LockRows.  A request without a plane (null) gets zeros.
__global__ void __launch_bounds__(256) window_lock_resample_h_kernel(const se_window* __restrict__ wins, int B,
                                                                     const int* __restrict__ bounds, const int* __restrict__ kk,
                                                                     int ksize, int hs, int Wout, int TX, int TY, int span, ResizeOut o) {
  if (!wins[B + blockIdx.z].frame_u8) {          // block-uniform
    const int xx = blockIdx.x * TX + threadIdx.x % TX, y = blockIdx.y * TY + threadIdx.x / TX;
    if (xx < Wout && y < hs) store_px(o, blockIdx.z, y, xx, 0, 1, 0);
    return;
  }
  resample_h_body<1>(LockRows{wins, B}, bounds, kk, ksize, hs, Wout, TX, TY, span, o);
}

// Vertical pass: in (B, Hin, RB bytes) -> (B, Hout, RB), RB = W * C; every byte of an output row takes the row's weights.
// One block = 256 lanes x 16 bytes of one output row; V = bytes per load (16, 4 or 1: what the alignment of `in`, RB and,
// for uint8 output, `o.u8` allows).
template <int V>
__global__ void __launch_bounds__(256) resample_v_kernel(const unsigned char* __restrict__ in, const int* __restrict__ bounds,
                                                         const int* __restrict__ kk, int ksize, int Hin, int RB, int C,
                                                         ResizeOut o) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int* coef = (int*)smem;
  const int yy = blockIdx.y, b = blockIdx.z;
  const int ymin = bounds[2 * yy], n = bounds[2 * yy + 1];
  for (int i = threadIdx.x; i < n; i += blockDim.x) coef[i] = kk[(size_t)yy * ksize + i];
  __syncthreads();
  const int j0 = (blockIdx.x * blockDim.x + threadIdx.x) * 16;
  if (j0 >= RB) return;
  const unsigned char* src = in + ((size_t)b * Hin + ymin) * RB + j0;
  int acc[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = kRoundOne;
  const int ne = min(16, RB - j0);             // < 16 only in the last lanes of a row (V == 1: RB need not be a multiple)
  for (int t = 0; t < n; ++t) {
    const int w = coef[t];
    const unsigned char* s = src + (size_t)t * RB;
    if (V == 16) {
      const uint4 q = *(const uint4*)s;
      const unsigned d[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] += (int)((d[e >> 2] >> (8 * (e & 3))) & 255u) * w;
    } else if (V == 4) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (4 * i < ne) {
          const unsigned d = *(const unsigned*)(s + 4 * i);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[4 * i + e] += (int)((d >> (8 * e)) & 255u) * w;
        }
      }
    } else {
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (e < ne) acc[e] += (int)s[e] * w;
    }
  }
  if (o.mode == RESIZE_OUT_U8) {
    unsigned char* d = o.u8 + ((size_t)b * o.H + yy) * RB + j0;
    if (V == 16) {
      *(uint4*)d = make_uint4(pack4(acc[0], acc[1], acc[2], acc[3]), pack4(acc[4], acc[5], acc[6], acc[7]),
                              pack4(acc[8], acc[9], acc[10], acc[11]), pack4(acc[12], acc[13], acc[14], acc[15]));
    } else if (V == 4) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (4 * i < ne) *(unsigned*)(d + 4 * i) = pack4(acc[4 * i], acc[4 * i + 1], acc[4 * i + 2], acc[4 * i + 3]);
    } else {
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (e < ne) d[e] = clip8(acc[e]);
    }
    return;
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    if (e < ne) {
      const int j = j0 + e, x = j / C;
      store_px(o, b, yy, x, j - x * C, C, clip8(acc[e]));
    }
  }
}

// The paste end of a scaled window edit: the vertical pass of the resize back to the frame-space window, whose epilogue is
// the paste rule of se_window.hip.  rgb (B, Hin, P, 3) and m8 (B, Hin, P): the working-size result after the horizontal pass,
// P = the row pitch in pixels, a multiple of 4 >= ws (columns >= ws are never used).  One lane = 4 consecutive pixels of row
// yy of the hs x ws window: the mask's column first -- four pixels that all resample to 0 are left without reading a colour
// byte -- then the twelve colour bytes.  frame[y0 + yy, x0 + x, :] is written only where the resampled mask byte is > 0:
// whole dwords where all four pixels are selected and the address allows it, single bytes otherwise, so a lane never
// rewrites a byte it does not own (concurrent lanes and disjoint windows of other requests on the frame do not race).
// LOCKED: wins holds 2 B records, wins[B + b].frame_u8 = request b's lock plane or null; a pixel whose byte of
// the plane, at its FRAME position, is non-zero leaves the selection -- after the mask's early exit, before the colour reads.
template <bool LOCKED>
__device__ __forceinline__ void window_paste_v(const se_window* __restrict__ wins, int B, const unsigned char* __restrict__ rgb,
                                               const unsigned char* __restrict__ m8, const int* __restrict__ bounds,
                                               const int* __restrict__ kk, int ksize, int Hin, int P, int ws) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int* coef = (int*)smem;
  const int yy = blockIdx.y, b = blockIdx.z;
  const int ymin = bounds[2 * yy], n = bounds[2 * yy + 1];
  for (int i = threadIdx.x; i < n; i += blockDim.x) coef[i] = kk[(size_t)yy * ksize + i];
  __syncthreads();
  const int x = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (x >= ws) return;
  const size_t first = ((size_t)b * Hin + ymin) * P + x;      // the lane's first tap, in pixels
  int am[4] = {kRoundOne, kRoundOne, kRoundOne, kRoundOne};
  for (int t = 0; t < n; ++t) {
    const unsigned d = *(const unsigned*)(m8 + first + (size_t)t * P);
    const int w = coef[t];
#pragma unroll
    for (int e = 0; e < 4; ++e) am[e] += (int)((d >> (8 * e)) & 255u) * w;
  }
  bool sel[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) sel[p] = x + p < ws && clip8(am[p]) > 0;
  if (!(sel[0] || sel[1] || sel[2] || sel[3])) return;
  if (LOCKED) {
    const unsigned char* plane = wins[B + b].frame_u8;
    if (plane) {
      const se_window w = wins[b];
      const unsigned char* row = plane + (size_t)(w.y0 + yy) * w.Wi + w.x0;      // the window row's lock bytes: [row, row + ws)
      const unsigned lk = load4_within(row + x, row, row + ws);
#pragma unroll
      for (int p = 0; p < 4; ++p) sel[p] = sel[p] && !((lk >> (8 * p)) & 255u);
      if (!(sel[0] || sel[1] || sel[2] || sel[3])) return;
    }
  }
  int acc[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) acc[e] = kRoundOne;
  const unsigned char* src = rgb + first * 3;
  for (int t = 0; t < n; ++t) {
    const unsigned* s = (const unsigned*)(src + (size_t)t * P * 3);
    const unsigned d[3] = {s[0], s[1], s[2]};
    const int w = coef[t];
#pragma unroll
    for (int e = 0; e < 12; ++e) acc[e] += (int)((d[e >> 2] >> (8 * (e & 3))) & 255u) * w;
  }
  const se_window w = wins[b];
  unsigned char* dst = w.frame_u8 + ((size_t)(w.y0 + yy) * w.Wi + w.x0 + x) * 3;
  if (sel[0] && sel[1] && sel[2] && sel[3] && ((uintptr_t)dst & 3) == 0) {
    unsigned* d = (unsigned*)dst;
    d[0] = pack4(acc[0], acc[1], acc[2], acc[3]);
    d[1] = pack4(acc[4], acc[5], acc[6], acc[7]);
    d[2] = pack4(acc[8], acc[9], acc[10], acc[11]);
    return;
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    if (sel[p]) {
#pragma unroll
      for (int c = 0; c < 3; ++c) dst[3 * p + c] = clip8(acc[3 * p + c]);
    }
  }
}

__global__ void __launch_bounds__(64) window_paste_v_kernel(const se_window* __restrict__ wins, const unsigned char* __restrict__ rgb,
                                                            const unsigned char* __restrict__ m8, const int* __restrict__ bounds,
                                                            const int* __restrict__ kk, int ksize, int Hin, int P, int ws) {
  window_paste_v<false>(wins, 0, rgb, m8, bounds, kk, ksize, Hin, P, ws);
}

__global__ void __launch_bounds__(64) window_paste_v_locked_kernel(const se_window* __restrict__ wins, int B,
                                                                   const unsigned char* __restrict__ rgb,
                                                                   const unsigned char* __restrict__ m8, const int* __restrict__ bounds,
                                                                   const int* __restrict__ kk, int ksize, int Hin, int P, int ws) {
  window_paste_v<true>(wins, B, rgb, m8, bounds, kk, ksize, Hin, P, ws);
}

bool aligned(const void* p, int a) { return ((uintptr_t)p & (uintptr_t)(a - 1)) == 0; }

}  // namespace

namespace {

// the block shape of a horizontal pass: TX outputs x TY rows, `span` staged bytes per row (0: rows read from global memory)
struct HShape {
  int TX, TY, span;
  size_t lds;
  dim3 grid;
};

bool resample_h_shape(const int* h_bounds, int ksize, int B, int Hrows, int Wout, int C, HShape* s) {
  int TX = 64;
  while (TX > 1 && TX / 2 >= Wout) TX /= 2;
  auto coef_lds = [ksize](int tx) { return ((tx * ksize * 4 + 15) & ~15) + ((tx * 8 + 15) & ~15); };
  while (TX > 1 && coef_lds(TX) > kLdsBudget) TX /= 2;       // long filters (large downscales): fewer outputs per block
  const int TY = 256 / TX, coef_bytes = coef_lds(TX);
  // widest input span of a block of TX outputs (+3 bytes of dword lead), rounded to 16 bytes
  int span_max = 0;
  for (int x0 = 0; x0 < Wout; x0 += TX) {
    const int xl = std::min(x0 + TX, Wout) - 1;
    span_max = std::max(span_max, (h_bounds[2 * xl] + h_bounds[2 * xl + 1] - h_bounds[2 * x0]) * C);
  }
  int span = (span_max + 3 + 15) & ~15;
  if (coef_bytes + TY * span > kLdsBudget) span = 0;       // rows read from global memory directly
  if (coef_bytes > kLdsBudget) return false;                 // (the caller refuses such tap counts first)
  s->TX = TX; s->TY = TY; s->span = span;
  s->lds = coef_bytes + (size_t)TY * span;
  s->grid = dim3((unsigned)((Wout + TX - 1) / TX), (unsigned)((Hrows + TY - 1) / TY), (unsigned)B);
  return true;
}

}  // namespace

hipError_t launch_resample_h(const unsigned char* in, const int* d_bounds, const int* d_kk, const int* h_bounds, int ksize,
                             int B, int Hrows, int Win, int Wout, int C, const ResizeOut& o, hipStream_t st) {
  HShape s;
  if (!resample_h_shape(h_bounds, ksize, B, Hrows, Wout, C, &s)) return hipErrorInvalidValue;
  // bytes: every input byte read once, every output element written once (fp32 outputs: 4 bytes)
  set_launch_cost(0.0, (double)B * Hrows * C * (Win + (o.mode == RESIZE_OUT_U8 ? 1.0 : 4.0) * Wout), "resize_h");
  set_launch_grid((long)s.grid.x * s.grid.y * s.grid.z);
  ProfScope ps_(st, PL_RESIZE_H);
  if (C == 3)
    hipLaunchKernelGGL(resample_h_kernel<3>, s.grid, dim3(s.TX * s.TY), s.lds, st, in, d_bounds, d_kk, ksize, Hrows, Win, Wout, s.TX, s.TY, s.span, o);
  else
    hipLaunchKernelGGL(resample_h_kernel<1>, s.grid, dim3(s.TX * s.TY), s.lds, st, in, d_bounds, d_kk, ksize, Hrows, Win, Wout, s.TX, s.TY, s.span, o);
  return hipGetLastError();
}

hipError_t launch_window_resample_h(const se_window* d_wins, const int* d_bounds, const int* d_kk, const int* h_bounds, int ksize,
                                    int B, int hs, int ws, int Wout, int C, const ResizeOut& o, hipStream_t st) {
  HShape s;
  if (!resample_h_shape(h_bounds, ksize, B, hs, Wout, C, &s)) return hipErrorInvalidValue;
  set_launch_cost(0.0, (double)B * hs * C * (ws + (o.mode == RESIZE_OUT_U8 ? 1.0 : 4.0) * Wout), "window_resample_h");
  set_launch_grid((long)s.grid.x * s.grid.y * s.grid.z);
  ProfScope ps_(st, PL_WINDOW_RESAMPLE_H);
  if (C == 3)
    hipLaunchKernelGGL(window_resample_h_kernel<3>, s.grid, dim3(s.TX * s.TY), s.lds, st, d_wins, d_bounds, d_kk, ksize, hs, ws, Wout, s.TX, s.TY, s.span, o);
  else
    hipLaunchKernelGGL(window_resample_h_kernel<1>, s.grid, dim3(s.TX * s.TY), s.lds, st, d_wins, d_bounds, d_kk, ksize, hs, ws, Wout, s.TX, s.TY, s.span, o);
  return hipGetLastError();
}

hipError_t launch_window_lock_resample_h(const se_window* d_wins, const int* d_bounds, const int* d_kk, const int* h_bounds, int ksize,
                                         int B, int hs, int ws, int Wout, const ResizeOut& o, hipStream_t st) {
  HShape s;
  if (!resample_h_shape(h_bounds, ksize, B, hs, Wout, 1, &s)) return hipErrorInvalidValue;
  set_launch_cost(0.0, (double)B * hs * (ws + Wout), "window_lock_gather");
  set_launch_grid((long)s.grid.x * s.grid.y * s.grid.z);
  ProfScope ps_(st, PL_WINDOW_LOCK_GATHER);
  hipLaunchKernelGGL(window_lock_resample_h_kernel, s.grid, dim3(s.TX * s.TY), s.lds, st, d_wins, B, d_bounds, d_kk, ksize, hs, Wout, s.TX, s.TY, s.span, o);
  return hipGetLastError();
}

hipError_t launch_window_paste_v(const se_window* d_wins, const unsigned char* rgb, const unsigned char* m8, const int* d_bounds,
                                 const int* d_kk, int ksize, int B, int Hin, int hs, int P, int ws, hipStream_t st, bool locked) {
  if (((ksize * 4 + 15) & ~15) > kLdsBudget || (P & 3) || P < ws || !aligned(rgb, 4) || !aligned(m8, 4)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((ws + 4 * 64 - 1) / (4 * 64)), (unsigned)hs, (unsigned)B);
  // bytes: an upper bound (every pixel selected): the taps of mask and colour read, the frame's window written
  set_launch_cost(0.0, (double)B * ws * 4.0 * Hin + (double)B * hs * ws * (locked ? 4.0 : 3.0), locked ? "window_paste_v_locked" : "window_paste_v");
  set_launch_grid((long)grid.x * grid.y * grid.z);
  ProfScope ps_(st, locked ? PL_WINDOW_PASTE_V_LOCKED : PL_WINDOW_PASTE_V);
  const size_t lds = (size_t)((ksize * 4 + 15) & ~15);
  if (locked) hipLaunchKernelGGL(window_paste_v_locked_kernel, grid, dim3(64), lds, st, d_wins, B, rgb, m8, d_bounds, d_kk, ksize, Hin, P, ws);
  else hipLaunchKernelGGL(window_paste_v_kernel, grid, dim3(64), lds, st, d_wins, rgb, m8, d_bounds, d_kk, ksize, Hin, P, ws);
  return hipGetLastError();
}

hipError_t launch_resample_v(const unsigned char* in, const int* d_bounds, const int* d_kk, int ksize, int B, int Hin, int Hout,
                             int W, int C, const ResizeOut& o, hipStream_t st) {
  if (((ksize * 4 + 15) & ~15) > kLdsBudget) return hipErrorInvalidValue;
  const int RB = W * C;
  const bool out_ok16 = o.mode != RESIZE_OUT_U8 || aligned(o.u8, 16), out_ok4 = o.mode != RESIZE_OUT_U8 || aligned(o.u8, 4);
  const int V = (RB % 16 == 0 && aligned(in, 16) && out_ok16) ? 16 : (RB % 4 == 0 && aligned(in, 4) && out_ok4) ? 4 : 1;
  const dim3 grid((unsigned)((RB + 16 * 256 - 1) / (16 * 256)), (unsigned)Hout, (unsigned)B);
  const size_t lds = (ksize * 4 + 15) & ~15;
  set_launch_cost(0.0, (double)B * RB * (Hin + (o.mode == RESIZE_OUT_U8 ? 1.0 : 4.0) * Hout), "resize_v");
  set_launch_grid((long)grid.x * grid.y * grid.z);
  ProfScope ps_(st, PL_RESIZE_V);
  if (V == 16)
    hipLaunchKernelGGL(resample_v_kernel<16>, grid, dim3(256), lds, st, in, d_bounds, d_kk, ksize, Hin, RB, C, o);
  else if (V == 4)
    hipLaunchKernelGGL(resample_v_kernel<4>, grid, dim3(256), lds, st, in, d_bounds, d_kk, ksize, Hin, RB, C, o);
  else
    hipLaunchKernelGGL(resample_v_kernel<1>, grid, dim3(256), lds, st, in, d_bounds, d_kk, ksize, Hin, RB, C, o);
  return hipGetLastError();
}

}  // namespace se

extern "C" int se_resample_coeffs(int in, int out, int filter, int* bounds, int* k, size_t cap) {
  const int ksize = se::resample_ksize(in, out, filter);
  if (ksize < 0) return -1;
  if (!bounds || !k || cap < (size_t)out * ksize) return ksize;
  return se::resample_coeffs(in, out, filter, bounds, k);
}
