// The canvas of an editing session: crop, extend, quarter turns and mirrors (the rule is stated in
// include/sketchedit_canvas.h and in plain numpy in tests/canvas_util.py).  Two integer-only kernels, plain vector loads and
// stores, no atomics, nothing polled, any alignment of in, out, Wi and Wn, no byte outside the two arrays read or written, every
// output byte written exactly once.
//
//  CanvasMap:    the rule as a gather: px(y, x) = the C bytes of output pixel (y, x), packed into a dword -- the fold, the pad
//                colour, the orientation.  Both kernels take their slow route through it.
//  canvas_map:   the orientations WITHOUT the transpose.  plane_shift's walk (se_move.hip; store_plane_dword): one lane per
//                aligned dword of the output's C Hn Wn flat bytes.  A dword whose bytes share an output row and whose pixels
//                all lie inside the oriented image reads its source bytes through load4_within bounded by the source row --
//                ascending as they are, or under the x mirror the four bytes swapped (C = 1) or the two pixels the dword
//                touches exchanged with their bytes in order (C = 3: the mirror reverses pixels, not bytes).  A dword across
//                a row's end, on the fold or in the pad area goes byte by byte through px.
//  canvas_turn:  the orientations WITH the transpose: output rows run along source columns, so a gather would read C bytes per
//                C Wi-byte stride.  One workgroup owns a tile of TURN_H = 64 output rows x TURN_W = 32 output columns, i.e. 32
//                source rows of 64 pixels.
//                 stage: lane t owns the tile's pixel (xl, yl) = (t >> 6, t & 63): a wave reads 64 consecutive pixels of ONE
//                        source row (ascending or, mirrored, descending: the same 64 C bytes), each lane its pixel's C bytes
//                        through load4_within bounded by the source row, and stores them as ONE dword at s_px[xl][yl].
//                 write: a half wave owns an output row of the tile, lane k the k-th aligned dword that holds bytes of the
//                        row's tw C-byte segment (at most (3 + 96 + 3) / 4 = 25): it reads the dword of each pixel it holds
//                        bytes of, s_px[xl][yl] with yl fixed, and stores an aligned dword -- or, where the dword is shared
//                        with the neighbouring tile or the row's end, the bytes of its own segment only: one writer per byte.
//                LDS banks: the pitch is TURN_PITCH = 65 dwords, 1 mod 32; the bank of s_px[xl][yl] is (xl + yl) mod 32.
//                ds_write_b32 and ds_read_b32 bank by 32 and conflict within a 32-lane half only.  The stage's half wave has xl
//                fixed and 32 consecutive yl: 32 banks.  The write's half wave has yl fixed and xl in [0, 32): lanes on distinct
//                xl are on distinct banks, lanes on the same xl read the same address (a broadcast).  Neither step conflicts.
//                A tile whose rectangle does not lie inside the oriented image -- in the pad area or on the fold -- or whose
//                input is NULL skips the stage and takes every pixel through px: a per-pixel gather, in the same write step.
#include "../../include/sketchedit_canvas.h"
#include "../../include/sketchedit_hip.h"
#include "se_device.h"
#include "se_kernels.h"

#include <cstdint>

namespace se {

namespace {

constexpr int TURN_W = 32, TURN_H = 64;               // output columns and rows of canvas_turn's tile
constexpr int TURN_PITCH = 65;                        // dwords: 1 mod 32, s_px[xl][yl] lies on bank (xl + yl) mod 32

struct CanvasMap {
  const unsigned char* in;                            // (Hi,Wi,C), or NULL: all zeros (C = 1)
  int Hi, Wi, C, Ho, Wo, oy, ox, orient, pad;
  unsigned rgb;                                       // the pad colour, its C bytes

  DEVFN int fold(int i, int n) const {
    if ((unsigned)i < (unsigned)n) return i;
    if (pad == SE_CANVAS_EDGE) return i < 0 ? 0 : n - 1;
    if (n == 1) return 0;
    const int p = 2 * n - 2;
    int j = i % p;
    if (j < 0) j += p;
    return j < n ? j : p - j;
  }
  // the pixel (Y, X) of the oriented image, 0 <= Y < Ho, 0 <= X < Wo: C bytes in the low end of a dword
  DEVFN unsigned src(int Y, int X) const {
    if (!in) return 0u;
    const int a = (orient & SE_CANVAS_TRANSPOSE) ? X : Y, b = (orient & SE_CANVAS_TRANSPOSE) ? Y : X;
    const int sy = (orient & SE_CANVAS_MIRROR_Y) ? Hi - 1 - a : a, sx = (orient & SE_CANVAS_MIRROR_X) ? Wi - 1 - b : b;
    const unsigned char* row = in + (size_t)sy * Wi * C;
    if (C == 1) return row[sx];
    return load4_within(row + 3 * sx, row, row + 3 * (size_t)Wi) & 0xffffffu;
  }
  // the output pixel (y, x)
  DEVFN unsigned px(int y, int x) const {
    const int Y = y + oy, X = x + ox;
    if (pad == SE_CANVAS_CONSTANT && ((unsigned)Y >= (unsigned)Ho || (unsigned)X >= (unsigned)Wo)) return rgb;
    return src(fold(Y, Ho), fold(X, Wo));
  }
};

// n = C Hn Wn bytes; lane q owns the aligned dword at (out - mis) + 4 q, mis = out & 3: the bytes 4 q - mis .. + 3
__global__ void __launch_bounds__(256) canvas_map_kernel(CanvasMap cm, unsigned char* __restrict__ out, int Wn, long n, long ndw) {
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= ndw) return;
  const int mis = (int)((uintptr_t)out & 3), C = cm.C;
  const long p0 = 4 * q - mis;                                       // the dword's first byte (may lie outside [0, n))
  const long first = p0 < 0 ? 0 : p0, last = p0 + 3 < n ? p0 + 3 : n - 1;      // the lane's bytes of the output
  const int rb = C * Wn;                                             // bytes of an output row
  const int y = (int)(first / rb), b = (int)(first - (long)y * rb), k = (int)(last - first);
  const int sh = 8 * (int)(first - p0);
  unsigned v = 0;
  const int xa = b / C, xb = (b + k) / C, Y = y + cm.oy;            // the lane's pixels xa .. xb, if they share the row y
  if (cm.in && b + k < rb && (unsigned)Y < (unsigned)cm.Ho && xa + cm.ox >= 0 && xb + cm.ox < cm.Wo) {
    // one row, every pixel inside the oriented image: the source bytes are neighbours in ONE source row (bytes past `last` are
    // never stored)
    const int sy = (cm.orient & SE_CANVAS_MIRROR_Y) ? cm.Hi - 1 - Y : Y;
    const unsigned char* row = cm.in + (size_t)sy * cm.Wi * C;
    const unsigned char* hi = row + (size_t)cm.Wi * C;
    if (!(cm.orient & SE_CANVAS_MIRROR_X)) {
      v = load4_within(row + (ptrdiff_t)(xa + cm.ox) * C + (b - xa * C), row, hi) << sh;
    } else if (C == 1) {
      const int sx = cm.Wi - 1 - (xa + cm.ox);                        // xa's source; xa + j comes from sx - j
      v = __builtin_bswap32(load4_within(row + (sx - 3), row, hi)) << sh;
    } else {
      // four bytes of 3-byte pixels touch xa and xa + 1, whose sources are sx and sx - 1: six neighbouring bytes
      const int sx = cm.Wi - 1 - (xa + cm.ox);
      const unsigned char* a = row + 3 * (ptrdiff_t)(sx - 1);
      const unsigned long long w = (unsigned long long)load4_within(a, row, hi) | ((unsigned long long)load4_within(a + 4, row, hi) << 32);
      for (int j = 0; j <= k; ++j) {
        const int x = (b + j) / 3, c = (b + j) - 3 * x;
        v |= (unsigned)((w >> (8 * ((x == xa ? 3 : 0) + c))) & 255u) << (sh + 8 * j);
      }
    }
  } else {
    for (long p = first; p <= last; ++p) {
      const int py = (int)(p / rb), pb = (int)(p - (long)py * rb), x = pb / C, c = pb - x * C;
      v |= ((cm.px(py, x) >> (8 * c)) & 255u) << (8 * (int)(p - p0));
    }
  }
  store_plane_dword(out, p0, n, v);
}

__global__ void __launch_bounds__(256) canvas_turn_kernel(CanvasMap cm, unsigned char* __restrict__ out, int Hn, int Wn) {
  __shared__ unsigned s_px[TURN_W * TURN_PITCH];
  const int tid = threadIdx.x, C = cm.C;
  const int x0 = blockIdx.x * TURN_W, y0 = blockIdx.y * TURN_H;       // the tile, in output pixels
  const int tw = min(TURN_W, Wn - x0), th = min(TURN_H, Hn - y0);
  // the same for every lane of the workgroup: the tile's rectangle is a plain rectangle of the oriented image
  const bool interior = cm.in && y0 + cm.oy >= 0 && y0 + th + cm.oy <= cm.Ho && x0 + cm.ox >= 0 && x0 + tw + cm.ox <= cm.Wo;
  if (interior) {
    // ---- stage: s_px[xl][yl] = the output pixel (y0 + yl, x0 + xl); a wave walks one source row
    for (int t = tid; t < TURN_W * TURN_H; t += 256) {
      const int xl = t >> 6, yl = t & 63;
      if (xl < tw && yl < th) s_px[xl * TURN_PITCH + yl] = cm.src(y0 + yl + cm.oy, x0 + xl + cm.ox);
    }
    __syncthreads();
  }
  // ---- write: a half wave per output row of the tile, a lane per aligned dword of the row's segment
  const int len = tw * C;                                             // bytes of the tile's segment of an output row
  for (int t = tid; t < TURN_H * 32; t += 256) {
    const int yl = t >> 5, k = t & 31;
    if (yl >= th) break;
    const size_t s0 = ((size_t)(y0 + yl) * Wn + x0) * C;              // the segment's first byte in the output
    const int m = (int)(((uintptr_t)out + s0) & 3);
    if (4 * k >= m + len) continue;
    unsigned v = 0, pv = 0;
    int pxl = -1;                                                     // the pixel pv holds
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int s = 4 * k + e - m;                                    // the byte of the segment
      if (s < 0 || s >= len) continue;
      const int xl = s / C, c = s - xl * C;
      if (xl != pxl) {
        pv = interior ? s_px[xl * TURN_PITCH + yl] : cm.px(y0 + yl, x0 + xl);
        pxl = xl;
      }
      v |= ((pv >> (8 * c)) & 255u) << (8 * e);
    }
    unsigned char* dst = out + s0 - m + 4 * k;                        // 4-byte aligned
    if (4 * k >= m && 4 * k + 4 <= m + len) {
      *(unsigned*)dst = v;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (4 * k + e >= m && 4 * k + e < m + len) dst[e] = (unsigned char)((v >> (8 * e)) & 255u);
    }
  }
}

}  // namespace

hipError_t launch_canvas(const unsigned char* in, int Hi, int Wi, int C, unsigned char* out, int Hn, int Wn, int oy, int ox, int orient,
                         int pad, unsigned rgb, hipStream_t st) {
  const bool turn = (orient & SE_CANVAS_TRANSPOSE) != 0;
  const CanvasMap cm{in, Hi, Wi, C, turn ? Wi : Hi, turn ? Hi : Wi, oy, ox, orient, pad, rgb & (C == 1 ? 0xffu : 0xffffffu)};
  const long n = (long)C * Hn * Wn;
  // bytes: the output written once, and read at most as many
  if (turn) {
    const dim3 grid((unsigned)((Wn + TURN_W - 1) / TURN_W), (unsigned)((Hn + TURN_H - 1) / TURN_H));
    set_launch_cost(0.0, 2.0 * (double)n, "canvas_turn");
    set_launch_grid((long)grid.x * grid.y);
    ProfScope ps_(st, PL_CANVAS_TURN);
    hipLaunchKernelGGL(canvas_turn_kernel, grid, dim3(256), 0, st, cm, out, Hn, Wn);
    return hipGetLastError();
  }
  const long ndw = (n + (long)((uintptr_t)out & 3) + 3) / 4;         // the aligned dwords that hold the output's bytes
  set_launch_cost(0.0, 2.0 * (double)n, "canvas_map");
  set_launch_grid((ndw + 255) / 256);
  ProfScope ps_(st, PL_CANVAS_MAP);
  hipLaunchKernelGGL(canvas_map_kernel, dim3((unsigned)((ndw + 255) / 256)), dim3(256), 0, st, cm, out, Wn, n, ndw);
  return hipGetLastError();
}

}  // namespace se
