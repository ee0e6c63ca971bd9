// Modify a selection's shape (the rule is stated in include/sketchedit_modify.h and in plain numpy in
// tests/modify_util.py): expand or contract a selection by a round brush, smooth it by a majority vote in a disc.  Two
// integer-only kernels, plain vector loads and stores, no atomics, nothing polled, any alignment of the planes and of Wi, no byte
// outside a plane read or written.  Both have the house shape -- one workgroup of 256 = one 64 x 16 tile of the frame -- and
// share their two ends:
//
//  staging: the tile with its halo of r, 16 + 2r rows of 64 + 2r columns, becomes one mask of two 64-bit words per staged row
//           (two ballots, as the grow of se_select.hip), kept in LDS.  Bit c of staged row i = pixel (ty0 - r + i, tx0 - r + c) lies
//           inside the frame and is selected (`invert`: is NOT selected).  Out-of-frame bits are 0.  A tile whose staged masks are
//           all 0, or all 1 on every in-frame bit, has a constant answer and skips the middle.
//  storing: the 16 output rows come as one 64-bit mask each, from LDS.  A row's bytes of the tile are walked in the ALIGNED dwords
//           that hold them (17 at most); a dword that lies inside the tile's bytes is one store, the others are single bytes of
//           the tile's own pixels: one writer per byte, whatever the alignment of the plane and of Wi.
//
//  modify_disc (expand; contract = the expansion of the inverted plane, inverted):
//           1. per staged column and output row j, the distance g to the nearest set bit of that column, counted from staged row
//              j + r and capped at r + 1: a thread per column gathers the column's bits from the row masks into two words and
//              reads the distance down and up off them by a count of trailing / leading zeros.  The g of output rows 4q .. 4q + 3
//              are the four bytes of one dword.
//           2. pixel (j, x) is set iff g[j][x + dx] <= lim[|dx|] for some dx in -r .. r, lim[d] = isqrt(r^2 - d^2) (an integer
//              loop): dy^2 + dx^2 <= r^2 holds for some set bit of the column iff it holds for the nearest.  Wave q, lane x takes
//              rows 4q .. 4q + 3 at once: every byte of (0x80 + lim) - g has its top bit set iff g <= lim, and no byte borrows from
//              its neighbour (g <= r + 1 < 0x80).  At most 2r + 1 LDS reads per four pixels.
//  modify_vote (smooth):
//           per staged row the exclusive prefix counts of its mask, uint16, in LDS: (16 + 2r) (64 + 2r + 2) entries, 20.3 KB at
//           r = 32.  c = the sum over dy of the prefix difference across x -+ lim[|dy|]; n = the same sum of the run lengths
//           clipped to the frame, over the rows inside it; out = 2c > n, or 2c == n and the pixel is selected.
#include "../../include/sketchedit_hip.h"
#include "../../include/sketchedit_modify.h"
#include "se_device.h"
#include "se_kernels.h"

#include <cstdint>

namespace se {

namespace {

typedef unsigned long long u64;

constexpr int MD_RMAX = SE_MODIFY_MAX_RADIUS;
constexpr int MD_TW = 64, MD_TH = 16;                 // the tile
constexpr int MD_ROWS = MD_TH + 2 * MD_RMAX;          // staged rows at the largest radius
constexpr int MD_COLS = MD_TW + 2 * MD_RMAX;          // staged columns at the largest radius
constexpr int MD_PSTRIDE = MD_COLS + 2;               // a row of prefix counts: MD_COLS + 1 entries, padded to an even number
constexpr int MD_SLOTS = MD_TW / 4 + 1;               // the aligned dwords that may hold a row's 64 bytes of a tile
static_assert(MD_COLS <= 128, "a staged row is two 64-bit words");
static_assert(MD_ROWS <= 128 && MD_TH - 1 + MD_RMAX < 64, "a staged column is two 64-bit words, the centre rows in the first");
static_assert(MD_RMAX + 1 < 0x80, "the byte-parallel compare of step 2 needs g < 0x80");
static_assert(MD_RMAX + 1 <= 256 && MD_COLS <= 256, "one thread per table entry / staged column");

// s_lim[d] <- isqrt(r^2 - d^2), d = 0 .. r (threads 0 .. r; visible after the next barrier)
__device__ __forceinline__ void make_lim(int r, int* s_lim) {
  const int d = threadIdx.x;
  if (d <= r) {
    const int v = r * r - d * d;
    int s = 0;
    while ((s + 1) * (s + 1) <= v) ++s;
    s_lim[d] = s;
  }
}

// The staging: s_m[i] <- the mask of staged row i, i < 16 + 2r.  Ends with a barrier.  -> 0: some bit is set and some in-frame bit
// is not; 1: no bit is set; 2: every in-frame bit is set (block-uniform)
__device__ __forceinline__ int stage_masks(const unsigned char* __restrict__ plane, int Hi, int Wi, int tx0, int ty0, int r, bool invert,
                                           u64 (*s_m)[2], int* s_flags) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rows = MD_TH + 2 * r;
  bool any = false, full = true;                                      // (wave-uniform)
  for (int i = wave; i < rows; i += 4) {
    const int y = ty0 - r + i;
    u64 lo = 0, hi = 0;
    if (y >= 0 && y < Hi) {                                           // (wave-uniform)
      const unsigned char* row = plane + (size_t)y * Wi;
      const int xa = tx0 - r + lane, xb = xa + 64;                    // staged columns lane and 64 + lane
      const bool in0 = xa >= 0 && xa < Wi, in1 = lane < 2 * r && xb < Wi;      // (xb >= 0: tx0 - r + 64 > 0)
      unsigned v0 = 0, v1 = 0;
      if (in0) v0 = row[xa];
      if (in1) v1 = row[xb];
      lo = __ballot(in0 && ((v0 != 0) != invert));
      hi = __ballot(in1 && ((v1 != 0) != invert));
      any = any || (lo | hi) != 0;
      full = full && lo == __ballot(in0) && hi == __ballot(in1);
    }
    if (lane == 0) { s_m[i][0] = lo; s_m[i][1] = hi; }
  }
  if (lane == 0) s_flags[wave] = (any ? 1 : 0) | (full ? 2 : 0);
  __syncthreads();
  const int f0 = s_flags[0], f1 = s_flags[1], f2 = s_flags[2], f3 = s_flags[3];
  if (!((f0 | f1 | f2 | f3) & 1)) return 1;
  if (f0 & f1 & f2 & f3 & 2) return 2;
  return 0;
}

// The storing: s_out[j] = the mask of output row j (bit x = pixel tx0 + x; bits past the frame's width are ignored) -> the tile's
// bytes of `out`, 0 / 255.  The caller has synchronised after the masks were written.
__device__ __forceinline__ void store_tile(unsigned char* __restrict__ out, int Hi, int Wi, int tx0, int ty0, const u64* s_out) {
  const int tw = min(MD_TW, Wi - tx0);                                // the tile's columns (>= 1)
  for (int item = threadIdx.x; item < MD_TH * MD_SLOTS; item += 256) {
    const int j = item / MD_SLOTS, k = item % MD_SLOTS;
    const int y = ty0 + j;
    if (y >= Hi) continue;
    unsigned char* a = out + (size_t)y * Wi + tx0;                    // the row's first byte of the tile
    const int p0 = 4 * k - (int)((uintptr_t)a & 3);                   // the slot's first pixel, relative to tx0 (may be < 0)
    if (p0 >= tw) continue;
    const u64 m = s_out[j];
    unsigned v = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (p0 + e >= 0 && p0 + e < tw && ((m >> (p0 + e)) & 1ull)) v |= 255u << (8 * e);
    if (p0 >= 0 && p0 + 4 <= tw) {
      *(unsigned*)(a + p0) = v;                                       // 4-byte aligned
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (p0 + e >= 0 && p0 + e < tw) a[p0 + e] = (unsigned char)((v >> (8 * e)) & 255u);
    }
  }
}

// ---- expand / contract -----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) modify_disc_kernel(const unsigned char* __restrict__ plane, unsigned char* __restrict__ out, int Hi,
                                                          int Wi, int ntx, int r, int invert) {
  __shared__ u64 s_m[MD_ROWS][2];
  __shared__ unsigned s_g[MD_TH / 4][MD_COLS];                        // [q][c]: byte b = g of output row 4q + b at staged column c
  __shared__ u64 s_out[MD_TH];
  __shared__ int s_lim[MD_RMAX + 1];
  __shared__ int s_flags[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tx0 = (int)(blockIdx.x % (unsigned)ntx) * MD_TW, ty0 = (int)(blockIdx.x / (unsigned)ntx) * MD_TH;
  make_lim(r, s_lim);
  const int flat = stage_masks(plane, Hi, Wi, tx0, ty0, r, invert != 0, s_m, s_flags);
  if (flat) {                                                         // (block-uniform) nothing set: nothing grows; all set: every pixel is set
    if (tid < MD_TH) s_out[tid] = ((flat == 2) != (invert != 0)) ? ~0ull : 0ull;
    __syncthreads();
    store_tile(out, Hi, Wi, tx0, ty0, s_out);
    return;
  }
  // step 1: a thread per staged column
  const int rows = MD_TH + 2 * r, cols = MD_TW + 2 * r;
  if (tid < cols) {
    const int w = tid >> 6, sh = tid & 63;
    u64 c0 = 0, c1 = 0;                                               // the column: bit i of (c1:c0) = staged row i
    for (int i = 0; i < rows; ++i) {
      const u64 bit = (s_m[i][w] >> sh) & 1ull;
      if (i < 64) c0 |= bit << i; else c1 |= bit << (i - 64);
    }
#pragma unroll
    for (int q = 0; q < MD_TH / 4; ++q) {
      unsigned pack = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int i = 4 * q + b + r;                                  // the centre row: 1 .. 47
        const u64 below = (c0 >> i) | (c1 << (64 - i));               // bit k = staged row i + k
        const u64 above = c0 << (63 - i);                             // bit 63 - k = staged row i - k
        const int dd = below ? __ffsll((long long)below) - 1 : 64, du = above ? __clzll((long long)above) : 64;
        pack |= (unsigned)min(min(dd, du), r + 1) << (8 * b);
      }
      s_g[q][tid] = pack;
    }
  }
  __syncthreads();
  // step 2: wave q, lane x: rows 4q .. 4q + 3 of column x
  unsigned acc = 0;
  for (int dx = -r; dx <= r; ++dx) {
    const unsigned limw = 0x80808080u + 0x01010101u * (unsigned)s_lim[dx < 0 ? -dx : dx];
    acc |= limw - s_g[wave][lane + r + dx];
  }
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const u64 m = __ballot((acc >> (8 * b + 7)) & 1u);
    if (lane == 0) s_out[4 * wave + b] = invert ? ~m : m;
  }
  __syncthreads();
  store_tile(out, Hi, Wi, tx0, ty0, s_out);
}

// ---- smooth ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) modify_vote_kernel(const unsigned char* __restrict__ plane, unsigned char* __restrict__ out, int Hi,
                                                          int Wi, int ntx, int r) {
  __shared__ u64 s_m[MD_ROWS][2];
  __shared__ unsigned short s_p[MD_ROWS][MD_PSTRIDE];                 // [i][c] = the set bits of staged row i below column c, c <= 64 + 2r
  __shared__ u64 s_out[MD_TH];
  __shared__ int s_lim[MD_RMAX + 1];
  __shared__ int s_flags[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tx0 = (int)(blockIdx.x % (unsigned)ntx) * MD_TW, ty0 = (int)(blockIdx.x / (unsigned)ntx) * MD_TH;
  make_lim(r, s_lim);
  const int flat = stage_masks(plane, Hi, Wi, tx0, ty0, r, false, s_m, s_flags);
  if (flat) {                                                         // (block-uniform) c == 0, or c == n, at every pixel
    if (tid < MD_TH) s_out[tid] = flat == 2 ? ~0ull : 0ull;
    __syncthreads();
    store_tile(out, Hi, Wi, tx0, ty0, s_out);
    return;
  }
  const int rows = MD_TH + 2 * r, cols = MD_TW + 2 * r;
  for (int e = tid; e < rows * 129; e += 256) {                       // entries c = 0 .. 128 of every staged row; those past cols are not read
    const int i = e / 129, c = e % 129;
    if (c > cols) continue;
    const u64 lo = s_m[i][0], hi = s_m[i][1];
    const int n = c >= 64 ? __popcll(lo) + (c >= 128 ? __popcll(hi) : __popcll(hi & ((1ull << (c - 64)) - 1ull)))
                          : __popcll(lo & ((1ull << c) - 1ull));
    s_p[i][c] = (unsigned short)n;
  }
  __syncthreads();
  // wave q, lane x: rows 4q .. 4q + 3 of column x
  const int x = tx0 + lane, cc = lane + r;                            // the pixel's column in the frame and in the staged rows
  int c4[4] = {0, 0, 0, 0}, n4[4] = {0, 0, 0, 0};
  for (int d = 0; d <= r; ++d) {
    const int L = s_lim[d];
    const int run = min(x + L, Wi - 1) - max(x - L, 0) + 1;           // the in-frame pixels of the run x - L .. x + L (x < Wi; else unused)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int j = 4 * wave + b, y = ty0 + j, i = j + r;
      c4[b] += (int)s_p[i + d][cc + L + 1] - (int)s_p[i + d][cc - L];
      n4[b] += y + d < Hi ? run : 0;
      if (d) {
        c4[b] += (int)s_p[i - d][cc + L + 1] - (int)s_p[i - d][cc - L];
        n4[b] += y - d >= 0 ? run : 0;
      }
    }
  }
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int i = 4 * wave + b + r;
    const bool self = (s_m[i][cc >> 6] >> (cc & 63)) & 1ull;
    const u64 m = __ballot(2 * c4[b] > n4[b] || (2 * c4[b] == n4[b] && self));
    if (lane == 0) s_out[4 * wave + b] = m;
  }
  __syncthreads();
  store_tile(out, Hi, Wi, tx0, ty0, s_out);
}

}  // namespace

hipError_t launch_plane_modify(const unsigned char* plane, int Hi, int Wi, int op, int radius, unsigned char* out, hipStream_t st) {
  const int ntx = (Wi + MD_TW - 1) / MD_TW, nty = (Hi + MD_TH - 1) / MD_TH;
  // bytes: the plane read with the halo's share, the output written once
  const double halo = (double)(MD_TW + 2 * radius) * (MD_TH + 2 * radius) / (double)(MD_TW * MD_TH);
  const bool vote = op == SE_MODIFY_SMOOTH;
  set_launch_cost(0.0, (double)Hi * Wi * (halo + 1.0), vote ? "modify_vote" : "modify_disc");
  set_launch_grid((long)ntx * nty);
  const dim3 grid((unsigned)((long)ntx * nty));
  if (vote) {
    ProfScope ps_(st, PL_MODIFY_VOTE);
    hipLaunchKernelGGL(modify_vote_kernel, grid, dim3(256), 0, st, plane, out, Hi, Wi, ntx, radius);
  } else {
    ProfScope ps_(st, PL_MODIFY_DISC);
    hipLaunchKernelGGL(modify_disc_kernel, grid, dim3(256), 0, st, plane, out, Hi, Wi, ntx, radius, op == SE_MODIFY_CONTRACT ? 1 : 0);
  }
  return hipGetLastError();
}

}  // namespace se
