// Selection by colour (the rule is stated in include/sketchedit_select.h and in plain numpy in
// tests/select_util.py): the "magic wand" of an editing session, made where the frame is.  All work is carried on a STATE plane,
// (Hi,Wi) uint8: 0 not similar, 1 similar and not (yet) reached, 255 reached.  Three integer-only kernels, plain vector loads
// and stores, any alignment of the planes and of Wi, no byte outside a plane (or the frame) read or written:
//
//  similar: state = 255 at the seed; elsewhere 1 (contiguous) or 255 (not) where max_c |F[y, x, c] - F[sy, sx, c]| <= t, else 0.
//           The seed's colour is read by every lane (one address: a broadcast).  The plane is walked as Hi Wi flat bytes in the
//           ALIGNED dwords that hold them: a lane owns one such dword, four consecutive pixels, reads their 12 frame bytes
//           through aligned dwords bounded by the frame's own bytes and stores the dword -- single bytes at the plane's two
//           ends, where the dword is not the plane's alone.
//  flood:   ONE pass.  One wave = one 64 x 64 tile (ragged at the right and bottom edges).  Lanes along x, one ballot per row,
//           give lane y the row masks S_y (state != 0) and R_y (state == 255) of its tile, and the one-pixel halo: the rows
//           above and below as masks of reached bits, one bit per row for the columns left and right.  The wave closes the tile
//           in registers until no lane changes -- horizontally the exact run fill A = R & S, R |= A | (((S + A) ^ S) & S) (the
//           carry of the sum runs up every run of S that holds a reached bit) and the same on the bit-reversed words for the
//           way down, vertically R_y |= S_y & (R_{y-1} | R_{y+1}) by wave shuffles -- and stores 255 to exactly the newly
//           reached bytes of its own tile; a wave that stored anything stores 1 to the pass's `changed` word.  A tile with no
//           reached bit in it or its halo does nothing.
//           ORDER: a pass may read halo bytes a neighbour stores in the same launch.  Bytes only ever go 1 -> 255, so either
//           value is a state the closure is monotone in: the fixed point is unique, and the caller's loop ends only after a
//           launch in which nobody stored, whose every read therefore saw the final state.  Nothing is handed off inside a
//           launch: no flag is polled, nothing spins, the launch boundary is the only synchronisation.
//  grow:    state -> another plane: 255 where a reached byte lies within Chebyshev distance r inside the frame, else 0; every
//           byte is written.  One workgroup = one 64 x 16 tile with its r-pixel halo: each of the 16 + 2r staged rows becomes a
//           mask of 64 + 2r bits (two ballots), its OR over 2r + 1 columns is formed on the mask by shifts (a window of p = the
//           largest power of two <= 2r + 1 by doubling, then OR'd with itself 2r + 1 - p further) and kept in LDS as one 64-bit
//           word; after the barrier each output row is the OR of 2r + 1 of those words and lane x stores byte x.
#include "../../include/sketchedit_hip.h"
#include "se_device.h"
#include "se_kernels.h"

#include <cstdint>

namespace se {

namespace {

typedef unsigned long long u64;

constexpr int SL_RMAX = 16;                           // SE_SELECT_MAX_GROW
constexpr int SL_GW = 64, SL_GH = 16;                 // the grow's tile
constexpr int SL_GROWS = SL_GH + 2 * SL_RMAX;         // staged rows at the largest radius

// ---- similar ------------------------------------------------------------------------------------------------------------
// n = Hi Wi pixels; lane q owns the aligned dword at (state - mis) + 4 q, mis = state & 3: the pixels 4 q - mis .. + 3
__global__ void __launch_bounds__(256) select_similar_kernel(const unsigned char* __restrict__ frame, unsigned char* __restrict__ state,
                                                             long n, long seed, int tol, int contiguous, long ndw) {
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= ndw) return;
  const int mis = (int)((uintptr_t)state & 3);
  const long p0 = 4 * q - mis;                                       // the dword's first pixel (may lie outside [0, n))
  const unsigned char* fend = frame + 3 * (size_t)n;
  const int s0 = frame[3 * seed], s1 = frame[3 * seed + 1], s2 = frame[3 * seed + 2];
  // the 12 frame bytes of the four pixels, read inside [frame, fend) only
  const unsigned char* a = frame + 3 * p0;
  const unsigned char* a0 = (const unsigned char*)((uintptr_t)a & ~(uintptr_t)3);
  const int sh = (int)((uintptr_t)a & 3) * 8;
  unsigned d[4], u[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) d[i] = load_dword_within(a0 + 4 * i, frame, fend);
  d[3] = sh ? load_dword_within(a0 + 12, frame, fend) : 0u;
#pragma unroll
  for (int i = 0; i < 3; ++i) u[i] = sh ? (d[i] >> sh) | (d[i + 1] << (32 - sh)) : d[i];
  const unsigned hit = contiguous ? 1u : 255u;
  unsigned out = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int j = 3 * e;
    const int c0 = (int)((u[j >> 2] >> (8 * (j & 3))) & 255u), c1 = (int)((u[(j + 1) >> 2] >> (8 * ((j + 1) & 3))) & 255u),
              c2 = (int)((u[(j + 2) >> 2] >> (8 * ((j + 2) & 3))) & 255u);
    const int dist = max(max(abs(c0 - s0), abs(c1 - s1)), abs(c2 - s2));
    const unsigned v = p0 + e == seed ? 255u : dist <= tol ? hit : 0u;
    out |= v << (8 * e);
  }
  unsigned char* dst = state + p0;                                   // 4-byte aligned
  if (p0 >= 0 && p0 + 4 <= n) {
    *(unsigned*)dst = out;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (p0 + e >= 0 && p0 + e < n) dst[e] = (unsigned char)((out >> (8 * e)) & 255u);
  }
}

// ---- flood --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 run_fill_up(u64 r, u64 s) {
  const u64 a = r & s;
  return r | a | (((s + a) ^ s) & s);
}

__global__ void __launch_bounds__(64) select_flood_kernel(unsigned char* __restrict__ state, int Hi, int Wi, int ntx,
                                                          unsigned* __restrict__ changed) {
  const int lane = threadIdx.x;
  const int ty0 = (int)(blockIdx.x / (unsigned)ntx) * 64, tx0 = (int)(blockIdx.x % (unsigned)ntx) * 64;
  const int th = min(64, Hi - ty0), tw = min(64, Wi - tx0);           // the tile's rows and columns (>= 1)
  const bool col = lane < tw;
  unsigned char* base = state + (size_t)ty0 * Wi + tx0;              // the tile's first byte
  // the tile: lane y keeps row y
  u64 S = 0, R = 0;
#pragma unroll 8
  for (int y = 0; y < 64; ++y) {
    unsigned v = 0;
    if (y < th && col) v = base[(size_t)y * Wi + lane];
    const u64 s = __ballot(v != 0), r = __ballot(v == 255u);
    if (lane == y) { S = s; R = r; }
  }
  // the halo: reached bits of the rows above and below (uniform), of the columns left and right (lane y: row y)
  unsigned va = 0, vb = 0, vl = 0, vr = 0;
  if (ty0 > 0 && col) va = (base - Wi)[lane];
  if (ty0 + th < Hi && col) vb = base[(size_t)th * Wi + lane];
  if (lane < th) {
    if (tx0 > 0) vl = base[(long)lane * Wi - 1];
    if (tx0 + tw < Wi) vr = base[(long)lane * Wi + tw];
  }
  const u64 Ra = __ballot(va == 255u), Rb = __ballot(vb == 255u);
  u64 halo = (lane == 0 ? Ra : 0ull) | (lane == th - 1 ? Rb : 0ull) | (vl == 255u ? 1ull : 0ull) | (vr == 255u ? 1ull << (tw - 1) : 0ull);
  const u64 R0 = R;
  R |= halo & S;
  if (!__any(R != 0)) return;                                         // nothing reached in the tile or next to it
  // the closure
  for (;;) {
    const u64 before = R;
    R = run_fill_up(R, S);
    R = __brevll(run_fill_up(__brevll(R), __brevll(S)));
    u64 up = __shfl_up(R, 1, 64), dn = __shfl_down(R, 1, 64);
    if (lane == 0) up = 0;
    if (lane == 63) dn = 0;
    R |= S & (up | dn);
    if (!__any(R != before)) break;
  }
  const u64 fresh = R & ~R0;                                          // (R is a subset of S: every fresh byte holds 1)
  if (!__any(fresh != 0)) return;
  for (int y = 0; y < th; ++y) {
    const u64 m = __shfl(fresh, y, 64);
    if (m == 0) continue;                                             // (wave-uniform)
    if ((m >> lane) & 1ull) base[(size_t)y * Wi + lane] = (unsigned char)255;
  }
  if (lane == 0) *changed = 1u;
}

// ---- grow ---------------------------------------------------------------------------------------------------------------
// (hi:lo) >> s, 0 < s < 64
__device__ __forceinline__ void shr128(u64& lo, u64& hi, int s) {
  lo = (lo >> s) | (hi << (64 - s));
  hi >>= s;
}

__global__ void __launch_bounds__(256) select_grow_kernel(const unsigned char* __restrict__ state, unsigned char* __restrict__ out, int Hi,
                                                          int Wi, int ntx, int r) {
  __shared__ u64 s_h[SL_GROWS];                                       // per staged row: bit x = a reached byte in columns x .. x + 2r
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tx0 = (int)(blockIdx.x % (unsigned)ntx) * SL_GW, ty0 = (int)(blockIdx.x / (unsigned)ntx) * SL_GH;
  const int rows = SL_GH + 2 * r, n = 2 * r + 1;
  int p = 1;                                                          // the largest power of two <= n
  while (2 * p <= n) p *= 2;
  for (int i = wave; i < rows; i += 4) {
    const int y = ty0 - r + i;
    u64 lo = 0, hi = 0;
    if (y >= 0 && y < Hi) {                                           // (wave-uniform)
      const unsigned char* row = state + (size_t)y * Wi;
      const int xa = tx0 - r + lane, xb = xa + 64;                    // staged columns lane and 64 + lane
      unsigned v0 = 0, v1 = 0;
      if (xa >= 0 && xa < Wi) v0 = row[xa];
      if (lane < 2 * r && xb < Wi) v1 = row[xb];                      // (xb >= 0: tx0 - r + 64 > 0)
      lo = __ballot(v0 == 255u);
      hi = __ballot(v1 == 255u);
      for (int k = 1; k < p; k *= 2) {                                // a window of 2k from one of k
        u64 l2 = lo, h2 = hi;
        shr128(l2, h2, k);
        lo |= l2; hi |= h2;
      }
      if (n > p) {
        u64 l2 = lo, h2 = hi;
        shr128(l2, h2, n - p);
        lo |= l2;
      }
    }
    if (lane == 0) s_h[i] = lo;
  }
  __syncthreads();
  const int x = tx0 + lane;
  for (int j = wave; j < SL_GH; j += 4) {
    const int y = ty0 + j;
    if (y >= Hi) break;
    u64 m = 0;
    for (int dy = 0; dy < n; ++dy) m |= s_h[j + dy];
    if (x < Wi) out[(size_t)y * Wi + x] = (m >> lane) & 1ull ? (unsigned char)255 : (unsigned char)0;
  }
}

}  // namespace

hipError_t launch_select_similar(const unsigned char* frame, int Hi, int Wi, int seed_y, int seed_x, int tolerance, int contiguous,
                                 unsigned char* state, hipStream_t st) {
  const long n = (long)Hi * Wi;
  const long ndw = (n + (long)((uintptr_t)state & 3) + 3) / 4;       // the aligned dwords that hold the plane's bytes
  // bytes: the frame read once, the plane written once
  set_launch_cost(0.0, 4.0 * (double)n, "select_similar");
  set_launch_grid((ndw + 255) / 256);
  ProfScope ps_(st, PL_SELECT_SIMILAR);
  hipLaunchKernelGGL(select_similar_kernel, dim3((unsigned)((ndw + 255) / 256)), dim3(256), 0, st, frame, state, n,
                     (long)seed_y * Wi + seed_x, tolerance, contiguous, ndw);
  return hipGetLastError();
}

hipError_t launch_select_flood(unsigned char* state, int Hi, int Wi, unsigned* changed, hipStream_t st) {
  const int ntx = (Wi + 63) / 64, nty = (Hi + 63) / 64;
  // bytes: an upper bound, the plane read once with the halo's share and every byte stored
  set_launch_cost(0.0, (double)Hi * Wi * (1.0 + 4.0 / 64.0 + 1.0), "select_flood");
  set_launch_grid((long)ntx * nty);
  ProfScope ps_(st, PL_SELECT_FLOOD);
  hipLaunchKernelGGL(select_flood_kernel, dim3((unsigned)((long)ntx * nty)), dim3(64), 0, st, state, Hi, Wi, ntx, changed);
  return hipGetLastError();
}

hipError_t launch_select_grow(const unsigned char* state, int Hi, int Wi, int grow, unsigned char* out, hipStream_t st) {
  const int ntx = (Wi + SL_GW - 1) / SL_GW, nty = (Hi + SL_GH - 1) / SL_GH;
  // bytes: the plane read with the halo's share, the output written once
  const double halo = (double)(SL_GW + 2 * grow) * (SL_GH + 2 * grow) / (double)(SL_GW * SL_GH);
  set_launch_cost(0.0, (double)Hi * Wi * (halo + 1.0), "select_grow");
  set_launch_grid((long)ntx * nty);
  ProfScope ps_(st, PL_SELECT_GROW);
  hipLaunchKernelGGL(select_grow_kernel, dim3((unsigned)((long)ntx * nty)), dim3(256), 0, st, state, out, Hi, Wi, ntx, grow);
  return hipGetLastError();
}

}  // namespace se
