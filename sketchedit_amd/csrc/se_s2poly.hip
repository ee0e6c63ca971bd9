// Polyphase F(2,2) form of the 3x3 stride-2 gated convolution 48 -> 96 and 48 -> 192 (xconv4_downsample; conv4_downsample,
// wconv4_downsample, pmconv4_downsample and netM's conv4_downsample of se_plan.hip: the 128x128 -> 64x64 step of every encoder).
// Per dimension a 3-tap stride-2 conv with padding 1 is a 1-tap conv on the even input phase plus a 2-tap stride-1 conv on the odd
// phase; F(2,2) on the 2-tap part takes 3 products per 2 outputs instead of 4: 5 positions per output pair (the table of
// se_s2poly.h).  Two-dimensional: the outer product, 25 positions (py, px) per 2x2 output tile instead of 36 taps, 1, 2 or 4 signed
// source pixels per position (49 in all), every coefficient 0 or +-1; the transformed weights are formed on the host
// (s2poly_pack_host).  Skeleton, rings, K pairing and epilogue are se_wino48.hip's -- read that header first:
//   * K per position is 48: two positions share three 32-k chunks; 12 pairs, and position 24 alone over chunks A and B whose
//     last k-half is not issued: 38 iterations, 1800 MFMAs per wave.
//   * 96 MIXED rows per workgroup, 64 tiles x 4 waves, two workgroups per CU.  cout = 192: blockIdx.y selects the 96-row half
//     (48 features with their own gates: the gate exchange stays inside a wave); upk [half][38 iterations][96 rows][32].
//   * A tile is 2x2 outputs = a 5x5 source patch at (4 ty - 1, 4 tx - 1).  Row offsets per thread (they carry the lane's
//     granule), column offsets per tile: 5 KB + 1.25 KB, 78.25 KB per workgroup.
#include "se_device.h"
#include "se_s2poly.h"

#include <cstdlib>
#include <type_traits>

namespace se {

// a compile-time loop index (se_wino48.hip static_for48)
template <int I, int N, typename F>
DEVFN void static_for_s2(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for_s2<I + 1, N>(f);
  }
}

__global__ __launch_bounds__(256, 2) void s2poly48_kernel(const WinoParams p) {
  constexpr int TILES = 64, NTHR = 256, NWV = 4;
  constexpr int XB = TILES * 128, WB = 96 * 128;
  constexpr int NPOS = S2POLY_NPOS, NIT = S2POLY_NIT;    // 12 position pairs x 3 chunks + chunks A, B of the pair (24, -)
  constexpr unsigned PSB = 192;                          // bytes per source pixel
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Xb = smem;
  char* Wb = smem + 3 * XB;

  const int tid = threadIdx.x, lane = tid & 63;
  const float eluw = p.act == 0 ? 1.f : 0.f;      // act_fast: ELU weight of the gated epilogue (wave-uniform)
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int chh = w & 1, tp = w >> 1;          // row half of this workgroup's 96 rows (3 MIXED tiles), tile pair (32 tiles)
  const int half = (int)blockIdx.y;            // which 96 of the layer's rows (cout = 192: two)
  const int tile_base = (p.xcd ? xcd_tile(blockIdx.x, gridDim.x) : (int)blockIdx.x) * TILES;
  const int tpi = p.th * p.tw;                 // tiles per image
  const float* upk = p.upk + (size_t)half * NIT * 96 * 32;
  const float* bias = p.bias + half * 96;

  // tile -> (batch, tile row, tile column): outputs (2 iy + a, 2 ix + b), source patch rows 4 iy - 1 .. 4 iy + 3
  auto tile_origin = [&](int t, int& b, int& iy, int& ix) {
    b = (int)udiv_magic((unsigned)t, p.div_tpi_m, p.div_tpi_l);
    const int rem = t - b * tpi;
    iy = (int)udiv_magic((unsigned)rem, p.div_tw_m, p.div_tw_l);
    ix = rem - iy * p.tw;
  };

  // ---- staging role: tile row srow, granule sg (4 channels) of each 16-channel k-half (se_wino48.hip)
  const int sg = tid & 3, srow = (tid >> 6) * 16 + ((tid >> 2) & 1) * 8 + ((tid >> 3) & 7);
  const int swz = (srow >> 1) & 7;
  char* xw0 = Xb + srow * 128 + ((sg ^ swz) << 4);             // k-half 0: logical slot sg
  char* xw1 = Xb + srow * 128 + (((4 + sg) ^ swz) << 4);       // k-half 1: logical slot 4 + sg
  // Source offsets of the 5x5 patch, kept in LDS (read once per position):
  //   Ysrc[i][tid]  = byte offset of pixel row 4 iy - 1 + i (+ this lane's granule), or 0x80000000 (+ granule) if outside / invalid tile
  //   Xsrc[i][tile] = byte offset of column 4 ix - 1 + i inside the row, or 0x80000000 if outside
  // A gather offset is their SATURATING sum: >= 2^31 as soon as either part is outside, and the buffer range check returns
  // zeros there (zero padding, se_wino48.hip)
  int* Ysrc = (int*)(smem + 3 * XB + 4 * WB);     // 5 * NTHR ints
  int* Xsrc = Ysrc + 5 * NTHR;                    // 5 * TILES ints
  {
    const int t = tile_base + srow;
    int b, iy, ix;
    tile_origin(t < p.total_tiles ? t : 0, b, iy, ix);
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const int y = 4 * iy - 1 + i;
      Ysrc[i * NTHR + tid] = (t < p.total_tiles && (unsigned)y < (unsigned)p.h) ? (int)((unsigned)((b * p.h + y) * p.w) * PSB + (unsigned)sg * 16u) : (int)(0x80000000u + (unsigned)sg * 16u);
    }
    if (tid < TILES) {
      const int t2 = tile_base + tid;
      tile_origin(t2 < p.total_tiles ? t2 : 0, b, iy, ix);
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        const int x = 4 * ix - 1 + i;
        Xsrc[i * TILES + tid] = ((unsigned)x < (unsigned)p.w) ? x * (int)PSB : (int)0x80000000;
      }
    }
  }
  __syncthreads();                                // (Xsrc is written by another thread than its readers)
  const unsigned lds_w = lds_addr_of(Wb);
  int off0, off1;
  frag_offsets(lane, off0, off1);

  // (1-D position -> patch index of its source a (sign +) and of its source b (sign -; -1: none): s2poly_src_a / _b, se_s2poly.h)
  // source pixel i of a position = (row a|b, column a|b): i = 0 (a,a), 1 (a,b), 2 (b,a), 3 (b,b).  Position 25 (the missing
  // partner of position 24) has no sources
  auto need = [&](int pos, int i) {
    if (pos >= NPOS) return false;
    return !((i >= 2 && s2poly_src_b(pos / 5) < 0) || ((i & 1) && s2poly_src_b(pos % 5) < 0));
  };
  unsigned o[2][4];     // [even / odd position of the pair]: byte offsets of the source pixels (>= 2^31: outside)
  auto set_pos = [&](int set, int pos) {    // compile-time arguments after unrolling
    const int py = pos / 5, px = pos % 5;
    const unsigned ya = (unsigned)Ysrc[s2poly_src_a(py) * NTHR + tid], xa = (unsigned)Xsrc[s2poly_src_a(px) * TILES + srow];
    o[set][0] = __builtin_elementwise_add_sat(ya, xa);
    if (s2poly_src_b(px) >= 0) o[set][1] = __builtin_elementwise_add_sat(ya, (unsigned)Xsrc[s2poly_src_b(px) * TILES + srow]);
    if (s2poly_src_b(py) >= 0) {
      const unsigned yb = (unsigned)Ysrc[s2poly_src_b(py) * NTHR + tid];
      o[set][2] = __builtin_elementwise_add_sat(yb, xa);
      if (s2poly_src_b(px) >= 0) o[set][3] = __builtin_elementwise_add_sat(yb, (unsigned)Xsrc[s2poly_src_b(px) * TILES + srow]);
    }
  };
  // k-half h of iteration it -> (position set, 16-channel group, position): the chunk table of se_wino48.hip
  auto half_set = [](int it, int h) { return (it % 3) * 2 + h >= 3 ? 1 : 0; };
  auto half_grp = [](int it, int h) { return ((it % 3) * 2 + h) % 3; };
  auto half_pos = [&](int it, int h) { return 2 * (it / 3) + half_set(it, h); };
  const __amdgpu_buffer_rsrc_t rs0 = __builtin_amdgcn_make_buffer_rsrc((void*)p.src, 0, (int)((unsigned)p.B * (unsigned)p.h * (unsigned)p.w * PSB), 0x00020000);
  // one raw granule (source pixel i) of k-half h of iteration `it`: one vector-memory instruction
  auto load_x1 = [&](int it, f32x4 (&r)[2][4], int h, int i) {
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    if (need(half_pos(it, h), i))
      r[h][i] = __builtin_bit_cast(f32x4, (u32x4)__builtin_amdgcn_raw_buffer_load_b128(rs0, (int)o[half_set(it, h)][i], half_grp(it, h) * 64, 0));
  };
  float negone = -1.f;
  asm volatile("" : "+v"(negone));      // opaque -1: a subtraction stays one packed fma (a plain - becomes 4 v_sub)
  // the granules of a position combined with their signs: (a,a) and (b,b) enter with +, (a,b) and (b,a) with -
  auto signed_sum = [&](const f32x4 (&q)[4], int pos) -> f32x4 {
    f32x4 ps = q[0], ns = {0.f, 0.f, 0.f, 0.f};
    bool hn = false;
    if (need(pos, 3)) ps = ps + q[3];
#pragma unroll
    for (int i = 1; i < 3; ++i)
      if (need(pos, i)) { ns = hn ? ns + q[i] : q[i]; hn = true; }
    return hn ? ns * negone + ps : ps;
  };
  auto write_x = [&](int it, int buf, const f32x4 (&r)[2][4]) {
    *(f32x4*)(xw0 + buf * XB) = signed_sum(r[0], half_pos(it, 0));
    if (half_pos(it, 1) < NPOS) *(f32x4*)(xw1 + buf * XB) = signed_sum(r[1], half_pos(it, 1));      // (the k-half behind position 24 is not issued)
  };
  // W tile: 12 row blocks of 8 rows; wave w stages blocks w, w + 4, w + 8
  auto dma_w = [&](int it, int buf, int j) {
    const int rbk = j * NWV + w;
    glds16_s(upk + (size_t)it * 96 * 32 + rbk * 256, (unsigned)lane * 16u, lds_w + buf * WB + rbk * 1024);
  };

  f32x4 am[3][2];                      // position accumulators (row tile, tile group)
  f32x4 oy[2][2][3][2];                // output accumulators (a, b, row tile, tile group)
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      am[j][q] = (f32x4){0.f, 0.f, 0.f, 0.f};
      // the output accumulators start at the bias (MIXED packed rows): one add less per value in the epilogue
      const f32x4 b4 = *(const f32x4*)(bias + (3 * chh + j) * 16 + (lane >> 4) * 4);
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) oy[a][b][j][q] = b4;
    }
  // fold the finished position: Y[a][b] += Ay[a][py] * Ax[b][px] * M with the 1-D fold rows of se_s2poly.h; pos compile-time,
  // so only the non-zero terms exist and they are plain adds / subtracts
  float neg1 = -1.f;
  asm volatile("" : "+v"(neg1));      // opaque multiplier: keeps the subtraction a packed fma
  auto fold = [&](int pos) {
    const int py = pos / 5, px = pos % 5;
    const int ay[2] = {s2poly_fold(py, 0), s2poly_fold(py, 1)};
    const int ax[2] = {s2poly_fold(px, 0), s2poly_fold(px, 1)};
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int q = 0; q < 2; ++q) {
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            const int c = ay[a] * ax[b];
            if (c > 0) oy[a][b][j][q] += am[j][q];
            else if (c < 0) oy[a][b][j][q] = am[j][q] * neg1 + oy[a][b][j][q];     // v_pk_fma (a plain -= becomes 4 scalar v_sub)
          }
        // pin the sums: hipcc would otherwise sink every fold to the end of the unrolled kernel
        asm volatile("" : "+v"(oy[0][0][j][q]), "+v"(oy[0][1][j][q]), "+v"(oy[1][0][j][q]), "+v"(oy[1][1][j][q]));
      }
  };

  // ---- pipeline (se_wino48.hip): X tiles in a 3-slot, W tiles in a 4-slot LDS ring, one barrier and one conservative
  // vmcnt(0) per iteration
  //   iteration it:  groups 0-3 | vmcnt(0); X(it+2) <- granules loaded in it-1 | groups 4-7: W DMA and granule loads
  //                  of it+3, k-half 0 fragments of it+1 | barrier
  auto end_barrier = [&]() {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
  };

  // ---- prologue: X slots 0, 1; W slots 0, 1, 2; granules of iteration 2 in flight
  f32x4 r[2][4];
  set_pos(0, 0);
  set_pos(1, 1);
#pragma unroll
  for (int i0 = 0; i0 < 3; ++i0) { dma_w(i0, i0, 0); dma_w(i0, i0, 1); dma_w(i0, i0, 2); }     // W DMA first: overlaps the granule round trip
  {
    f32x4 r1[2][4];                    // iterations 0 and 1: both sets of loads in flight before the first transform
#pragma unroll
    for (int i = 0; i < 4; ++i) { load_x1(0, r, 0, i); load_x1(0, r, 1, i); }
#pragma unroll
    for (int i = 0; i < 4; ++i) { load_x1(1, r1, 0, i); load_x1(1, r1, 1, i); }
    write_x(0, 0, r);
    write_x(1, 1, r1);
  }
  set_pos(0, 2);                       // even position of pair 1 (iteration 3 on)
  dma_wait_all();
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) { load_x1(2, r, 0, i); load_x1(2, r, 1, i); }

  const char* Xw = Xb + tp * 32 * 128;                   // this wave's 32 tile rows
  const char* Ww = Wb + (3 * chh) * 2048;                // this wave's 3 row tiles
  f32x4 wa[3], xa[2];                  // k-half 0 fragments of the current iteration (read one iteration ahead)
  xa[0] = *(const f32x4*)(Xw + off0);
  xa[1] = *(const f32x4*)(Xw + 2048 + off0);
#pragma unroll
  for (int j = 0; j < 3; ++j) wa[j] = *(const f32x4*)(Ww + j * 2048 + off0);

  // position pairs x chunks, fully unrolled through a compile-time index: everything below is compile-time
  static_for_s2<0, NIT>([&](auto it_c) __attribute__((always_inline)) {
    constexpr int it = decltype(it_c)::value;
    constexpr int pp = it / 3, c = it % 3;
    constexpr int b0 = it % 3, b1 = (it + 1) % 3, b2 = (it + 2) % 3;      // X ring
    constexpr int w0 = it % 4, w1 = (it + 1) % 4, w3 = (it + 3) % 4;      // W ring
    constexpr bool more1 = it + 1 < NIT, more2 = it + 2 < NIT, more3 = it + 3 < NIT;
    constexpr bool second = 2 * pp + (c >= 1 ? 1 : 0) < NPOS;             // k-half 1 carries a position (not behind position 24)
    f32x4 wb[3], xb[2];
    if (second) {
      xb[0] = *(const f32x4*)(Xw + b0 * XB + off1);                  // k-half 1 fragments of this iteration
      xb[1] = *(const f32x4*)(Xw + b0 * XB + 2048 + off1);
#pragma unroll
      for (int j = 0; j < 3; ++j) wb[j] = *(const f32x4*)(Ww + w0 * WB + j * 2048 + off1);
    }
    __builtin_amdgcn_sched_barrier(0);
    // one group = 6 MFMAs: k-step e of the 3 x 2 accumulator tiles; `first`: C = 0 (first k-step of a position)
    auto group = [&](const f32x4 (&wf)[3], const f32x4 (&xf)[2], int e, bool first) {
#pragma unroll
      for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const f32x4 cin = first ? (f32x4){0.f, 0.f, 0.f, 0.f} : am[j][q];
          am[j][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[j][e], xf[q][e], cin, 0, 0, 0);
        }
      __builtin_amdgcn_sched_barrier(0);
    };
    if (c == 0 && it > 0) {              // chunk A: the odd position of the previous pair is complete
      fold(2 * pp - 1);
      __builtin_amdgcn_sched_barrier(0);
    }
    group(wa, xa, 0, c == 0);
    group(wa, xa, 1, false);
    group(wa, xa, 2, false);
    group(wa, xa, 3, false);
    if (c == 1) {                        // chunk B: the even position ends with k-half 0, the odd one starts
      fold(2 * pp);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (more2) {
      dma_wait_all();                    // granules and W DMA issued in groups 4-7 of the previous iteration
      write_x(it + 2, b2, r);
    }
    // next use of a position set: even set after the last chunk-B write, odd set after the last chunk-C write
    if (c == 2 && 2 * (pp + 2) < NPOS) set_pos(0, 2 * (pp + 2));
    if (c == 0 && 2 * (pp + 1) + 1 < NPOS) set_pos(1, 2 * (pp + 1) + 1);
    __builtin_amdgcn_sched_barrier(0);
    // vector-memory instructions spread over the MFMA groups (a burst from all waves fills the CU's queue and stalls the
    // waves, MFMAs included, in front of it)
    if (second) group(wb, xb, 0, c == 1);
    if (more3) { dma_w(it + 3, w3, 0); load_x1(it + 3, r, 0, 0); load_x1(it + 3, r, 0, 1); }
    if (more1) {                                          // k-half 0 fragments of it+1 (published slots)
      xa[0] = *(const f32x4*)(Xw + b1 * XB + off0);
      xa[1] = *(const f32x4*)(Xw + b1 * XB + 2048 + off0);
#pragma unroll
      for (int j = 0; j < 3; ++j) wa[j] = *(const f32x4*)(Ww + w1 * WB + j * 2048 + off0);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (second) group(wb, xb, 1, false);
    if (more3) { dma_w(it + 3, w3, 1); load_x1(it + 3, r, 0, 2); load_x1(it + 3, r, 0, 3); }
    __builtin_amdgcn_sched_barrier(0);
    if (second) group(wb, xb, 2, false);
    if (more3) { dma_w(it + 3, w3, 2); load_x1(it + 3, r, 1, 0); load_x1(it + 3, r, 1, 1); }
    __builtin_amdgcn_sched_barrier(0);
    if (second) group(wb, xb, 3, false);
    if (more3) { load_x1(it + 3, r, 1, 2); load_x1(it + 3, r, 1, 3); }
    if (more1) end_barrier();
  });
  // (position 24 was folded in chunk B of the last pair)

  // ---- epilogue (se_wino48.hip): v_permlane32_swap gate exchange, two outputs per lane.  dst: [B][h/2][w/2][48 gridDim.y]
  const int q = lane >> 4;
  const int OH = p.h >> 1, OW = p.w >> 1;
  const unsigned pix_bytes = 192u * gridDim.y;
#pragma unroll
  for (int tq = 0; tq < 2; ++tq) {
    const int t = tile_base + tp * 32 + tq * 16 + (lane & 15);
    int b = 0, iy = 0, ix = 0;
    tile_origin(t < p.total_tiles ? t : 0, b, iy, ix);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int c0 = half * 48 + (3 * chh + j) * 8 + (q & 1) * 4 + (q >> 1) * 2;
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int bb = 0; bb < 2; ++bb) {
          const f32x4 v = oy[a][bb][j][tq];      // (bias already inside)
          const auto s02 = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[0]), __float_as_uint(v[2]), false, false);
          const auto s13 = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[1]), __float_as_uint(v[3]), false, false);
          const float f0 = __uint_as_float(s02[0]), g0 = __uint_as_float(s02[1]);
          const float f1 = __uint_as_float(s13[0]), g1 = __uint_as_float(s13[1]);
          float2 ov;
          ov.x = act_fast(f0, eluw) * sigmoid_fast(g0);
          ov.y = act_fast(f1, eluw) * sigmoid_fast(g1);
          if (t < p.total_tiles)
            *(float2*)((char*)p.dst + ((unsigned)((b * OH + 2 * iy + a) * OW + 2 * ix + bb) * pix_bytes + (unsigned)c0 * 4u)) = ov;      // 32-bit offset: the launch guards the bytes
        }
    }
  }
}

// src NHWC 48 at (h, w), h % 4 == w % 4 == 0; dst NHWC 48 `halves` at (h/2, w/2); th = h/4, tw = w/4
hipError_t launch_s2poly48(const WinoParams& p, int halves, hipStream_t st) {
  constexpr int TILES = 64;
  constexpr int LDS = 3 * TILES * 128 + 4 * 96 * 128 + 5 * TILES * 4 * 4 + 5 * TILES * 4;     // X ring 24 KB + W ring 48 KB + source offsets 6.25 KB
  static_assert(LDS <= 80 * 1024, "two workgroups per CU");
  if ((halves != 1 && halves != 2) || (p.h % 4) || (p.w % 4) || p.th != p.h / 4 || p.tw != p.w / 4) return hipErrorInvalidValue;
  // 32-bit byte offsets: the source (192 bytes per pixel) and the destination (at most 384 bytes per quarter as many pixels)
  if ((double)p.B * p.h * p.w * 192.0 >= 2147483648.0) return hipErrorInvalidValue;
  {
    hipError_t e = ensure_max_lds((const void*)s2poly48_kernel, LDS);
    if (e != hipSuccess) return e;
  }
  const int grid = (p.total_tiles + TILES - 1) / TILES;
  set_launch_grid((long)grid * halves);
  ProfScope ps_(st, PL_WINO_N96, "s2poly48");
  hipLaunchKernelGGL(s2poly48_kernel, dim3(grid, halves), dim3(TILES * 4), LDS, st, p);
  return hipGetLastError();
}

}  // namespace se
