// Streaming contextual attention: the space-to-depth form (se_attention.hip) without any R x R matrix.
//
// With the class grid hc x wc = h/2 x w/2, queries / keys q, k on its (hc-1) x (wc-1) sub-grid, D = {0, 1, wc, wc+1}:
//   E[r][s]  = <X_r, XN_s>          X_r, XN_s: the 2x2x96 = 384-vectors of x / xn = x rn at class-grid position r / s
//   S[q][k]  = sum_{d in D} E[q+d][k+d],   t = S * scale * valid[k] (log2 domain: * log2 e; an invalid key keeps t = 0)
//   P[q][k]  = exp2(t - m_q) / l_q         (m_q, l_q: maximum and sum of exp2(t - m_q) over all keys of query q)
//   out[2r+cls] = sum_s P~[r][s] x[2s+cls],   P~[r][s] = sum_{d in D} P[r-d][s-d]
// Two passes over the key axis, both recomputing E tiles on MFMA; nothing is stored between them but (m, 1/l) per query:
//   att_stream_stats_kernel : a workgroup owns 7 x 7 queries; per 7 x 7 key block the 8 x 8 x 8 x 8 (64 x 64, K = 384) E tile
//                             (block + one row / column of halo on both axes) goes to LDS, S is its 2x2 box sum, and every
//                             thread keeps an online (maximum, sum) over its share of the keys; the shares are combined in a
//                             fixed order at the end.
//   att_stream_out_kernel   : a workgroup owns 6 x 6 output class positions, i.e. the 7 x 7 queries that cover them (E rows:
//                             8 x 8 = 64 again); per 7 x 7 key block: E tile, P (exactly normalised with pass 1's statistics),
//                             P~ restricted to this block's keys (8 x 8 value positions s = k + d), then P~ . V on MFMA into
//                             a resident 48 x 384 fp32 accumulator (wave = parity class, 6 channel tiles x 3 row tiles).
// The key blocks partition the keys, so the sum over blocks is the full P~ . V; every output is written once by its owner:
// no atomics, deterministic, and an image's result does not depend on the rest of the batch.
// BF16: x, xn, xT and out hold bf16; the two GEMMs run v_mfma_f32_16x16x32_bf16, S and the statistics stay fp32, P is rounded
// to bf16 where the oracle rounds it (sketchedit_oracle.py attention_reconstruct) and P~, the sum of four rounded values, is
// rounded once more for the P~ . V product -- the rounding points of the materialised bf16 form.
// Inputs come from the O(R) preparation of the materialised form (launch_att2_prep: xn, key tables, transposed values).
#include "se_device.h"

namespace se {

namespace {

constexpr int KB = 7;          // queries / keys per block side
constexpr int ET = 8;          // E tile side: KB + 1 (halo of one on each axis)
constexpr int OB = 6;          // output class positions per block side (pass 2): its queries are OB + 1 = KB per side
constexpr int ELD = 65;        // LDS row stride (floats) of the 64 x 64 E tile
constexpr int PLD = 50;        // ... of the 49 x 49 P tile
constexpr int PTLD = 68;       // ... of the 48 x 64 P~ tile (floats; bf16: 2 x 68 elements, the same bytes)

typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));      // 4-byte aligned 16-byte loads (shifted columns)

DEVFN int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// E tile: Et[i][j] = <X_{row i}, XN_{column j}>, i = (i / 8, i % 8) from (ry0, rx0), j = (j / 8, j % 8) from (ky0, kx0), positions
// clamped into the class grid (a clamped row or column only feeds queries / keys that do not exist).  Wave w computes the
// 32 x 32 quadrant (w >> 1, w & 1) as 2 x 2 MFMA tiles.  The 384-vector of position (y, x) is two contiguous runs of 192
// (pixel rows 2y and 2y + 1, pixels 2x and 2x + 1); the k order inside a chunk is any permutation shared by both operands,
// so a lane loads consecutive k values (16 bytes) and feeds them to consecutive MFMAs.
template <bool BF16>
DEVFN void e_tile(const AttParams& p, int b, int ry0, int rx0, int ky0, int kx0, float* Et) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, i16 = lane & 15, g = lane >> 4;
  constexpr int ES = BF16 ? 2 : 4;
  const long rowb = (long)p.w * 96 * ES;      // bytes from pixel row 2y to 2y + 1
  const char* pa[2];
  const char* pb[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int i = 32 * (w >> 1) + 16 * t + i16, j = 32 * (w & 1) + 16 * t + i16;
    const int ay = clampi(ry0 + (i >> 3), 0, p.hc - 1), ax = clampi(rx0 + (i & 7), 0, p.wc - 1);
    const int by = clampi(ky0 + (j >> 3), 0, p.hc - 1), bx = clampi(kx0 + (j & 7), 0, p.wc - 1);
    pa[t] = (const char*)p.x + (((long)b * p.h + 2 * ay) * p.w + 2 * ax) * 96 * ES;
    pb[t] = (const char*)p.xn + (((long)b * p.h + 2 * by) * p.w + 2 * bx) * 96 * ES;
  }
  f32x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int c = 0; c < 2; ++c) acc[a][c] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int run = 0; run < 2; ++run) {
    if (BF16) {
#pragma unroll 2
      for (int k = 0; k < 192; k += 32) {
        const long off = run * rowb + (long)(k + 8 * g) * 2;
        bf16x8 va[2], vb[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          va[t] = *(const bf16x8*)(pa[t] + off);
          vb[t] = *(const bf16x8*)(pb[t] + off);
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int c = 0; c < 2; ++c) acc[a][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va[a], vb[c], acc[a][c], 0, 0, 0);
      }
    } else {
#pragma unroll 4
      for (int k = 0; k < 192; k += 16) {
        const long off = run * rowb + (long)(k + 4 * g) * 4;
        f32x4 va[2], vb[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          va[t] = *(const f32x4*)(pa[t] + off);
          vb[t] = *(const f32x4*)(pb[t] + off);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int c = 0; c < 2; ++c) acc[a][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(va[a][r], vb[c][r], acc[a][c], 0, 0, 0);
      }
    }
  }
  // D[i = 4 g + reg][j = lane & 15]
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) Et[(32 * (w >> 1) + 16 * a + 4 * g + r) * ELD + 32 * (w & 1) + 16 * c + i16] = acc[a][c][r];
}

// S[q][k] * scale * log2(e) * valid[k] from the E tile: query (qa, qc) and key (ka, kc) of the 7 x 7 blocks, E rows / columns
// at the same offsets plus d.  Summation order d = (0,0), (0,1), (1,0), (1,1).
DEVFN float s_log2(const float* Et, int qa, int qc, int ka, int kc, float kmul) {
  const float* e = Et + (qa * ET + qc) * ELD + ka * ET + kc;
  const float sum = ((e[0] + e[ELD + 1]) + e[ET * ELD + ET]) + e[(ET + 1) * ELD + ET + 1];
  return sum * kmul;
}

}  // namespace

// stats[b][q] = (m, 1 / l) in class-grid indexing, m in the log2 domain.  Thread: query tid & 63 (< 49), key share tid >> 6.
template <bool BF16>
__global__ __launch_bounds__(256) void att_stream_stats_kernel(const AttParams p, int nby, int nbx) {
  __shared__ float Et[64 * ELD];
  __shared__ float red[4][64][2];
  const int tid = threadIdx.x, nb = nby * nbx;
  const int b = blockIdx.x / nb, blk = blockIdx.x - b * nb;
  const int qy0 = (blk / nbx) * KB, qx0 = (blk % nbx) * KB;
  const int qi = tid & 63, part = tid >> 6;
  const int qa = qi / KB, qc = qi - (qi / KB) * KB;
  const bool qok = qi < KB * KB && qy0 + qa < p.hs && qx0 + qc < p.ws;
  const float* kmul = p.kmul + (long)b * p.Rp;
  float m = -1e30f, l = 0.f;
  for (int kb = 0; kb < nb; ++kb) {
    const int ky0 = (kb / nbx) * KB, kx0 = (kb % nbx) * KB;
    __syncthreads();
    e_tile<BF16>(p, b, qy0, qx0, ky0, kx0, Et);
    __syncthreads();
    if (qok) {
      for (int kk = part; kk < KB * KB; kk += 4) {
        const int ka = kk / KB, kc = kk - (kk / KB) * KB;
        if (ky0 + ka >= p.hs || kx0 + kc >= p.ws) continue;
        const float t = s_log2(Et, qa, qc, ka, kc, kmul[(ky0 + ka) * p.wc + kx0 + kc]);
        const float mn = fmaxf(m, t);
        l = l * __builtin_amdgcn_exp2f(m - mn) + __builtin_amdgcn_exp2f(t - mn);
        m = mn;
      }
    }
  }
  red[part][qi][0] = m;
  red[part][qi][1] = l;
  __syncthreads();
  if (tid < 64 && qok) {
    float M = red[0][qi][0];
#pragma unroll
    for (int i = 1; i < 4; ++i) M = fmaxf(M, red[i][qi][0]);
    float L = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) L += red[i][qi][1] * __builtin_amdgcn_exp2f(red[i][qi][0] - M);
    float* st = p.stats + ((long)b * p.R + (long)(qy0 + qa) * p.wc + qx0 + qc) * 2;
    st[0] = M;
    st[1] = 1.f / L;
  }
}

// out for the 6 x 6 class positions (r0y .. r0y + 5, r0x .. r0x + 5), all 4 classes x 96 channels.
template <bool BF16>
__global__ __launch_bounds__(256) void att_stream_out_kernel(const AttParams p, int nby, int nbx, int noy, int nox) {
  __shared__ float Et[64 * ELD];
  __shared__ float Pl[KB * KB * PLD];
  __shared__ float Pt[48 * PTLD];
  __shared__ float qm[64], qil[64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, i16 = lane & 15, g = lane >> 4;
  const int no = noy * nox, nb = nby * nbx;
  const int b = blockIdx.x / no, blk = blockIdx.x - b * no;
  const int r0y = (blk / nox) * OB, r0x = (blk % nox) * OB;
  const int qy0 = r0y - 1, qx0 = r0x - 1;      // the 7 x 7 queries r - d
  if (tid < 64) {
    const int qa = tid / KB, qc = tid - (tid / KB) * KB, qy = qy0 + qa, qx = qx0 + qc;
    const bool ok = tid < KB * KB && qy >= 0 && qx >= 0 && qy < p.hs && qx < p.ws;
    const float* st = p.stats + ((long)b * p.R + (ok ? (long)qy * p.wc + qx : 0)) * 2;
    qm[tid] = ok ? st[0] : 0.f;
    qil[tid] = ok ? st[1] : 0.f;      // a query that does not exist: P = 0
  }
  const float* kmul = p.kmul + (long)b * p.Rp;
  constexpr int ES = BF16 ? 2 : 4;
  // values: xT[b][cls = w][c][s]
  const char* vbase = (const char*)p.xT + ((long)b * 4 + w) * 96 * p.Rp * ES;
  f32x4 acc[3][6];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int c = 0; c < 6; ++c) acc[a][c] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int kb = 0; kb < nb; ++kb) {
    const int ky0 = (kb / nbx) * KB, kx0 = (kb % nbx) * KB;
    __syncthreads();
    e_tile<BF16>(p, b, qy0, qx0, ky0, kx0, Et);
    __syncthreads();
    for (int idx = tid; idx < KB * KB * KB * KB; idx += 256) {
      const int qi = idx / (KB * KB), kk = idx - qi * (KB * KB);
      const int qa = qi / KB, qc = qi - qa * KB, ka = kk / KB, kc = kk - ka * KB;
      float v = 0.f;
      if (ky0 + ka < p.hs && kx0 + kc < p.ws && qil[qi] != 0.f) {
        const float t = s_log2(Et, qa, qc, ka, kc, kmul[(ky0 + ka) * p.wc + kx0 + kc]);
        v = __builtin_amdgcn_exp2f(t - qm[qi]) * qil[qi];
        if (BF16) v = bf16_lo(pack_bf16x2(v, 0.f));      // P rounded where the oracle rounds it (as the materialised form)
      }
      Pl[qi * PLD + kk] = v;
    }
    __syncthreads();
    // P~ restricted to this block's keys: rows ri = (ra, rc) of the 6 x 6 outputs (36 .. 47: zero), columns e = (ey, ex) of the
    // 8 x 8 value positions s = (ky0 + ey, kx0 + ex); query r - d is (ra + 1 - dy, rc + 1 - dx) of the 7 x 7, key s - d is
    // (ey - dy, ex - dx) when inside the block.
    for (int idx = tid; idx < 48 * 64; idx += 256) {
      const int ri = idx >> 6, e = idx & 63, ey = e >> 3, ex = e & 7;
      float v = 0.f;
      if (ri < OB * OB) {
        const int ra = ri / OB, rc = ri - ra * OB;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          const int dy = d >> 1, dx = d & 1, ka = ey - dy, kc = ex - dx;
          if (ka >= 0 && kc >= 0 && ka < KB && kc < KB) v += Pl[((ra + 1 - dy) * KB + rc + 1 - dx) * PLD + ka * KB + kc];
        }
      }
      if (BF16) ((unsigned short*)Pt)[ri * 2 * PTLD + e] = (unsigned short)(pack_bf16x2(v, 0.f) & 0xffffu);
      else Pt[ri * PTLD + e] = v;
    }
    __syncthreads();
    // acc[row tile a][channel tile c] += P~[16 a + i][s] * V[s][cls = w][16 c + j], K = the 64 value positions
    if (BF16) {
#pragma unroll
      for (int kc = 0; kc < 2; ++kc) {      // 32 k per MFMA: lane group g holds value row ey = 4 kc + g, all 8 columns
        bf16x8 va[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) va[a] = *(const bf16x8*)((const char*)Pt + ((16 * a + i16) * 2 * PTLD + 32 * kc + 8 * g) * 2);
        const int sy = min(ky0 + 4 * kc + g, p.hc - 1);
        const long e0 = (long)sy * p.wc + kx0;      // first of 8 consecutive bf16 values (2-byte aligned)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          const unsigned* q = (const unsigned*)(vbase + ((long)(16 * c + i16) * p.Rp + (e0 & ~1L)) * 2);
          const unsigned u0 = q[0], u1 = q[1], u2 = q[2], u3 = q[3], u4 = q[4];
          uint4 u;
          if (e0 & 1) u = make_uint4(__builtin_amdgcn_alignbit(u1, u0, 16), __builtin_amdgcn_alignbit(u2, u1, 16),
                                     __builtin_amdgcn_alignbit(u3, u2, 16), __builtin_amdgcn_alignbit(u4, u3, 16));
          else u = make_uint4(u0, u1, u2, u3);
          bf16x8 vb;
          __builtin_memcpy(&vb, &u, 16);
#pragma unroll
          for (int a = 0; a < 3; ++a) acc[a][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va[a], vb, acc[a][c], 0, 0, 0);
        }
      }
    } else {
#pragma unroll
      for (int kc = 0; kc < 4; ++kc) {      // 16 k per step: lane group g holds value row ey = 2 kc + (g >> 1), columns 4 (g & 1) .. + 3
        f32x4 va[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) va[a] = *(const f32x4*)(Pt + (16 * a + i16) * PTLD + 16 * kc + 4 * g);
        const int sy = min(ky0 + 2 * kc + (g >> 1), p.hc - 1);
        const long e0 = (long)sy * p.wc + kx0 + 4 * (g & 1);
        f32x4 vb[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) vb[c] = *(const f32x4u*)(vbase + ((long)(16 * c + i16) * p.Rp + e0) * 4);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 6; ++c)
#pragma unroll
            for (int a = 0; a < 3; ++a) acc[a][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(va[a][r], vb[c][r], acc[a][c], 0, 0, 0);
      }
    }
  }
  // D[row 16 a + 4 g + reg][channel 16 c + i16] -> out[b][2 ry + py][2 rx + px][c], class w = (py, px)
  const int py = w >> 1, px = w & 1;
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ri = 16 * a + 4 * g + r;
      if (ri >= OB * OB) continue;
      const int ry = r0y + ri / OB, rx = r0x + ri % OB;
      if (ry >= p.hc || rx >= p.wc) continue;
      const long o = (((long)b * p.h + 2 * ry + py) * p.w + 2 * rx + px) * 96;
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        if (BF16) ((unsigned short*)p.out)[o + 16 * c + i16] = (unsigned short)(pack_bf16x2(acc[a][c][r], 0.f) & 0xffffu);
        else p.out[o + 16 * c + i16] = acc[a][c][r];
      }
    }
}

// Words of value tail the out pass may read past the last class-grid position of the last (image, class, channel) row of xT:
// a block at the right edge loads columns up to kx0 + 7 <= wc + 5 of the last row (plus one word of realignment in bf16).
int att_stream_xt_tail() { return 64; }

template <bool BF16>
static hipError_t launch_t(const AttParams& p0, hipStream_t st) {
  AttParams p = p0;
  p.sym = 0;      // keys xn = x rn, queries raw x
  p.guard = 0;    // no E: the preparation writes no guard bands
  hipError_t e = launch_att2_prep(p, st);
  if (e != hipSuccess) return e;
  // the tail behind xT is read (times P~ = 0): it must hold finite values
  {
    const size_t xt_bytes = (size_t)p.B * 4 * 96 * p.Rp * (BF16 ? 2 : 4);
    e = hipMemsetAsync((char*)p.xT + xt_bytes, 0, (size_t)att_stream_xt_tail() * 4, st);
    if (e != hipSuccess) return e;
  }
  const int nby = (p.hs + KB - 1) / KB, nbx = (p.ws + KB - 1) / KB;
  const int noy = (p.hc + OB - 1) / OB, nox = (p.wc + OB - 1) / OB;
  const double alg_flops = 2.0 * p.B * (double)p.L * p.L * 1536.0;
  const double gemm1 = 2.0 * 64 * 64 * 384;      // one E tile
  const double gemm2 = 2.0 * 48 * 64 * 384;      // one P~ . V step
  {
    const long grid = (long)p.B * nby * nbx;
    set_launch_cost(alg_flops, 0.0, nullptr, (double)grid * nby * nbx * gemm1);
    set_launch_grid(grid);
    ProfScope ps_(st, PL_ATT_STREAM_STATS);
    hipLaunchKernelGGL(att_stream_stats_kernel<BF16>, dim3((unsigned)grid), dim3(256), 0, st, p, nby, nbx);
  }
  {
    const long grid = (long)p.B * noy * nox;
    set_launch_cost(alg_flops, 0.0, nullptr, (double)grid * nby * nbx * (gemm1 + gemm2));
    set_launch_grid(grid);
    ProfScope ps_(st, PL_ATT_STREAM_OUT);
    hipLaunchKernelGGL(att_stream_out_kernel<BF16>, dim3((unsigned)grid), dim3(256), 0, st, p, nby, nbx, noy, nox);
  }
  return hipGetLastError();
}

hipError_t launch_attention_stream(const AttParams& p, hipStream_t st) {
  if (!p.xT || !p.stats || !p.kmul || !p.kadd || !p.validR || p.E || p.similar) return hipErrorInvalidValue;
  return p.bf16 ? launch_t<true>(p, st) : launch_t<false>(p, st);
}

}  // namespace se
