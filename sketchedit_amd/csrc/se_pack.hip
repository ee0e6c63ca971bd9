// Weight packing (host only): a layer's checkpoint weights (OIHW) transformed, reordered and swizzled into the exact LDS
// image of every kernel form that may run it, and uploaded once at load.  Which images a layer gets, and their numbers, is
// layer_facts (se_dispatch.h): pack_layer_images builds those, and choose_form picks a form only where the facts name its image.
#include "se_pack.h"
#include "se_kernels.h"
#include "se_s2poly.h"

#include <cstring>

namespace se {
namespace {

// allocate `dst` and copy `host` into it (a reload replaces the previous image)
template <class V>
int upload(DevBuf& dst, const std::vector<V>& host, std::string& err) {
  const size_t bytes = host.size() * sizeof(V);
  hipError_t e = dst.alloc(bytes);
  if (e == hipSuccess) e = hipMemcpy(dst, host.data(), bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) return 0;
  err = std::string("weight image upload failed: ") + hipGetErrorString(e);
  return 1;
}

// fp32 -> bf16, round to nearest even (the rounding of v_cvt_pk_bf16_f32 and of torch's .to(bfloat16))
unsigned short bf16_bits(float f) {
  unsigned u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);   // NaN stays NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}
float bf16_round(float f) {
  const unsigned u = (unsigned)bf16_bits(f) << 16;
  float r;
  memcpy(&r, &u, 4);
  return r;
}

// MIXED row order: tile t = features 8t..8t+7, then their gates.  Checkpoint output channel of row n, or -1 past G
int mixed_row_channel(int n, int G) {
  const int f = n / 16 * 8 + n % 8;
  if (f >= G) return -1;
  return n % 16 < 8 ? f : G + f;
}

// checkpoint output channel of packed row n of configuration cfg (features [0,G), gates [G,2G)), or -1
int out_channel_of_row(int cfg, int n, int G) {
  if (gconv_mixed(cfg)) return mixed_row_channel(n, G);
  const int NF = gconv_np(cfg) / 32;  // feature tiles
  const int nt = n / 16, r = n % 16;
  if (nt < NF) { int f = nt * 16 + r; return f < G ? f : -1; }
  int g = (nt - NF) * 16 + r;
  return g < G ? G + g : -1;
}

// the bias of a Winograd image whose NP rows are in the MIXED order
std::vector<float> mixed_bias(const Layer& L, int NP) {
  std::vector<float> bias(NP);
  for (int n = 0; n < NP; ++n) bias[n] = L.b[mixed_row_channel(n, NP / 2)];
  return bias;
}

// offset of element e of 16-byte slot s in row n of a 128-byte row image (`per` elements per slot): slot s of row n is
// stored at slot s ^ ((n >> 1) & 7)
int swz(int n, int s, int e, int per = 4) { return (s ^ ((n >> 1) & 7)) * per + e; }

// gen_deconv (nearest x2 + 3x3) in its sub-pixel form: 4 output parity classes, each a 2x2 conv on the source grid; tap
// (a, b) of class (py, px) sums the kernel taps that land on source pixel (yy + a - 1 + py, xx + b - 1 + px):
//   py=0: a=0 <- {ky 0}, a=1 <- {ky 1,2};   py=1: a=0 <- {ky 0,1}, a=1 <- {ky 2}      (same for columns)
// g = the 3x3 kernel of one (out, in) pair; summed in fp32
float subpixel_tap(const float* g, int py, int px, int a, int b) {
  float v = 0.f;
  for (int ky = a == 0 ? 0 : 1 + py; ky <= (a == 0 ? py : 2); ++ky)
    for (int kx = b == 0 ? 0 : 1 + px; kx <= (b == 0 ? px : 2); ++kx) v += g[ky * 3 + kx];
  return v;
}

// F(2,3) filter transform in float: u[nu] = sum_k G[nu][k] g[k * stride]
void wino_f23(const float* g, int stride, float u[4]) {
  static const float Gm[4][3] = {{1.f, 0.f, 0.f}, {.5f, .5f, .5f}, {.5f, -.5f, .5f}, {0.f, 0.f, 1.f}};
  for (int nu = 0; nu < 4; ++nu) u[nu] = Gm[nu][0] * g[0] + Gm[nu][1] * g[stride] + Gm[nu][2] * g[2 * stride];
}
// F(2x2,3x3) in float: U = G g G^T of a row-major 3x3 kernel, U[xi][nu] (position xi * 4 + nu)
void wino_f22(const float* g, float U[4][4]) {
  float t[3][4];      // t[kx] = G applied down column kx
  for (int kx = 0; kx < 3; ++kx) wino_f23(g + kx, 3, t[kx]);
  for (int xi = 0; xi < 4; ++xi) {
    const float r[3] = {t[0][xi], t[1][xi], t[2][xi]};
    wino_f23(r, 1, U[xi]);
  }
}
// F(2x2,2x2) of a gen_deconv class (se_wino_up.hip): the pre-summed 2x2 taps g transformed with G = [1 0; 1 1; 0 1]:
// U = G g G^T, 3x3 positions
void winoup_class(const float* w9, int py, int px, float U[3][3]) {
  static const float Gm[3][2] = {{1.f, 0.f}, {1.f, 1.f}, {0.f, 1.f}};
  float g[2][2];
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b) g[a][b] = subpixel_tap(w9, py, px, a, b);
  for (int xi = 0; xi < 3; ++xi)
    for (int nu = 0; nu < 3; ++nu) {
      float u = 0.f;
      for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) u += Gm[xi][a] * Gm[nu][b] * g[a][b];
      U[xi][nu] = u;
    }
}

template <class E> E to_elem(float v);
template <> float to_elem<float>(float v) { return v; }
template <> unsigned short to_elem<unsigned short>(float v) { return bf16_bits(v); }

// The direct image of a gated conv with elements E (float: fp32, unsigned short: bf16): [class][chunk][NP][128 bytes], a
// chunk = 128 / sizeof(E) k-values of k = flattened (tap, packed input channel), a 16-byte slot = 16 / sizeof(E) of them,
// row n = packed output channel, slots swizzled (swz).  cin_map[pc] = checkpoint input channel of packed channel pc (a whole
// number of slots per tap), or -1 for zero padding.  gen_deconv is packed in its sub-pixel form, the sums formed in fp32 and
// rounded once.
template <class E>
int pack_direct(Layer& L, const std::vector<int>& cin_map, std::string& err) {
  constexpr int KC = 128 / sizeof(E), PER = 16 / sizeof(E), BF = sizeof(E) == 2;
  const LayerDef& d = L.def;
  const LayerFacts& f = L.facts;
  if (f.cfg < 0) {
    err = std::string("layer ") + d.name + ": unsupported gated width " + std::to_string(f.G);
    return 1;
  }
  const int cfg = f.cfg, G = f.G, NP = f.NP, nch = f.nch[BF];
  const int Cp = (int)cin_map.size();
  const bool up2 = d.up != 0;
  const int KW = up2 ? 2 : d.k, K = f.T * Cp, ncls = up2 ? 4 : 1;
  std::vector<E> img((size_t)ncls * nch * NP * KC, E(0));
  for (int cls = 0; cls < ncls; ++cls)
    for (int n = 0; n < NP; ++n) {
      const int oc = out_channel_of_row(cfg, n, G);
      if (oc < 0) continue;
      for (int kf = 0; kf < K; ++kf) {
        const int tap = kf / Cp, ic = cin_map[kf % Cp];
        if (ic < 0) continue;
        const int ty = tap / KW, tx = tap % KW, kin = kf % KC;
        const float* g = &L.w[((size_t)oc * d.cin + ic) * d.k * d.k];
        const float v = up2 ? subpixel_tap(g, cls >> 1, cls & 1, ty, tx) : g[ty * d.k + tx];
        img[(((size_t)cls * nch + kf / KC) * NP + n) * KC + swz(n, kin / PER, kin % PER, PER)] = to_elem<E>(v);
      }
    }
  return upload(L.direct[BF], img, err);
}

int pack_wino(Layer& L, std::string& err);
int pack_wino24(Layer& L, std::string& err);
int pack_rtilew(Layer& L, std::string& err);
int pack_wino48(Layer& L, std::string& err);
int pack_wino48_c24(Layer& L, std::string& err);
int pack_winoup(Layer& L, std::string& err);
int pack_winoup48(Layer& L, std::string& err);

// fp32 direct image (cin_map: a multiple of 4 channels per tap) and its bias, then the Winograd-type image the facts name,
// in the layout of the kernel that runs a layer of this width
int pack_layer(Layer& L, const std::vector<int>& cin_map, std::string& err) {
  const LayerDef& d = L.def;
  const LayerFacts& f = L.facts;
  if (pack_direct<float>(L, cin_map, err)) return 1;
  std::vector<float> bias(f.NP, 0.f);
  for (int n = 0; n < f.NP; ++n) {
    const int oc = out_channel_of_row(f.cfg, n, f.G);
    if (oc >= 0) bias[n] = L.b[oc];
  }
  if (upload(L.d_b, bias, err)) return 1;
  L.packed = true;
  if (f.u && d.up) return d.cin == 96 ? pack_winoup(L, err) : pack_winoup48(L, err);
  if (f.u && f.u24) return pack_wino(L, err);                                       // ... and pack_wino24
  if (f.u24) return pack_wino24(L, err);                                            // xconv5
  if (f.wx) return pack_rtilew(L, err);                                             // conv16
  if (f.u) return d.cin == 48 ? pack_wino48(L, err) : pack_wino48_c24(L, err);      // (24: xconv3, pmconv3)
  return 0;
}

// dense_kin: j-th k of a chunk -> k-step j / 4, lane group j % 4 (instruction-major).  In the last chunk that packs the
// real k into the first k-steps (the others are not issued); in every chunk it makes the four lane groups of one
// k-step read four CONSECUTIVE dwords of the dense tile (bank-conflict-free; k-major order: 32-50 % conflict cycles)
int dense_kin(int j) {
  const int step = j / 4;
  return (step / 4) * 16 + (j % 4) * 4 + step % 4;
}

// Dense-K image of a 5x5 first layer (se_rtile.hip rtile_dense5_kernel): k = tap * Cd + channel over the Cd channels the
// stored input really carries (cin_map[pc] = checkpoint input channel of stored channel pc), no channel padding; in the
// last chunk the real k are packed instruction-major (dense_kin), so the kernel issues exactly ceil(K / 4) MFMA k-steps.
// Rows in the MIXED order of the N=48 configuration, slot swizzle as pack_layer.
int pack_layer_dense(Layer& L, const std::vector<int>& cin_map, std::string& err) {
  const LayerDef& d = L.def;
  const int Cd = L.facts.dense;
  const int G = d.cout / 2, NP = 48, T = d.k * d.k, K = T * Cd, nch = L.facts.nchd;
  std::vector<float> img((size_t)nch * NP * 32, 0.f);
  for (int n = 0; n < NP; ++n) {
    const int oc = out_channel_of_row(GC_N48, n, G);
    if (oc < 0) continue;
    for (int kf = 0; kf < K; ++kf) {
      const int tap = kf / Cd, ic = cin_map[kf % Cd], ty = tap / d.k, tx = tap % d.k;
      const int kin = dense_kin(kf % 32);
      img[((size_t)(kf / 32) * NP + n) * 32 + swz(n, kin / 4, kin % 4)] = L.w[(((size_t)oc * d.cin + ic) * d.k + ty) * d.k + tx];
    }
  }
  if (upload(L.d_wd, img, err)) return 1;
  // F(2,5)-along-x form (rtile_dense5w_kernel): U[nu][ky][c] = sum_kx Gx[nu][kx] w[ky][kx], formed in double; one chunk
  // per position with k = ky * Cd + c in the same instruction-major order
  static const double Gx[6][5] = {{1. / 4, 0., 0., 0., 0.}, {-1. / 6, -1. / 6, -1. / 6, -1. / 6, -1. / 6}, {-1. / 6, 1. / 6, -1. / 6, 1. / 6, -1. / 6},
                                  {1. / 24, 1. / 12, 1. / 6, 1. / 3, 2. / 3}, {1. / 24, -1. / 12, 1. / 6, -1. / 3, 2. / 3}, {0., 0., 0., 0., 1.}};
  std::vector<float> imw((size_t)6 * NP * 32, 0.f);
  for (int n = 0; n < NP; ++n) {
    const int oc = out_channel_of_row(GC_N48, n, G);
    if (oc < 0) continue;
    for (int j = 0; j < 5 * Cd; ++j) {
      const int ky = j / Cd, ic = cin_map[j % Cd];
      const float* g = &L.w[(((size_t)oc * d.cin + ic) * 5 + ky) * 5];
      const int kin = dense_kin(j);
      for (int nu = 0; nu < 6; ++nu) {
        double u = 0.;
        for (int kx = 0; kx < 5; ++kx) u += Gx[nu][kx] * (double)g[kx];
        imw[((size_t)nu * NP + n) * 32 + swz(n, kin / 4, kin % 4)] = (float)u;
      }
    }
  }
  return upload(L.d_wdw, imw, err);
}

// bf16 pair-of-taps image of a 5x5 first layer whose stored NHWC8 input carries at most four real channels (rtile_kernel<3, 8,
// true, true>): granule gi = 3 ky + j (j = 0..2) holds the taps (ky, 2j) and (ky, 2j + 1) x stored channels 0-3, i.e. element
// e = 4 (kx & 1) + c; kx = 5 does not exist (zero).  15 granules -> 2 chunks of 64 k; rows in the MIXED N=48 order, slot swizzle
// as the bf16 direct image.  cin4[c] = checkpoint input channel of stored channel c, or -1.
int pack_layer16_d4(Layer& L, const std::vector<int>& cin4, std::string& err) {
  const LayerDef& d = L.def;
  const int G = d.cout / 2, NP = 48, nch = 2;
  std::vector<unsigned short> img((size_t)nch * NP * 64, 0);
  for (int n = 0; n < NP; ++n) {
    const int oc = out_channel_of_row(GC_N48, n, G);
    if (oc < 0) continue;
    for (int ky = 0; ky < 5; ++ky)
      for (int kx = 0; kx < 5; ++kx)
        for (int cc = 0; cc < 4; ++cc) {
          const int ic = cin4[cc];
          if (ic < 0) continue;
          const int gi = 3 * ky + kx / 2, e = 4 * (kx & 1) + cc;
          img[((size_t)(gi / 8) * NP + n) * 64 + swz(n, gi % 8, e, 8)] = bf16_bits(L.w[(((size_t)oc * d.cin + ic) * 5 + ky) * 5 + kx]);
        }
  }
  return upload(L.d_w16d, img, err);
}

// bf16 image for rconv16b_kernel (96 -> 192, 3x3): [27 steps = tap * 3 + 32-channel group][12 row tiles][16 rows][32 k],
// rows in the N=192 order (features, then gates); granule g (8 k) of row r at slot g ^ F[r >> 2], F = {0, 2, 3, 1}.
int pack_rconv16(Layer& L, std::string& err) {
  const LayerDef& d = L.def;
  static const int F[4] = {0, 2, 3, 1};
  std::vector<unsigned short> img((size_t)27 * 192 * 32, 0);
  for (int n = 0; n < 192; ++n) {
    const int oc = out_channel_of_row(GC_N192, n, 96);
    const int rt = n / 16, r = n % 16;
    for (int s = 0; s < 27; ++s) {
      const int tap = s / 3, kk = s % 3, ty = tap / 3, tx = tap % 3;
      for (int e = 0; e < 32; ++e) {
        const int ic = kk * 32 + e, g = e / 8;
        const float v = L.w[(((size_t)oc * d.cin + ic) * 3 + ty) * 3 + tx];
        img[((size_t)s * 12 + rt) * 512 + r * 32 + ((g ^ F[r >> 2]) * 8) + (e % 8)] = bf16_bits(v);
      }
    }
  }
  return upload(L.d_w16s, img, err);
}

// bf16 image for rconv96_kernel (96 packed rows: 3x3 24/48 -> 96, gen_deconv 96 -> 96):
// [class][step][6 row tiles][16 rows][32 k], k = granule (8 channels) index tap * CG + cg, four granules per step; rows in
// the N=96 order (features, then gates); granule g of row r at slot g ^ F[r >> 2], F = {0, 2, 3, 1}.
int pack_rconv96(Layer& L, std::string& err) {
  const LayerDef& d = L.def;
  static const int F[4] = {0, 2, 3, 1};
  const bool up2 = d.up != 0;
  const int KW = up2 ? 2 : 3, T = KW * KW, CG = d.cin / 8, NG = T * CG, nstep = (NG + 3) / 4, ncls = up2 ? 4 : 1;
  std::vector<unsigned short> img((size_t)ncls * nstep * 96 * 32, 0);
  for (int cls = 0; cls < ncls; ++cls)
    for (int n = 0; n < 96; ++n) {
      const int oc = out_channel_of_row(GC_N96, n, 48);
      const int rt = n / 16, r = n % 16;
      for (int gi = 0; gi < NG; ++gi) {
        const int tap = gi / CG, cg = gi % CG, ty = tap / KW, tx = tap % KW, s_ = gi / 4, g = gi % 4;
        for (int e = 0; e < 8; ++e) {
          const float* w9 = &L.w[((size_t)oc * d.cin + cg * 8 + e) * 9];
          const float v = up2 ? subpixel_tap(w9, cls >> 1, cls & 1, ty, tx) : w9[ty * 3 + tx];
          img[(((size_t)cls * nstep + s_) * 6 + rt) * 512 + r * 32 + ((g ^ F[r >> 2]) * 8) + e] = bf16_bits(v);
        }
      }
    }
  return upload(L.d_w96, img, err);
}

// Winograd F(2x2,3x3) weights: U[pos] = (G g G^T)[xi][nu] per (out, in) pair, packed per position like a 1x1
// conv Cin -> 192 (Cin = 96, or 192 for the two-source layers) in the N=192 row order (features then gates)
// with the same slot swizzle.
int pack_wino(Layer& L, std::string& err) {
  const LayerDef& d = L.def;
  const int NP = 192, nch = d.cin / 32;
  std::vector<float> img((size_t)16 * nch * NP * 32, 0.f);
  for (int n = 0; n < NP; ++n) {
    const int oc = out_channel_of_row(GC_N192, n, 96);
    for (int ic = 0; ic < d.cin; ++ic) {
      float U[4][4];
      wino_f22(&L.w[((size_t)oc * d.cin + ic) * 9], U);
      for (int pos = 0; pos < 16; ++pos)
        img[(((size_t)pos * nch + ic / 32) * NP + n) * 32 + swz(n, ic % 32 / 4, ic % 4)] = U[pos >> 2][pos & 3];
    }
  }
  if (upload(L.d_u, img, err)) return 1;
  if (L.facts.u1) {
    // for a spatially constant second source (conv11 of netG: the pooled style vector) the layer runs as the single-source
    // kernel on the first 96 channels plus a per-image bias table (launch_vecbias): the first source's Winograd image
    // ([16 positions][3 chunks][192][32], the first three chunks of every position of `img`) and the second source's
    // DIRECT weights [tap][channel][packed row]
    std::vector<float> img1((size_t)16 * 3 * NP * 32), wv((size_t)9 * 96 * NP);
    for (int pos = 0; pos < 16; ++pos)
      memcpy(&img1[(size_t)pos * 3 * NP * 32], &img[(size_t)pos * nch * NP * 32], (size_t)3 * NP * 32 * 4);
    for (int n = 0; n < NP; ++n) {
      const int oc = out_channel_of_row(GC_N192, n, 96);
      for (int t = 0; t < 9; ++t)
        for (int ch = 0; ch < 96; ++ch) wv[((size_t)t * 96 + ch) * NP + n] = L.w[((size_t)oc * d.cin + 96 + ch) * 9 + t];
    }
    if (upload(L.d_u1, img1, err) || upload(L.d_wv, wv, err)) return 1;
    for (auto& v : wv) v = bf16_round(v);
    if (upload(L.d_wv16, wv, err)) return 1;
  }
  return pack_wino24(L, err);
}

// 24 -> 24 layers (se_rtilew.hip): U[nu][ky] = G g[ky][.] with the F(2,3) G along x; k = ky * 24 + channel in three 32-k
// chunks per position (72 k, the third chunk half empty), 24 PHYSICAL rows -- tile 0 = features 0-7, gates 0-7; then
// features 8-11, gates 8-11 (the padding rows of the second MIXED tile read these again) --, slot swizzle by physical row.
// Two-dimensional form: U = G g G^T per position; a row holds its 24 k as channels 0-15 in slots 0-3 and channels
// 16 + 2q, 17 + 2q in slot 4 + q, elements 0, 1 for even q and 2, 3 for odd q (k-half 1 issues two k-steps; the halves keep
// the 8-byte fragment reads of lane groups q, q ^ 1 off each other's banks, se_rtilew.hip)
int pack_rtilew(Layer& L, std::string& err) {
  const LayerDef& d = L.def;
  const int G = d.cout / 2;      // 12
  std::vector<float> img((size_t)4 * 3 * 24 * 32, 0.f), img2((size_t)16 * 24 * 32, 0.f);
  for (int prow = 0; prow < 24; ++prow) {
    const int oc = prow < 8 ? prow : prow < 16 ? G + (prow - 8) : prow < 20 ? 8 + (prow - 16) : G + 8 + (prow - 20);
    for (int ic = 0; ic < 24; ++ic) {
      const float* g = &L.w[((size_t)oc * d.cin + ic) * 9];
      for (int ky = 0; ky < 3; ++ky) {
        float u[4];
        wino_f23(g + 3 * ky, 1, u);
        const int k = ky * 24 + ic;
        for (int nu = 0; nu < 4; ++nu) img[(((size_t)nu * 3 + k / 32) * 24 + prow) * 32 + swz(prow, k % 32 / 4, k % 4)] = u[nu];
      }
      float U[4][4];
      wino_f22(g, U);
      const int s_ = ic < 16 ? ic / 4 : 4 + (ic - 16) / 2, e = ic < 16 ? ic % 4 : (ic - 16) % 2 + 2 * (((ic - 16) / 2) & 1);
      for (int pos = 0; pos < 16; ++pos) img2[((size_t)pos * 24 + prow) * 32 + swz(prow, s_, e)] = U[pos >> 2][pos & 3];
    }
  }
  if (upload(L.d_wx, img, err)) return 1;
  return upload(L.d_wx2, img2, err);
}

// Hybrid F(2,3) x F(4,3) image of the same layers (se_wino24.hip): U = Gy g Gx^T (4 x 6 positions) of the FIRST 96 input
// channels, 72 iterations in the kernel's order -- stage (xi, h) -> chunk -> j with column position nu = {0,1,2}[j] (h = 0)
// or {5,3,4}[j] (h = 1) --, 192 rows in the MIXED order, slot swizzle as everywhere.  U is formed in double and rounded once
// (Gx holds 1/6, 1/12, 1/24).
int pack_wino24(Layer& L, std::string& err) {
  const LayerDef& d = L.def;
  static const double Gy[4][3] = {{1., 0., 0.}, {.5, .5, .5}, {.5, -.5, .5}, {0., 0., 1.}};
  static const double Gx[6][3] = {{1. / 4, 0., 0.}, {-1. / 6, -1. / 6, -1. / 6}, {-1. / 6, 1. / 6, -1. / 6},
                                  {1. / 24, 1. / 12, 1. / 6}, {1. / 24, -1. / 12, 1. / 6}, {0., 0., 1.}};
  static const int NU[2][3] = {{0, 1, 2}, {5, 3, 4}};
  const int NP = 192;
  // two images for the two-source layers: the first source alone (vector source folded into a bias: conv11) and both
  // sources (allconv11: 6 chunks per position)
  // (a 48-channel layer -- xconv5 -- has one image of 2 chunks per position, the second half empty)
  const int nchk_first = d.cin == 48 ? 2 : 3, nchk_last = L.facts.u24b ? 6 : nchk_first;
  for (int nchk = nchk_first; nchk <= nchk_last; nchk += 3) {
    std::vector<float> img((size_t)24 * nchk * NP * 32, 0.f);
    for (int n = 0; n < NP; ++n) {
      const int oc = mixed_row_channel(n, 96);
      for (int ic = 0; ic < nchk * 32 && ic < d.cin; ++ic) {
        const float* g = &L.w[((size_t)oc * d.cin + ic) * 9];
        double tt[4][3];
        for (int i = 0; i < 4; ++i)
          for (int kx = 0; kx < 3; ++kx) tt[i][kx] = Gy[i][0] * g[kx] + Gy[i][1] * g[3 + kx] + Gy[i][2] * g[6 + kx];
        for (int xi = 0; xi < 4; ++xi)
          for (int h = 0; h < 2; ++h)
            for (int j = 0; j < 3; ++j) {
              const int nu = NU[h][j];
              const double u = tt[xi][0] * Gx[nu][0] + tt[xi][1] * Gx[nu][1] + tt[xi][2] * Gx[nu][2];
              const int it = ((xi * 2 + h) * nchk + ic / 32) * 3 + j;
              img[((size_t)it * NP + n) * 32 + swz(n, ic % 32 / 4, ic % 4)] = (float)u;
            }
      }
    }
    if (upload(nchk <= 3 ? L.d_u24 : L.d_u24b, img, err)) return 1;
    if (nchk <= 3 && upload(L.d_ub24, mixed_bias(L, NP), err)) return 1;
  }
  return 0;
}

// 48 -> 96 layers (se_wino48.hip): 24 iterations = 8 position pairs x 3 chunks; chunk c of pair pp holds in its
// k-half h the 16-channel group ((2c+h) % 3) of position 2pp + ((2c+h) >= 3).  Rows in the MIXED order.
int pack_wino48(Layer& L, std::string& err) {
  const LayerDef& d = L.def;
  const int NP = 96;
  std::vector<float> img((size_t)24 * NP * 32, 0.f);
  for (int n = 0; n < NP; ++n) {
    const int oc = mixed_row_channel(n, 48);
    for (int ic = 0; ic < 48; ++ic) {
      float U[4][4];
      wino_f22(&L.w[((size_t)oc * d.cin + ic) * 9], U);
      for (int pos = 0; pos < 16; ++pos) {
        const int pp = pos >> 1, u6 = (pos & 1) * 3 + ic / 16;        // index of the 16-channel group in the pair
        const int it = pp * 3 + u6 / 2, kin = (u6 % 2) * 16 + ic % 16;
        img[((size_t)it * NP + n) * 32 + swz(n, kin / 4, kin % 4)] = U[pos >> 2][pos & 3];
      }
    }
  }
  if (upload(L.d_u, img, err)) return 1;
  return upload(L.d_ub, mixed_bias(L, NP), err);
}

// 24 -> 96 layers on the same kernel (se_wino48.hip, CIN = 24): one iteration per position, U[pos] as a [96 MIXED rows][32 k]
// tile: channels 0-15 in slots 0-3, channels 16 + 2q, 17 + 2q in elements 0, 1 of slot 4 + q (k-half 1 issues two k-steps:
// a k-step takes one element of every slot), elements 2, 3 zero.
int pack_wino48_c24(Layer& L, std::string& err) {
  const LayerDef& d = L.def;
  const int NP = 96;
  std::vector<float> img((size_t)16 * NP * 32, 0.f);
  for (int n = 0; n < NP; ++n) {
    const int oc = mixed_row_channel(n, 48);
    for (int ic = 0; ic < 24; ++ic) {
      float U[4][4];
      wino_f22(&L.w[((size_t)oc * d.cin + ic) * 9], U);
      const int s_ = ic < 16 ? ic / 4 : 4 + (ic - 16) / 2, e = ic < 16 ? ic % 4 : (ic - 16) % 2;
      for (int pos = 0; pos < 16; ++pos) img[((size_t)pos * NP + n) * 32 + swz(n, s_, e)] = U[pos >> 2][pos & 3];
    }
  }
  if (upload(L.d_u, img, err)) return 1;
  return upload(L.d_ub, mixed_bias(L, NP), err);
}

// gen_deconv 96 -> 96 (se_wino_up.hip): per output parity class U = G g G^T of the pre-summed 2x2 weights (winoup_class),
// 27 iterations = 9 positions x 3 chunks of 32 channels, rows in the MIXED order.
int pack_winoup(Layer& L, std::string& err) {
  const LayerDef& d = L.def;
  const int NP = 96;
  std::vector<float> img((size_t)4 * 27 * NP * 32, 0.f);
  for (int cls = 0; cls < 4; ++cls)
    for (int n = 0; n < NP; ++n) {
      const int oc = mixed_row_channel(n, 48);
      for (int ic = 0; ic < 96; ++ic) {
        float U[3][3];
        winoup_class(&L.w[((size_t)oc * d.cin + ic) * 9], cls >> 1, cls & 1, U);
        for (int xi = 0; xi < 3; ++xi)
          for (int nu = 0; nu < 3; ++nu) {
            const int it = (xi * 3 + nu) * 3 + ic / 32, kin = ic % 32;
            img[(((size_t)cls * 27 + it) * NP + n) * 32 + swz(n, kin / 4, kin % 4)] = U[xi][nu];
          }
      }
    }
  if (upload(L.d_u, img, err)) return 1;
  return upload(L.d_ub, mixed_bias(L, NP), err);
}

// gen_deconv 48 -> 48 (se_wino_up48.hip): U = G g G^T per class as above; 14 iterations in the pairing of pack_wino48
// (chunk c of pair pp holds in k-half h the 16-channel group ((2c+h) % 3) of position 2pp + ((2c+h) >= 3)); position 8
// has no partner: the second k-half of iteration 13 stays zero.  48 rows in the MIXED order (8 features + their gates).
int pack_winoup48(Layer& L, std::string& err) {
  const LayerDef& d = L.def;
  const int NP = 48, NIT = 14;
  std::vector<float> img((size_t)4 * NIT * NP * 32, 0.f);
  for (int cls = 0; cls < 4; ++cls)
    for (int n = 0; n < NP; ++n) {
      const int oc = mixed_row_channel(n, 24);
      for (int ic = 0; ic < 48; ++ic) {
        float U[3][3];
        winoup_class(&L.w[((size_t)oc * d.cin + ic) * 9], cls >> 1, cls & 1, U);
        for (int pos = 0; pos < 9; ++pos) {
          const int pp = pos >> 1, u6 = (pos & 1) * 3 + ic / 16;        // index of the 16-channel group in the pair
          const int it = pp * 3 + u6 / 2, kin = (u6 % 2) * 16 + ic % 16;
          img[(((size_t)cls * NIT + it) * NP + n) * 32 + swz(n, kin / 4, kin % 4)] = U[pos / 3][pos % 3];
        }
      }
    }
  if (upload(L.d_u, img, err)) return 1;
  return upload(L.d_ub, mixed_bias(L, NP), err);
}

// 3x3 stride 2, 48 -> 96 / 192 (se_s2poly.hip): the polyphase F(2,2) image and its bias, as s2poly_pack_host (se_s2poly.h) lays
// them out
int pack_s2poly48(Layer& L, std::string& err) {
  const LayerDef& d = L.def;
  std::vector<float> img, bias;
  if (d.cin != 48 || (int)L.w.size() != d.cout * 48 * 9 || !s2poly_pack_host(L.w.data(), L.b.data(), d.cout, img, bias)) {
    err = std::string("layer ") + d.name + ": no polyphase image for this shape";
    return 1;
  }
  if (upload(L.d_s2p, img, err)) return 1;
  return upload(L.d_s2pb, bias, err);
}

// raw 3x3 conv 12 -> cout: [cout][9][12]; the bf16 mode runs the same fp32 kernel with bf16-rounded weights (every conv
// weight is rounded in that mode)
int pack_small(Layer& L, std::string& err) {
  const LayerDef& d = L.def;
  std::vector<float> img((size_t)d.cout * 9 * 12);
  for (int oc = 0; oc < d.cout; ++oc)
    for (int t = 0; t < 9; ++t)
      for (int ic = 0; ic < 12; ++ic) img[((size_t)oc * 9 + t) * 12 + ic] = L.w[(((size_t)oc * 12 + ic) * 3 + t / 3) * 3 + t % 3];
  if (upload(L.direct[0], img, err) || upload(L.d_b, L.b, err)) return 1;
  for (auto& v : img) v = bf16_round(v);
  if (upload(L.direct[1], img, err)) return 1;
  L.packed = true;
  return 0;
}

// the images of a gated layer, as L.facts names them
int pack_gated(Layer& L, const std::vector<int>& chans, std::string& err) {
  const LayerFacts& f = L.facts;
  const int nc = (int)chans.size();
  auto padded = [&](int per) {      // the stored channels padded to whole granules of `per`
    std::vector<int> m(chans);
    m.resize((nc + per - 1) / per * per, -1);
    return m;
  };
  // bf16: conv16's 12 gated outputs are stored with a 16-channel stride, so conv17 is not a gated layer and everything
  // else reads whole granules
  if (pack_direct<unsigned short>(L, padded(8), err)) return 1;
  if (f.w16d && pack_layer16_d4(L, padded(4), err)) return 1;
  if (f.w16s && pack_rconv16(L, err)) return 1;
  if (f.w96 && pack_rconv96(L, err)) return 1;
  if (f.wd && pack_layer_dense(L, chans, err)) return 1;
  if (f.s2p) {      // (48 stored channels that are the layer's 48, in order: layer_facts counts them, the identity is checked here)
    for (int i = 0; i < nc; ++i)
      if (chans[i] != i) { err = std::string("layer ") + L.def.name + ": the polyphase image needs its input channels in checkpoint order"; return 1; }
    if (pack_s2poly48(L, err)) return 1;
  }
  return pack_layer(L, padded(4), err);
}

}  // namespace

int pack_layer_images(Layer& L, const std::vector<int>& chans, std::string& err) {
  const LayerFacts f = L.facts = layer_facts(L.def, (int)chans.size());
  if (f.small ? pack_small(L, err) : pack_gated(L, chans, err)) return 1;
  // the images that exist are the images the facts name: choose_form decides on the facts, the launchers read the images
  const struct { const char* name; const float* img; bool fact; } have[] = {
      {"u", L.d_u, f.u}, {"ub", L.d_ub, f.ub}, {"u1", L.d_u1, f.u1}, {"wv", L.d_wv, f.wv}, {"wv16", L.d_wv16, f.wv16},
      {"u24", L.d_u24, f.u24}, {"ub24", L.d_ub24, f.ub24}, {"u24b", L.d_u24b, f.u24b}, {"wx", L.d_wx, f.wx}, {"wx2", L.d_wx2, f.wx2},
      {"wd", L.d_wd, f.wd}, {"wdw", L.d_wdw, f.wdw}, {"w16d", L.d_w16d, f.w16d}, {"w16s", L.d_w16s, f.w16s}, {"w96", L.d_w96, f.w96},
      {"s2p", L.d_s2p, f.s2p}, {"s2pb", L.d_s2pb, f.s2p}};
  for (const auto& h : have)
    if ((h.img != nullptr) != h.fact) {
      err = std::string("layer ") + L.def.name + ": weight image " + h.name + (h.fact ? " is missing" : " was built against the layer's facts");
      return 1;
    }
  return 0;
}

}  // namespace se
