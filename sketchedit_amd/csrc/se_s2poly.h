// The polyphase F(2,2) form of a 3x3 stride-2 conv with padding 1 (se_s2poly.hip), its tables in ONE place: the kernel's source
// offsets and fold, the weight packer (se_pack.hip) and the host checks (se_debug_get_option's SE_S2POLY_* entries, tools/s2poly_host_check.hip) read these.
// 1-D, per output pair o0 = out[2t], o1 = out[2t+1] over the patch i_m = in[4t+m], m = -1..3 (patch index m + 1 = 0..4):
//     q   source         1-D weight   folds into
//     0   i0             w1           +o0
//     1   i2             w1           +o1
//     2   i-1 - i1       w0           +o0
//     3   i1             w0 + w2      +o0 +o1
//     4   i1 - i3        w2           -o1
// Two-dimensional: position pos = 5 py + px, source / weight / fold the outer products of row py and column px.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <vector>

namespace se {

constexpr int S2POLY_NPOS = 25;      // positions
constexpr int S2POLY_NIT = 38;       // 32-k chunks of a 48-channel layer: 12 position pairs x 3 + chunks A, B of the pair (24, -)

// patch index of the source that enters with +, and of the one that enters with - (-1: none)
__host__ __device__ constexpr int s2poly_src_a(int q) { return q == 0 ? 1 : q == 1 ? 3 : q == 2 ? 0 : 2; }
__host__ __device__ constexpr int s2poly_src_b(int q) { return q == 2 ? 2 : q == 4 ? 4 : -1; }
// coefficient of 1-D tap k (0..2) in the weight of position q
__host__ __device__ constexpr int s2poly_wcoef(int q, int k) { return q < 2 ? k == 1 : q == 2 ? k == 0 : q == 3 ? k != 1 : k == 2; }
// coefficient of position q's product in output o (0, 1) of the pair
__host__ __device__ constexpr int s2poly_fold(int q, int o) {
  return o == 0 ? (q == 0 || q == 2 || q == 3 ? 1 : 0) : (q == 1 || q == 3 ? 1 : q == 4 ? -1 : 0);
}

// ---- the weight image, on the host alone (no device, no allocation but the two vectors) ----
// The image of a 3x3 stride-2 layer 48 -> cout (cout 96 or 192; w OIHW with cin 48, b [cout]):
//   img  [cout / 96 halves][38 iterations][96 rows][32 k], the layer's rows in the MIXED order (tile t = features 8t..8t+7, then
//        their gates), slot s of row n stored at slot s ^ ((n >> 1) & 7); chunk c of pair pp holds in its k-half h the 16-channel
//        group (2c + h) % 3 of position 2 pp + ((2c + h) >= 3) (se_wino48.hip); the k-half behind position 24 stays zero.
//        The weight of position (py, px) is the outer product of the two 1-D rows on the 3x3 kernel, in double, rounded once.
//   bias [cout] in the same row order.
// Returns false (nothing written) for another cout.
inline bool s2poly_pack_host(const float* w, const float* b, int cout, std::vector<float>& img, std::vector<float>& bias) {
  if (cout != 96 && cout != 192) return false;
  const int NP = cout, G = cout / 2;
  img.assign((size_t)(NP / 96) * S2POLY_NIT * 96 * 32, 0.f);
  bias.assign((size_t)NP, 0.f);
  for (int n = 0; n < NP; ++n) {
    const int f = n / 16 * 8 + n % 8, oc = n % 16 < 8 ? f : G + f;      // MIXED row n -> checkpoint output channel
    const int hf = n / 96, r = n % 96;
    bias[n] = b[oc];
    for (int ic = 0; ic < 48; ++ic) {
      const float* g = w + ((size_t)oc * 48 + ic) * 9;
      for (int pos = 0; pos < S2POLY_NPOS; ++pos) {
        const int py = pos / 5, px = pos % 5;
        double u = 0.;
        for (int ky = 0; ky < 3; ++ky)
          for (int kx = 0; kx < 3; ++kx) u += (double)(s2poly_wcoef(py, ky) * s2poly_wcoef(px, kx)) * (double)g[ky * 3 + kx];
        const int pp = pos >> 1, u6 = (pos & 1) * 3 + ic / 16;      // index of the 16-channel group in the pair
        const int it = pp * 3 + u6 / 2, kin = (u6 % 2) * 16 + ic % 16;
        const int slot = (kin / 4) ^ ((r >> 1) & 7);
        img[(((size_t)hf * S2POLY_NIT + it) * 96 + r) * 32 + slot * 4 + kin % 4] = (float)u;
      }
    }
  }
  return true;
}

}  // namespace se
