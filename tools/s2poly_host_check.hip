// Stand-alone host check of the polyphase F(2,2) form of the 48-channel stride-2 gated convs (sketchedit_amd/csrc/se_s2poly.h and its
// rule in se_dispatch.h), meant for a sanitizer build: its own main, no device, nothing loaded into an interpreter.  The rule, the
// tables and the packer are compiled into THIS program (instrumented); the library is linked for the switch table alone.
//   1. choose_form over a grid of sizes, batches, modes, nets and switch values: the form runs exactly where the rule says.
//   2. the tables: the 25 products of random 5x5 patches and 3x3 kernels, folded, equal the direct 2x2 outputs to 1e-12.
//   3. s2poly_pack_host for 96 and 192 rows: every element against the float64 model, every k written once, the k-half behind
//      position 24 zero, and the refusal of another width.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined tools/s2poly_host_check.hip \
//         -Lsketchedit_amd/lib -lsketchedit_hip -Wl,-rpath,$PWD/sketchedit_amd/lib -o s2poly_host_check && ./s2poly_host_check
#include "../include/sketchedit_hip.h"
#include "../sketchedit_amd/csrc/se_dispatch.h"
#include "../sketchedit_amd/csrc/se_s2poly.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

using namespace se;

static std::string answer(int cin, int cout, int stride, int rate, int B, int H, int W, int flags, int net) {
  const bool bf = (flags & SE_FLAG_BF16) != 0;
  const LayerDef d = {"check", cin, cout, 3, stride, rate, ACT_ELU, 0};
  const LayerFacts f = layer_facts(d, cin);
  const ConvCall q = {d, f, B, H, W, cin, 0, SRC2_NONE, bf, (flags & SE_FLAG_LOW_LATENCY) != 0, (flags & SE_FLAG_CONSERVATIVE) != 0, net, false};
  const Choice ch = choose_form(q);
  const char* name = form_name(ch, q);
  return name ? name : "?";
}

static int check_rule() {
  int bad = 0;
  long calls = 0;
  static const int SIZES[] = {1, 2, 3, 4, 7, 8, 12, 16, 17, 20, 64, 128, 255, 256, 1000, 1024, 4096, 30000};
  static const int FLAGSETS[] = {0, SE_FLAG_LOW_LATENCY, SE_FLAG_CONSERVATIVE, SE_FLAG_BF16, SE_FLAG_BF16 | SE_FLAG_LOW_LATENCY};
  for (int mode = 0; mode < 3; ++mode) {
    if (opt_set("SE_S2_POLY", mode)) { fprintf(stderr, "no switch SE_S2_POLY\n"); return 1; }
    for (int cin : {24, 48})
      for (int cout : {48, 96, 192})
        for (int stride : {1, 2})
          for (int rate : {1, 2})
            for (int H : SIZES)
              for (int W : SIZES)
                for (int B : {1, 3, 64, 4096})
                  for (int flags : FLAGSETS)
                    for (int net = 0; net < 2; ++net) {
                      const bool want = (mode == 1 || (mode == 2 && net == 0)) && cin == 48 && (cout == 96 || cout == 192) && stride == 2 && rate == 1 &&
                                        !(flags & (SE_FLAG_BF16 | SE_FLAG_LOW_LATENCY)) && H % 4 == 0 && W % 4 == 0 &&
                                        (double)B * H * W * 192.0 < 2147483648.0;
                      const std::string s = answer(cin, cout, stride, rate, B, H, W, flags, net);
                      ++calls;
                      if ((s == "s2poly48") != want || s.empty() || s.find('?') != std::string::npos) {
                        if (++bad < 10) fprintf(stderr, "rule: %d -> %d s%d d%d %dx%d B %d flags %d net %d mode %d: %s\n", cin, cout, stride, rate, H, W, B, flags, net, mode, s.c_str());
                      }
                    }
  }
  opt_reset();
  printf("rule: %ld calls, %d bad\n", calls, bad);
  return bad;
}

static int check_tables() {
  std::mt19937 rng(29);
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  double worst = 0.;
  int nsrc = 0;
  for (int q = 0; q < 5; ++q) nsrc += 1 + (s2poly_src_b(q) >= 0);
  for (int rep = 0; rep < 500; ++rep) {
    double g[3][3], p[5][5];
    for (auto& r : g) for (double& v : r) v = U(rng);
    for (auto& r : p) for (double& v : r) v = U(rng);
    if (rep % 5 == 0) for (int i = 0; i < 5; ++i) p[0][i] = p[i][0] = 0.;      // a border tile: the padding reads as zero
    double out[2][2] = {{0., 0.}, {0., 0.}};
    for (int pos = 0; pos < S2POLY_NPOS; ++pos) {
      const int py = pos / 5, px = pos % 5;
      const int ya = s2poly_src_a(py), yb = s2poly_src_b(py), xa = s2poly_src_a(px), xb = s2poly_src_b(px);
      double src = p[ya][xa];
      if (xb >= 0) src -= p[ya][xb];
      if (yb >= 0) src -= p[yb][xa];
      if (yb >= 0 && xb >= 0) src += p[yb][xb];
      double u = 0.;
      for (int ky = 0; ky < 3; ++ky)
        for (int kx = 0; kx < 3; ++kx) u += s2poly_wcoef(py, ky) * s2poly_wcoef(px, kx) * g[ky][kx];
      for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) out[a][b] += s2poly_fold(py, a) * s2poly_fold(px, b) * (src * u);
    }
    for (int a = 0; a < 2; ++a)
      for (int b = 0; b < 2; ++b) {
        double d = 0.;
        for (int ky = 0; ky < 3; ++ky)
          for (int kx = 0; kx < 3; ++kx) d += p[2 * a + ky][2 * b + kx] * g[ky][kx];
        worst = std::fmax(worst, std::fabs(d - out[a][b]));
      }
  }
  const int bad = (worst > 1e-12) + (nsrc * nsrc != 49);
  printf("tables: %d sources, worst |folded - direct| %.3g, %d bad\n", nsrc * nsrc, worst, bad);
  return bad;
}

static int check_packer() {
  int bad = 0;
  std::mt19937 rng(31);
  std::uniform_real_distribution<float> U(-0.07f, 0.07f);
  for (int cout : {96, 192}) {
    std::vector<float> w((size_t)cout * 48 * 9), b(cout), img, bias;
    for (float& v : w) v = U(rng);
    for (float& v : b) v = U(rng);
    if (!s2poly_pack_host(w.data(), b.data(), cout, img, bias)) { ++bad; continue; }
    if (img.size() != (size_t)(cout / 96) * S2POLY_NIT * 96 * 32 || bias.size() != (size_t)cout) { ++bad; continue; }
    std::vector<int> hits(img.size(), 0);
    long wrong = 0;
    for (int n = 0; n < cout; ++n) {
      const int f = n / 16 * 8 + n % 8, oc = n % 16 < 8 ? f : cout / 2 + f, r = n % 96;
      if (bias[n] != b[oc]) ++wrong;
      for (int ic = 0; ic < 48; ++ic)
        for (int pos = 0; pos < S2POLY_NPOS; ++pos) {
          const int py = pos / 5, px = pos % 5;
          double u = 0.;
          for (int ky = 0; ky < 3; ++ky)
            for (int kx = 0; kx < 3; ++kx) u += (double)(s2poly_wcoef(py, ky) * s2poly_wcoef(px, kx)) * (double)w[((size_t)oc * 48 + ic) * 9 + ky * 3 + kx];
          const int u6 = (pos & 1) * 3 + ic / 16, it = (pos >> 1) * 3 + u6 / 2, kin = (u6 % 2) * 16 + ic % 16;
          const size_t at = (((size_t)(n / 96) * S2POLY_NIT + it) * 96 + r) * 32 + (((kin / 4) ^ ((r >> 1) & 7)) * 4 + kin % 4);
          ++hits[at];
          if (img[at] != (float)u) ++wrong;
        }
    }
    long unwritten = 0;
    for (size_t i = 0; i < img.size(); ++i) {
      if (hits[i] > 1) ++wrong;
      if (hits[i] == 0) { ++unwritten; if (img[i] != 0.f) ++wrong; }
    }
    if (unwritten != (long)(cout / 96) * 96 * 16) ++wrong;
    printf("packer: %d rows, %zu floats, %ld unwritten (zero), %ld wrong\n", cout, img.size(), unwritten, wrong);
    bad += wrong != 0;
  }
  std::vector<float> w((size_t)48 * 48 * 9, 0.f), b(48, 0.f), img(3, 1.f), bias;
  if (s2poly_pack_host(w.data(), b.data(), 48, img, bias) || img.size() != 3) { ++bad; fprintf(stderr, "packer: 48 rows not refused\n"); }
  // ... and the library's own entry answers the same tables
  for (int q = 0; q < 5; ++q) {
    int t[7];
    for (int j = 0; j < 7; ++j) {
      char name[48];
      snprintf(name, sizeof name, "SE_S2POLY_TABLE:%d,%d", q, j);
      if (se_debug_get_option(name, &t[j])) ++bad;
    }
    if (t[0] != s2poly_src_a(q) || t[1] != s2poly_src_b(q) || t[2] != s2poly_wcoef(q, 0) || t[3] != s2poly_wcoef(q, 1) || t[4] != s2poly_wcoef(q, 2) ||
        t[5] != s2poly_fold(q, 0) || t[6] != s2poly_fold(q, 1)) ++bad;
  }
  return bad;
}

int main() {
  const int bad = check_rule() + check_tables() + check_packer();
  printf("%d bad\n", bad);
  return bad ? 1 : 0;
}
