// Stand-alone host check of the form chooser (sketchedit_amd/csrc/se_dispatch.h), meant for a sanitizer build: its own main,
// no device, nothing loaded into an interpreter.  Reads one call per line from stdin,
//   cin cin1 vector cout k stride rate act up B H W exec_flags net expected [SE_SWITCH=value ...]
// and holds two answers against `expected` (comma-separated form names): choose_form / form_name compiled into THIS program
// (instrumented), and se_debug_gconv_form of the library it links.  Then it walks choose_form over a grid of layers, sizes and
// modes no table lists (odd and huge sizes, every layer shape of the two networks), where only the sanitizers judge.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined tools/dispatch_host_check.hip \
//         -Lsketchedit_amd/lib -lsketchedit_hip -Wl,-rpath,$PWD/sketchedit_amd/lib -o dispatch_host_check
//   PYTHONPATH=tests python -c "import forms_util as F; F.dump_rows()" | ./dispatch_host_check
#include "../include/sketchedit_hip.h"
#include "../sketchedit_amd/csrc/se_dispatch.h"

#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>

using namespace se;

static std::string answer(int cin, int cin1, int vec, int cout, int k, int stride, int rate, int act, int up, int B, int H, int W, int flags,
                          int net) {
  const bool bf = (flags & SE_FLAG_BF16) != 0;
  const int gran = bf ? 8 : 4, Cp = (cin + gran - 1) & ~(gran - 1);
  const LayerDef d = {"check", cin + cin1, cout, k, stride, rate, act, up};
  const LayerFacts f = layer_facts(d, cin + cin1);
  const bool v = cin1 && vec;
  const ConvCall q = {d, f, B, H, W, Cp, cin1, cin1 ? (v ? SRC2_VECTOR : SRC2_TENSOR) : SRC2_NONE, bf, (flags & SE_FLAG_LOW_LATENCY) != 0,
                      (flags & SE_FLAG_CONSERVATIVE) != 0, net, v};
  const Choice ch = choose_form(q);
  const char* name = form_name(ch, q);
  return std::string(ch.fold ? "vecbias," : "") + (name ? name : "?");
}

int main() {
  int bad = 0, rows = 0;
  char line[1024];
  while (fgets(line, sizeof line, stdin)) {
    std::istringstream in(line);
    int a[14];
    std::string want, sw;
    for (int& v : a) in >> v;
    if (!(in >> want)) continue;
    while (in >> sw) {
      const size_t eq = sw.find('=');
      if (eq == std::string::npos || opt_set(sw.substr(0, eq).c_str(), atoi(sw.c_str() + eq + 1))) { fprintf(stderr, "bad switch %s\n", sw.c_str()); return 2; }
    }
    char buf[64] = "";
    const int rc = se_debug_gconv_form(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], a[12], a[13], buf, sizeof buf);
    const std::string mine = answer(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], a[12], a[13]);
    if (rc || want != buf || want != mine) {
      ++bad;
      fprintf(stderr, "MISMATCH want %s, library %s (rc %d), here %s: %s", want.c_str(), buf, rc, mine.c_str(), line);
    }
    opt_reset();
    ++rows;
  }
  // the grid: every answer must be a name, whatever the sizes
  static const int LAYERS[][7] = {{5, 48, 5, 1, 1, 0, 0}, {4, 48, 5, 1, 1, 0, 0}, {3, 48, 5, 1, 1, 0, 0}, {24, 96, 3, 2, 1, 0, 0}, {48, 96, 3, 1, 1, 0, 0},
                                  {48, 192, 3, 2, 1, 0, 0}, {96, 192, 3, 1, 1, 0, 0}, {96, 192, 3, 1, 2, 0, 0}, {96, 192, 3, 1, 16, 0, 0}, {96, 192, 3, 1, 1, 1, 0},
                                  {96, 96, 3, 1, 1, 0, 1}, {48, 48, 3, 1, 1, 0, 1}, {24, 24, 3, 1, 1, 0, 0}, {24, 48, 3, 2, 1, 0, 0}, {24, 96, 3, 1, 1, 0, 0},
                                  {48, 192, 3, 1, 1, 0, 0}, {48, 96, 3, 2, 1, 0, 0}, {8, 48, 5, 1, 1, 0, 0}, {16, 16, 1, 1, 1, 0, 0}, {200, 64, 7, 1, 3, 1, 0}};
  static const int SIZES[] = {1, 2, 3, 7, 8, 12, 16, 17, 64, 255, 256, 1000, 4096, 30000};
  static const int FLAGSETS[] = {0, SE_FLAG_LOW_LATENCY, SE_FLAG_CONSERVATIVE, SE_FLAG_BF16, SE_FLAG_BF16 | SE_FLAG_LOW_LATENCY};
  long calls = 0;
  for (const auto& L : LAYERS)
    for (int H : SIZES)
      for (int W : SIZES)
        for (int B : {1, 3, 64, 4096})
          for (int flags : FLAGSETS)
            for (int net = 0; net < 2; ++net)
              for (int src2 = 0; src2 < (L[0] == 96 && L[1] == 192 ? 3 : 1); ++src2) {
                const std::string s = answer(L[0], src2 ? 96 : 0, src2 == 2, L[1], L[2], L[3], L[4], L[5], L[6], B, H, W, flags, net);
                if (s.empty() || s.find('?') != std::string::npos) { ++bad; fprintf(stderr, "no name: %d -> %d %dx%d B %d flags %d\n", L[0], L[1], H, W, B, flags); }
                ++calls;
              }
  printf("%d rows, %ld grid calls, %d bad\n", rows, calls, bad);
  return bad ? 1 : 0;
}
