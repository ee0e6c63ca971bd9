// Stand-alone host check of the paired passes, meant for a sanitizer build: its own main, no device,
// nothing loaded into an interpreter.  It compiles the plans themselves (se_plan.hip: the arenas, plan_netM / plan_netG,
// pass_size, plan_peaks, and pair_rule of se_host.h) into THIS program, instrumented, and links the library only for what the
// plans reference and a dry run never calls.  Over a grid of (B, H, W, flags, outputs, SE_PAIR_MIN_PIXELS) it holds
//   * pair_rule against its definition: never for one image, in low-latency mode or with the option at 0, otherwise exactly
//     from B H W >= the option on, odd B included;
//   * plan_peaks of a paired pass against the single chains it is made of: its main peak is the main peak of the one-stream
//     plan of the first half, its side peak that of the second half's (both halves allocate what a pass of their size does);
//   * the sanitizers' silence over every dry run (the first-fit arena's block list, the per-plan ctx state).
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined tools/pair_host_check.hip \
//         -Lsketchedit_amd/lib -lsketchedit_hip -Wl,-rpath,$PWD/sketchedit_amd/lib -o pair_host_check
//   ./pair_host_check
#include "../sketchedit_amd/csrc/se_plan.hip"

namespace se {
thread_local std::string g_create_err;
}

int main() {
  se_ctx c;      // as se_create leaves it, without the device: a dry run reads the layer definitions and nothing else
  for (int i = 0; i < NG; ++i) c.G[G_LAYERS[i].name].def = G_LAYERS[i];
  for (int i = 0; i < NM; ++i) c.M[M_LAYERS[i].name].def = M_LAYERS[i];
  c.wconv1_j4.def = c.G.at("wconv1").def;
  c.st_side = (hipStream_t)(uintptr_t)0x1000;      // never used by a dry run; non-null as in a live ctx (Plan::forked, pair_pass)
  static const int SHAPES[][2] = {{16, 16}, {64, 64}, {40, 72}, {24, 1000}, {256, 256}, {512, 512}};
  static const int BATCHES[] = {1, 2, 3, 4, 5, 8, 16, 32, 33};
  static const int MINS[] = {0, 1, 1 << 20, 1 << 21, 1 << 22};
  long rules = 0, plans = 0;
  int bad = 0;
  for (int min_pixels : MINS) {
    if (opt_set("SE_PAIR_MIN_PIXELS", min_pixels)) { fprintf(stderr, "no such switch\n"); return 2; }
    c.fork2 = opt(OPT_FORK_DEFAULT) != 0;
    for (const auto& s : SHAPES)
      for (int B : BATCHES)
        for (int fl = 0; fl < 16; ++fl) {
          const int H = s[0], W = s[1];
          const int flags = ((fl & 1) ? SE_FLAG_USE_CAM : 0) | ((fl & 2) ? SE_FLAG_JOINT_TRAIN_INP : 0) | ((fl & 4) ? SE_FLAG_LOW_LATENCY : 0) |
                            ((fl & 8) ? SE_FLAG_BF16 : 0) | SE_FLAG_POOL_MAX;
          const bool ll = (fl & 4) != 0;
          const bool want = !ll && B >= 2 && min_pixels > 0 && (long long)B * H * W >= min_pixels;
          ++rules;
          if (pair_rule(B, H, W, flags) != want) { ++bad; fprintf(stderr, "rule: B %d %dx%d flags %d min %d\n", B, H, W, flags, min_pixels); }
          c.serial = true;
          if (pair_pass(&c, B, H, W, flags)) { ++bad; fprintf(stderr, "a profiled call pairs: B %d %dx%d\n", B, H, W); }
          c.serial = false;
          const int nb = pass_size(&c, B, H, W, flags);
          if (nb != B) { ++bad; fprintf(stderr, "unexpected passes: B %d %dx%d -> %d\n", B, H, W, nb); continue; }
          for (int mi = 0; mi < 2; ++mi) {
            const se_ctx::Peaks one = plan_peaks(&c, 3, B, H, W, flags, mi != 0);
            ++plans;
            if (!one.main || (ll && !one.side)) { ++bad; fprintf(stderr, "peaks: B %d %dx%d flags %d\n", B, H, W, flags); }
            if (!pair_pass(&c, B, H, W, flags)) continue;
            const se_ctx::Peaks two = plan_peaks(&c, 3, B, H, W, flags, mi != 0, true);
            c.serial = true;       // the one-stream plans of the halves: everything in the main arena
            const se_ctx::Peaks a = plan_peaks(&c, 3, pair_first(B), H, W, flags, mi != 0), b = plan_peaks(&c, 3, B - pair_first(B), H, W, flags, mi != 0);
            c.serial = false;
            plans += 3;
            if (a.side || b.side || two.main != a.main || two.side != b.main || c.paired || c.half) {
              ++bad;
              fprintf(stderr, "paired peaks: B %d %dx%d flags %d: %zu + %zu, halves %zu (+ %zu), %zu (+ %zu)\n", B, H, W, flags, two.main, two.side,
                      a.main, a.side, b.main, b.side);
            }
          }
        }
  }
  opt_reset();
  printf("%ld rule calls, %ld dry plans, %d bad\n", rules, plans, bad);
  return bad ? 1 : 0;
}
