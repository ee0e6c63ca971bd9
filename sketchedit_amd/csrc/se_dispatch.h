// Which kernel form a gated convolution runs, as two pure host functions of integers:
//   layer_facts  -- the packing numbers of a layer and which weight images it has (se_pack.hip builds exactly these);
//   choose_form  -- the form of one call, from the layer, its facts, the sizes, the mode and the developer switches (opt()).
// No memory, no device, no se_ctx: se_plan.hip (run_gconv) launches what choose_form says, se_debug_gconv_form reports it, and
// tests/test_forms_host.py holds it against the table of tests/forms_util.py without a GPU.
#pragma once
#include "se_kernels.h"      // opt(), GC_*, gconv_np(), rtile_rows()

namespace se {

enum { ACT_ELU = 0, ACT_RELU = 1, ACT_NONE = 2 };

struct LayerDef {
  const char* name;
  int cin, cout, k, stride, rate, act, up;
};

// raw (ungated) 3x3 conv 12 -> {1, 3}: the last layer of a decoder (utils.py:27)
inline bool small_layer(const LayerDef& d) { return d.act == ACT_NONE || d.cout == 3; }

// output size and padding of a gated conv on an Hin x Win source (utils.py:20); gen_deconv doubles the grid
struct ConvShape { int Ho, Wo, pad; };
inline ConvShape conv_shape(const LayerDef& d, int Hin, int Win) {
  const int pad = d.rate * (d.k - 1) / 2;
  if (d.up) return {2 * Hin, 2 * Win, pad};
  const int span = d.rate * (d.k - 1) + 1;
  return {(Hin + 2 * pad - span) / d.stride + 1, (Win + 2 * pad - span) / d.stride + 1, pad};
}

inline int choose_cfg(int G) {
  if (G <= 16) return GC_N24;
  if (G <= 24) return GC_N48;
  if (G <= 48) return GC_N96;
  if (G <= 96) return GC_N192;
  return -1;
}

// bf16 raw-tile form of the 96-row layers (se_rconv96.hip): 3x3 24/48 -> 96, the 24 -> 96 downsampling layers, gen_deconv 96 -> 96
inline bool rconv96_eligible(const LayerDef& d) {
  if (d.cout != 96 || d.rate != 1 || d.k != 3 || d.act == ACT_NONE) return false;
  if (d.stride == 2) return !d.up && d.cin == 24;                     // stride 2: the 24 -> 96 downsampling layers
  if (d.stride != 1) return false;
  return d.up ? d.cin == 96 : (d.cin == 48 || d.cin == 24);
}

// ---- what a layer is packed as: numbers of the direct images ([0] fp32, [1] bf16) and one flag per optional image (the
// d_<name> of se_pack.h Layer).  nchans = the channels its stored input carries (cin, but 4 for the 4-channel form of wconv1).
struct LayerFacts {
  bool small;                 // raw layer: [cout][9][12] weights only, nothing below
  int cfg, NP, G, T;          // gather-GEMM configuration (-1: unsupported width), packed rows, gated channels, taps (gen_deconv: 4)
  int nch[2], CG[2];          // chunks of 128-byte rows, granules (4 fp32 / 8 bf16 channels) per tap
  int dense, nchd;            // dense-K image of a 5x5 first layer: real channels per pixel, 32-k chunks (0: none)
  bool u, ub, u1, wv, wv16, u24, ub24, u24b, wx, wx2, wd, wdw, w16d, w16s, w96;
  bool s2p;                   // polyphase F(2,2) image of a 3x3 stride-2 layer with 48 stored input channels (se_s2poly.hip)
};

inline LayerFacts layer_facts(const LayerDef& d, int nchans) {
  LayerFacts f = {};
  f.cfg = -1;
  f.small = small_layer(d);
  if (f.small) return f;
  f.G = d.cout / 2;
  if (choose_cfg(f.G) < 0 || (f.G % 4)) return f;
  f.cfg = choose_cfg(f.G);
  f.NP = gconv_np(f.cfg);
  const int KW = d.up ? 2 : d.k;
  f.T = KW * KW;
  for (int bf = 0; bf < 2; ++bf) {      // the stored channels padded to whole granules, taps x channels to whole chunks
    const int per = bf ? 8 : 4, Cp = (nchans + per - 1) / per * per;
    f.CG[bf] = Cp / per;
    f.nch[bf] = (f.T * Cp + 8 * per - 1) / (8 * per);
  }
  // 5x5 first layers whose stored input has padding channels (5 of 8, 3 of 4): images over the real channels alone beside the
  // padded ones -- bf16 pair-of-taps (at most four real channels), fp32 dense K and its F(2,5)-along-x form
  const bool first = d.k == 5 && d.stride == 1 && d.rate == 1 && d.cout == 48;
  f.w16d = first && nchans >= 3 && nchans <= 4;
  f.wd = f.wdw = first && nchans >= 3 && nchans <= 5;
  f.dense = f.wd ? nchans : 0;
  f.nchd = (25 * f.dense + 31) / 32;
  // bf16 raw-tile images (cin == 192: of the FIRST source's 96 channels, for the folded-vector form of conv11)
  f.w16s = d.k == 3 && d.stride == 1 && !d.up && (d.cin == 96 || d.cin == 192) && d.cout == 192;
  f.w96 = rconv96_eligible(d);
  // the polyphase image of the 48-channel downsampling layers (48 -> 96, 48 -> 192): whole 96-row halves
  f.s2p = d.k == 3 && d.stride == 2 && d.rate == 1 && !d.up && nchans == 48 && d.cin == 48 && (d.cout == 96 || d.cout == 192);
  // the Winograd-type image of the 3x3 stride-1 layers whose packed channels are exactly the layer's
  if (d.k != 3 || d.stride != 1 || (nchans + 3) / 4 * 4 != d.cin) return f;
  if (d.up) {
    f.u = f.ub = (d.cin == 96 && d.cout == 96) || (d.cin == 48 && d.cout == 48);            // winoup, winoup48
  } else if ((d.cin == 96 || d.cin == 192) && d.cout == 192) {
    f.u = f.u24 = f.ub24 = true;                                                            // wino, wino24
    f.u1 = f.wv = f.wv16 = f.u24b = d.cin == 192;          // two sources: the first alone + the folded vector; both (wino24_2src)
  } else if (d.cin == 48 && d.cout == 192) {
    f.u24 = f.ub24 = true;                                                                  // wino24_c48 (xconv5)
  } else if (d.cin == 24 && d.cout == 24 && d.rate == 1) {
    f.wx = f.wx2 = true;                                                                    // rtilew, rtilew2 (conv16)
  } else if ((d.cin == 48 || d.cin == 24) && d.cout == 96) {
    f.u = f.ub = true;                                                                      // wino48, wino48_c24
  }
  return f;
}

// ---- one call ------------------------------------------------------------------------------------------------------------
enum { SRC2_NONE = 0, SRC2_TENSOR = 1, SRC2_VECTOR = 2 };
struct ConvCall {
  LayerDef def; LayerFacts facts;
  int B, Hin, Win, C0, C1;      // C0, C1: stored channels per pixel of the two sources (C1 = 0 without a second one)
  int src2;                     // SRC2_*
  bool bf16, low_latency, conservative;
  int net;                      // SE_NET_G (0) / SE_NET_M (1): the network whose plan is running
  bool fold_scratch;            // the scratch of the folded vector source exists: vbias_ws and, in bf16, vec32
};

enum Form {
  F_SMALL_CONV, F_WINO, F_WINO24, F_WINO24_C48, F_WINO48, F_WINO48_C24, F_WINOUP, F_WINOUP48, F_RTILEW, F_RTILEW2,
  F_RTILE_DENSE5, F_RTILE_DENSE5W, F_RTILE_D4, F_RTILE, F_RCONV16, F_RCONV16_DUAL, F_RCONV96, F_S2POLY48, F_GATHER
};
struct Choice {
  Form form;
  bool fold;              // the vector source folded into a bias table: vecbias launched in front, the form on the first source alone
  bool wino_range;        // a 96 -> 192 Winograd layer whose source exceeds the kernels' 32-bit byte offsets (run_gconv says so once)
};

// x / CG == (x * magicCG) >> 16 and t / KW == (t * magicKW) >> 8 on the ranges the direct kernels use
inline bool magic_cg_ok(int CG, int nch) {
  const int m = (65536 + CG - 1) / CG;
  for (int gi = 0; gi < nch * 8 + 8; ++gi)
    if (((gi * m) >> 16) != gi / CG) return false;
  return true;
}
inline bool magic_kw_ok(int KW, int T) {
  const int m = 256 / KW + 1;
  for (int t = 0; t <= T + 8; ++t)
    if (((t * m) >> 8) != t / KW) return false;
  return true;
}

// the narrow layers in raw-tile form (se_rtile.hip, se_rtilew.hip), or F_GATHER
inline Form choose_rtile(const ConvCall& q) {
  const LayerDef& d = q.def;
  const LayerFacts& f = q.facts;
  const bool bf = q.bf16;
  const int Hin = q.Hin, Win = q.Win, C0 = q.C0;
  const long long B = q.B;
  if (!opt(OPT_RTILE) || q.src2 || d.stride != 1 || d.rate != 1 || (f.cfg != GC_N48 && f.cfg != GC_N24)) return F_GATHER;
  // low-latency mode: only when the tiles still cover the CUs (the small-grid gather-GEMM splits rows over blockIdx.y).
  // Counted PER IMAGE like the Winograd grids: the kernel a layer runs depends on the image size and the mode only, never on
  // the batch (with B in the count a 128x128 image took the raw-tile kernel at B = 2 and the gather-GEMM at B = 1, and its
  // bits differed between the two calls)
  const int TR = rtile_rows(bf);
  const long tiles = (long)((Hin + TR - 1) / TR) * ((Win + 15) / 16) * (d.up ? 4 : 1);
  if (q.low_latency && tiles < opt(OPT_RTILE_LL_MIN)) return F_GATHER;
  const int es = bf ? 2 : 4, gran = bf ? 8 : 4;
  if (C0 != f.CG[bf] * gran) return F_GATHER;
  // 24 -> 24 3x3: F(2,3) along x on the raw tile, or two-dimensional (se_rtilew.hip).  SE_RTILE_WX=0: the direct form, 1: along x
  const int wx_mode = opt(OPT_RTILE_WX);
  if (wx_mode != 0 && !bf && f.wx && d.k == 3 && !d.up && C0 == 24 && d.cin == 24 && d.cout == 24 && (Win % 2) == 0 &&
      B * Hin * Win * 96 < (1ll << 31))
    return wx_mode != 1 && f.wx2 && (Hin % 2) == 0 ? F_RTILEW2 : F_RTILEW;
  // dense-K form of the 5x5 first layers (fp32): SE_RTILE_DENSE=0 keeps the channel-padded K.  (A batch beyond the 32-bit
  // byte range runs as sub-launches of the SAME form: one image has to fit.)  F(2,5) along x at even widths, SE_RTILE_D5W=0: direct
  if (opt(OPT_RTILE_DENSE) != 0 && !bf && f.wd && f.dense && d.k == 5 && !d.up && f.cfg == GC_N48 && (long long)Hin * Win * C0 * 4 < (1ll << 31))
    return opt(OPT_RTILE_D5W) != 0 && f.wdw && (Win % 2) == 0 ? F_RTILE_DENSE5W : F_RTILE_DENSE5;
  // bf16: pair-of-taps form of the 5x5 first layers whose stored NHWC8 input has at most four real channels
  if (opt(OPT_RTILE_DENSE) != 0 && bf && f.w16d && d.k == 5 && !d.up && f.cfg == GC_N48 && C0 == 8 && B * Hin * Win * 16 < (1ll << 31))
    return F_RTILE_D4;
  const int KW = d.up ? 2 : d.k;
  const int raw_bytes = ((TR + KW - 1) * (16 + KW - 1) * C0 * es + 1023) & ~1023;
  if (raw_bytes + f.nch[bf] * f.NP * 128 > 80 * 1024) return F_GATHER;       // two workgroups per CU or not at all
  if (B * Hin * Win * C0 * es >= (1ll << 31)) return F_GATHER;
  if (!magic_cg_ok(f.CG[bf], f.nch[bf]) || !magic_kw_ok(KW, f.T)) return F_GATHER;
  return F_RTILE;
}

// two polyphase sub-images of 8 columns (and at most 8 rows) share one 8 x 16 raw tile (rconv16b_kernel, p.dual)
inline bool rconv16_dual_ok(const LayerFacts& f, const LayerDef& d, int Hin, int Win) {
  if (opt(OPT_RCONV16_DUAL) == 0) return false;
  return f.w16s && (d.rate % 2) == 0 && Win / d.rate == 8 && Hin / d.rate <= 8 && Hin / d.rate >= 4;
}

// The ladder: the first form whose rule holds runs, the gather-GEMM where none does.  Every grid threshold of the low-latency
// mode counts workgroups PER IMAGE (the batch does not enter): which kernel a layer runs depends on the image size and the
// mode only, so an image's result stays bit-identical across batch sizes, batch positions and ranks within the mode.  The
// byte-range tests do contain B: a tensor one launch addresses stays below 2^31 bytes (32-bit byte offsets).
inline Choice choose_form(const ConvCall& q) {
  const LayerDef& d = q.def;
  const LayerFacts& f = q.facts;
  const int Hin = q.Hin, Win = q.Win, C0 = q.C0, C1 = q.C1;
  const long long B = q.B;
  const bool two = q.src2 != SRC2_NONE, vec = q.src2 == SRC2_VECTOR, ll = q.low_latency;
  const ConvShape sh = conv_shape(d, Hin, Win);
  Choice ch = {F_GATHER, false, false};
  auto is = [&](Form form) { ch.form = form; return ch; };
  if (f.small) return is(F_SMALL_CONV);
  if (q.bf16) {
    // bf16: no Winograd forms (the transforms would run in fp32 on bf16 data and round the transformed tiles again; at 16x the
    // MFMA rate the layers are bound by the LDS fill).  96 -> 192 3x3 stride 1 in raw-tile form where the polyphase sub-images
    // fill 8 x 16 tiles (se_rconv16.hip; SE_RCONV16=0: gather-GEMM); conv11's vector source folded into a bias table
    const bool use_rconv = opt(OPT_RCONV16) != 0 && !ll && d.k == 3 && d.stride == 1 && !d.up && d.cout == 192 && C0 == 96 && f.w16s &&
                           B * Hin * Win * 192 < (1ll << 31);
    if (opt(OPT_VECBIAS) != 0 && use_rconv && vec && q.fold_scratch && f.wv16 && d.rate == 1 && d.cin == 192 && C1 == 96 && Hin >= 12 && Win >= 12) {
      ch.fold = true;
      return is(F_RCONV16);
    }
    if (use_rconv && d.cin == 96 && !two && (Hin % d.rate) == 0 && (Win % d.rate) == 0 && f.nch[1] == 14) {
      if (Hin / d.rate >= 12 && Win / d.rate >= 12) return is(F_RCONV16);
      if (rconv16_dual_ok(f, d, Hin, Win)) return is(F_RCONV16_DUAL);
    }
    // 96-row layers (3x3 48/24 -> 96, gen_deconv 96 -> 96): raw-tile form, se_rconv96.hip (SE_RCONV96=0: gather-GEMM)
    if (opt(OPT_RCONV96) != 0 && !ll && f.w96 && !two && C0 == d.cin && Hin >= 12 && Win >= 12 &&
        B * sh.Ho * sh.Wo * 96 < (1ll << 31) && B * Hin * Win * C0 * 2 < (1ll << 31))
      return is(F_RCONV96);
    return is(choose_rtile(q));
  }
  // Low-latency mode: the Winograd kernels' 64/128-tile workgroups would occupy 16-32 of the 256 CUs, so a gated conv takes
  // the small-grid gather-GEMM instead (2.25x more multiply-adds on ~10x more CUs) unless its Winograd grid still covers enough
  // of the chip: the 96 -> 192 kernels pay from 64 workgroups on, the 96- and 48-row kernels from 128 on (SE_LL_WINO_MIN_WG /
  // SE_LL_WINO48_MIN_WG; 0: never; tools/ll_wino_sweep.sh)
  auto grid_ok = [&](long wgs, int min_wg) { return !ll || (min_wg > 0 && wgs >= min_wg); };
  const int min192 = opt(OPT_LL_WINO_MIN_WG), min48 = opt(OPT_LL_WINO48_MIN_WG);
  const int f43_mode = opt(OPT_WINOGRAD_F43);
  const bool use_wino = opt(OPT_WINOGRAD) != 0;
  const bool even2 = (Hin % (2 * d.rate)) == 0 && (Win % (2 * d.rate)) == 0;       // whole 2x2 tiles of every dilation phase
  const long wg64 = ((long)(Hin / 2) * (Win / 2) + 63) / 64;                       // workgroups of 64 such tiles
  const bool fits96 = B * Hin * Win * 384 < (1ll << 31), fits48 = B * Hin * Win * 192 < (1ll << 31);
  const bool wino_src_ok = (!two && C0 == 96 && d.cin == 96) || (two && C0 == 96 && C1 == 96 && d.cin == 192);
  if (use_wino && !d.up && f.u && wino_src_ok && !fits96) ch.wino_range = true;
  if (use_wino && !d.up && f.u && wino_src_ok && fits96 && even2 && grid_ok(wg64, min192)) {
    // A spatially constant second source is folded into a per-image, per-border-configuration bias (launch_vecbias) and the
    // layer runs as the SINGLE-source kernel (SE_VECBIAS=0: the two-source kernel reads the vector as a second input)
    ch.fold = opt(OPT_VECBIAS) != 0 && vec && d.rate == 1 && f.u1 && f.wv && q.fold_scratch && Hin >= 2 && Win >= 2;
    const bool s1 = two && !ch.fold;
    // Hybrid F(2,3) x F(4,3) (se_wino24.hip) where the width allows 4-column tiles.  SE_WINOGRAD_F43=0: F(2x2,3x3) everywhere;
    // 1 (default): the hybrid kernel everywhere; 2: netG only (netM's soft mask feeds the 0.5 threshold, DESIGN.md 3.1b').
    // SE_FLAG_CONSERVATIVE is mode 2 for this call, chosen by the caller through the ABI instead of the process-wide table
    const bool f43_net_ok = q.net == 0 || (f43_mode == 1 && !q.conservative);
    const bool f43 = (f43_mode == 1 || f43_mode == 2) && f43_net_ok && (s1 ? (!vec && f.u24b) : f.u24) && f.ub24 && (Win % (4 * d.rate)) == 0;
    return is(f43 ? F_WINO24 : F_WINO);
  }
  // 48 -> 192 (xconv5 of netG) on the hybrid kernel's 48-channel instantiation
  if (use_wino && f43_mode != 0 && !d.up && !two && C0 == 48 && d.cin == 48 && d.cout == 192 && d.stride == 1 && f.u24 && f.ub24 && fits96 &&
      (Hin % (2 * d.rate)) == 0 && (Win % (4 * d.rate)) == 0 && grid_ok(((long)(Hin / 2) * (Win / 4) + 31) / 32, min192))
    return is(F_WINO24_C48);
  // 48 -> 96, and 24 -> 96 (xconv3 / pmconv3 of netG) on the same kernel (se_wino48.hip)
  if (use_wino && opt(OPT_WINOGRAD48) != 0 && !d.up && f.u && f.ub && !two && fits48 && even2 && grid_ok(wg64, min48)) {
    if (C0 == 48 && d.cin == 48) return is(F_WINO48);
    if (C0 == 24 && d.cin == 24 && d.cout == 96 && d.stride == 1) return is(F_WINO48_C24);
  }
  // gen_deconv 96 -> 96 and 48 -> 48: F(2x2,2x2) on the four sub-pixel classes (se_wino_up.hip, se_wino_up48.hip)
  if (use_wino && opt(OPT_WINOGRAD_UP) != 0 && d.up && f.u && f.ub && !two && (Hin % 2) == 0 && (Win % 2) == 0 && grid_ok(4 * wg64, min48)) {
    if (C0 == 96 && d.cin == 96 && fits96) return is(F_WINOUP);
    if (opt(OPT_WINOGRAD_UP48) != 0 && C0 == 48 && d.cin == 48 && d.cout == 48 && fits48 && B * sh.Ho * sh.Wo * 96 < (1ll << 31)) return is(F_WINOUP48);
  }
  // 3x3 stride 2, 48 -> 96 / 192: polyphase F(2,2), 25 of 36 products on tiles of 2x2 outputs = 4x4 source pixels (se_s2poly.hip).
  // SE_S2_POLY=0: the gather-GEMM; 1 (default): everywhere; 2: netG only (netM's soft mask feeds the 0.5 threshold, as SE_WINOGRAD_F43).
  // Never in low-latency mode: a 64-tile workgroup covers 1024 source pixels, a 128x128 source is 16 workgroups per row half
  const int s2_mode = opt(OPT_S2_POLY);
  if ((s2_mode == 1 || (s2_mode == 2 && q.net == 0)) && !ll && f.s2p && !two && d.k == 3 && d.stride == 2 && d.rate == 1 && !d.up && C0 == 48 &&
      d.cin == 48 && (d.cout == 96 || d.cout == 192) && (Hin % 4) == 0 && (Win % 4) == 0 && fits48)
    return is(F_S2POLY48);
  return is(choose_rtile(q));
}

// the form name of a gather-GEMM launch (Profiler::Rec::form): gconv_n<rows>[_small][_up2][_2src][_bf16]
inline const char* gconv_form_name(int cfg, bool small_grid, bool up2, bool two_src, bool bf16) {
#define SE_GF(n) n, n "_bf16", n "_2src", n "_2src_bf16", n "_up2", n "_up2_bf16", n "_up2_2src", n "_up2_2src_bf16"
#define SE_GS(n) { SE_GF(n), SE_GF(n "_small") }
  static const char* const names[4][16] = {SE_GS("gconv_n192"), SE_GS("gconv_n96"), SE_GS("gconv_n48"), SE_GS("gconv_n24")};
#undef SE_GS
#undef SE_GF
  if (cfg < 0 || cfg > 3) return nullptr;
  return names[cfg][(small_grid ? 8 : 0) | (up2 ? 4 : 0) | (two_src ? 2 : 0) | (bf16 ? 1 : 0)];
}

// the name the launcher of the chosen form records (tests/forms_util.py FORMS)
inline const char* form_name(const Choice& ch, const ConvCall& q) {
  const LayerDef& d = q.def;
  const bool two = q.src2 != SRC2_NONE && !ch.fold;
  switch (ch.form) {
    case F_SMALL_CONV: return "small_conv";
    case F_WINO: return two ? "wino_2src" : "wino";
    case F_WINO24: return two ? "wino24_2src" : "wino24";
    case F_WINO24_C48: return "wino24_c48";
    case F_WINO48: return "wino48";
    case F_WINO48_C24: return "wino48_c24";
    case F_WINOUP: return "winoup";
    case F_WINOUP48: return "winoup48";
    case F_RTILEW: return "rtilew";
    case F_RTILEW2: return "rtilew2";
    case F_RTILE_DENSE5: return "rtile_dense5";
    case F_RTILE_DENSE5W: return "rtile_dense5w";
    case F_RTILE_D4: return "rtile_bf16_d4";
    case F_RTILE: return q.bf16 ? (d.up ? "rtile_bf16_up2" : "rtile_bf16") : (d.up ? "rtile_up2" : "rtile");
    case F_RCONV16: return "rconv16";
    case F_RCONV16_DUAL: return "rconv16_dual";
    case F_S2POLY48: return "s2poly48";
    case F_RCONV96: return d.up ? "rconv96_up" : d.stride == 2 ? "rconv96_s2" : q.C0 == 24 ? "rconv96_c24" : "rconv96";
    case F_GATHER: return gconv_form_name(q.facts.cfg, q.low_latency, d.up != 0, q.C0 / (q.bf16 ? 8 : 4) != q.facts.CG[q.bf16], q.bf16);
  }
  return nullptr;
}

}  // namespace se
