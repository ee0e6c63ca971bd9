// Internal (C++) interface between the host files (se_plan.hip, se_api*.hip; se_host.h) and the
// gfx950 kernels (se_gconv.hip, se_wino.hip, se_wino48.hip, se_attention.hip, se_misc.hip).  Not part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

struct se_window;   // include/sketchedit_hip.h

namespace se {

// ---------------------------------------------------------------------------------------------
// Optional per-launch timing (HIP events on the launch stream), used by bench.py for the roofline
// figures.  Off by default; when off the launch wrappers add nothing.
// ---------------------------------------------------------------------------------------------
enum ProfLabel { PL_GCONV_N192 = 0, PL_GCONV_N96, PL_GCONV_N48, PL_GCONV_N24, PL_WINO_N192, PL_WINO_N96, PL_WINO_UP96, PL_SMALL_CONV, PL_PACK, PL_COLREDUCE,
                 PL_ATT_PREP, PL_ATT_SCORE, PL_ATT_SOFTMAX, PL_ATT_BOXSUM, PL_ATT_PV, PL_LAYOUT,
                 PL_ATT_STREAM_STATS, PL_ATT_STREAM_OUT, PL_RESIZE_H, PL_RESIZE_V, PL_WINDOW_GATHER, PL_WINDOW_BORDER, PL_WINDOW_PASTE,
                 PL_WINDOW_RESAMPLE_H, PL_WINDOW_PASTE_V, PL_WINDOW_SAVE, PL_WINDOW_SWAP, PL_WINDOW_LOCK_GATHER, PL_WINDOW_PASTE_LOCKED,
                 PL_WINDOW_PASTE_V_LOCKED, PL_SKETCH_TILES, PL_SKETCH_STROKES, PL_PNG_ROWS, PL_PNG_STRIPES,
                 PL_PNG_FINISH, PL_JPG_BLOCKS, PL_JPG_ROWS, PL_JPG_FINISH, PL_JPG2_BLOCKS, PL_JPG2_HIST, PL_JPG2_TABLES,
                 PL_WINDOW_PASTE_FEATHER, PL_FILL_MASKS, PL_FILL_KEEP, PL_BLEND_INIT, PL_BLEND_PULL, PL_BLEND_RELAX, PL_BLEND_APPLY, PL_CANVAS_MAP, PL_CANVAS_TURN,
                 PL_SELECT_SIMILAR, PL_SELECT_FLOOD, PL_SELECT_GROW, PL_MODIFY_DISC, PL_MODIFY_VOTE,
                 PL_LASSO_FILL, PL_PLANE_COMBINE, PL_ADJUST, PL_HIST_TILES, PL_HIST_SUM, PL_ADJUST_LUT, PL_OUTLINE_COUNT, PL_OUTLINE_SCAN, PL_OUTLINE_EMIT, PL_FILTER_BLUR, PL_FILTER_MOSAIC, PL_MOVE_DROP,
                 PL_PLANE_SHIFT, PL_WARP_DROP, PL_PLANE_WARP, PL_COUNT };
const char* prof_label_name(int l);
// Rec::form: the kernel form of the launch (a static string, finer than the label: DESIGN.md 3.1f) -- what a test reads to
// know which kernel the dispatcher chose; the label's name where the launcher has one form only
struct Profiler {
  struct Rec { int label; const char* name; const char* form; double flops; double exec_flops; double bytes; long blocks; hipEvent_t a, b; };
  std::vector<Rec> recs;
  std::vector<hipEvent_t> pool;   // pre-created events (se_profile_enable), handed out two per launch
  size_t used = 0;
  bool on = false;
};
void set_profiler(Profiler* p);          // thread-local; set by the API under the ctx lock
// cost/name of the NEXT launch (consumed once).  flops = algorithmic FLOPs of the layer as the reference defines it;
// exec_flops = multiply-add FLOPs the kernel's MFMA pipe actually executes (Winograd / sub-pixel / space-to-depth forms
// execute fewer); < 0: same as flops.  The roofline fraction is computed from exec_flops.
void set_launch_cost(double flops, double bytes, const char* name = nullptr, double exec_flops = -1.0);
// workgroups of the NEXT launch (consumed once): lets the report say how much of the 256-CU machine a layer can occupy
void set_launch_grid(long blocks);
// hipFuncAttributeMaxDynamicSharedMemorySize is a per-device property of a kernel: set it once per (device, kernel)
hipError_t ensure_max_lds(const void* func, int bytes);

// ---------------------------------------------------------------------------------------------
// Developer switches.  ONE process-wide table: every entry is read from the environment exactly once (first use of the
// table) and can afterwards be changed only through the C-ABI test aid se_debug_set_option -- the launch path never calls
// getenv (ADVICE r4 / VERDICT r4 item 7c: getenv per launch is host latency at batch 1 and is not safe against a concurrent
// setenv from another thread).  opt() is a relaxed atomic load.
// ---------------------------------------------------------------------------------------------
#define SE_OPTIONS(X)                                                                                         \
  X(XCD_REMAP, 1)        /* 0: XCD-aware tile order off */                                                     \
  X(RTILE, 1)            /* 0: gather-GEMM instead of the raw-tile kernels */                                  \
  X(RTILE_LL_MIN, 256)   /* low-latency mode: fewest raw tiles for which the raw-tile kernels still run */      \
  X(RTILE_WX, 2)         /* 24 -> 24 layers: 0 direct raw tile, 1 F(2,3) along x, 2 two-dimensional F(2x2,3x3) */ \
  X(RTILE_DENSE, 1)      /* 0: channel-padded K for the 5x5 first layers */                                    \
  X(RTILE_D5W, 1)        /* 0: 5x5 first layers on the direct dense-K kernel */                                \
  X(TEST_OFFSET_LIMIT, 0) /* test aid, se_debug_set_option only: byte range of the 32-bit-offset kernels (0: 2^31) */ \
  X(TEST_POISON, 0)      /* test aid, se_debug_set_option only: 1..255 fills every scratch region with that byte when it is handed out, any other value is off (se_host.h poison) */ \
  X(RCONV16, 1) X(RCONV16_DUAL, 1) X(RCONV96, 1) X(VECBIAS, 1)                                                  \
  X(WINOGRAD, 1) X(WINOGRAD48, 1) X(WINOGRAD_UP, 1) X(WINOGRAD_UP48, 1)                                         \
  X(WINOGRAD_F43, 1)     /* hybrid F(2,3)xF(4,3): 0 off, 1 everywhere, 2 netG only */ \
  X(S2_POLY, 1)          /* polyphase F(2,2) form of the 48-channel stride-2 layers: 0 off, 1 everywhere, 2 netG only */ \
  X(GCONV_FAST, 1) X(FORK_DEFAULT, 1) X(LL_WINO_MIN_WG, 64) X(LL_WINO48_MIN_WG, 128)                            \
  X(ATT_FUSED, -1) X(ATT_FUSED_BF16, -1) X(ATT_PTILDE_LDS, 1) X(ATT_STATS_LDS, 1) X(ATT_E16, 1) X(ATT_SYM, 1)   \
  X(ATT_STREAM, 0)       /* attention form: 0 by size (streaming where R Rp 4 >= 2^31), 1 streaming wherever possible */ \
  X(PAIR_MIN_PIXELS, 1 << 21) /* default mode: fewest pixels (images x H x W) of a pass that runs as two half-batch chains on the two streams (se_host.h pair_rule); 0: never */
enum Opt {
#define X(name, dflt) OPT_##name,
  SE_OPTIONS(X)
#undef X
  OPT_COUNT
};
int opt(int o);                                   // current value
int opt_set(const char* name, int value);         // "SE_<NAME>" or "<NAME>"; returns 0, or 1 for an unknown name
int opt_get(const char* name, int* value);        // the same for reading
void opt_reset();                                 // every entry back to its environment / built-in default
long long opt_epoch();                            // number of opt_set / opt_reset calls so far (key of captured forwards)

// ---------------------------------------------------------------------------------------------
// Gather-GEMM gated convolution (the hot kernel).
//   D[n][p] = sum_k Wp[n][k] * X[p][k]   n: packed output channels, p: output pixels,
//   k: flattened (tap, channel) in 32-float chunks.  X rows are gathered on the fly from
//   one or two NHWC sources (im2col-free); Wp is packed on the host (se_pack.hip pack_layer).
// ---------------------------------------------------------------------------------------------
struct GConvParams {
  const float* src0;   // NHWC [B][Hin][Win][C0]  (fp32, or bf16 when `bf16` is set -- the pointer types stay float*)
  const float* src1;   // optional second source (channel concat): NHWC [B][Hin][Win][C1] or vector [B][C1]
  const float* wpk;    // packed weights [nch][NP][128 bytes] (LDS image, pre-swizzled): 32 fp32 or 64 bf16 k-values per row
  const float* bias;   // [NP] in packed-row order (always fp32)
  float* dst;          // NHWC [B][Ho][Wo][G]
  const float* zeros;  // >= 16 bytes of zeros (source of out-of-bounds granules)
  int B, Hin, Win, Ho, Wo;
  int C0, C1;          // channel counts (row strides, floats)
  int C0g, CG;         // granules (4 floats) per tap in src0 / in total
  int T, KW;           // taps, taps per kernel row
  int magicCG, magicKW; // x/CG == (x*magicCG)>>16, t/KW == (t*magicKW)>>8 on the ranges used (host-verified)
  int magicKH;          // kernel rows T / KW
  unsigned rep;         // sum over kernel rows j of 1 << (j*KW): replicates a column-validity mask to every row
  unsigned div_hw_m, div_w_m;   // exact x / (Ho*Wo) and x / Wo for x < 2^32 (se_device.h udiv_magic), with
  int div_hw_l, div_w_l;        // their shift counts
  int stride, dil, pad;
  int ushift;          // 1: source is read through a nearest x2 upsample (coords >> 1)
  int up2;             // 1: sub-pixel form of nearest-x2 + 3x3: one workgroup = one output parity class (py,px), a 2x2 conv
                       //    on the source grid with pre-summed weights; (Ho,Wo) is then the SOURCE grid, (OH,OW) the output
  int OH, OW;
  int Hlim, Wlim;      // validity limits of the pre-shift tap coordinates
  int src1_vec;        // src1 is a per-batch vector (spatially constant, still zero padded)
  int nch;             // number of 32-k chunks
  int G;               // gated (stored) output channels
  int act;             // 0 ELU, 1 ReLU
  int total_pix;       // B*Ho*Wo
  int xcd;             // 1: XCD-aware tile order (se_device.h xcd_tile)
  int np_full;         // packed rows of the whole layer (row count of one chunk of wpk)
  int nf_full;         // feature tiles of the whole layer (non-MIXED layouts: gates start at tile nf_full)
  int bf16;            // 1: sources, weights and dst are bf16 (granule = 8 channels, chunk = 64 k); C0, C1, G count elements
  int small_grid;      // 1: low-latency launch shape (small pixel tiles; the packed rows split over blockIdx.y) for grids
                       //    that would otherwise leave most of the 256 CUs idle (batch 1)
};

// magic numbers of se_device.h udiv_magic for divisor d >= 1
static inline void udiv_magic_host(unsigned d, unsigned* m, int* l) {
  int ll = 0;
  while ((1ull << ll) < d) ++ll;
  *l = ll;
  *m = (unsigned)(((1ull << 32) * ((1ull << ll) - d)) / d + 1);
}

enum GConvCfg { GC_N192 = 0, GC_N96 = 1, GC_N48 = 2, GC_N24 = 3 };
// rows (packed output channels) of each config
static inline int gconv_np(int cfg) { return cfg == GC_N192 ? 192 : cfg == GC_N96 ? 96 : cfg == GC_N48 ? 48 : 32; }
static inline bool gconv_mixed(int cfg) { return cfg >= GC_N48; }

hipError_t launch_gconv(int cfg, const GConvParams& p, hipStream_t st);

// ---------------------------------------------------------------------------------------------
// Winograd F(2x2,3x3) form of the 3x3 stride-1 gated conv 96 -> 192 (se_wino.hip)
// ---------------------------------------------------------------------------------------------
struct WinoParams {
  const float* src;    // NHWC [B][h][w][96]
  const float* src1;   // optional second 96-channel source (channel concat): NHWC tensor, or [B][96] vector; else null
  int src1_vec;        // src1 is a per-image vector (spatially constant, zero padded like a tensor)
  const float* upk;    // [16 positions][3 or 6 chunks][192 packed rows][32]: G g G^T, LDS image (pre-swizzled)
  const float* bias;   // [192] packed-row order (features, then gates)
  float* dst;          // NHWC [B][h][w][96]
  int B, h, w, d;      // dilation d; h % 2d == 0 and w % 2d == 0
  int th, tw;          // tile grid h/2 x w/2
  int total_tiles;     // B*th*tw
  int act;             // 0 ELU, 1 ReLU
  int xcd;             // 1: XCD-aware tile order
  unsigned div_tpi_m, div_tw_m, div_d_m;   // udiv_magic numbers for th*tw, tw and d
  int div_tpi_l, div_tw_l, div_d_l;
  const float* vbias;  // optional [B][9][192]: per-image, per-border-configuration bias (the folded vector source, launch_vecbias)
};
hipError_t launch_wino(const WinoParams& p, hipStream_t st);
// A spatially constant second source (the pooled style vector in front of conv11, editline_g.py:166-167) contributes
//   T[b][cfg][n] = sum over the taps inside the image in border configuration cfg, sum_c W[n][C0 + c][tap] * v[b][c]
// to output row n -- a per-image bias that depends only on WHICH taps fall inside the image (zero padding: 3 x 3 configurations
// for a 3x3 kernel at dilation 1): cfg = 3 * (y == 0 ? 0 : y == h-1 ? 2 : 1) + (x == 0 ? 0 : x == w-1 ? 2 : 1).
// wv: [9 taps][C1][192 packed rows] (row fastest), vec: [B][C1], T: [B][9][192].
// round_vec: the vector is rounded to bf16 on the way in (bf16 mode: wv then holds bf16-rounded weights; fp32 accumulate)
hipError_t launch_vecbias(const float* wv, const float* vec, float* T, int B, int C1, hipStream_t st, int round_vec = 0);
// Hybrid F(2,3) x F(4,3) form of the single-source 96 -> 192 layer (se_wino24.hip): 2x4 output tiles, th = h/2, tw = w/4,
// h % 2d == 0 and w % 4d == 0; upk [72 iterations][192 MIXED rows][32] (pack_wino24), bias [192] MIXED order
hipError_t launch_wino24(const WinoParams& p, hipStream_t st);
// the same for a 48-channel source (48 -> 192, xconv5): src NHWC 48, upk [48 iterations][192 MIXED rows][32] (pack_wino24)
hipError_t launch_wino24_c48(const WinoParams& p, hipStream_t st);
// 48 -> 96 form (se_wino48.hip): src / dst NHWC 48 channels, upk [24 iterations][96 MIXED rows][32], bias [96] MIXED order
hipError_t launch_wino48(const WinoParams& p, hipStream_t st);
// 24 -> 96 in the same kernel (round 5; xconv3 / pmconv3): src NHWC 24 channels, upk [16 positions][96 MIXED rows][32 k:
// channels 0-23, then zeros] (pack_wino48_c24), one iteration per position, k-half 1 issues two k-steps
hipError_t launch_wino48_c24(const WinoParams& p, hipStream_t st);
// gen_deconv 96 -> 96 (48 gated), F(2x2,2x2) on the 4 sub-pixel classes (se_wino_up.hip): src NHWC 96 at (h, w), dst NHWC
// 48 at (2h, 2w), upk [4 classes][27 iterations][96 MIXED rows][32], bias [96] MIXED order; h, w even; th = h/2, tw = w/2
hipError_t launch_winoup(const WinoParams& p, hipStream_t st);
// gen_deconv 48 -> 48 (24 gated) in the same form (se_wino_up48.hip): src NHWC 48 at (h, w), dst NHWC 24 at (2h, 2w), upk
// [4 classes][14 iterations][48 MIXED rows][32] in the K pairing of the 48-channel kernels, bias [48] MIXED order
hipError_t launch_winoup48(const WinoParams& p, hipStream_t st);
// 3x3 stride 2, 48 -> 96 / 192, polyphase F(2,2) form, 25 of 36 products (se_s2poly.hip): src NHWC 48 at (h, w), h % 4 == w % 4 == 0,
// dst NHWC 48 `halves` at (h/2, w/2), upk [halves][38 iterations][96 MIXED rows][32] (pack_s2poly48), bias [96 halves] MIXED order;
// th = h/4, tw = w/4: tiles of 2x2 outputs
hipError_t launch_s2poly48(const WinoParams& p, int halves, hipStream_t st);

// ---------------------------------------------------------------------------------------------
// bf16 raw-tile form of the 3x3 stride-1 gated conv 96 -> 192 (se_rconv16.hip)
// ---------------------------------------------------------------------------------------------
struct RConvParams {
  const void* src;     // bf16 NHWC [B][h][w][96]
  const void* wpk;     // bf16 weights: image of pack_rconv16 [27 steps][12 row tiles][16 rows][32 k]
  const float* bias;   // [192] packed-row order (features, then gates)
  void* dst;           // bf16 NHWC [B][h][w][96]
  int B, h, w, d;      // dilation d; h % d == 0 and w % d == 0
  int hs, ws;          // polyphase sub-image size h/d x w/d
  int ty, tx;          // 8 x 16 tiles per sub-image
  int act;             // 0 ELU, 1 ReLU
  int xcd;             // 1: XCD-aware tile order
  const float* vbias;  // optional [B][9][192] fp32: folded vector source (launch_vecbias; d == 1)
  int dual;            // ws == 8, d even: two phases (py, px), (py, px + 1) side by side in one tile
};
hipError_t launch_rconv16(const RConvParams& p, hipStream_t st);

// ---------------------------------------------------------------------------------------------
// Raw-tile form of the 96-row bf16 gated convs, stride 1 (se_rconv96.hip): 3x3 48 -> 96 / 24 -> 96, gen_deconv 96 -> 96
struct RConv96Params {
  const void* src;     // bf16 NHWC [B][h][w][8 CG]
  const void* wpk;     // bf16 image of pack_rconv96: [class][step][6 row tiles][16 rows][32 k]
  const float* bias;   // [96] packed-row order (48 features, then 48 gates)
  void* dst;           // bf16 NHWC [B][h][w][48], or [B][2h][2w][48] for gen_deconv
  int B, h, w;         // source size
  int CG;              // 8-channel granules per source pixel (3, 6, 12)
  int ty, tx;          // 16 x 16 tiles of the source grid (stride 2: of the OUTPUT grid)
  int stride, oh, ow;  // 1, or 2 with the output size (3x3, 24 -> 96: de-interleaved raw tile, se_rconv96.hip)
  int up2;             // gen_deconv: four 2x2 sub-pixel classes
  int act;             // 0 ELU, 1 ReLU
  int xcd;             // 1: XCD-aware tile order
};
hipError_t launch_rconv96(const RConv96Params& p, hipStream_t st);

// ---------------------------------------------------------------------------------------------
// Raw-tile form of the narrow (MIXED-row) stride-1 gated convs, fp32 and bf16 (se_rtile.hip)
// ---------------------------------------------------------------------------------------------
struct RTileParams {
  const float* src;    // NHWC [B][Hin][Win][C] (fp32, or bf16 when `bf16`)
  const float* wpk;    // packed weight image of pack_direct ([class][chunk][NP rows][128 bytes])
  const float* bias;   // [NP] packed-row order
  float* dst;          // NHWC [B][OH][OW][G]
  int B, Hin, Win;     // source grid (= output grid; for up2 the output grid is 2x)
  int C;               // elements per source pixel (whole granules)
  int CG;              // granules per tap
  int T, KW;           // taps, taps per kernel row (up2: 4, 2)
  int magicCG, magicKW;
  int pad;             // top / left zero padding (k / 2); up2: 1 - class parity
  int up2, OH, OW;
  int G;               // stored output channels (row stride of dst)
  int nch, NP;         // 32-k (fp32) / 64-k (bf16) chunks, packed rows (48 or 32)
  int RH, RW;          // raw tile: 8 + KH - 1 rows, 16 + KW - 1 columns
  int raw_bytes;       // RH * RW * C * element size, rounded up to 1 KB
  unsigned div_cg_m, div_rw_m;   // udiv_magic numbers for (granules per pixel) and RW
  int div_cg_l, div_rw_l;
  int ty, tx;          // 8 x 16 tiles per image
  int act, bf16, xcd;
  int dense;           // > 0: dense-K form of the 5x5 first layers (fp32): `dense` = real input channels (3 or 5) out of the C
                       // stored per pixel; wpk is then the image of pack_layer_dense (k = tap * dense + channel, no channel padding);
                       // + 100: its F(2,5)-along-x form; 204: the bf16 pair-of-taps form (rtile_kernel<3, 8, true, true>:
                       // 8-byte pixels = the first four stored channels, wpk = image of pack_layer16_d4, RW = 21)
};
hipError_t launch_rtile(const RTileParams& p, hipStream_t st);
// 24 -> 24 3x3 stride 1 with F(2,3) along x (se_rtilew.hip): src NHWC 24, wpk = image of pack_rtilew ([4 positions][3 chunks]
// [24 physical rows][32 k]), bias [32] in the MIXED packed-row order, dst NHWC 12; Win even; ty = ceil(H / 16), tx = ceil(W / 16): blocks of 16 x 16 outputs, walked by persistent workgroups
hipError_t launch_rtilew(const RTileParams& p, hipStream_t st);
// the same layers with the two-dimensional F(2x2,3x3) transform (Hin and Win even): wpk = image of pack_rtilew2
// ([16 positions][24 physical rows][32 floats]: channels 0-15 in slots 0-3, channels 16+2q, 17+2q in slot 4+q)
hipError_t launch_rtilew2(const RTileParams& p, hipStream_t st);
int rtile_rows(bool bf16);    // output rows per workgroup tile (8 fp32, 32 bf16)

// ---------------------------------------------------------------------------------------------
// 3x3 conv 12 -> {1,3} raw output + fused tanh/sigmoid/composite (final layer of each decoder)
// ---------------------------------------------------------------------------------------------
struct SmallConvParams {
  const float* x;      // NHWC [B][H][W][12]
  const float* w;      // [COUT][9][12]
  const float* b;      // [COUT]
  int B, H, W, cout;
  int mode;            // 0: sigmoid -> mask (+hard);  1: tanh -> out;  2: tanh -> coarse + xnow;  3: tanh -> fine + composed;  4: raw
  float* out_nchw;     // mask / maskim / coarse / fine, NCHW (may be null for modes 2,3)
  float* hard;         // mode 0: (B,1,H,W) thresholded mask (may be null)
  const float* img;    // NCHW (B,3,H,W)   modes 2,3
  const float* mask;   // (B,1,H,W)        mode 2: hard mask; mode 3: soft mask
  float* xnow;         // mode 2: NHWC4 next-stage input
  float* composed;     // mode 3: NCHW (B,3,H,W) (may be null)
  int no_mask_coarse;
  // batch strides in floats (0 = dense): the packed output of SE_FLAG_PACKED_OUT is one (B,4,H,W) buffer, composed in
  // planes 0-2 and the soft mask in plane 3 (one all-gather of the packed outputs)
  long out_bs;         // of out_nchw (mode 0: the soft mask)
  long mask_bs;        // of mask (mode 3: the soft mask)
  long comp_bs;        // of composed
  int bf16;            // x is bf16 NHWC with a 16-channel pixel stride; xnow (mode 2) is written as bf16 NHWC8
  // mode 3: the output quantisation of test.py:25-27 fused into this last kernel (either may be null)
  unsigned char* rgb8; // (B,H,W,3) uint8 = trunc((composed + 1) / 2 * 255)
  unsigned char* m8;   // (B,H,W)   uint8 = trunc(soft mask * 255)
  // mode 0: (B,H,W) uint8 lock plane of an editing session (may be null): the mask is 0 where it is non-zero
  const unsigned char* lock;
  // mode 3 with rgb8 (SE_FLAG_RAW_FINE): rgb8 = trunc((fine + 1) / 2 * 255), the tanh output uncomposed, at
  // every pixel; composed and m8 are unchanged.  The kernel's RAW form; any other use is an invalid value.
  int raw_fine;
};
hipError_t launch_small_conv(const SmallConvParams& p, hipStream_t st);

// ---------------------------------------------------------------------------------------------
// Elementwise / layout / reductions
// ---------------------------------------------------------------------------------------------
// netM input: [image(3), sketch(1)] NCHW -> NHWC4
hipError_t launch_pack_m(const float* image, const float* sketch, float* dst4, int B, int H, int W, hipStream_t st);
// netG inputs: coarse NHWC8 = [x*(1-m) (3), guide, m, 0,0,0]; style NHWC8 = [x2*m2 (3) (or x2), g2, m2, 0,0,0],
// or with joint (guide * 0): style NHWC4 = [x2*m2 (3) (or x2), m2]
hipError_t launch_pack_g(const float* x, const float* x2, const float* mask, const float* mask2, const float* guide,
                         float* coarse8, float* style8, int B, int H, int W, int no_mask_cc, int joint,
                         hipStream_t st);
hipError_t launch_nchw_to_nhwc(const float* src, float* dst, int B, int C, int Cpad, int H, int W, hipStream_t st);
hipError_t launch_dequantize_u8(const unsigned char* rgb, const unsigned char* sk8, const float* lut, float* image, float* sketch,
                                int B, int H, int W, hipStream_t st);
hipError_t launch_nhwc_to_nchw(const float* src, float* dst, int B, int C, int Cstride, int H, int W, hipStream_t st);
// test.py:25-27 output quantisation: composed NCHW (B,3,H,W) -> rgb HWC uint8, mask (B,1,H,W) -> uint8; W % 4 == 0
hipError_t launch_quantize_u8(const float* composed, const float* mask, unsigned char* rgb, unsigned char* m8, int B, int H,
                              int W, hipStream_t st);
// column reduce over pixels: x [B][HW][C] -> out [B][C].  op 0 max, 1 mean, 2 rsqrt(sum(x^2)+1e-8)
// x_bf16: x holds bf16; out_bf16 (optional): a bf16 copy of the result (the style vector as a bf16 conv source)
hipError_t launch_colreduce(const float* x, float* partial, float* out, int B, int HW, int C, int op, hipStream_t st,
                            int x_bf16 = 0, float* out_bf16 = nullptr);
// bf16 forms of the input packing (NHWC8 bf16 for every network input) and of the unit-test layout converters
hipError_t launch_pack_m16(const float* image, const float* sketch, float* dst8, int B, int H, int W, hipStream_t st);
hipError_t launch_pack_g16(const float* x, const float* x2, const float* mask, const float* mask2, const float* guide,
                           float* coarse8, float* style8, int B, int H, int W, int no_mask_cc, int joint, hipStream_t st);
hipError_t launch_nchw_to_nhwc16(const float* src, float* dst, int B, int C, int Cpad, int H, int W, hipStream_t st);
hipError_t launch_nhwc16_to_nchw(const float* src, float* dst, int B, int C, int Cstride, int H, int W, hipStream_t st);
static const int COLREDUCE_SPLITS = 128;

// ---------------------------------------------------------------------------------------------
// Contextual attention (patch 4, stride 2)
// ---------------------------------------------------------------------------------------------
struct AttParams {
  const float* x;      // NHWC [B][h][w][96]   raw features (queries, values)
  const float* rn;     // [B][96]  1/sqrt(sum x^2 + 1e-8)
  float* xn;           // NHWC [B][h][w][96]   workspace: x * rn (keys)
  const float* hard;   // (B,1,4h,4w) full-resolution hole mask
  float* valid;        // unused (kept so that no kernel's argument offsets move)
  float* S;            // unused (likewise)
  float* out;          // NHWC [B][h][w][96]
  int B, h, w, hs, ws, L, Lp;
  float scale;         // softmax scale (10)
  float th;            // validity threshold (0.1)
  // ---- space-to-depth form (se_attention.hip, "v2"): class grid hc x wc = h/2 x w/2, R = hc*wc rows, Rp = R rounded up to 32
  int hc, wc, R, Rp;
  float* xT;           // [B][4 classes][96][Rp]  workspace: x transposed per parity class (A operand of the P~.V GEMM)
  float* E;            // [B][R][Rp] workspace: pixel-pair dot products E (three-pass form: later overwritten by P~)
  float* P;            // [B][R][Rp] workspace (fp32, or bf16 in bf16 mode): softmax probabilities in class-grid indexing (row = query,
                       // column = key); fused form: P~ is written here directly and P never exists
  float* Pt;           // where att2_pv_kernel reads P~: E (three-pass form) or P (fused form)
  float* stats;        // [B][R][2] fused form: row maximum and 1 / row sum of every query, in class-grid indexing
  float* kmul;         // [B][Rp] fused form: scale * log2(e) for a valid key, 0 for an invalid key or a non-key position
  float* kadd;         // [B][Rp] fused form: 0 for a key, -inf for a position that is not a key
  int guard;           // floats of guard band allocated in front of and behind E and in front of validR (>= wc + 8)
  float* validR;       // [B][Rp]    workspace: key validity in class-grid indexing: 1 / 0, -1 where the position is not a key
  float* similar;      // optional (B, L, hs, ws) NCHW copy of P for the unit-test entry point
  int bf16;            // x, xn, xT, P~ (in the E buffer) and out hold bf16; Rp is then a multiple of 64
  int e16;             // set by the launcher: E holds fp16 (bf16 mode, LDS-staged fused passes), as E[r][s] - ea[r] - eb[s]
  float* emean;        // [B][2][384] fp16-E form: mean over the class-grid positions of the query blocks X_r; rn times that (the key blocks' mean)
  float* epart;        // [B][hc][384] scratch of that mean's two-stage sum
  float* ea;           // [B][Rp] fp16-E form: row offset <X_r, mean XN>            (0 in the pad)
  float* eb;           // [B][Rp] fp16-E form: column offset <mean X, XN_s> - <mean X, mean XN>
  float* ea4;          // [B][Rp] fp16-E form: ea[q] + ea[q+1] + ea[q+wc] + ea[q+wc+1], the offset of S[q][.] owed to the query
  float* kadd2;        // [B][Rp] fp16-E form: kadd + (eb[k] + eb[k+1] + eb[k+wc] + eb[k+wc+1]) * kmul: the key half, folded into the key test
  int sym;             // set by the launcher: att2_pair_kernel computes the tiles on / right of the diagonal and mirrors them (fp32)
  int symT;            //   ... computed tiles per image (1-D grid)
};
hipError_t launch_attention(const AttParams& p, hipStream_t st);    // materialised space-to-depth form (E, P non-null)
// O(R) preparation of the space-to-depth form: xn, key tables (validR, kmul, kadd), transposed values xT (att2_prep, _transpose)
hipError_t launch_att2_prep(const AttParams& p, hipStream_t st);
// streaming form (se_att_stream.hip): E = P = null; needs xn, xT (plus att_stream_xt_tail() zeroed floats behind it), validR,
// kmul, kadd, stats ([B][R][2]); nothing R x R
hipError_t launch_attention_stream(const AttParams& p, hipStream_t st);
int att_stream_xt_tail();

// ---------------------------------------------------------------------------------------------
// Pillow-exact uint8 resampling (se_resize.hip; the resize steps of demo.py:39-73).  Coefficient tables per axis:
// bounds[2 * out] = (first input index, tap count), kk[out * ksize] = fixed-point weights (22 fractional bits).
// ---------------------------------------------------------------------------------------------
int resample_ksize(int in, int out, int filter);            // taps per output (the table's row length), -1 for bad arguments
int resample_coeffs(int in, int out, int filter, int* bounds, int* kk);     // host only; returns ksize
enum { RESIZE_OUT_U8 = 0, RESIZE_OUT_IMAGE_F32 = 1, RESIZE_OUT_SKETCH_F32 = 2, RESIZE_OUT_LOCK_U8 = 3 };
// what the LAST pass writes: uint8 (B,H,W,C); or the forward's fp32 NCHW inputs -- (B,C,H,W) = lut[v], or (v > 0); or, for a
// lock plane (C == 1), uint8 (B,H,W) = (v > 0) in {0, 1}
struct ResizeOut {
  int mode;
  unsigned char* u8;
  float* f32;
  const float* lut;    // RESIZE_OUT_IMAGE_F32: 256 floats (the ctx's dequantisation table)
  int H, W;            // output size of the whole resize
};
// horizontal pass: (B, Hrows, Win, C) -> (B, Hrows, Wout, C); h_bounds = the host copy of d_bounds (LDS sizing)
hipError_t launch_resample_h(const unsigned char* in, const int* d_bounds, const int* d_kk, const int* h_bounds, int ksize,
                             int B, int Hrows, int Win, int Wout, int C, const ResizeOut& o, hipStream_t st);
// vertical pass: (B, Hin, W, C) -> (B, Hout, W, C)
hipError_t launch_resample_v(const unsigned char* in, const int* d_bounds, const int* d_kk, int ksize, int B, int Hin, int Hout,
                             int W, int C, const ResizeOut& o, hipStream_t st);
// the ends of a scaled window edit; d_wins = B se_window records in DEVICE memory, as below.
// gather end: the horizontal pass with its rows taken from the hs x ws windows of the frames (C == 3) or from the requests'
// contiguous (hs, ws) window sketches (C == 1) -> (B, hs, Wout, C) as `o` says; reads no byte outside a window's own rows
hipError_t launch_window_resample_h(const se_window* d_wins, const int* d_bounds, const int* d_kk, const int* h_bounds, int ksize,
                                    int B, int hs, int ws, int Wout, int C, const ResizeOut& o, hipStream_t st);
// paste end: the vertical pass Hin -> hs of rgb (B,Hin,P,3) and m8 (B,Hin,P) (row pitch P pixels, P % 4 == 0, P >= ws, both
// 4-byte aligned) with the paste rule as its epilogue: frame[y0 + y, x0 + x, :] = the resampled colour where the resampled
// mask byte is > 0, every other byte of the frame untouched
// locked: d_wins = 2 B records, wins[B + b].frame_u8 = request b's (Hi,Wi) lock plane or null; a pixel whose
// byte of the plane at its frame position is non-zero is not written, whatever the resampled mask says
hipError_t launch_window_paste_v(const se_window* d_wins, const unsigned char* rgb, const unsigned char* m8, const int* d_bounds,
                                 const int* d_kk, int ksize, int B, int Hin, int hs, int P, int ws, hipStream_t st, bool locked = false);
// the gather end for lock planes: d_wins = 2 B records as above; the horizontal pass over the planes' hs x ws windows ->
// (B, hs, Wout) as `o` says (zeros for a null plane); reads no byte outside a window's own rows
hipError_t launch_window_lock_resample_h(const se_window* d_wins, const int* d_bounds, const int* d_kk, const int* h_bounds, int ksize,
                                         int B, int hs, int ws, int Wout, const ResizeOut& o, hipStream_t st);
// largest tap count the kernels take (48 KiB of LDS per block): a bicubic downscale by more than ~2000x is refused
constexpr int RESAMPLE_MAX_KSIZE = 8191;

// ---------------------------------------------------------------------------------------------
// Window edits of a resident frame (se_window.hip).  d_wins = B se_window records in DEVICE memory (the ctx's table).
// ---------------------------------------------------------------------------------------------
// each frame's H x W window -> image (B,3,H,W) = lut[v], sketch (B,1,H,W) = (v > 0); either output may be NULL; W % 4 == 0,
// outputs 16-byte aligned
hipError_t launch_window_gather(const se_window* d_wins, const float* lut, float* image, float* sketch, int B, int H, int W,
                                hipStream_t st);
// m8 (B,H,W) -> hits (B,4): pixels >= 128 on the mask's top / bottom / left / right edge, 0 for a side on which the hs x ws
// frame-space window lies on the frame's own edge (hs x ws == H x W unless the edit runs at a working size)
hipError_t launch_window_border(const se_window* d_wins, const unsigned char* m8, int* hits, int B, int H, int W, int hs, int ws,
                                hipStream_t st);
// frame[y0 + y, x0 + x, :] = rgb[b, y, x, :] where m8[b, y, x] > 0; rgb (B,H,W,3) and m8 (B,H,W) 4-byte aligned, W % 4 == 0
// locked: d_wins = 2 B records, wins[B + b].frame_u8 = request b's (Hi,Wi) lock plane or null, and the rule
// gains `and lock[y0 + y, x0 + x] == 0`
hipError_t launch_window_paste(const se_window* d_wins, const unsigned char* rgb, const unsigned char* m8, int B, int H, int W,
                               hipStream_t st, bool locked = false);
// the feathered paste (include/sketchedit_feather.h; se_feather.hip): d_wins = 2 B records as for the locked paste;
// rgb (B,hs,ws,3) and m8 (B,hs,ws) at the window's size, any hs, ws >= 16 and any alignment; radius 0 .. 16.  Only bytes of
// selected pixels are written; no byte outside a window's own rows is read.
hipError_t launch_window_paste_feather(const se_window* d_wins, const unsigned char* rgb, const unsigned char* m8, int B, int hs, int ws,
                                       int radius, hipStream_t st);
// d_wins = 2 B records as above: each plane's H x W window -> out (B,H,W) uint8 = (v > 0) in {0, 1}, zeros for a null plane;
// W % 8 == 0, out 8-byte aligned; no byte outside a window's rows is read
hipError_t launch_window_lock_gather(const se_window* d_wins, unsigned char* out, int B, int H, int W, hipStream_t st);
// the undo journal.  d_wins = 2 B records: the requests, then B records whose frame_u8 is the request's slot
// (hs rows of round_up(3 ws, 16) bytes, 16-byte aligned).  save: the hs x ws rectangle -> the slot; swap: rectangle <-> slot.
// Any hs, ws; no byte outside a window's rows is read, none outside the rectangle written.
hipError_t launch_window_journal(const se_window* d_wins, int B, int hs, int ws, bool swap, hipStream_t st);
// region edits: the (Hi,Wi) uint8 plane (any alignment) in tile x tile squares, tile in {16, 32, 64} -> tiles_out
// (ceil(Hi / tile), ceil(Wi / tile), 5) int32 = [count of pixels > 0, y0, x0, y1, x1] (the tight half-open box in frame
// coordinates; five zeros for an empty square).  Every record is written; no byte outside the plane is read.
hipError_t launch_sketch_tiles(const unsigned char* plane, int Hi, int Wi, int tile, int* tiles_out, hipStream_t st);
// strokes as polylines: segs (N,5) int32 [ax, ay, bx, by, r] in quarter pixels of the frame -> sketch_out (B,hs,ws)
// uint8, any alignment: 255 where a segment of request b's range covers the pixel's centre, else 0.  d_wins = 2 B records, the
// second B carrying the ranges (Hi = first, Wi = count).  Every byte of sketch_out is written, none outside it; any int32 in
// segs is safe (clamped to the rule's limits).  nseg_sum = the ranges' counts added up (the profiler's byte estimate).
hipError_t launch_sketch_strokes(const se_window* d_wins, int B, int hs, int ws, const int* segs, long nseg_sum, unsigned char* sketch_out,
                                 hipStream_t st);
// fills of a painted region (include/sketchedit_fill.h; se_fill.hip).  masks: fill (B,H,W) and lock (B,H,W) or null,
// uint8, non-zero = set -> hole (B,H,W) fp32 = fill & ~lock in {0, 1}, the same into `hard` and zeros into `zero` where those are
// not null; every pointer 16-byte aligned, H % 8 == W % 8 == 0; every float of every plane is written.
hipError_t launch_fill_masks(const unsigned char* fill, const unsigned char* lock, float* hole, float* hard, float* zero, int B, int H,
                             int W, hipStream_t st);
// keep: d_wins = 4 B records -- the requests, then B records each whose frame_u8 is the request's (Hi,Wi) fill plane, lock plane
// or null, keep plane.  The hs x ws rectangle of the keep plane = 255 where fill == 0 or lock != 0, else 0.  Any hs, ws and any
// alignment; no byte outside the rectangle's rows is read, none outside the rectangle written.
hipError_t launch_fill_keep(const se_window* d_wins, int B, int hs, int ws, hipStream_t st);
// selection by colour (include/sketchedit_select.h; se_select.hip), on a state plane (Hi,Wi) uint8: 0 not similar,
// 1 similar and not reached, 255 reached.  Any Hi, Wi and any alignment; no byte outside a plane or the frame is read or written.
// similar: every byte of `state` written from the frame (Hi,Wi,3) and the seed's colour, read on the device.
hipError_t launch_select_similar(const unsigned char* frame, int Hi, int Wi, int seed_y, int seed_x, int tolerance, int contiguous,
                                 unsigned char* state, hipStream_t st);
// flood: ONE pass, a wave per 64 x 64 tile; stores 255 to newly reached bytes and 1 to *changed if it stored any (never 0)
hipError_t launch_select_flood(unsigned char* state, int Hi, int Wi, unsigned* changed, hipStream_t st);
// grow: out (another buffer) = 255 where a reached byte lies within Chebyshev distance `grow` (0 .. 16), else 0; every byte written
hipError_t launch_select_grow(const unsigned char* state, int Hi, int Wi, int grow, unsigned char* out, hipStream_t st);
// modify a selection's shape (include/sketchedit_modify.h; se_modify.hip).  Any Hi, Wi >= 16 and any alignment of the
// planes; no byte outside a plane is read or written.  Every byte of `out` (another buffer) <- `plane` expanded or contracted by
// the disc of `radius` (1 .. 32), or smoothed by the majority vote in it (op: SE_MODIFY_*), as 0 / 255.  ONE launch.
hipError_t launch_plane_modify(const unsigned char* plane, int Hi, int Wi, int op, int radius, unsigned char* out, hipStream_t st);
// lasso selections and their algebra (include/sketchedit_lasso.h; se_lasso.hip).  Any Hi, Wi >= 16 and any alignment
// of the planes; no byte outside a plane or the edge buffer is read or written.
// lasso_fill: every byte of plane_out (Hi,Wi) <- the even-odd fill of the N edges [ax, ay, bx, by] (int32, quarter pixels)
hipError_t launch_lasso_fill(const int* edges, int N, int Hi, int Wi, unsigned char* plane_out, hipStream_t st);
// plane_combine: out <- a op b as 0 / 255 (op: SE_COMBINE_*; b null for INVERT); out may be exactly a or exactly b
hipError_t launch_plane_combine(const unsigned char* a, const unsigned char* b, int Hi, int Wi, int op, unsigned char* out, hipStream_t st);
// the outline of a selection (include/sketchedit_outline.h; se_outline.hip): the boundary runs of plane != 0 per
// 64 x 64 tile as lasso edges.  Any Hi, Wi >= 16 and any alignment of the plane; no byte outside it is read.  cnt: 4 int32 per
// tile (N, S, E, W).  count: every cnt word <- its tile's run count.  scan: cnt <- its exclusive scan, in place;
// info_out = {total, min(total, cap)}.  emit: the records whose index in the definition's order is < cap -> edges_out (4-byte
// aligned); no other byte of it is written.
hipError_t launch_outline_count(const unsigned char* plane, int Hi, int Wi, int* cnt, hipStream_t st);
hipError_t launch_outline_scan(int* cnt, int Hi, int Wi, int cap, int* info_out, hipStream_t st);
hipError_t launch_outline_emit(const unsigned char* plane, int Hi, int Wi, const int* offs, int* edges_out, int cap, hipStream_t st);
// move or clone a selection (include/sketchedit_move.h; se_move.hip).  Any Hi, Wi >= 16 and any alignment of the
// frame and the planes.  move_drop: the selected pixels of the box, as the lift (a journal slot of the rectangle at (ly0, lx0),
// lw wide, rows of lpitch bytes) holds them, blended into the frame at the offset / flip; only the tiles of the shifted box
// clipped to the frame are launched, none when that is empty.  plane_shift: every byte of `out` <- the moved selection, 0 / 255.
hipError_t launch_move_drop(unsigned char* frame, int Hi, int Wi, const unsigned char* lift, int ly0, int lx0, int lw, int lpitch,
                            const unsigned char* sel, const unsigned char* lock, int by0, int bx0, int by1, int bx1, int dy, int dx, int flip,
                            int radius, hipStream_t st);
hipError_t launch_plane_shift(const unsigned char* sel, int Hi, int Wi, int by0, int bx0, int by1, int bx1, int dy, int dx, int flip,
                              unsigned char* out, hipStream_t st);
// seamless move and clone (include/sketchedit_blend.h; se_blend.hip): move_drop's arguments and a workspace of
// blend_workspace_bytes(eh, ew) bytes, 16-byte aligned, for the eh x ew rectangle E -- the shifted box clipped to the frame, grown
// by one pixel and clipped again.  The launches are a function of eh and ew alone; none when the box lands outside the frame.
size_t blend_workspace_bytes(int eh, int ew);
hipError_t launch_move_blend(unsigned char* frame, int Hi, int Wi, const unsigned char* lift, int ly0, int lx0, int lh, int lw, int lpitch,
                             const unsigned char* sel, const unsigned char* lock, int by0, int bx0, int by1, int bx1, int dy, int dx, int flip,
                             void* ws, hipStream_t st);
// the canvas of a session (include/sketchedit_canvas.h; se_canvas.hip): out (Hn,Wn,C) <- the rectangle at (oy, ox) of
// in (Hi,Wi,C; NULL: zeros) under `orient`, folded by `pad` (SE_CANVAS_*; rgb: the constant's C bytes).  Any sizes >= 1 and any
// alignment.  ONE launch: canvas_map without the transpose bit, canvas_turn (64 x 32 tiles through the LDS) with it.
hipError_t launch_canvas(const unsigned char* in, int Hi, int Wi, int C, unsigned char* out, int Hn, int Wn, int oy, int ox, int orient,
                         int pad, unsigned rgb, hipStream_t st);
// blur, sharpen or pixelate a selection (include/sketchedit_filter.h; se_filter.hip).  Any Hi, Wi >= 16 and any
// alignment of the frame and the planes; the frame is only written, every input pixel comes from the lift.  taps: radius + 1 ints
// on the host.  filter_blur: the grid is the box's 64 x 16 tiles, the LDS that of the radius' class; filter_mosaic: a wave per cell.
hipError_t launch_filter_blur(unsigned char* frame, int Hi, int Wi, const unsigned char* lift, int ly0, int lx0, int lw, int lpitch,
                              const unsigned char* sel, const unsigned char* lock, int by0, int bx0, int by1, int bx1, const int* taps,
                              int radius, int amount, int feather, hipStream_t st);
hipError_t launch_filter_mosaic(unsigned char* frame, int Hi, int Wi, const unsigned char* lift, int ly0, int lx0, int lw, int lpitch,
                                const unsigned char* sel, const unsigned char* lock, int by0, int bx0, int by1, int bx1, int cell, int amount,
                                int feather, hipStream_t st);
// adjust a selection's tone and colour (include/sketchedit_adjust.h; se_adjust.hip).  Any Hi, Wi >= 16 and any
// alignment of the frame, the planes and the table.  adjust: the grid is the box's 64 x 16 tiles, the frame is only written, every
// input pixel comes from the lift; lut: 768 bytes on the device or nullptr, matrix: 12 ints on the host or nullptr.  hist_tiles:
// adjust_hist_groups(box height, box width) workgroups, each writing 1024 words of `slabs`; hist_sum adds them into `hist`.
int adjust_hist_groups(int bh, int bw);
hipError_t launch_adjust(unsigned char* frame, int Hi, int Wi, const unsigned char* lift, int ly0, int lx0, int lw, int lpitch,
                         const unsigned char* sel, const unsigned char* lock, int by0, int bx0, int by1, int bx1, const unsigned char* lut,
                         const int* matrix, int amount, int feather, hipStream_t st);
hipError_t launch_hist_tiles(const unsigned char* frame, int Wi, const unsigned char* sel, int by0, int bx0, int by1, int bx1, unsigned* slabs,
                             hipStream_t st);
hipError_t launch_hist_sum(const unsigned* slabs, int groups, unsigned* hist, hipStream_t st);
hipError_t launch_adjust_lut(const unsigned* hist_src, const unsigned* hist_ref, int mode, int which, int clip, unsigned char* lut, hipStream_t st);
// scale and rotate a selection (include/sketchedit_warp.h; se_warp.hip).  Any Hi, Wi >= 16 and any alignment of the
// frame and the planes.  m: the six Q16 values of the inverse map, on the host.  warp_drop: the selected pixels of the box, as
// the lift holds them, gathered through m with bilinear taps and blended by their coverage into the rectangle (ry0, rx0, rh, rw)
// of the frame, whose tiles are the grid.  plane_warp: every byte of `out` <- 255 where the coverage is at least a half, else 0.
hipError_t launch_warp_drop(unsigned char* frame, int Hi, int Wi, const unsigned char* lift, int ly0, int lx0, int lw, int lpitch,
                            const unsigned char* sel, const unsigned char* lock, int by0, int bx0, int by1, int bx1, int ry0, int rx0,
                            int rh, int rw, const long long* m, hipStream_t st);
hipError_t launch_plane_warp(const unsigned char* sel, int Hi, int Wi, int by0, int bx0, int by1, int bx1, const long long* m,
                             unsigned char* out, hipStream_t st);
// the device PNG encoder (include/sketchedit_png.h): the hs x ws rectangles of d_wins (B records) -> their zlib
// streams.  rows: ftype (B,hs) uint8, each row's filter type.  stripes: one workgroup per stripe of 32 rows -> its deflate blocks
// in its slot of png_slot_bytes(ws) bytes (16-byte aligned), its size in sizes (B,S) and its Adler parts in parts (B,S,2), S =
// png_stripes(hs).  finish: the streams, concatenated, at out + b cap (any alignment) and their lengths in sizes_out (B).
int png_stripes(int hs);
size_t png_stripe_bound(size_t n);
size_t png_slot_bytes(int ws);
hipError_t launch_png_rows(const se_window* d_wins, int B, int hs, int ws, unsigned char* ftype, hipStream_t st);
hipError_t launch_png_stripes(const se_window* d_wins, int B, int hs, int ws, const unsigned char* ftype, unsigned* sizes, unsigned* parts,
                              unsigned char* slots, hipStream_t st);
hipError_t launch_png_finish(int B, int hs, int ws, const unsigned* sizes, const unsigned* parts, const unsigned char* slots, unsigned char* out,
                             size_t cap, unsigned long long* sizes_out, hipStream_t st);
// the device JPEG encoder (include/sketchedit_jpg.h and sketchedit_jpg2.h; flags = SE_JPG_420 |
// SE_JPG_OPTIMIZE): the hs x ws rectangles of d_wins (B records) -> their entropy-coded segments.  blocks: coef (B,R,n,64) int16,
// the quantised coefficients in zigzag order, R = jpg_rows(hs, flags) rows of n = jpg_row_blocks(ws, flags) blocks (Y, Cb, Cr per
// MCU of 8 pixel rows; blocks420, under SE_JPG_420: 4 Y, Cb, Cr per MCU of 16).  hist (SE_JPG_OPTIMIZE): one partial histogram of
// 4 x 256 counters per row, hist (B,R,4,256).  tables: per image the codes (B,4,256), (code << 5) | length per symbol, and the
// record of 4 x 272 bytes at tables_out + 1088 b (4-byte aligned).  rows: one workgroup per row -> its restart interval, stuffed,
// with its marker, in its slot of jpg_slot_bytes(n, flags) bytes (16-byte aligned) and its size in sizes (B,R); the tables from
// `codes` or, where that is null, Annex K's.  finish: the rows, concatenated, at out + b cap (any alignment) and their lengths in
// sizes_out (B).
int jpg_rows(int hs, int flags);
int jpg_row_blocks(int ws, int flags);
size_t jpg_row_bound(int nblk, int flags);
size_t jpg_slot_bytes(int nblk, int flags);
hipError_t launch_jpg_blocks(const se_window* d_wins, int B, int hs, int ws, int quality, short* coef, hipStream_t st);
hipError_t launch_jpg2_blocks420(const se_window* d_wins, int B, int hs, int ws, int quality, short* coef, hipStream_t st);
hipError_t launch_jpg2_hist(int B, int R, int nblk, int flags, const short* coef, unsigned* hist, hipStream_t st);
hipError_t launch_jpg2_tables(int B, int R, const unsigned* hist, unsigned* codes, unsigned char* tables_out, hipStream_t st);
hipError_t launch_jpg_rows(int B, int R, int nblk, int flags, const short* coef, const unsigned* codes, unsigned* sizes,
                           unsigned char* slots, hipStream_t st);
hipError_t launch_jpg_finish(int B, int R, int nblk, size_t slot_bytes, const unsigned* sizes, const unsigned char* slots,
                             unsigned char* out, size_t cap, unsigned long long* sizes_out, hipStream_t st);

}  // namespace se
