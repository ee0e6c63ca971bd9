// Host side of libsketchedit_hip.so: context, workspace arena, kernel dispatch and the forward plans of
// netM / netG / inference behind the C-ABI declared in include/sketchedit_hip.h (weight images: se_pack.hip).
//
// Layer tables restate the reference constructors
//   DeepFillC2Generator.__init__  /root/reference/models/networks/editline_g.py:44-100
//   MDGenerator.__init__          /root/reference/models/networks/editline2_g.py:18-43
// and the plans restate the forward methods (editline_g.py:119-221, editline2_g.py:59-94,
// editline2_model.py:128-133,338-370).
#include "../../include/sketchedit_hip.h"
#include "../../include/sketchedit_png.h"
#include "../../include/sketchedit_jpg.h"
#include "../../include/sketchedit_jpg2.h"
#include "../../include/sketchedit_feather.h"
#include "../../include/sketchedit_fill.h"
#include "../../include/sketchedit_select.h"
#include "../../include/sketchedit_lasso.h"
#include "../../include/sketchedit_outline.h"
#include "se_kernels.h"
#include "se_pack.h"

#include <cstdarg>
#include <cstdint>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <map>
#include <mutex>
#include <numeric>
#include <string>
#include <vector>

using namespace se;

namespace {


#define ENC(p)                                                                                    \
  {p "2_downsample", 24, 96, 3, 2, 1, ACT_ELU, 0}, {p "3", 48, 96, 3, 1, 1, ACT_ELU, 0},          \
      {p "4_downsample", 48, 192, 3, 2, 1, ACT_ELU, 0}, {p "5", 96, 192, 3, 1, 1, ACT_ELU, 0},    \
      {p "6", 96, 192, 3, 1, 1, ACT_ELU, 0}, {p "7_atrous", 96, 192, 3, 1, 2, ACT_ELU, 0},        \
      {p "8_atrous", 96, 192, 3, 1, 4, ACT_ELU, 0}, {p "9_atrous", 96, 192, 3, 1, 8, ACT_ELU, 0}, \
      {p "10_atrous", 96, 192, 3, 1, 16, ACT_ELU, 0}
#define DEC(p, c11in, c17out)                                                                        \
  {p "11", c11in, 192, 3, 1, 1, ACT_ELU, 0}, {p "12", 96, 192, 3, 1, 1, ACT_ELU, 0},                 \
      {p "13_upsample_conv", 96, 96, 3, 1, 1, ACT_ELU, 1}, {p "14", 48, 96, 3, 1, 1, ACT_ELU, 0},    \
      {p "15_upsample_conv", 48, 48, 3, 1, 1, ACT_ELU, 1}, {p "16", 24, 24, 3, 1, 1, ACT_ELU, 0},    \
      {p "17", 12, c17out, 3, 1, 1, ACT_NONE, 0}

const LayerDef G_LAYERS[] = {
    {"conv1", 5, 48, 5, 1, 1, ACT_ELU, 0}, ENC("conv"), DEC("conv", 192, 3),
    {"wconv1", 5, 48, 5, 1, 1, ACT_ELU, 0}, ENC("wconv"),
    {"xconv1", 3, 48, 5, 1, 1, ACT_ELU, 0},
    {"xconv2_downsample", 24, 48, 3, 2, 1, ACT_ELU, 0}, {"xconv3", 24, 96, 3, 1, 1, ACT_ELU, 0},
    {"xconv4_downsample", 48, 96, 3, 2, 1, ACT_ELU, 0}, {"xconv5", 48, 192, 3, 1, 1, ACT_ELU, 0},
    {"xconv6", 96, 192, 3, 1, 1, ACT_ELU, 0}, {"xconv7_atrous", 96, 192, 3, 1, 2, ACT_ELU, 0},
    {"xconv8_atrous", 96, 192, 3, 1, 4, ACT_ELU, 0}, {"xconv9_atrous", 96, 192, 3, 1, 8, ACT_ELU, 0},
    {"xconv10_atrous", 96, 192, 3, 1, 16, ACT_ELU, 0},
    {"pmconv1", 3, 48, 5, 1, 1, ACT_ELU, 0},
    {"pmconv2_downsample", 24, 48, 3, 2, 1, ACT_ELU, 0}, {"pmconv3", 24, 96, 3, 1, 1, ACT_ELU, 0},
    {"pmconv4_downsample", 48, 192, 3, 2, 1, ACT_ELU, 0}, {"pmconv5", 96, 192, 3, 1, 1, ACT_ELU, 0},
    {"pmconv6", 96, 192, 3, 1, 1, ACT_RELU, 0}, {"pmconv9", 96, 192, 3, 1, 1, ACT_ELU, 0},
    {"pmconv10", 96, 192, 3, 1, 1, ACT_ELU, 0},
    DEC("allconv", 192, 3),
};
const LayerDef M_LAYERS[] = {
    {"conv1", 4, 48, 5, 1, 1, ACT_ELU, 0}, ENC("conv"), DEC("conv", 96, 3), DEC("conv_mask_", 96, 1),
};
const int NG = sizeof(G_LAYERS) / sizeof(LayerDef), NM = sizeof(M_LAYERS) / sizeof(LayerDef);


// ---- workspace arena: first-fit free list over [0, cap) in bytes, 256-B aligned ------------------
struct Arena {
  struct Blk { size_t off, size; bool used; };
  std::vector<Blk> blks;
  size_t cap = 0, peak = 0;
  bool dry = false;
  char* base = nullptr;
  void reset(char* b, size_t c, bool d, int which = 0) {
    // dry runs only measure: any non-null fake base (the two arenas of a plan get disjoint fake ranges)
    base = d ? (char*)(which ? ((size_t)1 << 62) + 4096 : 4096) : b;
    cap = d ? (size_t)1 << 61 : c; dry = d; peak = 0;
    blks.clear(); blks.push_back({0, cap, false});
  }
  bool owns(const void* p) const { return (size_t)p >= (size_t)base && (size_t)p < (size_t)base + cap; }
  float* alloc(size_t nfloats) {
    size_t need = (nfloats * 4 + 255) & ~(size_t)255;
    for (size_t i = 0; i < blks.size(); ++i) {
      if (!blks[i].used && blks[i].size >= need) {
        size_t off = blks[i].off;
        if (blks[i].size > need) {
          Blk rest{off + need, blks[i].size - need, false};
          blks[i].size = need;
          blks.insert(blks.begin() + i + 1, rest);
        }
        blks[i].used = true;
        if (off + need > peak) peak = off + need;
        return (float*)(base + off);
      }
    }
    return nullptr;
  }
  void release(const float* p) {
    if (!p) return;
    size_t off = (const char*)p - base;
    for (size_t i = 0; i < blks.size(); ++i) {
      if (blks[i].off == off && blks[i].used) {
        blks[i].used = false;
        if (i + 1 < blks.size() && !blks[i + 1].used) { blks[i].size += blks[i + 1].size; blks.erase(blks.begin() + i + 1); }
        if (i > 0 && !blks[i - 1].used) { blks[i - 1].size += blks[i].size; blks.erase(blks.begin() + i); }
        return;
      }
    }
  }
};

}  // namespace

struct se_ctx {
  int device = 0;
  std::mutex mu;
  std::string err;
  std::map<std::string, Layer> G, M;
  Layer wconv1_j4;          // G.wconv1 packed for a 4-channel input: with --joint_train_inp its guide channel is zero
  float* zeros = nullptr;   // zero page for out-of-bounds granules
  float* lut8 = nullptr;    // 256 floats: (v/255 - 0.5)/0.5, the dataset's normalisation of a uint8 value (se_dequantize_u8)
  Arena arena;              // workspace arena of the main branch
  Arena arena2;             // low-latency mode: arena of the concurrent side branch (disjoint region of the workspace)
  hipStream_t st = nullptr; // stream the next launch goes to
  hipStream_t st_main = nullptr;
  hipStream_t st_side = nullptr;        // side-branch stream (created with the ctx, non-blocking)
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  bool dry = false;
  bool low_latency = false; // SE_FLAG_LOW_LATENCY of the running call
  int cur_net = SE_NET_G;   // network whose plan is running (plan_netM / plan_netG; per-op entry points: G)
  bool bf16 = false;        // SE_FLAG_BF16 of the running call: bf16 activations / weights, fp32 accumulate
  bool serial = false;             // default mode on one stream (set while the profiler is on: per-kernel durations)
  bool fork2 = true;               // SE_FORK_DEFAULT, snapshot taken where a call enters the library
  bool conservative = false;       // SE_FLAG_CONSERVATIVE of the running call: netM's 96 -> 192 layers on F(2x2,3x3)
  const se_netG_taps* taps = nullptr;      // se_netG_forward_taps: intermediate outputs of the running netG plan
  float* vbias_ws = nullptr;       // [B][9][192] scratch for the folded vector source of the next two-source layer (plan_netG)
  const float* vec32 = nullptr;    // bf16 mode: the fp32 copy of the vector source (the conv source itself is its bf16 rounding)
  unsigned char* rgb8 = nullptr;   // se_inference_u8: uint8 outputs written by the last kernel of the running call
  unsigned char* m8 = nullptr;
  Profiler prof;
  struct Peaks { size_t main, side; };
  std::map<std::vector<long long>, Peaks> peaks;      // dry-run arena peaks per (B, H, W, flags, outputs wanted)
  size_t dry_max_act = 0;                             // dry runs: bytes of the largest activation tensor the plan allocated
  std::map<std::vector<long long>, long long> act_per_img;      // (H, W, bf16) -> bytes per image of the largest activation
  struct GraphEntry {
    std::vector<long long> key;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    hipStream_t stream = nullptr;        // stream of the last launch: synchronised before the exec is destroyed
    unsigned long long last_use = 0;     // LRU stamp
  };
  unsigned long long graph_clock = 0;
  std::vector<GraphEntry> graphs;                     // SE_FLAG_GRAPH: captured forwards, keyed by every argument
  // Pillow-exact resize (se_resize.hip): coefficient tables per (in, out, filter), least recently used evicted beyond 64;
  // the uint8 intermediate of the two passes; the stream the last resize ran on (a call on another stream waits for it)
  struct ResampleTable {
    int in, out, filter, ksize;
    std::vector<int> host;            // bounds (2 out) then weights (out ksize): the upload's source, kept while cached
    int* dev = nullptr;
    unsigned long long last_use = 0;
  };
  std::vector<ResampleTable> rs_tables;
  unsigned long long rs_clock = 0;
  unsigned char* rs_scratch = nullptr;
  size_t rs_scratch_bytes = 0;
  hipStream_t rs_stream = nullptr;
  bool rs_used = false;
  hipEvent_t rs_event = nullptr;
  // window edits (se_window.hip): the se_window records of a call reach the device through a ring -- pinned host memory and
  // its device mirror, a call takes the next B records of both.  The ring has two halves: a half is reused only after the
  // event recorded when it was last left, i.e. after every copy and kernel that used it (win_put).  Like the resize
  // resources it is used in the order of one stream; a call on another stream waits for the previous one's work.
  se_window* win_host = nullptr;
  se_window* win_dev = nullptr;
  size_t win_cap = 0, win_pos = 0;
  hipEvent_t win_half_done[2] = {nullptr, nullptr};
  bool win_half_used[2] = {false, false};
  hipStream_t win_stream = nullptr;
  bool win_used = false;
  hipEvent_t win_event = nullptr;
};

namespace {

thread_local std::string g_create_err;

int fail(se_ctx* c, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf; else g_create_err = buf;
  return 1;
}
#define HIPCHK(c, call)                                                                   \
  do {                                                                                    \
    hipError_t e_ = (call);                                                               \
    if (e_ != hipSuccess) return fail(c, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

int xcd_remap_enabled() { return opt(OPT_XCD_REMAP); }     // SE_XCD_REMAP=0 switches the XCD-aware tile order off (A/B measurements)

// Every raw-tile / Winograd / gather kernel addresses its source through a buffer resource with 32-bit BYTE offsets and uses
// byte offset 0x80000000 as the "outside the image -> hardware zero fill" sentinel, so a tensor one launch addresses must stay
// below 2^31 BYTES (the guards used to count elements).  The forwards never reach the limit: they split
// the batch into passes (batch_passes).  SE_TEST_OFFSET_LIMIT (se_debug_set_option only) lowers it so that the tests reach the
// split with a handful of small images.
long long addr_limit() {
  const int v = opt(OPT_TEST_OFFSET_LIMIT);
  return v > 0 ? (long long)v : (1ll << 31);
}

// SE_TEST_POISON (se_debug_set_option only; 0, the default: nothing happens, no call is added).  A value v in 1..255: every
// scratch region is filled with the byte v when it is handed out, on the stream its first producer will be enqueued on -- so a
// kernel that reads a byte nobody wrote (pad channels and columns, guard bands, ragged tiles) reads v, whatever the memory held
// before (tests/test_gpu_poison.py: 0xFF is a NaN in every float type, 0x47 / 0xC7 are large finite values of either sign).
// Regions: every arena block (Plan::alloc_raw), the scratch of the per-op entry points, every region a call carves out of the
// workspace outside the arenas, the resize intermediate at each use.  Not the weight images, not the window record ring.
// While it is set, an SE_FLAG_GRAPH call runs uncaptured and enters nothing into the graph cache (se_inference).
// (A value outside 1..255 is off, like 0: 256 must not turn into a fill with zeros, the one byte the aid exists to avoid.)
int poison_byte() {
  const int v = opt(OPT_TEST_POISON);
  return v >= 1 && v <= 255 ? v : 0;
}
int poison(se_ctx* c, void* p, size_t bytes, hipStream_t st) {
  const int v = poison_byte();
  if (!v || !p || !bytes) return 0;
  HIPCHK(c, hipMemsetAsync(p, v, bytes, st));
  return 0;
}

// ---- launching one gated conv ---------------------------------------------------------------------------------------
// choose_form (se_dispatch.h) decides the kernel form of a call; run_gconv below switches into one launcher per family, which
// fills that family's params and launch cost and launches.  A launcher decides nothing: what it reads of `ch` is the choice.
struct ConvLaunch {       // one call: where it runs, the layer, the sources (src1: a tensor, a vector or null), the sizes
  se_ctx* c;
  const Layer& L; const LayerDef& d; const LayerFacts& f;
  const float* src0; int C0; const float* src1; int C1, src1_vec; float* dst;
  int B, Hin, Win, Ho, Wo, pad;
  bool bf;
  double alg(int taps) const { return 2.0 * (double)B * Ho * Wo * d.cout * d.cin * taps; }       // the layer's cost as the reference defines it

  // a Winograd launch on tiles of 2 rows x `tcols` columns at dilation `dil` (no second source, no folded bias: the caller sets those)
  WinoParams wino_params(const float* upk, const float* bias, int dil, int tcols) const {
    WinoParams wp;
    memset(&wp, 0, sizeof wp);
    wp.src = src0; wp.upk = upk; wp.bias = bias; wp.dst = dst;
    wp.B = B; wp.h = Hin; wp.w = Win; wp.d = dil; wp.th = Hin / 2; wp.tw = Win / tcols;
    wp.total_tiles = B * wp.th * wp.tw; wp.act = d.act;
    wp.xcd = xcd_remap_enabled();
    udiv_magic_host((unsigned)(wp.th * wp.tw), &wp.div_tpi_m, &wp.div_tpi_l);
    udiv_magic_host((unsigned)wp.tw, &wp.div_tw_m, &wp.div_tw_l);
    udiv_magic_host((unsigned)wp.d, &wp.div_d_m, &wp.div_d_l);
    return wp;
  }
  // 96 (+ 96) -> 192 and 48 -> 192: F(2x2,3x3), 16 of 36 products (se_wino.hip); hybrid F(2,3) x F(4,3) on 2x4 tiles, 24 of 72
  // (se_wino24.hip).  Folded vector source: half the positions' K, only the first source's half executed (311 -> 170 us at 256x256 B=32)
  int launch_form_wino(const Choice& ch) const {
    const double alg3x3 = alg(9);
    if (ch.form == F_WINO24_C48) {       // xconv5: 2 chunks per position, the second half empty
      const WinoParams wp = wino_params(L.d_u24, L.d_ub24, d.rate, 4);
      set_launch_cost(alg3x3, 4.0 * ((double)B * Hin * Win * 48 + (double)B * Hin * Win * 96), d.name, alg3x3 * 24.0 / 72.0);
      HIPCHK(c, launch_wino24_c48(wp, c->st));
      return 0;
    }
    const bool folded = ch.fold, f43 = ch.form == F_WINO24;
    if (folded) HIPCHK(c, launch_vecbias(L.d_wv, src1, c->vbias_ws, B, 96, c->st));
    const float* s1 = folded ? nullptr : src1;
    WinoParams wp = f43 ? wino_params(s1 ? L.d_u24b : L.d_u24, L.d_ub24, d.rate, 4) : wino_params(folded ? L.d_u1 : L.d_u, L.d_b, d.rate, 2);
    wp.src1 = s1; wp.src1_vec = folded ? 0 : src1_vec; wp.vbias = folded ? c->vbias_ws : nullptr;
    if ((double)B * Hin * Win * 384.0 >= 2147483648.0) return fail(c, "layer %s: tensor exceeds 2^31 bytes", d.name);
    set_launch_cost(alg3x3, 4.0 * 2.0 * (double)B * Hin * Win * 96, d.name,
                    f43 ? alg3x3 * 24.0 / 72.0 * (folded ? 0.5 : 1.0) : alg3x3 * 16.0 / 36.0 * (folded ? 0.5 : 1.0));
    HIPCHK(c, f43 ? launch_wino24(wp, c->st) : launch_wino(wp, c->st));
    return 0;
  }
  // 48 -> 96, and 24 -> 96 with one chunk per position (se_wino48.hip): 16 of 36 products
  int launch_form_wino48(const Choice& ch) const {
    const WinoParams wp = wino_params(L.d_u, L.d_ub, d.rate, 2);
    const bool c24 = ch.form == F_WINO48_C24;
    set_launch_cost(alg(9), c24 ? 4.0 * ((double)B * Hin * Win * 24 + (double)B * Hin * Win * 48) : 4.0 * 2.0 * (double)B * Hin * Win * 48, d.name,
                    alg(9) * 16.0 / 36.0);
    HIPCHK(c, c24 ? launch_wino48_c24(wp, c->st) : launch_wino48(wp, c->st));
    return 0;
  }
  // gen_deconv 96 -> 96 and 48 -> 48: F(2x2,2x2) on the sub-pixel classes, 9 of 36 products (se_wino_up.hip, se_wino_up48.hip;
  // 48: in the K pairing of the 48-channel kernels, 28 k-halves executed for 27 of work)
  int launch_form_winoup(const Choice& ch) const {
    const WinoParams wp = wino_params(L.d_u, L.d_ub, 1, 2);
    if (ch.form == F_WINOUP) {
      set_launch_cost(alg(9), 4.0 * ((double)B * Hin * Win * 96 + (double)B * Ho * Wo * 48), d.name, alg(9) * 9.0 / 36.0);
      HIPCHK(c, launch_winoup(wp, c->st));
      return 0;
    }
    set_launch_cost(alg(9), 4.0 * ((double)B * Hin * Win * 48 + (double)B * Ho * Wo * 24), d.name, alg(9) * 9.0 / 36.0 * 28.0 / 27.0);
    HIPCHK(c, launch_winoup48(wp, c->st));
    return 0;
  }

  // what every raw-tile launch of the narrow layers starts from: `trows` output rows x 16 columns per tile
  RTileParams rtile_params(const float* wpk, int trows) const {
    RTileParams p;
    memset(&p, 0, sizeof p);
    p.src = src0; p.wpk = wpk; p.bias = L.d_b; p.dst = dst;
    p.B = B; p.Hin = Hin; p.Win = Win; p.C = C0; p.OH = Ho; p.OW = Wo;
    p.G = bf ? (f.G + 7) & ~7 : f.G; p.NP = f.NP;
    p.ty = (Hin + trows - 1) / trows; p.tx = (Win + 15) / 16;
    p.act = d.act; p.bf16 = bf ? 1 : 0; p.xcd = xcd_remap_enabled();
    return p;
  }
  // 24 -> 24 3x3: F(2,3) along x on the raw tile, 160 instead of 224 MFMAs per wave, or two-dimensional, 96 (se_rtilew.hip)
  int launch_form_rtilew(const Choice& ch) const {
    const bool two_d = ch.form == F_RTILEW2;
    RTileParams p = rtile_params(two_d ? L.d_wx2 : L.d_wx, 16);       // blocks of 16 x 16 outputs
    udiv_magic_host((unsigned)(p.ty * p.tx), &p.div_cg_m, &p.div_cg_l);      // (reused fields: blk / (ty * tx), t2 / tx)
    udiv_magic_host((unsigned)p.tx, &p.div_rw_m, &p.div_rw_l);
    set_launch_cost(alg(9), 4.0 * ((double)B * Hin * Win * d.cin + (double)B * Ho * Wo * (d.cout / 2)), d.name,
                    (double)B * p.ty * p.tx * 8.0 * (two_d ? 96.0 : 160.0) * 2048.0);       // MFMAs of 16x16x4 per wave and block
    HIPCHK(c, two_d ? launch_rtilew2(p, c->st) : launch_rtilew(p, c->st));
    return 0;
  }
  // dense-K form of the 5x5 first layers (fp32), direct or F(2,5) along x (rtile_dense5w_kernel: 6 positions x ceil(5 Cd / 4)
  // k-steps per 2 outputs).  The kernel addresses its source with 32-bit byte offsets: a batch beyond that range is run as
  // sub-launches of the SAME kernel form over image ranges (switching to the channel-padded kernel would change the
  // summation order, i.e. the bit-identity of an image's result across batch compositions within one execution mode).
  int launch_form_rtile_dense5(const Choice& ch) const {
    const bool along_x = ch.form == F_RTILE_DENSE5W;
    const long long per_img = (long long)Hin * Win * C0 * 4;
    const long long lim = addr_limit();       // (SE_TEST_OFFSET_LIMIT, a test aid: a smaller byte range forces the sub-launches)
    const int bmax = (int)std::max<long long>(1, (lim - 1) / per_img);
    for (int b0 = 0; b0 < B; b0 += bmax) {
      const int nb = std::min(bmax, B - b0);
      RTileParams p = rtile_params(along_x ? L.d_wdw : L.d_wd, 8);
      p.src = src0 + (size_t)b0 * Hin * Win * C0; p.dst = dst + (size_t)b0 * Ho * Wo * f.G; p.B = nb;
      p.dense = along_x ? f.dense + 100 : f.dense; p.nch = f.nchd;
      const double algn = 2.0 * (double)nb * Ho * Wo * d.cout * d.cin * 25;
      set_launch_cost(algn, 4.0 * ((double)nb * Hin * Win * d.cin + (double)nb * Ho * Wo * (d.cout / 2)), d.name,
                      along_x ? (double)nb * p.ty * p.tx * 4.0 * (6.0 * ((5 * f.dense + 3) / 4) * 3.0) * 2048.0
                              : 2.0 * (double)nb * Hin * Win * 48.0 * (4.0 * ((25 * f.dense + 3) / 4)));       // ceil(K / 4) k-steps of 4
      HIPCHK(c, launch_rtile(p, c->st));
    }
    return 0;
  }
  // the raw-tile kernel on the direct image (se_rtile.hip), fp32 and bf16; bf16 pair-of-taps form of the 5x5 first layers
  int launch_form_rtile(const Choice& ch) const {
    const int es = bf ? 2 : 4, TR = rtile_rows(bf);
    RTileParams p = rtile_params(ch.form == F_RTILE_D4 ? L.d_w16d : L.direct[bf], TR);
    p.pad = pad;
    if (ch.form == F_RTILE_D4) {
      p.CG = 1; p.T = 25; p.KW = 5; p.nch = 2; p.dense = 204;
      p.RH = 32 + 4; p.RW = 21;                     // one column more than the halo: the sixth tap of a pair row
      p.raw_bytes = (p.RH * p.RW * 8 + 1023) & ~1023;
      udiv_magic_host(1u, &p.div_cg_m, &p.div_cg_l);
      set_launch_cost(alg(25), 2.0 * ((double)B * Hin * Win * d.cin + (double)B * Ho * Wo * (d.cout / 2)), d.name, 2.0 * (double)B * Hin * Win * 48.0 * 128.0);
    } else {
      const int KW = d.up ? 2 : d.k, CG = f.CG[bf], nch = f.nch[bf];
      p.CG = CG; p.T = f.T; p.KW = KW; p.nch = nch; p.up2 = d.up ? 1 : 0;
      p.RH = TR + KW - 1; p.RW = 16 + KW - 1;
      p.raw_bytes = (p.RH * p.RW * C0 * es + 1023) & ~1023;
      p.magicCG = (65536 + CG - 1) / CG; p.magicKW = 256 / KW + 1;        // (choose_form verified both on the ranges used)
      udiv_magic_host((unsigned)(C0 * es / 16), &p.div_cg_m, &p.div_cg_l);
      set_launch_cost(alg(d.k * d.k), (double)es * ((double)B * Hin * Win * d.cin + (double)B * Ho * Wo * (d.cout / 2)), d.name,
                      2.0 * (double)B * Hin * Win * (d.up ? 4.0 : 1.0) * f.NP * (nch * (bf ? 64.0 : 32.0)));
    }
    udiv_magic_host((unsigned)p.RW, &p.div_rw_m, &p.div_rw_l);
    HIPCHK(c, launch_rtile(p, c->st));
    return 0;
  }

  // bf16, 96 -> 192 3x3 stride 1 on 8 x 16 raw tiles of the polyphase sub-images (se_rconv16.hip).  dual: sub-images of 8 x 8
  // (dilation 16 at 128 x 128, 8 at 64 x 64), two phases share a tile.  fold (conv11 of netG): the spatially constant second
  // source folded into a bias table, the layer on the first source alone
  int launch_form_rconv16(const Choice& ch) const {
    if (ch.fold) HIPCHK(c, launch_vecbias(L.d_wv16, c->vec32, c->vbias_ws, B, 96, c->st, 1));
    RConvParams rp;
    memset(&rp, 0, sizeof rp);
    rp.dual = ch.form == F_RCONV16_DUAL;
    rp.src = src0; rp.wpk = L.d_w16s; rp.bias = L.d_b; rp.dst = dst; rp.vbias = ch.fold ? c->vbias_ws : nullptr;
    rp.B = B; rp.h = Hin; rp.w = Win; rp.d = d.rate; rp.hs = Hin / d.rate; rp.ws = Win / d.rate;
    rp.ty = (rp.hs + 7) / 8; rp.tx = (rp.ws + 15) / 16;
    rp.act = d.act; rp.xcd = xcd_remap_enabled();
    set_launch_cost(alg(9), 2.0 * 2.0 * (double)B * Hin * Win * 96, d.name, 2.0 * (double)B * Hin * Win * 192.0 * 864.0);
    HIPCHK(c, launch_rconv16(rp, c->st));
    return 0;
  }
  // bf16, the 96-row layers (3x3 48/24 -> 96 at stride 1, 24 -> 96 at stride 2, gen_deconv 96 -> 96): se_rconv96.hip
  int launch_form_rconv96(const Choice&) const {
    RConv96Params rp;
    memset(&rp, 0, sizeof rp);
    rp.src = src0; rp.wpk = L.d_w96; rp.bias = L.d_b; rp.dst = dst;
    rp.B = B; rp.h = Hin; rp.w = Win; rp.CG = C0 / 8;
    rp.stride = d.stride; rp.oh = Ho; rp.ow = Wo;
    rp.ty = ((d.stride == 2 ? Ho : Hin) + 15) / 16; rp.tx = ((d.stride == 2 ? Wo : Win) + 15) / 16;
    rp.up2 = d.up ? 1 : 0; rp.act = d.act; rp.xcd = xcd_remap_enabled();
    const int T = d.up ? 4 : 9, nstep = (T * rp.CG + 3) / 4;
    set_launch_cost(alg(9), 2.0 * ((double)B * Hin * Win * d.cin + (double)B * Ho * Wo * 48), d.name,
                    2.0 * (double)B * (d.stride == 2 ? (double)Ho * Wo : (double)Hin * Win) * (d.up ? 4.0 : 1.0) * 96.0 * (nstep * 32.0));
    HIPCHK(c, launch_rconv96(rp, c->st));
    return 0;
  }

  // the direct gather-GEMM (se_gconv.hip) on the image of one precision: the fallback of every gated conv
  int launch_form_gather(const Choice&) const {
    const int es = bf ? 2 : 4, gran = bf ? 8 : 4, CG = f.CG[bf], nch = f.nch[bf], KW = d.up ? 2 : d.k;
    GConvParams p;
    memset(&p, 0, sizeof p);
    p.bf16 = bf ? 1 : 0;
    p.src0 = src0; p.src1 = src1 ? src1 : src0; p.wpk = L.direct[bf]; p.bias = L.d_b; p.dst = dst; p.zeros = c->zeros;
    p.B = B; p.Hin = Hin; p.Win = Win; p.Ho = d.up ? Hin : Ho; p.Wo = d.up ? Win : Wo;   // up2: rows walk the source grid
    p.up2 = d.up ? 1 : 0; p.OH = Ho; p.OW = Wo;
    p.C0 = C0; p.C1 = C1 ? C1 : C0; p.C0g = C0 / gran; p.CG = CG;
    p.T = f.T; p.KW = KW; p.stride = d.stride; p.dil = d.rate; p.pad = pad;
    p.magicCG = (65536 + CG - 1) / CG; p.magicKW = 256 / KW + 1; p.magicKH = f.T / KW;
    if (!magic_cg_ok(CG, nch)) return fail(c, "layer %s: magic division check failed", d.name);
    if (!magic_kw_ok(KW, f.T)) return fail(c, "layer %s: magic tap division check failed", d.name);
    const int Gs = bf ? (f.G + 7) & ~7 : f.G;      // stored channel stride of the output
    // 32-bit byte offsets (sentinel 0x80000000): source and destination below 2^31 BYTES
    if ((double)B * Hin * Win * (C0 > C1 ? C0 : C1) * es >= 2147483648.0 || (double)B * Ho * Wo * Gs * es >= 2147483648.0)
      return fail(c, "layer %s: a tensor of this launch exceeds 2^31 bytes (32-bit byte offsets) -- split the batch", d.name);
    for (int j = 0; j < p.magicKH; ++j) p.rep |= 1u << (j * KW);
    udiv_magic_host((unsigned)(p.Ho * p.Wo), &p.div_hw_m, &p.div_hw_l);
    udiv_magic_host((unsigned)p.Wo, &p.div_w_m, &p.div_w_l);
    p.Hlim = Hin; p.Wlim = Win;
    p.src1_vec = src1_vec; p.nch = nch; p.G = Gs; p.act = d.act; p.total_pix = B * p.Ho * p.Wo;
    p.xcd = xcd_remap_enabled();
    p.np_full = f.NP; p.nf_full = f.NP / 32; p.small_grid = c->low_latency ? 1 : 0;
    // cost: algorithmic as the reference defines the layer (3x3 on the upsampled grid for gen_deconv); executed: the packed K
    // (channels padded to granules, taps x channels padded to whole chunks) and row (NP) sizes the MFMAs really run over; the
    // sub-pixel form of gen_deconv runs 4 classes x 4 taps instead of 9 taps on the upsampled grid
    set_launch_cost(alg(d.k * d.k), (double)es * ((double)B * Hin * Win * d.cin + (double)B * Ho * Wo * (d.cout / 2)), d.name,
                    2.0 * (double)B * p.Ho * p.Wo * (d.up ? 4.0 : 1.0) * f.NP * (nch * (bf ? 64.0 : 32.0)));
    HIPCHK(c, launch_gconv(f.cfg, p, c->st));
    return 0;
  }
};

int run_gconv(se_ctx* c, const Layer& L, const float* src0, int C0, const float* src1, int C1, int src1_vec, float* dst,
              int B, int Hin, int Win) {
  const LayerDef& d = L.def;
  const LayerFacts& f = L.facts;
  const ConvShape sh = conv_shape(d, Hin, Win);
  const bool bf = c->bf16;
  if (!L.packed) return fail(c, "layer %s: weights not loaded", d.name);
  if (bf && !L.direct[1]) return fail(c, "layer %s: no bf16 weight image", d.name);
  if (bf && (C0 + C1) != f.CG[1] * 8) return fail(c, "layer %s: bf16 source channels %d+%d != packed %d", d.name, C0, C1, f.CG[1] * 8);
  if (!bf && (C0 + C1) != f.CG[0] * 4) return fail(c, "layer %s: source channels %d+%d != packed %d", d.name, C0, C1, f.CG[0] * 4);
  const ConvCall q = {d, f, B, Hin, Win, C0, C1, src1 ? (src1_vec ? SRC2_VECTOR : SRC2_TENSOR) : SRC2_NONE, bf, c->low_latency,
                      c->conservative, c->cur_net, c->vbias_ws && (!bf || c->vec32)};
  const Choice ch = choose_form(q);
  static bool said = false;
  if (ch.wino_range && !said) {
    said = true;
    fprintf(stderr, "sketchedit_hip: layer %s: %d x %dx%d x 96 floats exceed the Winograd kernel's 32-bit byte offsets; "
                    "using the direct kernel (about 2x slower) -- split the batch\n", d.name, B, Hin, Win);
  }
  const ConvLaunch a = {c, L, d, f, src0, C0, src1, C1, src1_vec, dst, B, Hin, Win, sh.Ho, sh.Wo, sh.pad, bf};
  switch (ch.form) {
    case F_WINO: case F_WINO24: case F_WINO24_C48: return a.launch_form_wino(ch);
    case F_WINO48: case F_WINO48_C24: return a.launch_form_wino48(ch);
    case F_WINOUP: case F_WINOUP48: return a.launch_form_winoup(ch);
    case F_RTILEW: case F_RTILEW2: return a.launch_form_rtilew(ch);
    case F_RTILE_DENSE5: case F_RTILE_DENSE5W: return a.launch_form_rtile_dense5(ch);
    case F_RTILE: case F_RTILE_D4: return a.launch_form_rtile(ch);
    case F_RCONV16: case F_RCONV16_DUAL: return a.launch_form_rconv16(ch);
    case F_RCONV96: return a.launch_form_rconv96(ch);
    case F_GATHER: return a.launch_form_gather(ch);
    case F_SMALL_CONV: break;      // (a raw layer has no gated image: refused above)
  }
  return fail(c, "layer %s: not a gated conv", d.name);
}

struct Act {   // an NHWC activation living in the arena
  float* p = nullptr;
  int H = 0, W = 0, C = 0;
};

struct Plan {
  se_ctx* c;
  std::map<std::string, Layer>& net;
  int B;
  int rc = 0;
  Arena* ar;                // arena of the branch being planned
  Plan(se_ctx* c_, std::map<std::string, Layer>& n, int B_) : c(c_), net(n), B(B_), ar(&c_->arena) {}
  float* alloc_raw(size_t nfloats) {
    float* p = ar->alloc(nfloats);
    if (!p && !rc) rc = fail(c, "workspace too small (need more than %zu bytes)", ar->cap);
    // SE_TEST_POISON: the whole block (its 256-byte rounding included) is filled on c->st, the stream of the branch being
    // planned, where the block's first producer is enqueued next.  The fill is ordered after every earlier user of the bytes:
    // a block is reused within one arena, and an arena is used in the order of one stream -- the main arena on the main stream,
    // the side arena between side_begin() and side_end() on the side stream, which starts behind the fork event, i.e. behind
    // everything the main stream did with side-arena blocks before (the style input, `vec`, a previous plan's joined side
    // branch).  A block both branches read (xnow, vec, pm) is released only after join(), and nothing is allocated from the
    // side arena between a side_end() and the next side_begin() except before the first fork, when that arena is still unused.
    if (p && !rc && !c->dry && poison(c, p, (nfloats * 4 + 255) & ~(size_t)255, c->st)) rc = 1;
    return p;
  }
  Act alloc(int H, int W, int C) {
    Act a; a.H = H; a.W = W;
    if (c->bf16) {       // bf16 activations: whole 8-channel granules per pixel (12 -> 16, 4 / 5 -> 8), two per float slot
      a.C = (C + 7) & ~7;
      a.p = alloc_raw(((size_t)B * H * W * a.C + 1) / 2);
    } else {
      a.C = C;
      a.p = alloc_raw((size_t)B * H * W * C);
    }
    if (c->dry) c->dry_max_act = std::max(c->dry_max_act, (size_t)B * H * W * a.C * (c->bf16 ? 2 : 4));
    return a;
  }
  void release(const float* p) {          // to whichever arena the block came from
    if (!p) return;
    if (c->arena2.owns(p)) c->arena2.release(p); else c->arena.release(p);
  }
  void free(Act& a) { release(a.p); a.p = nullptr; }
  // ---- concurrent branches (low-latency mode).  side_begin() .. side_end() plans a branch on the side stream and in the
  // side arena; it starts after everything enqueued on the main stream so far (fork event) and join() makes the main
  // stream wait for it.  A buffer shared by both branches must be released only after join().  Outside low-latency mode
  // the calls do nothing: the branch is planned in line, on the main stream and arena.
  // Default mode (round 6): the same two-stream plan (SE_FORK_DEFAULT=0: one stream) -- the tail of one branch's kernel runs
  // under the head of the other's: +2 % on configs 2, 3 and 5.  While the in-library profiler is on, the default mode is
  // planned on ONE stream (c->serial): an event pair around a launch measures that kernel only when nothing else shares the chip.
  // (c->fork2 = SE_FORK_DEFAULT as it was when the call entered the library: one snapshot per call, so a switch flipped by
  // another thread cannot leave a plan with a fork and no join)
  bool forked() const { return (c->low_latency || (c->fork2 && !c->serial)) && c->st_side; }
  int side_begin() {
    if (!forked()) return 0;
    ar = &c->arena2;
    if (c->dry) return 0;
    HIPCHK(c, hipEventRecord(c->ev_fork, c->st_main));
    HIPCHK(c, hipStreamWaitEvent(c->st_side, c->ev_fork, 0));
    c->st = c->st_side;
    return 0;
  }
  int side_end() {
    if (!forked()) return 0;
    ar = &c->arena;
    if (c->dry) return 0;
    HIPCHK(c, hipEventRecord(c->ev_join, c->st_side));
    c->st = c->st_main;
    return 0;
  }
  int join() {
    if (!forked() || c->dry) return 0;
    HIPCHK(c, hipStreamWaitEvent(c->st_main, c->ev_join, 0));
    return 0;
  }
  // gated conv layer: consumes (and releases, if `rel`) `in`
  Act conv(const char* name, Act& in, bool rel = true, const float* src1 = nullptr, int C1 = 0, int vec = 0) {
    if (rc) return Act();
    return conv_layer(net.at(name), in, rel, src1, C1, vec);
  }
  Act conv_layer(Layer& L, Act& in, bool rel = true, const float* src1 = nullptr, int C1 = 0, int vec = 0) {
    Act out;
    if (rc) return out;
    const ConvShape sh = conv_shape(L.def, in.H, in.W);
    out = alloc(sh.Ho, sh.Wo, L.def.cout / 2);
    if (rc) return out;
    if (!c->dry) rc = run_gconv(c, L, in.p, in.C, src1, C1, vec, out.p, B, in.H, in.W);
    if (rel) free(in);
    return out;
  }
};

// encoder: conv1 (5x5) .. conv10_atrous; returns conv10 output, optionally keeps conv9's
Act encoder(Plan& P, const std::string& p, Act& in, Act* keep9, Layer* first = nullptr) {
  Act x = first ? P.conv_layer(*first, in) : P.conv((p + "1").c_str(), in);
  x = P.conv((p + "2_downsample").c_str(), x);
  x = P.conv((p + "3").c_str(), x);
  x = P.conv((p + "4_downsample").c_str(), x);
  x = P.conv((p + "5").c_str(), x);
  x = P.conv((p + "6").c_str(), x);
  x = P.conv((p + "7_atrous").c_str(), x);
  x = P.conv((p + "8_atrous").c_str(), x);
  Act x9 = P.conv((p + "9_atrous").c_str(), x);
  Act x10 = P.conv((p + "10_atrous").c_str(), x9, keep9 == nullptr);
  if (keep9) *keep9 = x9;
  return x10;
}

// decoder conv11..conv16 (returns the 12-channel full-resolution activation feeding conv17)
Act decoder(Plan& P, const std::string& p, Act& in, const float* src1 = nullptr, int C1 = 0, int vec = 0) {
  Act x = P.conv((p + "11").c_str(), in, true, src1, C1, vec);
  x = P.conv((p + "12").c_str(), x);
  x = P.conv((p + "13_upsample_conv").c_str(), x);
  x = P.conv((p + "14").c_str(), x);
  x = P.conv((p + "15_upsample_conv").c_str(), x);
  x = P.conv((p + "16").c_str(), x);
  return x;
}

int small(Plan& P, const char* name, Act& in, int mode, float* out_nchw, float* hard, const float* img,
          const float* mask, float* xnow, float* composed, int no_mask_coarse, long packed_bs = 0,
          const unsigned char* lock = nullptr) {
  if (P.rc) return P.rc;
  se_ctx* c = P.c;
  if (!c->dry) {
    Layer& L = P.net.at(name);
    if (!L.packed) return P.rc = fail(c, "layer %s: weights not loaded", name);
    SmallConvParams sp;
    memset(&sp, 0, sizeof sp);
    sp.x = in.p; sp.w = L.direct[c->bf16]; sp.b = L.d_b; sp.B = P.B; sp.H = in.H; sp.W = in.W; sp.cout = L.def.cout;
    sp.bf16 = c->bf16 ? 1 : 0;
    sp.mode = mode; sp.out_nchw = out_nchw; sp.hard = hard; sp.img = img; sp.mask = mask; sp.xnow = xnow;
    sp.composed = composed; sp.no_mask_coarse = no_mask_coarse;
    if (mode == 3) { sp.rgb8 = c->rgb8; sp.m8 = c->m8; }
    if (mode == 0) sp.lock = lock;
    if (packed_bs) {      // SE_FLAG_PACKED_OUT: soft mask and composite live in one (B,4,H,W) buffer
      if (mode == 0) sp.out_bs = packed_bs;
      if (mode == 3) { sp.mask_bs = packed_bs; sp.comp_bs = packed_bs; }
    }
    set_launch_cost(2.0 * (double)P.B * in.H * in.W * L.def.cout * 108.0,
                    4.0 * (double)P.B * in.H * in.W * (12 + L.def.cout), L.def.name);
    hipError_t e = launch_small_conv(sp, c->st);
    if (e != hipSuccess) return P.rc = fail(c, "small conv %s: %s", name, hipGetErrorString(e));
  }
  P.free(in);
  return 0;
}

// MDGenerator.forward, editline2_g.py:59-94.  lock (B,H,W) uint8 or null: the mask is 0 where it is non-zero
int plan_netM(se_ctx* c, const float* image, const float* sketch, float* mask_out, float* hard_out, float* maskim_out,
              int B, int H, int W, long packed_bs = 0, const unsigned char* lock = nullptr) {
  Plan P(c, c->M, B);
  c->cur_net = SE_NET_M;
  Act in = P.alloc(H, W, 4);
  if (P.rc) return P.rc;
  if (!c->dry) HIPCHK(c, c->bf16 ? launch_pack_m16(image, sketch, in.p, B, H, W, c->st) : launch_pack_m(image, sketch, in.p, B, H, W, c->st));
  Act x9;
  const bool want_img = maskim_out != nullptr;
  Act x10 = encoder(P, "conv", in, want_img ? &x9 : nullptr);
  if (want_img) {   // image decoder consumes conv9's output (quirk, editline2_g.py:76-77)
    Act d = decoder(P, "conv", x9);
    small(P, "conv17", d, 1, maskim_out, nullptr, nullptr, nullptr, nullptr, nullptr, 0);
  }
  Act d = decoder(P, "conv_mask_", x10);
  small(P, "conv_mask_17", d, 0, mask_out, hard_out, nullptr, nullptr, nullptr, nullptr, 0, packed_bs, lock);
  return P.rc;
}

int run_attention(se_ctx* c, Plan& P, Act& x, const float* mask_full, Act& out, float* similar_nchw);

// DeepFillC2Generator.forward, editline_g.py:119-221.  The two encoders of stage 1 and the two branches of stage 2 are
// independent until their concat: in low-latency mode the second one of each pair runs on the side stream.
int plan_netG(se_ctx* c, const float* x, const float* x2, const float* mask, const float* mask2, const float* guide,
              float* coarse_out, float* fine_out, const float* soft_mask, float* composed_out, int B, int H, int W,
              int flags, long packed_bs = 0) {
  Plan P(c, c->G, B);
  c->cur_net = SE_NET_G;
  const int joint = (flags & SE_FLAG_JOINT_TRAIN_INP) ? 1 : 0;
  // joint_train_inp: the style input is packed without its (zero) guide channel and wconv1 runs as a 4-channel conv
  Act cin = P.alloc(H, W, 8);
  P.ar = P.forked() ? &c->arena2 : &c->arena;       // the style branch's input lives in the style branch's arena
  Act sin = P.alloc(H, W, joint ? 4 : 8);
  P.ar = &c->arena;
  if (P.rc) return P.rc;
  if (!c->dry)
    HIPCHK(c, (c->bf16 ? launch_pack_g16 : launch_pack_g)(x, x2, mask, mask2, guide, cin.p, sin.p, B, H, W,
                                                          (flags & SE_FLAG_NO_MASK_CC) ? 1 : 0, joint, c->st));
  // ---- style branch :149-163 -> (B,96) pooled vector, consumed by conv11 as a second (spatially constant) source
  if (P.side_begin()) return 1;
  Act xs = encoder(P, "wconv", sin, nullptr, joint ? &c->wconv1_j4 : nullptr);
  // (in bf16 mode `part` / `vec32` hold fp32 values in twice the room they need; `vec` is the bf16 vector conv11 reads)
  Act part = P.alloc(1, COLREDUCE_SPLITS, 192), vec32 = P.alloc(1, 1, 192), vec = P.alloc(1, 1, 96);
  if (P.rc) return P.rc;
  if (!c->dry)
    HIPCHK(c, launch_colreduce(xs.p, part.p, c->bf16 ? vec32.p : vec.p, B, xs.H * xs.W, 96, (flags & SE_FLAG_POOL_MAX) ? 0 : 1,
                               c->st, c->bf16 ? 1 : 0, c->bf16 ? vec.p : nullptr));
  if (!c->dry && c->taps && c->taps->style_vec)
    HIPCHK(c, hipMemcpyAsync(c->taps->style_vec, c->bf16 ? vec32.p : vec.p, (size_t)B * 96 * 4, hipMemcpyDeviceToDevice, c->st));
  P.free(xs);
  P.free(part);
  if (!c->bf16) P.free(vec32);        // bf16 mode: the fp32 vector feeds the bias table of conv11 (released after the decoder)
  if (P.side_end()) return 1;
  // ---- coarse branch :138-147
  Act xc = encoder(P, "conv", cin, nullptr);
  if (P.rc) return P.rc;
  if (P.join()) return 1;
  float* vb = P.alloc_raw((size_t)B * 9 * 192);     // bias table of the folded style vector (run_gconv)
  if (P.rc) return P.rc;
  c->vbias_ws = vb;
  c->vec32 = c->bf16 ? vec32.p : nullptr;
  Act d = decoder(P, "conv", xc, vec.p, 96, 1);     // :167-175 (cat is virtual)
  c->vbias_ws = nullptr; c->vec32 = nullptr;
  P.release(vb);
  if (c->bf16) P.free(vec32);
  P.free(vec);
  Act xnow = P.alloc(H, W, 4);
  if (P.rc) return P.rc;
  small(P, "conv17", d, 2, coarse_out, nullptr, x, mask, xnow.p, nullptr, (flags & SE_FLAG_NO_MASK_COARSE) ? 1 : 0);
  if (P.rc) return P.rc;
  // ---- patch-match branch :197-209 (side)
  if (P.side_begin()) return 1;
  Act pm = P.conv("pmconv1", xnow, false);
  pm = P.conv("pmconv2_downsample", pm);
  pm = P.conv("pmconv3", pm);
  pm = P.conv("pmconv4_downsample", pm);
  pm = P.conv("pmconv5", pm);
  pm = P.conv("pmconv6", pm);
  if (P.rc) return P.rc;
  if (!c->dry && c->taps && c->taps->pmconv6)
    HIPCHK(c, (c->bf16 ? launch_nhwc16_to_nchw : launch_nhwc_to_nchw)(pm.p, c->taps->pmconv6, B, 96, 96, pm.H, pm.W, c->st));
  if (flags & SE_FLAG_USE_CAM) {
    Act att = P.alloc(pm.H, pm.W, 96);
    if (P.rc) return P.rc;
    if (run_attention(c, P, pm, mask, att, nullptr)) return P.rc ? P.rc : 1;
    P.free(pm);
    pm = att;
    if (!c->dry && c->taps && c->taps->attn_out)
      HIPCHK(c, (c->bf16 ? launch_nhwc16_to_nchw : launch_nhwc_to_nchw)(pm.p, c->taps->attn_out, B, 96, 96, pm.H, pm.W, c->st));
  }
  pm = P.conv("pmconv9", pm);
  pm = P.conv("pmconv10", pm);
  if (P.rc) return P.rc;
  if (P.side_end()) return 1;
  // ---- hallucination branch :184-194
  Act hcur = P.conv("xconv1", xnow, false);
  hcur = P.conv("xconv2_downsample", hcur);
  hcur = P.conv("xconv3", hcur);
  hcur = P.conv("xconv4_downsample", hcur);
  hcur = P.conv("xconv5", hcur);
  hcur = P.conv("xconv6", hcur);
  hcur = P.conv("xconv7_atrous", hcur);
  hcur = P.conv("xconv8_atrous", hcur);
  hcur = P.conv("xconv9_atrous", hcur);
  Act hallu = P.conv("xconv10_atrous", hcur);
  if (P.rc) return P.rc;
  if (P.join()) return 1;
  P.free(xnow);                                         // read by both branches: released after the join
  Act d2 = decoder(P, "allconv", hallu, pm.p, 96, 0);   // cat([x_hallu, pm]) :211 is virtual
  P.free(pm);
  small(P, "allconv17", d2, 3, fine_out, nullptr, x, soft_mask, nullptr, soft_mask ? composed_out : nullptr, 0, packed_bs);
  c->rgb8 = nullptr; c->m8 = nullptr;
  return P.rc;
}

// Row stride (in elements) of the R x R matrices E, P, P~ and of the transposed values: R rounded up to whole k-chunks
// (32 fp32 / 64 bf16 keys).  (Padding the power-of-two strides of 256x256 / 512x512 inputs by one chunk was measured:
// no gain for the row-streaming passes -- they are not camping on HBM channels.)
int att_row_stride(int R, bool bf) {
  const int chunk = bf ? 64 : 32;
  int Rp = (R + chunk - 1) / chunk * chunk;
  return Rp;
}

// Whether attention on an h x w feature map runs in the streaming form (se_att_stream.hip: nothing R x R): wherever the
// materialised space-to-depth form cannot address its R x R matrices with 32-bit offsets (R Rp 4 >= 2^31), and everywhere
// with SE_ATT_STREAM=1 unless `similar_out` -- P itself -- is asked for.  `similar_out` is refused exactly where
// R Rp 4 >= 2^31, whatever the options (Engine.attention checks the same rule before it allocates the L x L output).
bool att_streaming(int h, int w, bool bf, bool want_similar) {
  const int R = (h / 2) * (w / 2), Rp = att_row_stride(R, bf);
  const bool fits = (double)R * Rp * 4.0 < 2147483648.0;
  if (want_similar && !fits) return true;              // (run_attention refuses: similar_out is P itself)
  if (opt(OPT_ATT_STREAM) == 1 && !want_similar) return true;
  return !fits;
}

int run_attention(se_ctx* c, Plan& P, Act& x, const float* mask_full, Act& out, float* similar_nchw) {
  const int h = x.H, w = x.W, B = P.B;
  const int hs = (h - 4) / 2 + 1, ws = (w - 4) / 2 + 1, L = hs * ws, Lp = (L + 31) & ~31;
  const bool bf = c->bf16;
  const bool stream = att_streaming(h, w, bf, similar_nchw != nullptr);
  const int hc = h / 2, wc = w / 2, R = hc * wc;
  const int Rp = att_row_stride(R, bf);
  const int guard = (wc + 8 + 63) & ~63;               // floats; att2_ptilde_kernel reads up to wc + 5 columns outside a row
  if (stream && similar_nchw)
    return P.rc = fail(c, "attention: similar_out (the %d x %d score matrix) is not available on a %dx%d feature map: "
                          "it runs in the streaming form, which never forms it", L, L, h, w);
  // fp32 scratch is sized in floats whatever the activation type
  float* part = P.alloc_raw((size_t)B * COLREDUCE_SPLITS * 96);
  float* rn = P.alloc_raw((size_t)B * 96);
  float* xn = P.alloc_raw(bf ? ((size_t)B * h * w * 96 + 1) / 2 : (size_t)B * h * w * 96);
  float *valid = nullptr, *S = nullptr, *S2 = nullptr, *xT = nullptr, *stats = nullptr;
  if (stream) {      // O(R): validR, kmul, kadd; (max, 1 / sum) per query; V^T plus the tail the out pass may read
    valid = P.alloc_raw(3 * (size_t)B * Rp);
    stats = P.alloc_raw((size_t)B * R * 2);
    xT = P.alloc_raw((bf ? (size_t)B * 4 * 96 * Rp / 2 : (size_t)B * 4 * 96 * Rp) + att_stream_xt_tail());
  } else {
    valid = P.alloc_raw(7 * ((size_t)B * Rp + guard) + (size_t)B * 768 + (size_t)B * hc * 384);      // validR, kmul, kadd (+ fp16-E form: kadd2, ea4, ea, eb), each behind its guard band; emean, epart
    stats = P.alloc_raw((size_t)B * R * 2);    // fused streaming pass: (row max, 1 / row sum) per query
    xT = P.alloc_raw(bf ? (size_t)B * 4 * 96 * Rp / 2 : (size_t)B * 4 * 96 * Rp);
    S = P.alloc_raw((size_t)B * R * Rp + 2 * guard);       // E (fp32) between two guard bands; three-pass form: then P~
    S2 = P.alloc_raw(bf ? (size_t)B * R * Rp / 2 : (size_t)B * R * Rp);      // P (fp32 / bf16)
  }
  if (P.rc) return P.rc;
  if (!c->dry) {
    HIPCHK(c, launch_colreduce(x.p, part, rn, B, h * w, 96, 2, c->st, bf ? 1 : 0));
    AttParams a;
    memset(&a, 0, sizeof a);
    a.x = x.p; a.rn = rn; a.xn = xn; a.hard = mask_full; a.out = out.p;
    a.B = B; a.h = h; a.w = w; a.hs = hs; a.ws = ws; a.L = L; a.Lp = Lp;
    a.scale = 10.f; a.th = 0.1f;                        // editline_g.py:35-38
    if (stream) {
      a.hc = hc; a.wc = wc; a.R = R; a.Rp = Rp; a.bf16 = bf ? 1 : 0;
      a.validR = valid; a.kmul = valid + (size_t)B * Rp; a.kadd = valid + 2 * (size_t)B * Rp;
      a.xT = xT; a.stats = stats;
      HIPCHK(c, launch_attention_stream(a, c->st));
    } else {
      a.hc = hc; a.wc = wc; a.R = R; a.Rp = Rp; a.bf16 = bf ? 1 : 0;
      a.validR = valid + guard; a.xT = xT; a.E = S + guard; a.P = S2; a.stats = stats; a.guard = guard; a.similar = similar_nchw;
      a.kmul = valid + ((size_t)B * Rp + guard) + guard; a.kadd = valid + 2 * ((size_t)B * Rp + guard) + guard;
      a.kadd2 = valid + 3 * ((size_t)B * Rp + guard) + guard; a.ea4 = valid + 4 * ((size_t)B * Rp + guard) + guard;
      a.ea = valid + 5 * ((size_t)B * Rp + guard) + guard; a.eb = valid + 6 * ((size_t)B * Rp + guard) + guard;
      a.emean = valid + 7 * ((size_t)B * Rp + guard); a.epart = a.emean + (size_t)B * 768;
      HIPCHK(c, launch_attention(a, c->st));
    }
  }
  P.release(S2); P.release(S); P.release(xT); P.release(stats); P.release(valid);
  P.release(xn); P.release(rn); P.release(part);
  return 0;
}

int check_dims(se_ctx* c, int B, int H, int W) {
  if (B < 1 || H < 16 || W < 16 || (H % 8) || (W % 8)) return fail(c, "bad shape B=%d H=%d W=%d (H, W must be multiples of 8, >= 16)", B, H, W);
  return 0;
}

// Passes of a forward over a large batch.  The kernels address a tensor with 32-bit byte offsets (addr_limit); the largest
// tensor of either network is the 24-channel full-resolution activation (conv1 / conv15_upsample outputs: 96 bytes per
// pixel in fp32, 48 in bf16 -- max_act_bytes_per_image derives it from the plans), so a forward runs over at most
// (limit - 1) / (H W 96) images at a time and a larger batch is
// run as several passes of the SAME plan over image ranges -- same kernels, same execution mode, so an image's result does
// not depend on the pass it lands in (bit for bit: test_large_batch_is_split_into_passes).  Passes are balanced
// (ceil(B / passes) images each).  Returns the images per pass, or 0 (error set) when ONE image exceeds the range.
// bytes per image of the LARGEST activation tensor either plan allocates at this size -- derived from a dry run of the plans
// themselves (the literal "24 channels at full resolution = 96 / 48 bytes per pixel" would silently go stale with
// a wider layer); cached per (H, W, precision)
long long max_act_bytes_per_image(se_ctx* c, int H, int W, int flags) {
  const std::vector<long long> key = {H, W, (flags & SE_FLAG_BF16) ? 1 : 0};
  auto it = c->act_per_img.find(key);
  if (it != c->act_per_img.end()) return it->second;
  const bool dry0 = c->dry, ll0 = c->low_latency, bf0 = c->bf16;
  c->dry = true; c->low_latency = false; c->bf16 = (flags & SE_FLAG_BF16) != 0;
  c->dry_max_act = 0;
  float dummy;
  c->arena.reset(nullptr, 0, true, 0); c->arena2.reset(nullptr, 0, true, 1);
  plan_netM(c, nullptr, nullptr, nullptr, nullptr, &dummy, 1, H, W, 0);
  c->arena.reset(nullptr, 0, true, 0); c->arena2.reset(nullptr, 0, true, 1);
  plan_netG(c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, H, W, SE_FLAG_USE_CAM | SE_FLAG_POOL_MAX, 0);
  c->dry = dry0; c->low_latency = ll0; c->bf16 = bf0;
  const long long v = (long long)c->dry_max_act;
  c->act_per_img[key] = v;
  return v;
}

int pass_size(se_ctx* c, int B, int H, int W, int flags) {
  const long long per_img = max_act_bytes_per_image(c, H, W, flags);
  const long long lim = addr_limit();
  if (per_img <= 0) { fail(c, "internal: no activation size for %dx%d", H, W); return 0; }
  if (per_img >= lim) {
    fail(c, "a %dx%d image exceeds the kernels' 32-bit byte offsets (%lld bytes per activation, limit %lld)", H, W, per_img, lim);
    return 0;
  }
  const long long bmax = (lim - 1) / per_img;
  if (B <= bmax) return B;
  const long long passes = (B + bmax - 1) / bmax;
  return (int)((B + passes - 1) / passes);
}

// Arena peaks of a forward, from a dry run of the very plan that will be launched (nothing is enqueued): main-branch
// arena and, in low-latency mode, the side-branch arena.  which: 1 netM, 2 netG, 3 netM then netG (se_inference).
se_ctx::Peaks plan_peaks(se_ctx* c, int which, int B, int H, int W, int flags, bool want_maskim) {
  const std::vector<long long> key = {which, B, H, W,
                                      flags & (SE_FLAG_USE_CAM | SE_FLAG_JOINT_TRAIN_INP | SE_FLAG_LOW_LATENCY | SE_FLAG_BF16),
                                      want_maskim ? 1 : 0, c->fork2 ? 1 : 0, opt_epoch(), c->serial ? 1 : 0};
  auto it = c->peaks.find(key);
  if (it != c->peaks.end()) return it->second;
  const bool dry0 = c->dry, ll0 = c->low_latency, bf0 = c->bf16;
  c->dry = true;
  c->low_latency = (flags & SE_FLAG_LOW_LATENCY) != 0;
  c->bf16 = (flags & SE_FLAG_BF16) != 0;
  float dummy;      // non-null marker for optional outputs
  se_ctx::Peaks pk{0, 0};
  if (which & 1) {
    c->arena.reset(nullptr, 0, true, 0); c->arena2.reset(nullptr, 0, true, 1);
    plan_netM(c, nullptr, nullptr, nullptr, nullptr, want_maskim ? &dummy : nullptr, B, H, W);
    pk.main = c->arena.peak; pk.side = c->arena2.peak;
  }
  if (which & 2) {
    c->arena.reset(nullptr, 0, true, 0); c->arena2.reset(nullptr, 0, true, 1);
    plan_netG(c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, B, H, W, flags);
    if (c->arena.peak > pk.main) pk.main = c->arena.peak;
    if (c->arena2.peak > pk.side) pk.side = c->arena2.peak;
  }
  c->dry = dry0; c->low_latency = ll0; c->bf16 = bf0;
  c->peaks[key] = pk;
  return pk;
}

// carve the caller's workspace into the arenas of this call; `tail` bytes at the end stay reserved
int carve(se_ctx* c, const se_ctx::Peaks& pk, void* ws, size_t ws_bytes, size_t tail) {
  if (ws_bytes < pk.main + pk.side + tail)
    return fail(c, "workspace too small: %zu bytes, this call needs %zu", ws_bytes, pk.main + pk.side + tail);
  // the main arena gets whatever the side arena does not need
  c->arena.reset((char*)ws, ws_bytes - tail - pk.side, false);
  c->arena2.reset((char*)ws + (ws_bytes - tail - pk.side), pk.side, false);
  return 0;
}

void begin_call(se_ctx* c, void* stream, int flags) {
  c->st = c->st_main = (hipStream_t)stream;
  c->dry = false;
  c->low_latency = (flags & SE_FLAG_LOW_LATENCY) != 0;
  c->bf16 = (flags & SE_FLAG_BF16) != 0;
  c->conservative = (flags & SE_FLAG_CONSERVATIVE) != 0;
  c->serial = c->prof.on;
  c->taps = nullptr;
  c->rgb8 = nullptr; c->m8 = nullptr;
  c->cur_net = SE_NET_G;       // per-op entry points run as netG layers whatever plan ran last; the plans set their own
  set_profiler(&c->prof);
}

// what every entry that plans a forward does once its arguments are checked (the mutex is held)
int forward_enter(se_ctx* c) {
  HIPCHK(c, hipSetDevice(c->device));
  c->serial = c->prof.on;      // profiler on: default mode planned on one stream (Plan::forked)
  c->fork2 = opt(OPT_FORK_DEFAULT) != 0;
  return 0;
}

// A captured forward may still be executing on the stream it was last launched on: destroying an in-flight hipGraphExec
// is not safe on every ROCm version, so that stream is drained first (eviction and weight reloads are rare events).
void destroy_graph(se_ctx::GraphEntry& g) {
  if (g.exec) {
    if (g.stream) (void)hipStreamSynchronize(g.stream);
    (void)hipGraphExecDestroy(g.exec);
  }
  if (g.graph) (void)hipGraphDestroy(g.graph);
  g.exec = nullptr; g.graph = nullptr;
}
void drop_graphs(se_ctx* c) {
  for (auto& g : c->graphs) destroy_graph(g);
  c->graphs.clear();
}
// cache full: evict the ONE least recently used entry (hot graphs survive callers that pass fresh output tensors)
void evict_lru_graph(se_ctx* c) {
  size_t lru = 0;
  for (size_t i = 1; i < c->graphs.size(); ++i)
    if (c->graphs[i].last_use < c->graphs[lru].last_use) lru = i;
  destroy_graph(c->graphs[lru]);
  c->graphs.erase(c->graphs.begin() + lru);
}

// ---- Pillow-exact resize (se_resize.hip): the ctx's tables and intermediate, and the one host routine behind the C-ABI ----
// Every resize resource is used in the order of ONE stream: a call on another stream than the previous one first waits for
// the previous stream's work (event), so freeing or overwriting a resource only needs that stream drained.
int rs_enter(se_ctx* c, hipStream_t st) {
  if (c->rs_used && c->rs_stream != st) {
    if (!c->rs_event) HIPCHK(c, hipEventCreateWithFlags(&c->rs_event, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(c->rs_event, c->rs_stream));
    HIPCHK(c, hipStreamWaitEvent(st, c->rs_event, 0));
  }
  c->rs_stream = st;
  c->rs_used = true;
  return 0;
}

const se_ctx::ResampleTable* rs_table(se_ctx* c, int in, int out, int filter) {
  for (auto& t : c->rs_tables)
    if (t.in == in && t.out == out && t.filter == filter) { t.last_use = ++c->rs_clock; return &t; }
  const int ksize = resample_ksize(in, out, filter);
  if (ksize < 0) { fail(c, "resize: bad arguments (in %d, out %d, filter %d)", in, out, filter); return nullptr; }
  if (ksize > RESAMPLE_MAX_KSIZE) { fail(c, "resize: %d -> %d needs %d taps per output, more than the kernels take (%d)", in, out, ksize, RESAMPLE_MAX_KSIZE); return nullptr; }
  if (c->rs_tables.size() >= 64) {
    size_t lru = 0;
    for (size_t i = 1; i < c->rs_tables.size(); ++i)
      if (c->rs_tables[i].last_use < c->rs_tables[lru].last_use) lru = i;
    (void)hipStreamSynchronize(c->rs_stream);       // earlier resizes may still read it
    (void)hipFree(c->rs_tables[lru].dev);
    c->rs_tables.erase(c->rs_tables.begin() + lru);
  }
  se_ctx::ResampleTable t;
  t.in = in; t.out = out; t.filter = filter; t.ksize = ksize;
  t.host.resize((size_t)out * (2 + ksize));
  resample_coeffs(in, out, filter, t.host.data(), t.host.data() + 2 * (size_t)out);
  hipError_t e = hipMalloc(&t.dev, t.host.size() * sizeof(int));
  if (e == hipSuccess) e = hipMemcpyAsync(t.dev, t.host.data(), t.host.size() * sizeof(int), hipMemcpyHostToDevice, c->rs_stream);
  if (e != hipSuccess) {
    if (t.dev) (void)hipFree(t.dev);
    fail(c, "resize: coefficient upload failed: %s", hipGetErrorString(e));
    return nullptr;
  }
  t.last_use = ++c->rs_clock;
  c->rs_tables.push_back(std::move(t));
  return &c->rs_tables.back();
}

unsigned char* rs_scratch(se_ctx* c, size_t bytes) {
  if (bytes > c->rs_scratch_bytes) {
    if (c->rs_scratch) {
      (void)hipStreamSynchronize(c->rs_stream);
      (void)hipFree(c->rs_scratch);
      c->rs_scratch = nullptr; c->rs_scratch_bytes = 0;
    }
    const size_t sz = (bytes + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1);
    if (hipMalloc(&c->rs_scratch, sz) != hipSuccess) { c->rs_scratch = nullptr; fail(c, "resize: cannot allocate %zu bytes", sz); return nullptr; }
    c->rs_scratch_bytes = sz;
  }
  return c->rs_scratch;
}

// in (B,Hin,Win,C) uint8 -> the resize to Hout x Wout, written as `o` says (o.H, o.W are set here).  Called under the ctx lock.
int resize_locked(se_ctx* c, hipStream_t st, const unsigned char* in, int B, int Hin, int Win, int C, ResizeOut o, int Hout,
                  int Wout, int filter) {
  if (!in || (o.mode == RESIZE_OUT_U8 ? !o.u8 : !o.f32)) return fail(c, "null pointer argument");
  if (B < 1 || B > 65535 || Hin < 1 || Win < 1 || Hout < 1 || Wout < 1 || Hin > 65535 || Hout > 65535 || (C != 1 && C != 3))
    return fail(c, "resize: bad shape B=%d %dx%dx%d -> %dx%d (C in {1, 3}, heights and B < 65536)", B, Hin, Win, C, Hout, Wout);
  if (filter != SE_RESAMPLE_BILINEAR && filter != SE_RESAMPLE_BICUBIC && filter != SE_RESAMPLE_LANCZOS)
    return fail(c, "resize: unsupported filter %d", filter);
  if (o.mode == RESIZE_OUT_IMAGE_F32) o.lut = c->lut8;
  if (rs_enter(c, st)) return 1;
  set_profiler(&c->prof);
  o.H = Hout; o.W = Wout;
  const bool need_h = Win != Wout, need_v = Hin != Hout;
  if (!need_h && !need_v) {       // Image.resize returns a copy
    if (o.mode == RESIZE_OUT_U8) {
      HIPCHK(c, hipMemcpyAsync(o.u8, in, (size_t)B * Hin * Win * C, hipMemcpyDeviceToDevice, st));
      return 0;
    }
    // the dequantisation kernel moves 4 pixels per lane (dword loads, float4 stores)
    if (((size_t)Hin * Win) % 4 || ((uintptr_t)in & 3) || ((uintptr_t)o.f32 & 15))
      return fail(c, "resize: an unresized fp32 output needs H W %% 4 == 0, a 4-byte aligned input and a 16-byte aligned output");
    // (the kernel stages the whole table in LDS whichever output it writes: always the ctx's table, never o.lut)
    if (o.mode == RESIZE_OUT_IMAGE_F32 && C == 3)
      HIPCHK(c, launch_dequantize_u8(in, nullptr, c->lut8, o.f32, nullptr, B, Hin, Win, st));
    else if (o.mode == RESIZE_OUT_SKETCH_F32 && C == 1)
      HIPCHK(c, launch_dequantize_u8(nullptr, in, c->lut8, nullptr, o.f32, B, Hin, Win, st));
    else
      return fail(c, "resize: fp32 outputs are a 3-channel image or a 1-channel sketch");
    return 0;
  }
  const se_ctx::ResampleTable* th = need_h ? rs_table(c, Win, Wout, filter) : nullptr;
  const se_ctx::ResampleTable* tv = need_v ? rs_table(c, Hin, Hout, filter) : nullptr;
  if ((need_h && !th) || (need_v && !tv)) return 1;
  // the second lookup may have moved the table vector: look the first table up again (it is the most recently used
  // entry, so the second lookup did not evict it)
  if (need_h && need_v) th = rs_table(c, Win, Wout, filter);
  const unsigned char* src = in;
  if (need_h) {
    ResizeOut oh = o;
    if (need_v) {
      unsigned char* mid = rs_scratch(c, (size_t)B * Hin * Wout * C);
      if (!mid) return 1;
      if (poison(c, mid, (size_t)B * Hin * Wout * C, st)) return 1;
      oh.mode = RESIZE_OUT_U8; oh.u8 = mid; oh.H = Hin;
      src = mid;
    }
    const int* d = th->dev;
    HIPCHK(c, launch_resample_h(in, d, d + 2 * (size_t)Wout, th->host.data(), th->ksize, B, Hin, Win, Wout, C, oh, st));
  }
  if (need_v) {
    const int* d = tv->dev;
    HIPCHK(c, launch_resample_v(src, d, d + 2 * (size_t)Hout, tv->ksize, B, Hin, Hout, Wout, C, o, st));
  }
  return 0;
}

}  // namespace

// ====================================================================================================
extern "C" {

const char* se_version(void) { return "sketchedit_hip 0.2 (gfx950)"; }

int se_create(int device_id, se_ctx** out) {
  if (!out) return 1;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device_id < 0 || device_id >= n) return fail(nullptr, "no such HIP device %d (count %d)", device_id, n);
  se_ctx* c = new (std::nothrow) se_ctx();
  if (!c) return 1;
  c->device = device_id;
  if (hipSetDevice(device_id) != hipSuccess || hipMalloc(&c->zeros, 4096) != hipSuccess ||
      hipMemset(c->zeros, 0, 4096) != hipSuccess) {
    delete c;
    return fail(nullptr, "device init failed");
  }
  // side-branch stream + fork/join events of the low-latency mode (concurrent branches of netG)
  if (hipStreamCreateWithFlags(&c->st_side, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess) {
    se_destroy(c);
    return fail(nullptr, "stream / event creation failed");
  }
  {
    // data/testimage_dataset.py:89-111 of the reference (ToTensor: /255, Normalize: -0.5, /0.5), one IEEE fp32 operation at a
    // time on the host (volatile: no reassociation, no reciprocal): the table the device looks up
    float lut[256];
    for (int v = 0; v < 256; ++v) {
      volatile float t = (float)v;
      t = t / 255.0f;
      t = t - 0.5f;
      t = t / 0.5f;
      lut[v] = t;
    }
    if (hipMalloc(&c->lut8, sizeof lut) != hipSuccess || hipMemcpy(c->lut8, lut, sizeof lut, hipMemcpyHostToDevice) != hipSuccess) {
      se_destroy(c);
      return fail(nullptr, "device init failed (dequantisation table)");
    }
  }
  for (int i = 0; i < NG; ++i) c->G[G_LAYERS[i].name].def = G_LAYERS[i];
  for (int i = 0; i < NM; ++i) c->M[M_LAYERS[i].name].def = M_LAYERS[i];
  // (the 4-channel form of wconv1 is planned by the dry runs of se_workspace_bytes before any weight exists: a zero stride in
  // its definition was a division by zero for a ctx that had only netM's weights -- found by tools/f43_flips.py, round 5)
  c->wconv1_j4.def = c->G.at("wconv1").def;
  *out = c;
  return 0;
}

void se_destroy(se_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  c->G.clear(); c->M.clear(); c->wconv1_j4 = Layer();       // the layers' device images
  if (c->zeros) (void)hipFree(c->zeros);
  if (c->lut8) (void)hipFree(c->lut8);
  for (auto& t : c->rs_tables) (void)hipFree(t.dev);
  if (c->rs_scratch) (void)hipFree(c->rs_scratch);
  if (c->rs_event) (void)hipEventDestroy(c->rs_event);
  if (c->win_host) (void)hipHostFree(c->win_host);
  if (c->win_dev) (void)hipFree(c->win_dev);
  for (hipEvent_t e : c->win_half_done) if (e) (void)hipEventDestroy(e);
  if (c->win_event) (void)hipEventDestroy(c->win_event);
  for (auto& e : c->prof.pool) (void)hipEventDestroy(e);
  drop_graphs(c);
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  if (c->ev_join) (void)hipEventDestroy(c->ev_join);
  if (c->st_side) (void)hipStreamDestroy(c->st_side);
  delete c;
}

// the message of the last failed call on this ctx, copied under the ctx lock into a per-thread buffer (threaded callers)
const char* se_last_error(se_ctx* c) {
  if (!c) return g_create_err.c_str();
  thread_local std::string copy;
  std::lock_guard<std::mutex> lk(c->mu);
  copy = c->err;
  return copy.c_str();
}

int se_load_weights(se_ctx* c, int net_id, const char* name, const float* host, const int* shape, int ndim) {
  if (!c || !name || !host || !shape) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  (void)hipSetDevice(c->device);
  drop_graphs(c);                       // captured forwards hold the old weight images
  std::string key(name);
  if (key.rfind("module.", 0) == 0) key = key.substr(7);          // util/util.py:221-222
  const size_t dot = key.rfind('.');
  if (dot == std::string::npos) return fail(c, "bad key %s", name);
  const std::string lname = key.substr(0, dot), kind = key.substr(dot + 1);
  auto& net = net_id == SE_NET_G ? c->G : c->M;
  auto it = net.find(lname);
  if (it == net.end()) return fail(c, "unexpected key %s for net %d", name, net_id);
  Layer& L = it->second;
  const LayerDef& d = L.def;
  if (kind == "weight") {
    if (ndim != 4 || shape[0] != d.cout || shape[1] != d.cin || shape[2] != d.k || shape[3] != d.k)
      return fail(c, "size mismatch for %s", name);
    L.w.assign(host, host + (size_t)d.cout * d.cin * d.k * d.k);
    L.have_w = true;
  } else if (kind == "bias") {
    if (ndim != 1 || shape[0] != d.cout) return fail(c, "size mismatch for %s", name);
    L.b.assign(host, host + d.cout);
    L.have_b = true;
  } else {
    return fail(c, "unexpected key %s", name);
  }
  if (!L.have_w || !L.have_b) return 0;
  std::vector<int> chans(d.cin);
  std::iota(chans.begin(), chans.end(), 0);
  if (pack_layer_images(L, chans, c->err)) return 1;
  if (std::string(d.name) == "wconv1" && d.cin == 5) {
    // editline_g.py:132-133: with joint_train_inp the style branch sees guide * 0, so its first layer is a 4-channel
    // conv (image*mask, mask) with the guide column of the weights dropped: K = 100 instead of 200 (NHWC8 padding)
    Layer& J = c->wconv1_j4;
    J.def = d; J.w = L.w; J.b = L.b; J.have_w = J.have_b = true;
    return pack_layer_images(J, {0, 1, 2, 4}, c->err);
  }
  return 0;
}

int se_weights_ready(se_ctx* c) {
  if (!c) return 0;
  std::lock_guard<std::mutex> lk(c->mu);
  for (auto* net : {&c->G, &c->M})
    for (auto& kv : *net)
      if (!kv.second.packed) return 0;
  return 1;
}

size_t se_workspace_bytes(se_ctx* c, int B, int H, int W) {
  if (!c) return 0;
  std::lock_guard<std::mutex> lk(c->mu);
  if (check_dims(c, B, H, W)) return 0;
  c->fork2 = opt(OPT_FORK_DEFAULT) != 0;
  // every flag combination that changes the allocation sequence (a first-fit arena does not peak monotonically):
  // attention on/off, 4- or 8-channel style input, in-line or concurrent branches, fp32 or bf16 activations
  size_t peak = 0;
  for (int cam = 0; cam < 2; ++cam)
    for (int joint = 0; joint < 2; ++joint)
      for (int ll = 0; ll < 2; ++ll)
        for (int bf = 0; bf < 2; ++bf) {      // (bf16 activations are smaller, but its attention scratch need not be)
          const int flags = (cam ? SE_FLAG_USE_CAM : 0) | (joint ? SE_FLAG_JOINT_TRAIN_INP : 0) | (ll ? SE_FLAG_LOW_LATENCY : 0) |
                            (bf ? SE_FLAG_BF16 : 0) | SE_FLAG_POOL_MAX;
          // a batch beyond the kernels' 32-bit byte offsets runs as passes (pass_size): the workspace serves one pass at a time
          const int nb = pass_size(c, B, H, W, flags);
          if (!nb) return 0;
          const int last = B % nb;                      // size of a ragged last pass (0: none)
          // with and without netM's image decoder (mode='visualize' vs 'inference'): two allocation sequences
          // ... each on two streams and on one (the profiler's plan of the default mode: c->serial)
          for (int ser = 0; ser < 2; ++ser)
            for (int mi = 0; mi < 2; ++mi)
              for (int bb : {nb, last}) {
                if (!bb) continue;
                c->serial = ser != 0;
                const se_ctx::Peaks pk = plan_peaks(c, 3, bb, H, W, flags, mi != 0);
                if (pk.main + pk.side > peak) peak = pk.main + pk.side;
              }
          c->serial = false;
        }
  // + hard-mask (se_inference) and soft-mask (se_inference_u8) planes + the fp32 image / sketch of se_inference_u8io (4 planes)
  return peak + 6 * (((size_t)B * H * W * 4 + 255) & ~(size_t)255);
}

int se_netM_forward_ex(se_ctx* c, void* stream, const float* image, const float* sketch, float* mask_out,
                       float* maskim_out, void* ws, size_t ws_bytes, int B, int H, int W, int exec_flags) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (check_dims(c, B, H, W)) return 1;
  if (!image || !sketch || !mask_out || !ws) return fail(c, "null pointer argument");
  if (forward_enter(c)) return 1;
  exec_flags &= SE_FLAG_LOW_LATENCY | SE_FLAG_BF16 | SE_FLAG_CONSERVATIVE;
  const int nb = pass_size(c, B, H, W, exec_flags);
  if (!nb) return 1;
  const size_t HW = (size_t)H * W;
  for (int b0 = 0; b0 < B; b0 += nb) {
    const int bb = std::min(nb, B - b0);
    if (carve(c, plan_peaks(c, 1, bb, H, W, exec_flags, maskim_out != nullptr), ws, ws_bytes, 0)) return 1;
    begin_call(c, stream, exec_flags);
    const int rc = plan_netM(c, image + b0 * 3 * HW, sketch + b0 * HW, mask_out + b0 * HW, nullptr,
                             maskim_out ? maskim_out + b0 * 3 * HW : nullptr, bb, H, W);
    if (rc) return rc;
  }
  return 0;
}

int se_netM_forward(se_ctx* c, void* stream, const float* image, const float* sketch, float* mask_out,
                    float* maskim_out, void* ws, size_t ws_bytes, int B, int H, int W) {
  return se_netM_forward_ex(c, stream, image, sketch, mask_out, maskim_out, ws, ws_bytes, B, H, W, 0);
}

int se_netG_forward_taps(se_ctx* c, void* stream, const float* x, const float* x2, const float* mask, const float* mask2,
                         const float* guide, float* coarse_out, float* fine_out, void* ws, size_t ws_bytes, int B, int H,
                         int W, int flags, const se_netG_taps* taps) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (check_dims(c, B, H, W)) return 1;
  if (!x || !x2 || !mask || !mask2 || !guide || !fine_out || !ws) return fail(c, "null pointer argument");
  if (forward_enter(c)) return 1;
  const int nb = pass_size(c, B, H, W, flags);
  if (!nb) return 1;
  if (taps && nb < B) return fail(c, "se_netG_forward_taps: %d images do not fit one pass (%d)", B, nb);
  const size_t HW = (size_t)H * W;
  for (int b0 = 0; b0 < B; b0 += nb) {
    const int bb = std::min(nb, B - b0);
    if (carve(c, plan_peaks(c, 2, bb, H, W, flags, false), ws, ws_bytes, 0)) return 1;
    begin_call(c, stream, flags);
    c->taps = taps;
    const int rc = plan_netG(c, x + b0 * 3 * HW, x2 + b0 * 3 * HW, mask + b0 * HW, mask2 + b0 * HW, guide + b0 * HW,
                             coarse_out ? coarse_out + b0 * 3 * HW : nullptr, fine_out + b0 * 3 * HW, nullptr, nullptr, bb, H, W, flags);
    c->taps = nullptr;
    if (rc) return rc;
  }
  return 0;
}

int se_netG_forward(se_ctx* c, void* stream, const float* x, const float* x2, const float* mask, const float* mask2,
                    const float* guide, float* coarse_out, float* fine_out, void* ws, size_t ws_bytes, int B, int H,
                    int W, int flags) {
  return se_netG_forward_taps(c, stream, x, x2, mask, mask2, guide, coarse_out, fine_out, ws, ws_bytes, B, H, W, flags, nullptr);
}

namespace {
// netM -> threshold -> netG -> composite, enqueued on `stream` (and, in low-latency mode, the ctx's side stream)
int enqueue_inference(se_ctx* c, void* stream, const float* image, const float* sketch, float* composed_out, float* mask_out,
                      float* hard_out, float* maskim_out, float* coarse_out, float* fine_out, void* ws, size_t ws_bytes,
                      int B, int H, int W, int flags, const unsigned char* lock8 = nullptr) {
  // the hard mask lives at the end of the workspace for the whole call
  const size_t plane = ((size_t)B * H * W * 4 + 255) & ~(size_t)255;
  float* hard_all = hard_out ? hard_out : (float*)((char*)ws + ws_bytes - plane);
  // SE_FLAG_PACKED_OUT: composed_out is one (B,4,H,W) buffer, planes 0-2 the composite, plane 3 the soft mask
  const size_t HW = (size_t)H * W;
  const long packed_bs = (flags & SE_FLAG_PACKED_OUT) ? 4l * H * W : 0;
  if (packed_bs) mask_out = composed_out + 3 * HW;
  const size_t comp_bs = packed_bs ? (size_t)packed_bs : 3 * HW, mask_bs = packed_bs ? (size_t)packed_bs : HW;
  // a batch beyond the kernels' 32-bit byte offsets runs as passes over image ranges (pass_size)
  const int nb = pass_size(c, B, H, W, flags);
  if (!nb) return 1;
  if (!hard_out && poison(c, hard_all, plane, (hipStream_t)stream)) return 1;
  for (int b0 = 0; b0 < B; b0 += nb) {
    const int bb = std::min(nb, B - b0);
    const se_ctx::Peaks pk = plan_peaks(c, 3, bb, H, W, flags, maskim_out != nullptr);
    if (carve(c, pk, ws, ws_bytes, plane)) return 1;
    const float *img = image + b0 * 3 * HW, *sk = sketch + b0 * HW;
    float *hard = hard_all + b0 * HW, *mk = mask_out + b0 * mask_bs;
    begin_call(c, stream, flags);
    int rc = plan_netM(c, img, sk, mk, hard, maskim_out ? maskim_out + b0 * 3 * HW : nullptr, bb, H, W, packed_bs,     // editline2_model.py:339,346-347
                       lock8 ? lock8 + b0 * HW : nullptr);
    if (rc) return rc;
    if (carve(c, pk, ws, ws_bytes, plane)) return 1;
    // netG(inputs, inputs, mask_inpaint, mask_inpaint, line)  :366-368 ; composite with the soft mask :132
    rc = plan_netG(c, img, img, hard, hard, sk, coarse_out ? coarse_out + b0 * 3 * HW : nullptr, fine_out ? fine_out + b0 * 3 * HW : nullptr,
                   mk, composed_out + b0 * comp_bs, bb, H, W, flags, packed_bs);
    if (rc) return rc;
  }
  return 0;
}
}  // namespace

int se_inference(se_ctx* c, void* stream, const float* image, const float* sketch, float* composed_out,
                 float* mask_out, float* hard_out, float* maskim_out, float* coarse_out, float* fine_out, void* ws,
                 size_t ws_bytes, int B, int H, int W, int flags) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (check_dims(c, B, H, W)) return 1;
  if (!image || !sketch || !composed_out || (!mask_out && !(flags & SE_FLAG_PACKED_OUT)) || !ws) return fail(c, "null pointer argument");
  if (forward_enter(c)) return 1;
  // (SE_TEST_POISON set: uncaptured, and nothing enters the graph cache -- the fills belong to the test aid, not to a graph)
  if (!(flags & SE_FLAG_GRAPH) || c->prof.on || poison_byte() != 0)
    return enqueue_inference(c, stream, image, sketch, composed_out, mask_out, hard_out, maskim_out, coarse_out, fine_out, ws,
                             ws_bytes, B, H, W, flags);
  // SE_FLAG_GRAPH: the forward for these exact arguments (every pointer is baked into the kernel nodes) is captured
  // into a hipGraph the second time it is seen and replayed from then on: one launch instead of ~85, and the two
  // branches of the low-latency mode become parallel graph nodes.  The first call runs eagerly (it also sets the
  // per-device kernel attributes, which must not happen under capture).
  const std::vector<long long> key = {(long long)(size_t)image, (long long)(size_t)sketch, (long long)(size_t)composed_out,
                                      (long long)(size_t)mask_out, (long long)(size_t)hard_out, (long long)(size_t)maskim_out,
                                      (long long)(size_t)coarse_out, (long long)(size_t)fine_out, (long long)(size_t)ws,
                                      (long long)ws_bytes, B, H, W, flags, opt_epoch()};
  se_ctx::GraphEntry* ge = nullptr;
  for (auto& g : c->graphs)
    if (g.key == key) { ge = &g; break; }
  if (!ge) {
    if (c->graphs.size() >= 16) evict_lru_graph(c);
    c->graphs.emplace_back();
    c->graphs.back().key = key;
    c->graphs.back().last_use = ++c->graph_clock;
    return enqueue_inference(c, stream, image, sketch, composed_out, mask_out, hard_out, maskim_out, coarse_out, fine_out, ws,
                             ws_bytes, B, H, W, flags);
  }
  ge->last_use = ++c->graph_clock;
  if (!ge->exec) {
    if (!stream) return fail(c, "SE_FLAG_GRAPH needs a non-default stream (capture is not permitted on the legacy stream)");
    HIPCHK(c, hipStreamBeginCapture((hipStream_t)stream, hipStreamCaptureModeThreadLocal));
    const int rc = enqueue_inference(c, stream, image, sketch, composed_out, mask_out, hard_out, maskim_out, coarse_out,
                                     fine_out, ws, ws_bytes, B, H, W, flags);
    hipGraph_t graph = nullptr;
    const hipError_t e = hipStreamEndCapture((hipStream_t)stream, &graph);
    if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    if (e != hipSuccess) return fail(c, "hipStreamEndCapture failed: %s", hipGetErrorString(e));
    hipGraphExec_t exec = nullptr;
    const hipError_t e2 = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    if (e2 != hipSuccess) { (void)hipGraphDestroy(graph); return fail(c, "hipGraphInstantiate failed: %s", hipGetErrorString(e2)); }
    ge->graph = graph; ge->exec = exec;
  }
  ge->stream = (hipStream_t)stream;
  ge->last_use = ++c->graph_clock;
  HIPCHK(c, hipGraphLaunch(ge->exec, (hipStream_t)stream));
  return 0;
}

// se_inference with a lock plane: the soft mask is 0 where lock_u8 is non-zero, before the threshold
int se_inference_locked(se_ctx* c, void* stream, const float* image, const float* sketch, const unsigned char* lock_u8,
                        float* composed_out, float* mask_out, float* hard_out, float* maskim_out, float* coarse_out, float* fine_out,
                        void* ws, size_t ws_bytes, int B, int H, int W, int flags) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (check_dims(c, B, H, W)) return 1;
  if (!image || !sketch || !composed_out || (!mask_out && !(flags & SE_FLAG_PACKED_OUT)) || !ws) return fail(c, "null pointer argument");
  if (forward_enter(c)) return 1;
  return enqueue_inference(c, stream, image, sketch, composed_out, mask_out, hard_out, maskim_out, coarse_out, fine_out, ws,
                           ws_bytes, B, H, W, flags & ~SE_FLAG_GRAPH, lock_u8);
}

// The forward with the output quantisation of test.py:25-27 fused into its last kernel: the composite and the soft mask
// leave the device as uint8 only (a quarter of the fp32 bytes, no separate pass); the soft mask needed between netM and
// the final composite lives in the workspace.
namespace {
// `tail_planes` fp32 (B,H,W) planes at the end of the workspace are the caller's; the soft and hard masks sit in front of them
// (`_locked` = the ctx's mutex is held; lock8 = the (B,H,W) lock plane of DESIGN.md 6g, or null)
int inference_u8_locked(se_ctx* c, void* stream, const float* image, const float* sketch, unsigned char* rgb_out,
                        unsigned char* mask_u8_out, void* ws, size_t ws_bytes, int B, int H, int W, int flags, int tail_planes,
                        const unsigned char* lock8 = nullptr) {
  flags &= ~(SE_FLAG_GRAPH | SE_FLAG_PACKED_OUT);
  const size_t plane = ((size_t)B * H * W * 4 + 255) & ~(size_t)255;
  const size_t tail = (2 + (size_t)tail_planes) * plane;
  if (ws_bytes < tail) return fail(c, "workspace too small: %zu bytes", ws_bytes);
  float* hard_all = (float*)((char*)ws + ws_bytes - tail + plane);
  float* soft_all = (float*)((char*)ws + ws_bytes - tail);
  const size_t HW = (size_t)H * W;
  const int nb = pass_size(c, B, H, W, flags);       // passes over image ranges beyond the kernels' 32-bit byte offsets
  if (!nb) return 1;
  if (poison(c, soft_all, 2 * plane, (hipStream_t)stream)) return 1;      // (the caller's tail planes are the caller's to fill)
  for (int b0 = 0; b0 < B; b0 += nb) {
    const int bb = std::min(nb, B - b0);
    const se_ctx::Peaks pk = plan_peaks(c, 3, bb, H, W, flags, false);
    if (carve(c, pk, ws, ws_bytes, tail)) return 1;
    const float *img = image + b0 * 3 * HW, *sk = sketch + b0 * HW;
    float *hard = hard_all + b0 * HW, *soft = soft_all + b0 * HW;
    begin_call(c, stream, flags);
    int rc = plan_netM(c, img, sk, soft, hard, nullptr, bb, H, W, 0, lock8 ? lock8 + b0 * HW : nullptr);
    if (rc) return rc;
    if (carve(c, pk, ws, ws_bytes, tail)) return 1;
    c->rgb8 = rgb_out + b0 * 3 * HW; c->m8 = mask_u8_out ? mask_u8_out + b0 * HW : nullptr;
    rc = plan_netG(c, img, img, hard, hard, sk, nullptr, nullptr, soft, nullptr, bb, H, W, flags);
    if (rc) return rc;
  }
  return 0;
}
}  // namespace

int se_inference_u8(se_ctx* c, void* stream, const float* image, const float* sketch, unsigned char* rgb_out,
                    unsigned char* mask_u8_out, void* ws, size_t ws_bytes, int B, int H, int W, int flags) {
  return se_inference_u8_locked(c, stream, image, sketch, nullptr, rgb_out, mask_u8_out, ws, ws_bytes, B, H, W, flags);      // (locks there)
}

int se_inference_u8_locked(se_ctx* c, void* stream, const float* image, const float* sketch, const unsigned char* lock_u8,
                           unsigned char* rgb_out, unsigned char* mask_u8_out, void* ws, size_t ws_bytes, int B, int H, int W, int flags) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (check_dims(c, B, H, W)) return 1;
  if (!image || !sketch || !rgb_out || !ws) return fail(c, "null pointer argument");
  if (forward_enter(c)) return 1;
  return inference_u8_locked(c, stream, image, sketch, rgb_out, mask_u8_out, ws, ws_bytes, B, H, W, flags, 0, lock_u8);
}

// data/testimage_dataset.py:89-111 on the device (table lookup; see se_create)
int se_dequantize_u8(se_ctx* c, void* stream, const unsigned char* image_u8, const unsigned char* sketch_u8, float* image_out,
                     float* sketch_out, int B, int H, int W) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (check_dims(c, B, H, W)) return 1;
  if ((image_out && !image_u8) || (sketch_out && !sketch_u8)) return fail(c, "null pointer argument");
  HIPCHK(c, hipSetDevice(c->device));
  set_profiler(&c->prof);
  HIPCHK(c, launch_dequantize_u8(image_u8, sketch_u8, c->lut8, image_out, sketch_out, B, H, W, (hipStream_t)stream));
  return 0;
}

// uint8 in, uint8 out: the fp32 image (3 planes) and sketch (1 plane) live at the very end of the workspace
int se_inference_u8io(se_ctx* c, void* stream, const unsigned char* image_u8, const unsigned char* sketch_u8,
                      unsigned char* rgb_out, unsigned char* mask_u8_out, void* ws, size_t ws_bytes, int B, int H, int W,
                      int flags) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (check_dims(c, B, H, W)) return 1;
  if (!image_u8 || !sketch_u8 || !rgb_out || !ws) return fail(c, "null pointer argument");
  if (forward_enter(c)) return 1;
  const size_t plane = ((size_t)B * H * W * 4 + 255) & ~(size_t)255;
  if (ws_bytes < 6 * plane) return fail(c, "workspace too small: %zu bytes", ws_bytes);
  float* image = (float*)((char*)ws + ws_bytes - 4 * plane);      // (B,3,H,W) contiguous: 3 B H W floats <= 3 planes
  float* sketch = (float*)((char*)ws + ws_bytes - plane);
  set_profiler(&c->prof);
  if (poison(c, image, 4 * plane, (hipStream_t)stream)) return 1;
  HIPCHK(c, launch_dequantize_u8(image_u8, sketch_u8, c->lut8, image, sketch, B, H, W, (hipStream_t)stream));
  return inference_u8_locked(c, stream, image, sketch, rgb_out, mask_u8_out, ws, ws_bytes, B, H, W, flags, 4);
}

// test.py:25-27 on the device
int se_quantize_u8(se_ctx* c, void* stream, const float* composed, const float* mask, unsigned char* rgb_out,
                   unsigned char* mask_u8_out, int B, int H, int W) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (check_dims(c, B, H, W)) return 1;
  if ((rgb_out && !composed) || (mask_u8_out && !mask)) return fail(c, "null pointer argument");
  HIPCHK(c, hipSetDevice(c->device));
  set_profiler(&c->prof);
  HIPCHK(c, launch_quantize_u8(composed, mask, rgb_out, mask_u8_out, B, H, W, (hipStream_t)stream));
  return 0;
}

// ---- the demo's per-request steps (demo.py:39-73) on the device -----------------------------------------------------
int se_resize_u8(se_ctx* c, void* stream, const unsigned char* in, int B, int Hin, int Win, int C, unsigned char* out, int Hout,
                 int Wout, int filter) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCHK(c, hipSetDevice(c->device));
  ResizeOut o{RESIZE_OUT_U8, out, nullptr, nullptr, 0, 0};
  return resize_locked(c, (hipStream_t)stream, in, B, Hin, Win, C, o, Hout, Wout, filter);
}

namespace {
// demo.py:40-56 for B requests of one raw size: the BICUBIC resizes, written as the forward's fp32 inputs
int prepare_locked(se_ctx* c, hipStream_t st, const unsigned char* image_u8, int B, int Hi, int Wi, const unsigned char* sketch_u8,
                   int Hs, int Ws, float* image_out, float* sketch_out, int H, int W) {
  if (check_dims(c, B, H, W)) return 1;
  if ((image_out && !image_u8) || (sketch_out && !sketch_u8)) return fail(c, "null pointer argument");
  if (image_out) {
    ResizeOut o{RESIZE_OUT_IMAGE_F32, nullptr, image_out, c->lut8, 0, 0};
    if (resize_locked(c, st, image_u8, B, Hi, Wi, 3, o, H, W, SE_RESAMPLE_BICUBIC)) return 1;
  }
  if (sketch_out) {
    ResizeOut o{RESIZE_OUT_SKETCH_F32, nullptr, sketch_out, nullptr, 0, 0};
    if (resize_locked(c, st, sketch_u8, B, Hs, Ws, 1, o, H, W, SE_RESAMPLE_BICUBIC)) return 1;
  }
  return 0;
}

// working size of a raw request (demo.py:43-45), or an error where the host path refuses it
int edit_dims(se_ctx* c, int B, int Hi, int Wi, int* H, int* W) {
  *H = Hi / 8 * 8; *W = Wi / 8 * 8;
  if (B < 1 || *H < 16 || *W < 16) return fail(c, "image too small: %dx%d (working size %dx%d, needs >= 16)", Wi, Hi, *W, *H);
  return 0;
}
}  // namespace

int se_prepare_u8(se_ctx* c, void* stream, const unsigned char* image_u8, int Hi, int Wi, const unsigned char* sketch_u8, int Hs,
                  int Ws, float* image_out, float* sketch_out, int H, int W) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCHK(c, hipSetDevice(c->device));
  return prepare_locked(c, (hipStream_t)stream, image_u8, 1, Hi, Wi, sketch_u8, Hs, Ws, image_out, sketch_out, H, W);
}

size_t se_edit_u8_workspace_bytes(se_ctx* c, int B, int Hi, int Wi) {
  if (!c) return 0;
  int H, W;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    if (edit_dims(c, B, Hi, Wi, &H, &W)) return 0;
  }
  const size_t fwd = se_workspace_bytes(c, B, H, W);
  if (!fwd) return 0;
  // + the uint8 result at the working size, in front of the forward's part
  return fwd + (((size_t)B * H * W * 3 + 255) & ~(size_t)255);
}

// [uint8 result at the working size | the workspace of se_inference_u8io: arenas, masks, fp32 image and sketch at its end]
int se_edit_u8(se_ctx* c, void* stream, const unsigned char* image_u8, const unsigned char* sketch_u8, unsigned char* rgb_out,
               void* ws, size_t ws_bytes, int B, int Hi, int Wi, int Hs, int Ws, int flags) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  int H, W;
  if (edit_dims(c, B, Hi, Wi, &H, &W)) return 1;
  if (check_dims(c, B, H, W)) return 1;
  if (!image_u8 || !sketch_u8 || !rgb_out || !ws) return fail(c, "null pointer argument");
  if (forward_enter(c)) return 1;
  const size_t plane = ((size_t)B * H * W * 4 + 255) & ~(size_t)255, rgbw = ((size_t)B * H * W * 3 + 255) & ~(size_t)255;
  if (ws_bytes < rgbw + 6 * plane) return fail(c, "workspace too small: %zu bytes", ws_bytes);
  unsigned char* rgb_work = (unsigned char*)ws;
  char* fws = (char*)ws + rgbw;
  const size_t fws_bytes = ws_bytes - rgbw;
  float* image = (float*)(fws + fws_bytes - 4 * plane);      // where se_inference_u8io keeps them
  float* sketch = (float*)(fws + fws_bytes - plane);
  const hipStream_t st = (hipStream_t)stream;
  if (poison(c, rgb_work, rgbw, st) || poison(c, image, 4 * plane, st)) return 1;
  if (prepare_locked(c, st, image_u8, B, Hi, Wi, sketch_u8, Hs, Ws, image, sketch, H, W)) return 1;
  if (inference_u8_locked(c, stream, image, sketch, rgb_work, nullptr, fws, fws_bytes, B, H, W, flags, 4)) return 1;
  ResizeOut o{RESIZE_OUT_U8, rgb_out, nullptr, nullptr, 0, 0};
  return resize_locked(c, st, rgb_work, B, H, W, 3, o, Hi, Wi, SE_RESAMPLE_BICUBIC);
}

// ---- editing sessions: window edits of a resident frame (se_window.hip) ------------------------------
namespace {

// the records of a call: frames given, sizes sane, every hs x ws window inside its frame
int win_check_records(se_ctx* c, const se_window* wins, int B, int hs, int ws, bool need_sketch) {
  for (int i = 0; i < B; ++i) {
    const se_window& w = wins[i];
    if (!w.frame_u8) return fail(c, "wins[%d].frame_u8 is null", i);
    if (need_sketch && !w.sketch_u8) return fail(c, "wins[%d].sketch_u8 is null", i);
    if (w.Hi < 1 || w.Wi < 1) return fail(c, "wins[%d]: bad frame size Hi=%d Wi=%d", i, w.Hi, w.Wi);
    if (w.y0 < 0 || (long long)w.y0 + hs > w.Hi)
      return fail(c, "wins[%d].y0=%d: rows [%d, %lld) of the window lie outside the frame (Hi=%d)", i, w.y0, w.y0, (long long)w.y0 + hs, w.Hi);
    if (w.x0 < 0 || (long long)w.x0 + ws > w.Wi)
      return fail(c, "wins[%d].x0=%d: columns [%d, %lld) of the window lie outside the frame (Wi=%d)", i, w.x0, w.x0, (long long)w.x0 + ws, w.Wi);
  }
  return 0;
}

// a launch that writes the frames runs concurrently for all requests: their windows must not share a byte
int win_check_disjoint(se_ctx* c, const se_window* wins, int B, int hs, int ws) {
  for (int i = 0; i < B; ++i)
    for (int j = i + 1; j < B; ++j) {
      const se_window &a = wins[i], &b = wins[j];
      const uintptr_t a0 = (uintptr_t)a.frame_u8, a1 = a0 + (size_t)a.Hi * a.Wi * 3, b0 = (uintptr_t)b.frame_u8, b1 = b0 + (size_t)b.Hi * b.Wi * 3;
      if (a1 <= b0 || b1 <= a0) continue;                 // frames apart in memory
      if (a0 != b0 || a.Wi != b.Wi || a.Hi != b.Hi)
        return fail(c, "wins[%d] and wins[%d]: frames overlap in memory without being the same frame", i, j);
      if (a.y0 < b.y0 + hs && b.y0 < a.y0 + hs && a.x0 < b.x0 + ws && b.x0 < a.x0 + ws)
        return fail(c, "wins[%d] and wins[%d] name overlapping windows of one frame", i, j);
    }
  return 0;
}

// every argument check of the window calls, on the host, before anything is enqueued.  H x W = the size the forward runs at,
// hs x ws = the window's extent in the frame (the same unless the edit runs at a working size)
int win_check(se_ctx* c, const se_window* wins, int B, int H, int W, int hs, int ws, bool need_sketch, bool writes) {
  if (check_dims(c, B, H, W)) return 1;
  if (hs < 16 || ws < 16) return fail(c, "bad window hs=%d ws=%d (a window is at least 16 x 16 frame pixels)", hs, ws);
  if (hs != H || ws != W) {
    if (hs > 65535) return fail(c, "bad window hs=%d (a resampled window has at most 65535 rows)", hs);
    const int io[4][2] = {{ws, W}, {hs, H}, {W, ws}, {H, hs}};       // a tap count the resize kernels refuse
    for (const auto& a : io)
      if (resample_ksize(a[0], a[1], SE_RESAMPLE_BICUBIC) > RESAMPLE_MAX_KSIZE)
        return fail(c, "window hs=%d ws=%d at H=%d W=%d: the resize %d -> %d needs more taps per output than the kernels take (%d)",
                    hs, ws, H, W, a[0], a[1], RESAMPLE_MAX_KSIZE);
  }
  if (!wins) return fail(c, "null pointer argument: wins");
  if (B > 65535 || (long long)B * H * W / 1024 >= (1ll << 31) || (long long)B * hs * ws / 1024 >= (1ll << 31))
    return fail(c, "window: B=%d %dx%d (window %dx%d) is more than one launch takes", B, H, W, hs, ws);
  if (win_check_records(c, wins, B, hs, ws, need_sketch)) return 1;
  return writes ? win_check_disjoint(c, wins, B, hs, ws) : 0;
}

// the records of one call -> the next B slots of the ctx's ring, copied to the device on `st`; returns the device address
const se_window* win_put(se_ctx* c, hipStream_t st, const se_window* wins, int B) {
  auto bad = [c](const char* what, hipError_t e) { fail(c, "window table: %s failed: %s", what, hipGetErrorString(e)); return (const se_window*)nullptr; };
  hipError_t e;
  if (c->win_used && c->win_stream != st) {
    if (!c->win_event && (e = hipEventCreateWithFlags(&c->win_event, hipEventDisableTiming)) != hipSuccess) return bad("hipEventCreate", e);
    if ((e = hipEventRecord(c->win_event, c->win_stream)) != hipSuccess) return bad("hipEventRecord", e);
    if ((e = hipStreamWaitEvent(st, c->win_event, 0)) != hipSuccess) return bad("hipStreamWaitEvent", e);
  }
  if ((size_t)B * 2 > c->win_cap) {       // (first use, or a group larger than half the ring: a new ring)
    if (c->win_used) (void)hipStreamSynchronize(c->win_stream);
    if (c->win_host) (void)hipHostFree(c->win_host);
    if (c->win_dev) (void)hipFree(c->win_dev);
    c->win_host = nullptr; c->win_dev = nullptr; c->win_cap = 0; c->win_pos = 0;
    c->win_half_used[0] = c->win_half_used[1] = false;
    size_t cap = 1024;
    while (cap < (size_t)B * 2) cap *= 2;
    if ((e = hipHostMalloc((void**)&c->win_host, cap * sizeof(se_window), hipHostMallocDefault)) != hipSuccess) { c->win_host = nullptr; return bad("hipHostMalloc", e); }
    if ((e = hipMalloc((void**)&c->win_dev, cap * sizeof(se_window))) != hipSuccess) { c->win_dev = nullptr; return bad("hipMalloc", e); }
    for (hipEvent_t& ev : c->win_half_done)
      if (!ev && (e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess) return bad("hipEventCreate", e);
    c->win_cap = cap;
  }
  c->win_stream = st;
  c->win_used = true;
  // win_pos = the next free record; a half is left when the group does not fit into what remains of it
  const size_t half = c->win_cap / 2;
  int h = c->win_pos <= half ? 0 : 1;                // (win_pos == half: half 0 is full, the group will not fit, it is left below)
  size_t off = c->win_pos - (size_t)h * half;
  if (off + (size_t)B > half) {       // leave this half: everything that used it is enqueued by now
    if ((e = hipEventRecord(c->win_half_done[h], st)) != hipSuccess) return bad("hipEventRecord", e);
    h ^= 1;
    off = 0;
    c->win_pos = (size_t)h * half;
    // entering a half used before: its last user was enqueued at least half a ring of records ago, so this returns at once
    if (c->win_half_used[h] && (e = hipEventSynchronize(c->win_half_done[h])) != hipSuccess) return bad("hipEventSynchronize", e);
  }
  c->win_half_used[h] = true;
  se_window* hst = c->win_host + c->win_pos;
  se_window* dev = c->win_dev + c->win_pos;
  memcpy(hst, wins, (size_t)B * sizeof(se_window));
  if ((e = hipMemcpyAsync(dev, hst, (size_t)B * sizeof(se_window), hipMemcpyHostToDevice, st)) != hipSuccess) return bad("hipMemcpyAsync", e);
  c->win_pos += (size_t)B;
  return dev;
}

bool aligned_to(const void* p, int a) { return ((uintptr_t)p & (uintptr_t)(a - 1)) == 0; }

size_t pad256(size_t n) { return (n + 255) & ~(size_t)255; }

// ---- window edits at a working size: the window resampled into the forward's inputs, the result resampled
// back with the paste rule as the last pass's epilogue.  Both ends use the resize's tables (and so its one-stream order).

// n coefficient tables (BICUBIC) at once.  A lookup that inserts may move the table vector, so everything is looked up a
// second time: the n most recently used entries are not evicted (n <= 2 here, the cache holds 64).
int rs_tables_n(se_ctx* c, int n, const int (*in_out)[2], const se_ctx::ResampleTable** out) {
  for (int pass = 0; pass < 2; ++pass)
    for (int i = 0; i < n; ++i)
      if (!(out[i] = rs_table(c, in_out[i][0], in_out[i][1], SE_RESAMPLE_BICUBIC))) return 1;
  return 0;
}

// pitch in pixels of the paste end's intermediates: rows start dword aligned
int paste_pitch(int ws) { return (ws + 3) & ~3; }
// intermediates of the two ends.  gather: (B,hs,W,3) uint8, reused for the sketch's (B,hs,W); paste: (B,H,P,3) and (B,H,P)
size_t gather_mid_bytes(int B, int hs, int W) { return pad256((size_t)B * hs * W * 3); }
size_t paste_mid_bytes(int B, int H, int ws) { return pad256((size_t)B * H * paste_pitch(ws) * 3) + pad256((size_t)B * H * paste_pitch(ws)); }

// the hs x ws windows -> the forward's fp32 inputs at H x W (not both equal).  The horizontal pass always runs: where ws == W
// its table is the identity (one tap of weight 1), which copies the window's rows as Pillow's skipped pass would.
int gather_resize_locked(se_ctx* c, hipStream_t st, const se_window* d, int B, int hs, int ws, int H, int W, float* image,
                         float* sketch, unsigned char* mid) {
  const bool need_v = hs != H;
  const int io[2][2] = {{ws, W}, {hs, H}};
  const se_ctx::ResampleTable* t[2] = {nullptr, nullptr};
  if (rs_tables_n(c, need_v ? 2 : 1, io, t)) return 1;
  for (int C = 3; C >= 1; C -= 2) {
    float* out = C == 3 ? image : sketch;
    if (!out) continue;
    ResizeOut o{C == 3 ? RESIZE_OUT_IMAGE_F32 : RESIZE_OUT_SKETCH_F32, nullptr, out, c->lut8, H, W};
    ResizeOut oh = o;
    if (need_v) { oh.mode = RESIZE_OUT_U8; oh.u8 = mid; oh.H = hs; }
    if (need_v && poison(c, mid, gather_mid_bytes(B, hs, W), st)) return 1;      // (each pass: the sketch's reuses the image's)
    HIPCHK(c, launch_window_resample_h(d, t[0]->dev, t[0]->dev + 2 * (size_t)W, t[0]->host.data(), t[0]->ksize, B, hs, ws, W, C, oh, st));
    if (need_v) HIPCHK(c, launch_resample_v(mid, t[1]->dev, t[1]->dev + 2 * (size_t)H, t[1]->ksize, B, hs, H, W, C, o, st));
  }
  return 0;
}

// rgb (B,H,W,3), m8 (B,H,W) -> resampled to hs x ws and pasted into the windows (not both sizes equal).  The vertical pass
// always runs (it carries the paste): where hs == H its table is the identity.
int paste_resize_locked(se_ctx* c, hipStream_t st, const se_window* d, int B, int hs, int ws, int H, int W, const unsigned char* rgb,
                        const unsigned char* m8, unsigned char* mid, bool locked = false) {
  const bool need_h = ws != W;
  const int io[2][2] = {{H, hs}, {W, ws}};
  const se_ctx::ResampleTable* t[2] = {nullptr, nullptr};
  if (rs_tables_n(c, need_h ? 2 : 1, io, t)) return 1;
  int P = W;
  if (need_h) {
    P = paste_pitch(ws);
    if (poison(c, mid, paste_mid_bytes(B, H, ws), st)) return 1;
    unsigned char* mid_rgb = mid;
    unsigned char* mid_m = mid + pad256((size_t)B * H * P * 3);
    const int* dk = t[1]->dev;
    ResizeOut o{RESIZE_OUT_U8, mid_rgb, nullptr, nullptr, H, P};      // (o.W is the row pitch of what the pass writes)
    HIPCHK(c, launch_resample_h(rgb, dk, dk + 2 * (size_t)ws, t[1]->host.data(), t[1]->ksize, B, H, W, ws, 3, o, st));
    o.u8 = mid_m;
    HIPCHK(c, launch_resample_h(m8, dk, dk + 2 * (size_t)ws, t[1]->host.data(), t[1]->ksize, B, H, W, ws, 1, o, st));
    rgb = mid_rgb; m8 = mid_m;
  }
  HIPCHK(c, launch_window_paste_v(d, rgb, m8, t[0]->dev, t[0]->dev + 2 * (size_t)hs, t[0]->ksize, B, H, hs, P, ws, st, locked));
  return 0;
}

// ---- locked regions: locks = a HOST array of B device pointers, request b's (Hi,Wi) uint8 lock plane or null

bool any_lock(const unsigned char* const* locks, int B) {
  for (int i = 0; locks && i < B; ++i)
    if (locks[i]) return true;
  return false;
}

// a call that writes frames: no lock plane may share a byte with one of them (the paste reads the plane while it writes)
int win_check_locks(se_ctx* c, const se_window* wins, const unsigned char* const* locks, int B) {
  for (int i = 0; i < B; ++i) {
    if (!locks[i]) continue;
    const uintptr_t l0 = (uintptr_t)locks[i], l1 = l0 + (size_t)wins[i].Hi * wins[i].Wi;
    for (int j = 0; j < B; ++j) {
      const uintptr_t f0 = (uintptr_t)wins[j].frame_u8, f1 = f0 + (size_t)wins[j].Hi * wins[j].Wi * 3;
      if (l0 < f1 && f0 < l1) return fail(c, "locks[%d] overlaps the frame of wins[%d]", i, j);
    }
  }
  return 0;
}

// the records of a locked call: the requests, then B records whose frame_u8 is the request's lock plane (as the journal's
// slots travel); one group of the ctx's ring
const se_window* win_put_locks(se_ctx* c, hipStream_t st, const se_window* wins, const unsigned char* const* locks, int B) {
  std::vector<se_window> recs(wins, wins + B);
  for (int i = 0; i < B; ++i) recs.push_back(se_window{const_cast<unsigned char*>(locks[i]), nullptr, 0, 0, 0, 0});
  return win_put(c, st, recs.data(), 2 * B);
}

size_t lock_mid_bytes(int B, int hs, int W) { return pad256((size_t)B * hs * W); }

// the hs x ws windows of the lock planes -> lock_out (B,H,W) in {0, 1} at the working size; d = the 2 B records.  Unscaled: one
// gather launch.  Scaled: the sketch's resample -- BICUBIC, then > 0 -- over the plane's rows, with the axis tables the image
// uses; mid = (B,hs,W) bytes where hs != H.
int lock_gather_locked(se_ctx* c, hipStream_t st, const se_window* d, int B, int hs, int ws, int H, int W, unsigned char* lock_out,
                       unsigned char* mid) {
  if (hs == H && ws == W) {
    HIPCHK(c, launch_window_lock_gather(d, lock_out, B, H, W, st));
    return 0;
  }
  const bool need_v = hs != H;
  const int io[2][2] = {{ws, W}, {hs, H}};
  const se_ctx::ResampleTable* t[2] = {nullptr, nullptr};
  if (rs_tables_n(c, need_v ? 2 : 1, io, t)) return 1;
  ResizeOut o{RESIZE_OUT_LOCK_U8, lock_out, nullptr, nullptr, H, W};
  ResizeOut oh = o;
  if (need_v) { oh.mode = RESIZE_OUT_U8; oh.u8 = mid; oh.H = hs; }
  if (need_v && poison(c, mid, lock_mid_bytes(B, hs, W), st)) return 1;
  HIPCHK(c, launch_window_lock_resample_h(d, t[0]->dev, t[0]->dev + 2 * (size_t)W, t[0]->host.data(), t[0]->ksize, B, hs, ws, W, oh, st));
  if (need_v) HIPCHK(c, launch_resample_v(mid, t[1]->dev, t[1]->dev + 2 * (size_t)H, t[1]->ksize, B, hs, H, W, 1, o, st));
  return 0;
}

// [uint8 result | uint8 mask | counts | working-size lock plane (a call with a lock only) | intermediates of the resample ends
// (scaled only) | the workspace of se_inference_u8io: arenas, masks, fp32 image and sketch at its end].  hs x ws == H x W: the
// window edit at the frame's own resolution.  locks null, or all its entries null: the edit without locks.
int edit_window_locked(se_ctx* c, void* stream, const se_window* wins, int B, int hs, int ws, int H, int W, unsigned char* rgb_out,
                       unsigned char* mask_u8_out, int* hits_out, int commit, void* wsp, size_t ws_bytes, int flags,
                       const unsigned char* const* locks = nullptr) {
  const bool scaled = hs != H || ws != W;
  if (win_check(c, wins, B, H, W, hs, ws, true, commit != 0)) return 1;
  const bool locked = any_lock(locks, B);
  if (locked && commit && win_check_locks(c, wins, locks, B)) return 1;
  if (!wsp) return fail(c, "null pointer argument: workspace");
  if (!aligned_to(wsp, 256)) return fail(c, "workspace must be 256-byte aligned");
  if (!aligned_to(rgb_out, 4) || !aligned_to(mask_u8_out, 4) || !aligned_to(hits_out, 4)) return fail(c, "rgb_out / mask_u8_out / hits_out must be 4-byte aligned");
  if (forward_enter(c)) return 1;
  const size_t plane = pad256((size_t)B * H * W * 4), rgbw = pad256((size_t)B * H * W * 3), mw = pad256((size_t)B * H * W),
               hw = pad256((size_t)B * 4 * sizeof(int)),
               midw = scaled ? std::max(gather_mid_bytes(B, hs, W), paste_mid_bytes(B, H, ws)) : 0, lockw = locked ? mw : 0;
  if (ws_bytes < rgbw + mw + hw + lockw + midw + 6 * plane) return fail(c, "workspace too small: %zu bytes", ws_bytes);
  unsigned char* rgb = rgb_out ? rgb_out : (unsigned char*)wsp;
  unsigned char* m8 = mask_u8_out ? mask_u8_out : (unsigned char*)wsp + rgbw;
  int* hits = hits_out ? hits_out : (int*)((char*)wsp + rgbw + mw);
  unsigned char* lock8 = locked ? (unsigned char*)wsp + rgbw + mw + hw : nullptr;
  unsigned char* mid = (unsigned char*)wsp + rgbw + mw + hw + lockw;
  char* fws = (char*)wsp + rgbw + mw + hw + lockw + midw;
  const size_t fws_bytes = ws_bytes - (rgbw + mw + hw + lockw + midw);
  float* image = (float*)(fws + fws_bytes - 4 * plane);      // where se_inference_u8io keeps them
  float* sketch = (float*)(fws + fws_bytes - plane);
  if (!aligned_to(image, 16)) return fail(c, "workspace_bytes must be a multiple of 16");
  const hipStream_t st = (hipStream_t)stream;
  if (scaled && rs_enter(c, st)) return 1;
  set_profiler(&c->prof);
  // SE_TEST_POISON: the regions in front of the forward's part that the caller left to the workspace, and the fp32 inputs
  // (`mid` is filled where it is used: gather_resize_locked, lock_gather_locked, paste_resize_locked)
  if ((!rgb_out && poison(c, rgb, rgbw, st)) || (!mask_u8_out && poison(c, m8, mw, st)) || (!hits_out && poison(c, hits, hw, st)) ||
      poison(c, lock8, lockw, st) || poison(c, image, 4 * plane, st))
    return 1;
  const se_window* d = locked ? win_put_locks(c, st, wins, locks, B) : win_put(c, st, wins, B);
  if (!d) return 1;
  if (scaled) {
    if (gather_resize_locked(c, st, d, B, hs, ws, H, W, image, sketch, mid)) return 1;
  } else {
    HIPCHK(c, launch_window_gather(d, c->lut8, image, sketch, B, H, W, st));
  }
  if (locked && lock_gather_locked(c, st, d, B, hs, ws, H, W, lock8, mid)) return 1;
  if (inference_u8_locked(c, stream, image, sketch, rgb, m8, fws, fws_bytes, B, H, W, flags, 4, lock8)) return 1;
  set_profiler(&c->prof);
  HIPCHK(c, launch_window_border(d, m8, hits, B, H, W, hs, ws, st));
  if (commit && scaled) return paste_resize_locked(c, st, d, B, hs, ws, H, W, rgb, m8, mid, locked);
  // (unscaled: m8 is 0 at a locked pixel, so the rule's second condition is implied and the paste need not read the planes)
  if (commit) HIPCHK(c, launch_window_paste(d, rgb, m8, B, H, W, st));
  return 0;
}

// the gather step alone: se_window_gather_u8 (hs x ws == H x W) and se_window_gather_resize_u8
int window_gather_locked(se_ctx* c, void* stream, const se_window* wins, int B, int hs, int ws, int H, int W, float* image_out,
                         float* sketch_out) {
  if (win_check(c, wins, B, H, W, hs, ws, sketch_out != nullptr, false)) return 1;
  if (!aligned_to(image_out, 16) || !aligned_to(sketch_out, 16)) return fail(c, "image_out / sketch_out must be 16-byte aligned");
  HIPCHK(c, hipSetDevice(c->device));
  const hipStream_t st = (hipStream_t)stream;
  const bool scaled = hs != H || ws != W;
  unsigned char* mid = nullptr;
  if (scaled) {
    if (rs_enter(c, st)) return 1;
    if (hs != H && !(mid = rs_scratch(c, gather_mid_bytes(B, hs, W)))) return 1;
  }
  set_profiler(&c->prof);
  const se_window* d = win_put(c, st, wins, B);
  if (!d) return 1;
  if (scaled) return gather_resize_locked(c, st, d, B, hs, ws, H, W, image_out, sketch_out, mid);
  HIPCHK(c, launch_window_gather(d, c->lut8, image_out, sketch_out, B, H, W, st));
  return 0;
}

// the paste step alone, for the three paste entries.  `locked`: se_window_paste_locked_u8 -- the 2 B records and the locked
// kernels whatever `locks` holds; the other two pass locks = null and never take either
int window_paste_locked(se_ctx* c, void* stream, const se_window* wins, const unsigned char* const* locks, bool locked, int B, int hs,
                        int ws, int H, int W, const unsigned char* rgb, const unsigned char* mask_u8) {
  if (win_check(c, wins, B, H, W, hs, ws, false, true)) return 1;
  if (locked && !locks) return fail(c, "null pointer argument: locks");
  if (!rgb || !mask_u8) return fail(c, "null pointer argument: rgb / mask_u8");
  if (!aligned_to(rgb, 4) || !aligned_to(mask_u8, 4)) return fail(c, "rgb / mask_u8 must be 4-byte aligned");
  if (locked && win_check_locks(c, wins, locks, B)) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  const hipStream_t st = (hipStream_t)stream;
  const bool scaled = hs != H || ws != W;
  unsigned char* mid = nullptr;
  if (scaled) {
    if (rs_enter(c, st)) return 1;
    if (ws != W && !(mid = rs_scratch(c, paste_mid_bytes(B, H, ws)))) return 1;
  }
  set_profiler(&c->prof);
  const se_window* d = locked ? win_put_locks(c, st, wins, locks, B) : win_put(c, st, wins, B);
  if (!d) return 1;
  if (scaled) return paste_resize_locked(c, st, d, B, hs, ws, H, W, rgb, mask_u8, mid, locked);
  HIPCHK(c, launch_window_paste(d, rgb, mask_u8, B, H, W, st, locked));
  return 0;
}

}  // namespace

int se_window_gather_u8(se_ctx* c, void* stream, const se_window* wins, int B, int H, int W, float* image_out, float* sketch_out) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  return window_gather_locked(c, stream, wins, B, H, W, H, W, image_out, sketch_out);
}

int se_window_border_u8(se_ctx* c, void* stream, const se_window* wins, int B, int H, int W, const unsigned char* mask_u8,
                        int* hits_out) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (win_check(c, wins, B, H, W, H, W, false, false)) return 1;
  if (!mask_u8 || !hits_out) return fail(c, "null pointer argument: mask_u8 / hits_out");
  if (!aligned_to(hits_out, 4)) return fail(c, "hits_out must be 4-byte aligned");
  HIPCHK(c, hipSetDevice(c->device));
  set_profiler(&c->prof);
  const se_window* d = win_put(c, (hipStream_t)stream, wins, B);
  if (!d) return 1;
  HIPCHK(c, launch_window_border(d, mask_u8, hits_out, B, H, W, H, W, (hipStream_t)stream));
  return 0;
}

int se_window_paste_u8(se_ctx* c, void* stream, const se_window* wins, int B, int H, int W, const unsigned char* rgb,
                       const unsigned char* mask_u8) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  return window_paste_locked(c, stream, wins, nullptr, false, B, H, W, H, W, rgb, mask_u8);
}

// the uint8 result, the uint8 mask and the border counts in front of the forward's part (used where the caller passes NULL)
size_t se_edit_window_u8_workspace_bytes(se_ctx* c, int B, int H, int W) {
  if (!c) return 0;
  const size_t fwd = se_workspace_bytes(c, B, H, W);
  if (!fwd) return 0;
  return fwd + pad256((size_t)B * H * W * 3) + pad256((size_t)B * H * W) + pad256((size_t)B * 4 * sizeof(int));
}

int se_edit_window_u8(se_ctx* c, void* stream, const se_window* wins, int B, int H, int W, unsigned char* rgb_out,
                      unsigned char* mask_u8_out, int* hits_out, int commit, void* ws, size_t ws_bytes, int flags) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  return edit_window_locked(c, stream, wins, B, H, W, H, W, rgb_out, mask_u8_out, hits_out, commit, ws, ws_bytes, flags);
}

// ---- the same at a working size ---------------------------------------------------------------
int se_window_gather_resize_u8(se_ctx* c, void* stream, const se_window* wins, int B, int hs, int ws, int H, int W, float* image_out,
                               float* sketch_out) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  return window_gather_locked(c, stream, wins, B, hs, ws, H, W, image_out, sketch_out);
}

int se_window_paste_resize_u8(se_ctx* c, void* stream, const se_window* wins, int B, int hs, int ws, int H, int W,
                              const unsigned char* rgb, const unsigned char* mask_u8) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  return window_paste_locked(c, stream, wins, nullptr, false, B, hs, ws, H, W, rgb, mask_u8);
}

size_t se_edit_window_scaled_u8_workspace_bytes(se_ctx* c, int B, int hs, int ws, int H, int W) {
  if (!c) return 0;
  const size_t base = se_edit_window_u8_workspace_bytes(c, B, H, W);
  if (!base) return 0;
  if (hs < 16 || ws < 16) {
    std::lock_guard<std::mutex> lk(c->mu);
    fail(c, "bad window hs=%d ws=%d (a window is at least 16 x 16 frame pixels)", hs, ws);
    return 0;
  }
  return base + ((hs != H || ws != W) ? std::max(gather_mid_bytes(B, hs, W), paste_mid_bytes(B, H, ws)) : 0);
}

int se_edit_window_scaled_u8(se_ctx* c, void* stream, const se_window* wins, int B, int hs, int ws, int H, int W,
                             unsigned char* rgb_out, unsigned char* mask_u8_out, int* hits_out, int commit, void* workspace,
                             size_t workspace_bytes, int flags) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  return edit_window_locked(c, stream, wins, B, hs, ws, H, W, rgb_out, mask_u8_out, hits_out, commit, workspace, workspace_bytes, flags);
}

// ---- locked regions --------------------------------------------------------------------------------
int se_window_gather_lock_u8(se_ctx* c, void* stream, const se_window* wins, const unsigned char* const* locks, int B, int hs, int ws,
                             int H, int W, unsigned char* lock_out) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (win_check(c, wins, B, H, W, hs, ws, false, false)) return 1;
  if (!locks || !lock_out) return fail(c, "null pointer argument: locks / lock_out");
  if (!aligned_to(lock_out, 8)) return fail(c, "lock_out must be 8-byte aligned");
  HIPCHK(c, hipSetDevice(c->device));
  const hipStream_t st = (hipStream_t)stream;
  unsigned char* mid = nullptr;
  if (hs != H || ws != W) {
    if (rs_enter(c, st)) return 1;
    if (hs != H && !(mid = rs_scratch(c, lock_mid_bytes(B, hs, W)))) return 1;
  }
  set_profiler(&c->prof);
  const se_window* d = win_put_locks(c, st, wins, locks, B);
  if (!d) return 1;
  return lock_gather_locked(c, st, d, B, hs, ws, H, W, lock_out, mid);
}

int se_window_paste_locked_u8(se_ctx* c, void* stream, const se_window* wins, const unsigned char* const* locks, int B, int hs, int ws,
                              int H, int W, const unsigned char* rgb, const unsigned char* mask_u8) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  return window_paste_locked(c, stream, wins, locks, true, B, hs, ws, H, W, rgb, mask_u8);
}

size_t se_edit_window_locked_u8_workspace_bytes(se_ctx* c, int B, int hs, int ws, int H, int W) {
  const size_t base = se_edit_window_scaled_u8_workspace_bytes(c, B, hs, ws, H, W);
  return base ? base + pad256((size_t)B * H * W) : 0;
}

int se_edit_window_locked_u8(se_ctx* c, void* stream, const se_window* wins, const unsigned char* const* locks, int B, int hs, int ws,
                             int H, int W, unsigned char* rgb_out, unsigned char* mask_u8_out, int* hits_out, int commit,
                             void* workspace, size_t workspace_bytes, int flags) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (!locks) return fail(c, "null pointer argument: locks");
  return edit_window_locked(c, stream, wins, B, hs, ws, H, W, rgb_out, mask_u8_out, hits_out, commit, workspace, workspace_bytes,
                            flags, locks);
}

// ---- the feathered paste (include/sketchedit_feather.h) -----------------------------------------------------
// Every check on the host, then ONE launch that reads the caller's arrays and writes the frames: no workspace, nothing for
// SE_TEST_POISON to fill.  The window's sides take any value >= 16 (no forward runs here, so win_check's multiples of 8 do not
// apply); the records, the windows' disjointness and the lock planes are checked as the locked paste checks them.
int se_window_paste_feather_u8(se_ctx* c, void* stream, const se_window* wins, const unsigned char* const* locks, int B, int hs, int ws,
                               int radius, const unsigned char* rgb, const unsigned char* mask_u8) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (B < 1 || B > 65535) return fail(c, "bad B=%d (1 .. 65535 requests per call)", B);
  if (hs < 16 || ws < 16) return fail(c, "bad window hs=%d ws=%d (a window is at least 16 x 16 frame pixels)", hs, ws);
  if (radius < 0 || radius > SE_FEATHER_MAX_RADIUS) return fail(c, "bad radius=%d (0 .. %d)", radius, SE_FEATHER_MAX_RADIUS);
  if (!wins) return fail(c, "null pointer argument: wins");
  if (!rgb || !mask_u8) return fail(c, "null pointer argument: rgb / mask_u8");
  if ((hs + 15) / 16 > 65535 || (long long)B * hs * ws / 1024 >= (1ll << 31))
    return fail(c, "window: B=%d window %dx%d is more than one launch takes", B, hs, ws);
  if (win_check_records(c, wins, B, hs, ws, false) || win_check_disjoint(c, wins, B, hs, ws)) return 1;
  const std::vector<const unsigned char*> none((size_t)B, nullptr);
  if (!locks) locks = none.data();
  if (win_check_locks(c, wins, locks, B)) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  const hipStream_t st = (hipStream_t)stream;
  set_profiler(&c->prof);
  const se_window* d = win_put_locks(c, st, wins, locks, B);
  if (!d) return 1;
  HIPCHK(c, launch_window_paste_feather(d, rgb, mask_u8, B, hs, ws, radius, st));
  return 0;
}

// ---- fills of a painted region (include/sketchedit_fill.h) ------------------------------------------------
// netG alone on a hole the caller gives: hole = fill & ~lock is mask, mask2 AND the composite's soft mask of plan_netG.
namespace {

// the passes of a netG-only forward (as se_netG_forward_taps plans them): `hole` (B,H,W) fp32 is read as hard and as soft
// mask; `tail` bytes at the end of the workspace are the caller's.  rgb8 / m8 (either may be null): the fused uint8 outputs.
int fill_passes(se_ctx* c, void* stream, const float* image, const float* sketch, const float* hole, float* composed_out,
                float* coarse_out, float* fine_out, unsigned char* rgb8, unsigned char* m8, void* ws, size_t ws_bytes, size_t tail, int B,
                int H, int W, int flags) {
  const int nb = pass_size(c, B, H, W, flags);
  if (!nb) return 1;
  const size_t HW = (size_t)H * W;
  for (int b0 = 0; b0 < B; b0 += nb) {
    const int bb = std::min(nb, B - b0);
    if (carve(c, plan_peaks(c, 2, bb, H, W, flags, false), ws, ws_bytes, tail)) return 1;
    begin_call(c, stream, flags);
    c->rgb8 = rgb8 ? rgb8 + b0 * 3 * HW : nullptr; c->m8 = m8 ? m8 + b0 * HW : nullptr;
    const float *img = image + b0 * 3 * HW, *h = hole + b0 * HW;
    const int rc = plan_netG(c, img, img, h, h, sketch + b0 * HW, coarse_out ? coarse_out + b0 * 3 * HW : nullptr,
                             fine_out ? fine_out + b0 * 3 * HW : nullptr, h, composed_out ? composed_out + b0 * 3 * HW : nullptr, bb, H, W,
                             flags);
    if (rc) return rc;
  }
  return 0;
}

// holes: every entry given
int fill_check_holes(se_ctx* c, const unsigned char* const* holes, int B) {
  if (!holes) return fail(c, "null pointer argument: holes");
  for (int i = 0; i < B; ++i)
    if (!holes[i]) return fail(c, "holes[%d] is null", i);
  return 0;
}

}  // namespace

int se_fill(se_ctx* c, void* stream, const float* image, const float* sketch, const unsigned char* hole_u8, const unsigned char* lock_u8,
            float* composed_out, float* coarse_out, float* fine_out, float* hard_out, void* ws, size_t ws_bytes, int B, int H, int W,
            int flags) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (check_dims(c, B, H, W)) return 1;
  if (!image) return fail(c, "null pointer argument: image");
  if (!hole_u8) return fail(c, "null pointer argument: hole_u8");
  if (!composed_out) return fail(c, "null pointer argument: composed_out");
  if (!ws) return fail(c, "null pointer argument: workspace");
  if (!aligned_to(hole_u8, 16) || !aligned_to(lock_u8, 16) || !aligned_to(hard_out, 16)) return fail(c, "hole_u8 / lock_u8 / hard_out must be 16-byte aligned");
  if (!aligned_to(ws, 256) || (ws_bytes & 15)) return fail(c, "workspace must be 256-byte aligned and workspace_bytes a multiple of 16");
  if (forward_enter(c)) return 1;
  flags &= ~(SE_FLAG_GRAPH | SE_FLAG_PACKED_OUT);
  // the hole plane and the zero sketch of a call without one live at the end of the workspace for the whole call
  const size_t plane = pad256((size_t)B * H * W * 4), tail = 2 * plane;
  if (ws_bytes < tail) return fail(c, "workspace too small: %zu bytes", ws_bytes);
  float* hole = (float*)((char*)ws + ws_bytes - tail);
  float* zero = sketch ? nullptr : (float*)((char*)ws + ws_bytes - plane);
  const hipStream_t st = (hipStream_t)stream;
  set_profiler(&c->prof);
  if (poison(c, hole, tail, st)) return 1;
  HIPCHK(c, launch_fill_masks(hole_u8, lock_u8, hole, hard_out, zero, B, H, W, st));
  return fill_passes(c, stream, image, sketch ? sketch : zero, hole, composed_out, coarse_out, fine_out, nullptr, nullptr, ws, ws_bytes, tail,
                     B, H, W, flags);
}

// [uint8 result | uint8 mask | working-size fill plane | working-size lock plane (a call with a lock only) | a zero (hs,ws) sketch (a
// call with a request without one only) | intermediates of the resample end (scaled only) | the forward's part: the arenas, then
// the fp32 hole plane, then the fp32 image (3 planes) and sketch -- where se_inference_u8io keeps them]
size_t se_fill_window_u8_workspace_bytes(se_ctx* c, int B, int hs, int ws, int H, int W) {
  const size_t base = se_edit_window_locked_u8_workspace_bytes(c, B, hs, ws, H, W);      // (its lock plane and its counts included)
  return base ? base + pad256((size_t)B * H * W) + pad256((size_t)hs * ws) : 0;
}

int se_fill_window_u8(se_ctx* c, void* stream, const se_window* wins, const unsigned char* const* holes, const unsigned char* const* locks,
                      int B, int hs, int ws, int H, int W, unsigned char* rgb_out, unsigned char* mask_u8_out, void* wsp, size_t ws_bytes,
                      int flags) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  const bool scaled = hs != H || ws != W;
  if (win_check(c, wins, B, H, W, hs, ws, false, false)) return 1;
  if (fill_check_holes(c, holes, B)) return 1;
  if (!wsp) return fail(c, "null pointer argument: workspace");
  if (!aligned_to(wsp, 256)) return fail(c, "workspace must be 256-byte aligned");
  if (!aligned_to(rgb_out, 4) || !aligned_to(mask_u8_out, 4)) return fail(c, "rgb_out / mask_u8_out must be 4-byte aligned");
  if (ws_bytes & 15) return fail(c, "workspace_bytes must be a multiple of 16");
  const bool locked = any_lock(locks, B);
  bool bare = false;                                      // a request without a sketch
  for (int i = 0; i < B; ++i) bare = bare || !wins[i].sketch_u8;
  if (forward_enter(c)) return 1;
  flags &= ~(SE_FLAG_GRAPH | SE_FLAG_PACKED_OUT);
  const size_t plane = pad256((size_t)B * H * W * 4), rgbw = pad256((size_t)B * H * W * 3), mw = pad256((size_t)B * H * W),
               zw = bare ? pad256((size_t)hs * ws) : 0, midw = scaled ? gather_mid_bytes(B, hs, W) : 0, lockw = locked ? mw : 0;
  const size_t head = rgbw + mw + mw + lockw + zw + midw, tail = 5 * plane;
  if (ws_bytes < head + tail) return fail(c, "workspace too small: %zu bytes", ws_bytes);
  unsigned char* rgb = rgb_out ? rgb_out : (unsigned char*)wsp;
  unsigned char* m8 = mask_u8_out ? mask_u8_out : (unsigned char*)wsp + rgbw;
  unsigned char* fill8 = (unsigned char*)wsp + rgbw + mw;
  unsigned char* lock8 = locked ? fill8 + mw : nullptr;
  unsigned char* zsk = bare ? fill8 + mw + lockw : nullptr;
  unsigned char* mid = fill8 + mw + lockw + zw;
  char* fws = (char*)wsp + head;
  const size_t fws_bytes = ws_bytes - head;
  float* hole = (float*)(fws + fws_bytes - tail);
  float* image = (float*)(fws + fws_bytes - 4 * plane);
  float* sketch = (float*)(fws + fws_bytes - plane);
  const hipStream_t st = (hipStream_t)stream;
  if (scaled && rs_enter(c, st)) return 1;
  set_profiler(&c->prof);
  if ((!rgb_out && poison(c, rgb, rgbw, st)) || (!mask_u8_out && poison(c, m8, mw, st)) || poison(c, fill8, mw + lockw, st) ||
      poison(c, hole, tail, st))
    return 1;
  // a request without a sketch reads the zero plane: the gathers at either scale then give it an all-zero sketch
  if (bare) HIPCHK(c, hipMemsetAsync(zsk, 0, (size_t)hs * ws, st));
  std::vector<se_window> recs(wins, wins + B);
  for (se_window& w : recs)
    if (!w.sketch_u8) w.sketch_u8 = zsk;
  // one group of records per plane: the requests, then the plane's pointers (the gathers of 6g take them so)
  const se_window* d = win_put_locks(c, st, recs.data(), holes, B);
  if (!d) return 1;
  if (scaled) {
    if (gather_resize_locked(c, st, d, B, hs, ws, H, W, image, sketch, mid)) return 1;
  } else {
    HIPCHK(c, launch_window_gather(d, c->lut8, image, sketch, B, H, W, st));
  }
  if (lock_gather_locked(c, st, d, B, hs, ws, H, W, fill8, mid)) return 1;
  if (locked) {
    const se_window* dl = win_put_locks(c, st, recs.data(), locks, B);
    if (!dl) return 1;
    if (lock_gather_locked(c, st, dl, B, hs, ws, H, W, lock8, mid)) return 1;
  }
  HIPCHK(c, launch_fill_masks(fill8, lock8, hole, nullptr, nullptr, B, H, W, st));
  return fill_passes(c, stream, image, sketch, hole, nullptr, nullptr, nullptr, rgb, m8, fws, fws_bytes, tail, B, H, W, flags);
}

int se_fill_keep_u8(se_ctx* c, void* stream, const se_window* wins, const unsigned char* const* holes, const unsigned char* const* locks,
                    unsigned char* const* keeps, int B, int hs, int ws) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (B < 1 || B > 16383) return fail(c, "bad B=%d (1 .. 16383 requests per call)", B);
  if (hs < 16 || ws < 16) return fail(c, "bad window hs=%d ws=%d (a window is at least 16 x 16 frame pixels)", hs, ws);
  if (!wins) return fail(c, "null pointer argument: wins");
  if ((long long)B * hs * ws / 1024 >= (1ll << 31)) return fail(c, "window: B=%d window %dx%d is more than one launch takes", B, hs, ws);
  if (win_check_records(c, wins, B, hs, ws, false)) return 1;
  if (fill_check_holes(c, holes, B)) return 1;
  if (!keeps) return fail(c, "null pointer argument: keeps");
  for (int i = 0; i < B; ++i)
    if (!keeps[i]) return fail(c, "keeps[%d] is null", i);
  auto meets = [](uintptr_t a0, size_t an, uintptr_t b0, size_t bn) { return a0 < b0 + bn && b0 < a0 + an; };
  for (int i = 0; i < B; ++i) {
    const uintptr_t k0 = (uintptr_t)keeps[i];
    const size_t kn = (size_t)wins[i].Hi * wins[i].Wi;
    for (int j = 0; j < B; ++j) {
      const size_t pn = (size_t)wins[j].Hi * wins[j].Wi;
      if (meets(k0, kn, (uintptr_t)wins[j].frame_u8, 3 * pn)) return fail(c, "keeps[%d] overlaps the frame of wins[%d]", i, j);
      if (meets(k0, kn, (uintptr_t)holes[j], pn)) return fail(c, "keeps[%d] overlaps holes[%d]", i, j);
      if (locks && locks[j] && meets(k0, kn, (uintptr_t)locks[j], pn)) return fail(c, "keeps[%d] overlaps locks[%d]", i, j);
      if (j <= i || !meets(k0, kn, (uintptr_t)keeps[j], pn)) continue;
      // two requests of one keep plane: the same plane, rectangles apart
      const se_window &a = wins[i], &b = wins[j];
      if (keeps[i] != keeps[j] || a.Hi != b.Hi || a.Wi != b.Wi)
        return fail(c, "keeps[%d] and keeps[%d] overlap in memory without being the same plane", i, j);
      if (a.y0 < b.y0 + hs && b.y0 < a.y0 + hs && a.x0 < b.x0 + ws && b.x0 < a.x0 + ws)
        return fail(c, "keeps[%d] and keeps[%d]: overlapping rectangles of one keep plane", i, j);
    }
  }
  HIPCHK(c, hipSetDevice(c->device));
  const hipStream_t st = (hipStream_t)stream;
  set_profiler(&c->prof);
  std::vector<se_window> recs(wins, wins + B);
  for (int k = 0; k < 3; ++k)
    for (int i = 0; i < B; ++i)
      recs.push_back(se_window{k == 0 ? const_cast<unsigned char*>(holes[i]) : k == 1 ? (locks ? const_cast<unsigned char*>(locks[i]) : nullptr) : keeps[i],
                               nullptr, 0, 0, 0, 0});
  const se_window* d = win_put(c, st, recs.data(), 4 * B);
  if (!d) return 1;
  HIPCHK(c, launch_fill_keep(d, B, hs, ws, st));
  return 0;
}

// ---- selection by colour (include/sketchedit_select.h) ------------------------------------------------------
// Every check on the host, then launches that write the caller's planes directly: no workspace, nothing for SE_TEST_POISON to
// fill.
namespace {

int select_check_plane(se_ctx* c, int Hi, int Wi) {
  if (Hi < 16 || Wi < 16) return fail(c, "bad Hi=%d Wi=%d (a state plane is at least 16 x 16)", Hi, Wi);
  // the largest grid of the three kernels: the grow's 64 x 16 tiles
  if ((long long)Hi * Wi > (1ll << 40) || (long long)((Hi + 15) / 16) * ((Wi + 63) / 64) >= (1ll << 31))
    return fail(c, "select: Hi=%d Wi=%d is more than one launch takes", Hi, Wi);
  return 0;
}

bool select_meets(const void* a, size_t an, const void* b, size_t bn) {
  return (uintptr_t)a < (uintptr_t)b + bn && (uintptr_t)b < (uintptr_t)a + an;
}

}  // namespace

int se_select_similar_u8(se_ctx* c, void* stream, const unsigned char* frame_u8, int Hi, int Wi, int seed_y, int seed_x, int tolerance,
                         int contiguous, unsigned char* state_u8) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (select_check_plane(c, Hi, Wi)) return 1;
  if (!frame_u8) return fail(c, "null pointer argument: frame_u8");
  if (!state_u8) return fail(c, "null pointer argument: state_u8");
  if (seed_y < 0 || seed_y >= Hi || seed_x < 0 || seed_x >= Wi)
    return fail(c, "seed_y=%d seed_x=%d: the seed lies outside the frame (Hi=%d Wi=%d)", seed_y, seed_x, Hi, Wi);
  if (tolerance < 0 || tolerance > 255) return fail(c, "bad tolerance=%d (0 .. 255)", tolerance);
  const size_t n = (size_t)Hi * Wi;
  if (select_meets(state_u8, n, frame_u8, 3 * n)) return fail(c, "state_u8 overlaps frame_u8");
  HIPCHK(c, hipSetDevice(c->device));
  set_profiler(&c->prof);
  HIPCHK(c, launch_select_similar(frame_u8, Hi, Wi, seed_y, seed_x, tolerance, contiguous ? 1 : 0, state_u8, (hipStream_t)stream));
  return 0;
}

int se_select_flood_u8(se_ctx* c, void* stream, unsigned char* state_u8, int Hi, int Wi, int passes, unsigned* changed_out) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (select_check_plane(c, Hi, Wi)) return 1;
  if (!state_u8) return fail(c, "null pointer argument: state_u8");
  if (!changed_out) return fail(c, "null pointer argument: changed_out");
  if (passes < 1 || passes > SE_SELECT_MAX_PASSES) return fail(c, "bad passes=%d (1 .. %d)", passes, SE_SELECT_MAX_PASSES);
  if (!aligned_to(changed_out, 4)) return fail(c, "changed_out must be 4-byte aligned");
  if (select_meets(changed_out, (size_t)passes * sizeof(unsigned), state_u8, (size_t)Hi * Wi)) return fail(c, "changed_out overlaps state_u8");
  HIPCHK(c, hipSetDevice(c->device));
  const hipStream_t st = (hipStream_t)stream;
  set_profiler(&c->prof);
  HIPCHK(c, hipMemsetAsync(changed_out, 0, (size_t)passes * sizeof(unsigned), st));
  for (int p = 0; p < passes; ++p) HIPCHK(c, launch_select_flood(state_u8, Hi, Wi, changed_out + p, st));
  return 0;
}

int se_select_grow_u8(se_ctx* c, void* stream, const unsigned char* state_u8, int Hi, int Wi, int grow, unsigned char* plane_out) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (select_check_plane(c, Hi, Wi)) return 1;
  if (!state_u8) return fail(c, "null pointer argument: state_u8");
  if (!plane_out) return fail(c, "null pointer argument: plane_out");
  if (grow < 0 || grow > SE_SELECT_MAX_GROW) return fail(c, "bad grow=%d (0 .. %d)", grow, SE_SELECT_MAX_GROW);
  const size_t n = (size_t)Hi * Wi;
  if (select_meets(plane_out, n, state_u8, n)) return fail(c, "plane_out overlaps state_u8");
  HIPCHK(c, hipSetDevice(c->device));
  set_profiler(&c->prof);
  HIPCHK(c, launch_select_grow(state_u8, Hi, Wi, grow, plane_out, (hipStream_t)stream));
  return 0;
}

// ---- lasso selections and their algebra (include/sketchedit_lasso.h) ---------------------------------------
// Every check on the host, then ONE launch that writes the caller's plane directly: no workspace, nothing for SE_TEST_POISON to
// fill.
namespace {

int lasso_check_plane(se_ctx* c, int Hi, int Wi) {
  if (Hi < 16 || Wi < 16 || Hi > SE_LASSO_MAX_EXTENT || Wi > SE_LASSO_MAX_EXTENT)
    return fail(c, "bad Hi=%d Wi=%d (a selection's plane is 16 .. %d on a side)", Hi, Wi, SE_LASSO_MAX_EXTENT);
  return 0;
}

}  // namespace

int se_lasso_fill_u8(se_ctx* c, void* stream, const int* edges, int N, int Hi, int Wi, unsigned char* plane_out) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (lasso_check_plane(c, Hi, Wi)) return 1;
  if (N < 0 || N > SE_LASSO_MAX_EDGES) return fail(c, "bad N=%d (0 .. %d edges)", N, SE_LASSO_MAX_EDGES);
  if (!plane_out) return fail(c, "null pointer argument: plane_out");
  if (!edges && N > 0) return fail(c, "null pointer argument: edges");
  if (edges && !aligned_to(edges, 4)) return fail(c, "edges must be 4-byte aligned");
  if (edges && N > 0 && select_meets(edges, (size_t)N * 4 * sizeof(int), plane_out, (size_t)Hi * Wi)) return fail(c, "edges overlaps plane_out");
  HIPCHK(c, hipSetDevice(c->device));
  set_profiler(&c->prof);
  HIPCHK(c, launch_lasso_fill(edges, N, Hi, Wi, plane_out, (hipStream_t)stream));
  return 0;
}

int se_plane_combine_u8(se_ctx* c, void* stream, const unsigned char* a, const unsigned char* b, int Hi, int Wi, int op, unsigned char* out) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (lasso_check_plane(c, Hi, Wi)) return 1;
  if (op < SE_COMBINE_ADD || op > SE_COMBINE_INVERT) return fail(c, "bad op=%d (0 .. 4)", op);
  if (!a) return fail(c, "null pointer argument: a");
  if (!out) return fail(c, "null pointer argument: out");
  if (op == SE_COMBINE_INVERT && b) return fail(c, "b must be NULL for SE_COMBINE_INVERT");
  if (op != SE_COMBINE_INVERT && !b) return fail(c, "null pointer argument: b");
  const size_t n = (size_t)Hi * Wi;
  if (out != a && select_meets(out, n, a, n)) return fail(c, "out overlaps a (it may be a itself)");
  if (b && out != b && select_meets(out, n, b, n)) return fail(c, "out overlaps b (it may be b itself)");
  HIPCHK(c, hipSetDevice(c->device));
  set_profiler(&c->prof);
  HIPCHK(c, launch_plane_combine(a, b, Hi, Wi, op, out, (hipStream_t)stream));
  return 0;
}

// ---- the outline of a selection (include/sketchedit_outline.h) ---------------------------------------------
// Every check on the host, then three launches (two when cap == 0: nothing to emit).  The workspace is one block, the tiles' run
// counts: SE_TEST_POISON fills it on the stream before the count kernel, which writes every word of it, is enqueued.
namespace {

size_t outline_ws_bytes(int Hi, int Wi) {
  return pad256((size_t)((Hi + SE_OUTLINE_TILE - 1) / SE_OUTLINE_TILE) * ((Wi + SE_OUTLINE_TILE - 1) / SE_OUTLINE_TILE) * 4 * sizeof(int));
}

}  // namespace

size_t se_outline_u8_workspace_bytes(se_ctx* c, int Hi, int Wi) {
  if (!c) return 0;
  std::lock_guard<std::mutex> lk(c->mu);
  if (lasso_check_plane(c, Hi, Wi)) return 0;
  return outline_ws_bytes(Hi, Wi);
}

int se_outline_u8(se_ctx* c, void* stream, const unsigned char* plane, int Hi, int Wi, int* edges_out, int cap, int* info_out,
                  void* workspace, size_t workspace_bytes) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (lasso_check_plane(c, Hi, Wi)) return 1;
  if (cap < 0 || cap > SE_OUTLINE_MAX_CAP) return fail(c, "bad cap=%d (0 .. %d records)", cap, SE_OUTLINE_MAX_CAP);
  if (!plane) return fail(c, "null pointer argument: plane");
  if (!edges_out && cap > 0) return fail(c, "null pointer argument: edges_out");
  if (!info_out) return fail(c, "null pointer argument: info_out");
  if (!workspace) return fail(c, "null pointer argument: workspace");
  if (edges_out && !aligned_to(edges_out, 4)) return fail(c, "edges_out must be 4-byte aligned");
  if (!aligned_to(info_out, 4)) return fail(c, "info_out must be 4-byte aligned");
  const size_t need = outline_ws_bytes(Hi, Wi);
  if (workspace_bytes < need) return fail(c, "workspace too small: %zu bytes, need %zu", workspace_bytes, need);
  if (!aligned_to(workspace, 256)) return fail(c, "workspace must be 256-byte aligned");
  const size_t pn = (size_t)Hi * Wi, en = edges_out ? (size_t)cap * 4 * sizeof(int) : 0, in = 2 * sizeof(int);
  if (en && select_meets(edges_out, en, plane, pn)) return fail(c, "edges_out overlaps plane");
  if (select_meets(info_out, in, plane, pn)) return fail(c, "info_out overlaps plane");
  if (select_meets(workspace, need, plane, pn)) return fail(c, "workspace overlaps plane");
  if (en && select_meets(edges_out, en, info_out, in)) return fail(c, "edges_out overlaps info_out");
  if (en && select_meets(edges_out, en, workspace, need)) return fail(c, "edges_out overlaps the workspace");
  if (select_meets(info_out, in, workspace, need)) return fail(c, "info_out overlaps the workspace");
  HIPCHK(c, hipSetDevice(c->device));
  set_profiler(&c->prof);
  const hipStream_t st = (hipStream_t)stream;
  if (poison(c, workspace, need, st)) return 1;
  int* cnt = (int*)workspace;
  HIPCHK(c, launch_outline_count(plane, Hi, Wi, cnt, st));
  HIPCHK(c, launch_outline_scan(cnt, Hi, Wi, cap, info_out, st));
  if (cap > 0) HIPCHK(c, launch_outline_emit(plane, Hi, Wi, cnt, edges_out, cap, st));
  return 0;
}

// ---- the undo journal of a session ---------------------------------------------------------------
size_t se_window_saved_bytes(int hs, int ws) {
  if (hs < 16 || ws < 16) return 0;
  return (size_t)hs * (((size_t)3 * ws + 15) & ~(size_t)15);
}

namespace {

// save (the windows -> their slots) or swap (windows <-> slots): every check on the host, then ONE launch.  The slot pointers
// travel with the records: 2 B consecutive entries of the ctx's ring (win_put takes them as one group), the second B carrying
// a slot in frame_u8.
int window_journal_call(se_ctx* c, void* stream, const se_window* wins, int B, int hs, int ws, unsigned char* const* slots, bool swap) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (B < 1) return fail(c, "bad B=%d", B);
  if (hs < 16 || ws < 16) return fail(c, "bad window hs=%d ws=%d (a window is at least 16 x 16 frame pixels)", hs, ws);
  if (!wins) return fail(c, "null pointer argument: wins");
  if (!slots) return fail(c, "null pointer argument: slots");
  if (B > 32767 || (long long)B * hs * ws / 1024 >= (1ll << 31))
    return fail(c, "window: B=%d (window %dx%d) is more than one launch takes", B, hs, ws);
  if (win_check_records(c, wins, B, hs, ws, false)) return 1;
  const size_t bytes = se_window_saved_bytes(hs, ws);
  for (int i = 0; i < B; ++i) {
    if (!slots[i]) return fail(c, "slots[%d] is null", i);
    if (!aligned_to(slots[i], 16)) return fail(c, "slots[%d] must be 16-byte aligned", i);
    const uintptr_t s0 = (uintptr_t)slots[i], s1 = s0 + bytes;
    for (int j = 0; j < B; ++j) {
      const uintptr_t f0 = (uintptr_t)wins[j].frame_u8, f1 = f0 + (size_t)wins[j].Hi * wins[j].Wi * 3;
      if (s0 < f1 && f0 < s1) return fail(c, "slots[%d] overlaps the frame of wins[%d]", i, j);
      const uintptr_t t0 = (uintptr_t)slots[j];
      if (j > i && s0 < t0 + bytes && t0 < s1) return fail(c, "slots[%d] and slots[%d] overlap", i, j);
    }
  }
  if (swap && win_check_disjoint(c, wins, B, hs, ws)) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  set_profiler(&c->prof);
  std::vector<se_window> recs(wins, wins + B);
  for (int i = 0; i < B; ++i) recs.push_back(se_window{slots[i], nullptr, 0, 0, 0, 0});
  const se_window* d = win_put(c, (hipStream_t)stream, recs.data(), 2 * B);
  if (!d) return 1;
  HIPCHK(c, launch_window_journal(d, B, hs, ws, swap, (hipStream_t)stream));
  return 0;
}

}  // namespace

int se_window_save_u8(se_ctx* c, void* stream, const se_window* wins, int B, int hs, int ws, unsigned char* const* slots) {
  return window_journal_call(c, stream, wins, B, hs, ws, slots, false);
}

int se_window_swap_u8(se_ctx* c, void* stream, const se_window* wins, int B, int hs, int ws, unsigned char* const* slots) {
  return window_journal_call(c, stream, wins, B, hs, ws, slots, true);
}

// ---- region edits: where a full-size sketch is drawn, per tile ----------------------------------------
// Every check on the host, then ONE launch that writes the caller's records directly: no workspace, nothing for SE_TEST_POISON
// to fill.
int se_sketch_tiles_u8(se_ctx* c, void* stream, const unsigned char* sketch_u8, int Hi, int Wi, int tile, int* tiles_out) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (Hi < 16 || Wi < 16) return fail(c, "bad Hi=%d Wi=%d (a sketch plane is at least 16 x 16)", Hi, Wi);
  if (tile != 16 && tile != 32 && tile != 64) return fail(c, "bad tile=%d (16, 32 or 64)", tile);
  if (!sketch_u8 || !tiles_out) return fail(c, "null pointer argument: sketch_u8 / tiles_out");
  if (!aligned_to(tiles_out, 4)) return fail(c, "tiles_out must be 4-byte aligned");
  if ((long long)((Hi + tile - 1) / tile) * ((Wi + tile - 1) / tile) > (1ll << 30))
    return fail(c, "sketch tiles: Hi=%d Wi=%d at tile=%d is more than one launch takes", Hi, Wi, tile);
  HIPCHK(c, hipSetDevice(c->device));
  set_profiler(&c->prof);
  HIPCHK(c, launch_sketch_tiles(sketch_u8, Hi, Wi, tile, tiles_out, (hipStream_t)stream));
  return 0;
}

// ---- strokes as polylines: the windows' sketches rasterised from segments ----------------------------
// Every check on the host, then the records (with the ranges behind them, as the journal's slots travel) and ONE launch that
// writes the caller's sketches directly: no workspace, nothing for SE_TEST_POISON to fill.
int se_sketch_strokes_u8(se_ctx* c, void* stream, const se_window* wins, int B, int hs, int ws, const int* segs, int N, const int* ranges,
                         unsigned char* sketch_out) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (B < 1 || B > 32767) return fail(c, "bad B=%d (1 .. 32767 requests per call)", B);
  if (hs < 16 || ws < 16) return fail(c, "bad window hs=%d ws=%d (a window is at least 16 x 16 frame pixels)", hs, ws);
  if (N < 0) return fail(c, "bad N=%d", N);
  if (!wins || !segs || !ranges || !sketch_out) return fail(c, "null pointer argument: wins / segs / ranges / sketch_out");
  if (!aligned_to(segs, 4)) return fail(c, "segs must be 4-byte aligned");
  std::vector<se_window> recs(2 * (size_t)B, se_window{nullptr, nullptr, 0, 0, 0, 0});
  long nseg_sum = 0;
  for (int i = 0; i < B; ++i) {
    const se_window& w = wins[i];
    if (w.Hi < 1 || w.Wi < 1 || w.Hi > 8192 || w.Wi > 8192)
      return fail(c, "wins[%d]: bad frame size Hi=%d Wi=%d (1 .. 8192: the range the rule's 64-bit arithmetic is stated for)", i, w.Hi, w.Wi);
    if (w.y0 < 0 || (long long)w.y0 + hs > w.Hi)
      return fail(c, "wins[%d].y0=%d: rows [%d, %lld) of the window lie outside the frame (Hi=%d)", i, w.y0, w.y0, (long long)w.y0 + hs, w.Hi);
    if (w.x0 < 0 || (long long)w.x0 + ws > w.Wi)
      return fail(c, "wins[%d].x0=%d: columns [%d, %lld) of the window lie outside the frame (Wi=%d)", i, w.x0, w.x0, (long long)w.x0 + ws, w.Wi);
    const int first = ranges[2 * i], count = ranges[2 * i + 1];
    if (first < 0 || count < 0 || (long long)first + count > N)
      return fail(c, "ranges[%d] = [first %d, count %d] lies outside the %d segments", i, first, count, N);
    recs[i].Hi = w.Hi; recs[i].Wi = w.Wi; recs[i].y0 = w.y0; recs[i].x0 = w.x0;
    recs[B + i].Hi = first; recs[B + i].Wi = count;
    nseg_sum += count;
  }
  const uintptr_t s0 = (uintptr_t)segs, s1 = s0 + (size_t)N * 5 * sizeof(int), o0 = (uintptr_t)sketch_out, o1 = o0 + (size_t)B * hs * ws;
  if (s0 < o1 && o0 < s1) return fail(c, "segs overlaps sketch_out");
  HIPCHK(c, hipSetDevice(c->device));
  set_profiler(&c->prof);
  const hipStream_t st = (hipStream_t)stream;
  const se_window* d = win_put(c, st, recs.data(), 2 * B);
  if (!d) return 1;
  HIPCHK(c, launch_sketch_strokes(d, B, hs, ws, segs, nseg_sum, sketch_out, st));
  return 0;
}

// ---- the device PNG encoder (include/sketchedit_png.h): a window of a frame -> the zlib stream of its PNG --
// Every check on the host, then the records and three launches.  The workspace is handed out by the main arena, block by block,
// as a forward's activations are: SE_TEST_POISON fills each block on the stream before its producer is enqueued.
size_t se_png_bound(int hs, int ws) {
  if (hs < 16 || ws < 16 || hs > 8192 || ws > 8192) return 0;
  const size_t row = 1 + 3 * (size_t)ws;
  const int full = hs / 32, rest = hs % 32;
  return 2 + (size_t)full * png_stripe_bound(32 * row) + (rest ? png_stripe_bound((size_t)rest * row) : 0) + 9;
}

namespace {

struct PngLayout { size_t ftype, sizes, parts, slots; };      // bytes of the four blocks, each a multiple of 256
PngLayout png_layout(int B, int hs, int ws) {
  const size_t q = (size_t)B * png_stripes(hs);
  return PngLayout{pad256((size_t)B * hs), pad256(q * 4), pad256(q * 8), pad256(q * png_slot_bytes(ws))};
}

}  // namespace

size_t se_png_encode_u8_workspace_bytes(se_ctx* c, int B, int hs, int ws) {
  if (!c) return 0;
  std::lock_guard<std::mutex> lk(c->mu);
  if (B < 1 || B > 65535) { fail(c, "bad B=%d (1 .. 65535 images per call)", B); return 0; }
  if (hs < 16 || ws < 16 || hs > 8192 || ws > 8192) { fail(c, "bad rectangle hs=%d ws=%d (sides are 16 .. 8192)", hs, ws); return 0; }
  const PngLayout L = png_layout(B, hs, ws);
  return L.ftype + L.sizes + L.parts + L.slots;
}

int se_png_encode_u8(se_ctx* c, void* stream, const se_window* wins, int B, int hs, int ws, unsigned char* out, size_t cap,
                     unsigned long long* sizes_out, void* workspace, size_t workspace_bytes) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (B < 1 || B > 65535) return fail(c, "bad B=%d (1 .. 65535 images per call)", B);
  if (hs < 16 || ws < 16 || hs > 8192 || ws > 8192) return fail(c, "bad rectangle hs=%d ws=%d (sides are 16 .. 8192)", hs, ws);
  if (!wins) return fail(c, "null pointer argument: wins");
  if (!out) return fail(c, "null pointer argument: out");
  if (!sizes_out) return fail(c, "null pointer argument: sizes_out");
  if (!workspace) return fail(c, "null pointer argument: workspace");
  if (win_check_records(c, wins, B, hs, ws, false)) return 1;
  const size_t bound = se_png_bound(hs, ws);
  if (cap < bound) return fail(c, "cap=%zu is less than se_png_bound(%d, %d) = %zu", cap, hs, ws, bound);
  if (cap > ((size_t)1 << 40) / (size_t)B) return fail(c, "cap=%zu: B cap is more than one call takes", cap);
  const PngLayout L = png_layout(B, hs, ws);
  const size_t need = L.ftype + L.sizes + L.parts + L.slots;
  if (workspace_bytes < need) return fail(c, "workspace too small: %zu bytes, need %zu", workspace_bytes, need);
  if (!aligned_to(workspace, 256)) return fail(c, "workspace must be 256-byte aligned");
  if (!aligned_to(sizes_out, 8)) return fail(c, "sizes_out must be 8-byte aligned");
  const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (size_t)B * cap, w0 = (uintptr_t)workspace, w1 = w0 + need;
  const uintptr_t z0 = (uintptr_t)sizes_out, z1 = z0 + (size_t)B * sizeof(unsigned long long);
  for (int i = 0; i < B; ++i) {
    const uintptr_t f0 = (uintptr_t)wins[i].frame_u8, f1 = f0 + (size_t)wins[i].Hi * wins[i].Wi * 3;
    if (o0 < f1 && f0 < o1) return fail(c, "out overlaps the frame of wins[%d]", i);
    if (z0 < f1 && f0 < z1) return fail(c, "sizes_out overlaps the frame of wins[%d]", i);
    if (w0 < f1 && f0 < w1) return fail(c, "workspace overlaps the frame of wins[%d]", i);
  }
  if (o0 < w1 && w0 < o1) return fail(c, "out overlaps the workspace");
  if (o0 < z1 && z0 < o1) return fail(c, "out overlaps sizes_out");
  if (z0 < w1 && w0 < z1) return fail(c, "sizes_out overlaps the workspace");
  HIPCHK(c, hipSetDevice(c->device));
  set_profiler(&c->prof);
  const hipStream_t st = (hipStream_t)stream;
  c->arena.reset((char*)workspace, need, false);
  c->arena2.reset(nullptr, 0, false);
  void* blk[4];
  const size_t bytes[4] = {L.ftype, L.sizes, L.parts, L.slots};
  for (int i = 0; i < 4; ++i) {
    blk[i] = c->arena.alloc(bytes[i] / 4);
    if (!blk[i]) return fail(c, "workspace arena exhausted");
    if (poison(c, blk[i], bytes[i], st)) return 1;
  }
  const se_window* d = win_put(c, st, wins, B);
  if (!d) return 1;
  HIPCHK(c, launch_png_rows(d, B, hs, ws, (unsigned char*)blk[0], st));
  HIPCHK(c, launch_png_stripes(d, B, hs, ws, (const unsigned char*)blk[0], (unsigned*)blk[1], (unsigned*)blk[2], (unsigned char*)blk[3], st));
  HIPCHK(c, launch_png_finish(B, hs, ws, (const unsigned*)blk[1], (const unsigned*)blk[2], (const unsigned char*)blk[3], out, cap, sizes_out, st));
  return 0;
}

// ---- the device JPEG encoder (DESIGN.md sections 6k and 6l, include/sketchedit_jpg.h and sketchedit_jpg2.h): a window of a frame
// -> the entropy-coded segment.  As the PNG encoder above: every check on the host, then the records and the launches; the
// workspace's blocks come from the main arena, so SE_TEST_POISON fills each on the stream before its producer is enqueued.
// se_jpg_encode_u8 is se_jpg2_encode_u8 without flags: three launches (blocks, rows, finish).  se_jpg2_code_i16 shares the stages
// behind the DCT (jpg2_code): with SE_JPG_OPTIMIZE the histogram and the tables in front of the rows, five launches from pixels.
size_t se_jpg_bound(int hs, int ws) { return se_jpg2_bound(hs, ws, 0); }

size_t se_jpg2_bound(int hs, int ws, int flags) {
  if (hs < 16 || ws < 16 || hs > 8192 || ws > 8192 || flags < 0 || flags > 3) return 0;
  return (size_t)jpg_rows(hs, flags) * jpg_row_bound(jpg_row_blocks(ws, flags), flags);
}

namespace {

struct Jpg2Layout { size_t coef, sizes, slots, hist, codes; };             // bytes of the blocks, each a multiple of 256 (or 0: no block)
Jpg2Layout jpg2_layout(int B, int R, int nblk, int flags, bool with_coef) {
  const size_t q = (size_t)B * R;
  const bool opt_ = (flags & SE_JPG_OPTIMIZE) != 0;
  return Jpg2Layout{with_coef ? pad256(q * nblk * 128) : 0, pad256(q * 4), pad256(q * jpg_slot_bytes(nblk, flags)), opt_ ? pad256(q * 4096) : 0,
                    opt_ ? pad256((size_t)B * 4096) : 0};
}
size_t jpg2_need(const Jpg2Layout& L) { return L.coef + L.sizes + L.slots + L.hist + L.codes; }

struct Span { uintptr_t a, b; const char* name; };
bool meets(const Span& x, const Span& y) { return x.a < y.b && y.a < x.b; }

// the checks both entries share, after their own: cap, the workspace, sizes_out, tables_out, and that nothing written overlaps
// anything else (`srcs`: what the call only reads).  0 = ok.
int jpg2_check(se_ctx* c, int B, int flags, unsigned char* out, size_t cap, size_t bound, unsigned long long* sizes_out,
               unsigned char* tables_out, void* workspace, size_t workspace_bytes, size_t need, const std::vector<Span>& srcs,
               const char* src_fmt) {
  const bool opt_ = (flags & SE_JPG_OPTIMIZE) != 0;
  if (cap < bound) return fail(c, "cap=%zu is less than the bound of this call, %zu", cap, bound);
  if (cap > ((size_t)1 << 40) / (size_t)B) return fail(c, "cap=%zu: B cap is more than one call takes", cap);
  if (workspace_bytes < need) return fail(c, "workspace too small: %zu bytes, need %zu", workspace_bytes, need);
  if (!aligned_to(workspace, 256)) return fail(c, "workspace must be 256-byte aligned");
  if (!aligned_to(sizes_out, 8)) return fail(c, "sizes_out must be 8-byte aligned");
  if (opt_ && !aligned_to(tables_out, 16)) return fail(c, "tables_out must be 16-byte aligned");
  std::vector<Span> dst = {{(uintptr_t)out, (uintptr_t)out + (size_t)B * cap, "out"},
                           {(uintptr_t)sizes_out, (uintptr_t)sizes_out + (size_t)B * sizeof(unsigned long long), "sizes_out"},
                           {(uintptr_t)workspace, (uintptr_t)workspace + need, "the workspace"}};
  if (opt_) dst.push_back({(uintptr_t)tables_out, (uintptr_t)tables_out + (size_t)B * SE_JPG_TABLE_RECORD_BYTES, "tables_out"});
  for (size_t i = 0; i < srcs.size(); ++i)
    for (const Span& d : dst)
      if (meets(d, srcs[i])) {
        char what[64];
        snprintf(what, sizeof what, src_fmt, (int)i);
        return fail(c, "%s overlaps %s", d.name, what);
      }
  for (size_t i = 0; i < dst.size(); ++i)
    for (size_t j = i + 1; j < dst.size(); ++j)
      if (meets(dst[i], dst[j])) return fail(c, "%s overlaps %s", dst[i].name, dst[j].name);
  return 0;
}

// the arena's blocks in the layout's order (poisoned under SE_TEST_POISON); a block of 0 bytes is null
int jpg2_blocks(se_ctx* c, void* workspace, const Jpg2Layout& L, hipStream_t st, void** blk) {
  c->arena.reset((char*)workspace, jpg2_need(L), false);
  c->arena2.reset(nullptr, 0, false);
  const size_t bytes[5] = {L.coef, L.sizes, L.slots, L.hist, L.codes};
  for (int i = 0; i < 5; ++i) {
    blk[i] = nullptr;
    if (!bytes[i]) continue;
    blk[i] = c->arena.alloc(bytes[i] / 4);
    if (!blk[i]) return fail(c, "workspace arena exhausted");
    if (poison(c, blk[i], bytes[i], st)) return 1;
  }
  return 0;
}

// histogram and tables (SE_JPG_OPTIMIZE), rows, finish
int jpg2_code(se_ctx* c, int B, int R, int nblk, int flags, const short* coef, void** blk, unsigned char* out, size_t cap,
              unsigned long long* sizes_out, unsigned char* tables_out, hipStream_t st) {
  const unsigned* codes = nullptr;
  if (flags & SE_JPG_OPTIMIZE) {
    HIPCHK(c, launch_jpg2_hist(B, R, nblk, flags, coef, (unsigned*)blk[3], st));
    HIPCHK(c, launch_jpg2_tables(B, R, (const unsigned*)blk[3], (unsigned*)blk[4], tables_out, st));
    codes = (const unsigned*)blk[4];
  }
  HIPCHK(c, launch_jpg_rows(B, R, nblk, flags, coef, codes, (unsigned*)blk[1], (unsigned char*)blk[2], st));
  HIPCHK(c, launch_jpg_finish(B, R, nblk, jpg_slot_bytes(nblk, flags), (const unsigned*)blk[1], (const unsigned char*)blk[2], out, cap, sizes_out,
                              st));
  return 0;
}

// the encoder from pixels, for both headers' entries; the caller holds c->mu (a plain mutex: no public entry calls another)
size_t jpg2_encode_workspace_bytes(se_ctx* c, int B, int hs, int ws, int flags) {
  if (B < 1 || B > 65535) { fail(c, "bad B=%d (1 .. 65535 images per call)", B); return 0; }
  if (hs < 16 || ws < 16 || hs > 8192 || ws > 8192) { fail(c, "bad rectangle hs=%d ws=%d (sides are 16 .. 8192)", hs, ws); return 0; }
  if (flags < 0 || flags > 3) { fail(c, "bad flags=%d (SE_JPG_420 | SE_JPG_OPTIMIZE: 0 .. 3)", flags); return 0; }
  return jpg2_need(jpg2_layout(B, jpg_rows(hs, flags), jpg_row_blocks(ws, flags), flags, true));
}

int jpg2_encode(se_ctx* c, void* stream, const se_window* wins, int B, int hs, int ws, int quality, int flags, unsigned char* out, size_t cap,
                unsigned long long* sizes_out, unsigned char* tables_out, void* workspace, size_t workspace_bytes) {
  if (B < 1 || B > 65535) return fail(c, "bad B=%d (1 .. 65535 images per call)", B);
  if (hs < 16 || ws < 16 || hs > 8192 || ws > 8192) return fail(c, "bad rectangle hs=%d ws=%d (sides are 16 .. 8192)", hs, ws);
  if (quality < 1 || quality > 100) return fail(c, "bad quality=%d (1 .. 100)", quality);
  if (flags < 0 || flags > 3) return fail(c, "bad flags=%d (SE_JPG_420 | SE_JPG_OPTIMIZE: 0 .. 3)", flags);
  if (!wins) return fail(c, "null pointer argument: wins");
  if (!out) return fail(c, "null pointer argument: out");
  if (!sizes_out) return fail(c, "null pointer argument: sizes_out");
  if ((flags & SE_JPG_OPTIMIZE) && !tables_out) return fail(c, "null pointer argument: tables_out (SE_JPG_OPTIMIZE)");
  if (!workspace) return fail(c, "null pointer argument: workspace");
  if (win_check_records(c, wins, B, hs, ws, false)) return 1;
  const int R = jpg_rows(hs, flags), nblk = jpg_row_blocks(ws, flags);
  const Jpg2Layout L = jpg2_layout(B, R, nblk, flags, true);
  std::vector<Span> srcs;
  for (int i = 0; i < B; ++i)
    srcs.push_back({(uintptr_t)wins[i].frame_u8, (uintptr_t)wins[i].frame_u8 + (size_t)wins[i].Hi * wins[i].Wi * 3, nullptr});
  if (jpg2_check(c, B, flags, out, cap, se_jpg2_bound(hs, ws, flags), sizes_out, tables_out, workspace, workspace_bytes, jpg2_need(L), srcs,
                 "the frame of wins[%d]"))
    return 1;
  HIPCHK(c, hipSetDevice(c->device));
  set_profiler(&c->prof);
  const hipStream_t st = (hipStream_t)stream;
  void* blk[5];
  if (jpg2_blocks(c, workspace, L, st, blk)) return 1;
  const se_window* d = win_put(c, st, wins, B);
  if (!d) return 1;
  if (flags & SE_JPG_420) {
    HIPCHK(c, launch_jpg2_blocks420(d, B, hs, ws, quality, (short*)blk[0], st));
  } else {
    HIPCHK(c, launch_jpg_blocks(d, B, hs, ws, quality, (short*)blk[0], st));
  }
  return jpg2_code(c, B, R, nblk, flags, (const short*)blk[0], blk, out, cap, sizes_out, tables_out, st);
}

}  // namespace

size_t se_jpg_encode_u8_workspace_bytes(se_ctx* c, int B, int hs, int ws) {
  if (!c) return 0;
  std::lock_guard<std::mutex> lk(c->mu);
  return jpg2_encode_workspace_bytes(c, B, hs, ws, 0);
}

int se_jpg_encode_u8(se_ctx* c, void* stream, const se_window* wins, int B, int hs, int ws, int quality, unsigned char* out, size_t cap,
                     unsigned long long* sizes_out, void* workspace, size_t workspace_bytes) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  return jpg2_encode(c, stream, wins, B, hs, ws, quality, 0, out, cap, sizes_out, nullptr, workspace, workspace_bytes);
}

size_t se_jpg2_encode_u8_workspace_bytes(se_ctx* c, int B, int hs, int ws, int flags) {
  if (!c) return 0;
  std::lock_guard<std::mutex> lk(c->mu);
  return jpg2_encode_workspace_bytes(c, B, hs, ws, flags);
}

int se_jpg2_encode_u8(se_ctx* c, void* stream, const se_window* wins, int B, int hs, int ws, int quality, int flags, unsigned char* out,
                      size_t cap, unsigned long long* sizes_out, unsigned char* tables_out, void* workspace, size_t workspace_bytes) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  return jpg2_encode(c, stream, wins, B, hs, ws, quality, flags, out, cap, sizes_out, tables_out, workspace, workspace_bytes);
}

namespace {

int jpg2_code_shape(se_ctx* c, int B, int R, int nblk, int flags) {
  if (B < 1 || B > 65535) return fail(c, "bad B=%d (1 .. 65535 images per call)", B);
  if (R < 1 || R > 1024) return fail(c, "bad R=%d (1 .. 1024 rows of blocks)", R);
  if (flags < 0 || flags > 3) return fail(c, "bad flags=%d (SE_JPG_420 | SE_JPG_OPTIMIZE: 0 .. 3)", flags);
  const int per = flags & SE_JPG_420 ? 6 : 3;
  if (nblk < per || nblk > 3072 || nblk % per) return fail(c, "bad nblk=%d (a multiple of %d, at most 3072)", nblk, per);
  return 0;
}

}  // namespace

size_t se_jpg2_code_i16_workspace_bytes(se_ctx* c, int B, int R, int nblk, int flags) {
  if (!c) return 0;
  std::lock_guard<std::mutex> lk(c->mu);
  if (jpg2_code_shape(c, B, R, nblk, flags)) return 0;
  return jpg2_need(jpg2_layout(B, R, nblk, flags, false));
}

int se_jpg2_code_i16(se_ctx* c, void* stream, const short* coef, int B, int R, int nblk, int flags, unsigned char* out, size_t cap,
                     unsigned long long* sizes_out, unsigned char* tables_out, void* workspace, size_t workspace_bytes) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (jpg2_code_shape(c, B, R, nblk, flags)) return 1;
  if (!coef) return fail(c, "null pointer argument: coef");
  if (!out) return fail(c, "null pointer argument: out");
  if (!sizes_out) return fail(c, "null pointer argument: sizes_out");
  if ((flags & SE_JPG_OPTIMIZE) && !tables_out) return fail(c, "null pointer argument: tables_out (SE_JPG_OPTIMIZE)");
  if (!workspace) return fail(c, "null pointer argument: workspace");
  if (!aligned_to(coef, 2)) return fail(c, "coef must be 2-byte aligned");
  const Jpg2Layout L = jpg2_layout(B, R, nblk, flags, false);
  const std::vector<Span> srcs = {{(uintptr_t)coef, (uintptr_t)coef + (size_t)B * R * nblk * 128, nullptr}};
  if (jpg2_check(c, B, flags, out, cap, (size_t)R * jpg_row_bound(nblk, flags), sizes_out, tables_out, workspace, workspace_bytes, jpg2_need(L),
                 srcs, "coef"))
    return 1;
  HIPCHK(c, hipSetDevice(c->device));
  set_profiler(&c->prof);
  const hipStream_t st = (hipStream_t)stream;
  void* blk[5];
  if (jpg2_blocks(c, workspace, L, st, blk)) return 1;
  return jpg2_code(c, B, R, nblk, flags, coef, blk, out, cap, sizes_out, tables_out, st);
}

// ---- measurement support (bench.py): per-kernel HIP-event timing ---------------------------------
int se_profile_enable(se_ctx* c, int on) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCHK(c, hipSetDevice(c->device));
  c->prof.recs.clear();
  c->prof.used = 0;
  if (on && c->prof.pool.empty()) {
    c->prof.pool.resize(2 * 1024);           // enough for ~12 forwards of ~80 launches
    for (auto& e : c->prof.pool) HIPCHK(c, hipEventCreate(&e));
  }
  c->prof.on = on != 0;
  return 0;
}

int se_profile_report(se_ctx* c, char* buf, size_t cap) {
  if (!c || !buf || cap < 64) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());
  double ms[PL_COUNT] = {0}, fl[PL_COUNT] = {0}, by[PL_COUNT] = {0}, ex[PL_COUNT] = {0}, bl[PL_COUNT] = {0};
  long n[PL_COUNT] = {0};
  for (auto& r : c->prof.recs) {
    float t = 0.f;
    if (hipEventElapsedTime(&t, r.a, r.b) == hipSuccess) { ms[r.label] += t; fl[r.label] += r.flops; ex[r.label] += r.exec_flops; by[r.label] += r.bytes; bl[r.label] += (double)r.blocks; n[r.label]++; }
  }
  std::string s = "{\"kernels\": [";
  bool first = true;
  for (int l = 0; l < PL_COUNT; ++l) {
    if (!n[l]) continue;
    char t[384];
    snprintf(t, sizeof t, "%s{\"kernel\": \"%s\", \"launches\": %ld, \"total_ms\": %.6f, \"flops\": %.6e, \"flops_executed\": %.6e, \"bytes\": %.6e, \"workgroups\": %.1f}",
             first ? "" : ", ", prof_label_name(l), n[l], ms[l], fl[l], ex[l], by[l], bl[l] / (double)n[l]);
    s += t;
    first = false;
  }
  s += "], \"layers\": [";
  // per (kernel, layer name) in first-seen order
  std::vector<std::string> keys;
  std::map<std::string, std::pair<double, double>> agg;   // ms, flops
  std::map<std::string, double> aggx;                       // executed flops
  std::map<std::string, long> cnt;
  for (auto& r : c->prof.recs) {
    if (!r.name) continue;
    float t = 0.f;
    if (hipEventElapsedTime(&t, r.a, r.b) != hipSuccess) continue;
    std::string k = std::string(prof_label_name(r.label)) + ":" + r.name;
    if (!cnt.count(k)) keys.push_back(k);
    agg[k].first += t; agg[k].second += r.flops; aggx[k] += r.exec_flops; cnt[k]++;
  }
  first = true;
  for (auto& k : keys) {
    char t[384];
    snprintf(t, sizeof t, "%s{\"layer\": \"%s\", \"launches\": %ld, \"total_ms\": %.6f, \"flops\": %.6e, \"flops_executed\": %.6e}",
             first ? "" : ", ", k.c_str(), cnt[k], agg[k].first, agg[k].second, aggx[k]);
    s += t;
    first = false;
  }
  s += "], \"launches\": [";
  // every record in launch order, with the kernel form the dispatcher chose (Profiler::Rec::form): what the tests read
  first = true;
  for (auto& r : c->prof.recs) {
    char t[256];
    snprintf(t, sizeof t, "%s{\"form\": \"%s\", \"kernel\": \"%s\", \"layer\": \"%s\", \"workgroups\": %ld}", first ? "" : ", ",
             r.form ? r.form : "?", prof_label_name(r.label), r.name ? r.name : "", r.blocks);
    s += t;
    first = false;
  }
  s += "]}";
  if (s.size() + 1 > cap) return fail(c, "profile buffer too small");
  memcpy(buf, s.c_str(), s.size() + 1);
  return 0;
}

// ---- developer switches (se_kernels.h SE_OPTIONS): process-wide, read from the environment once ----
int se_debug_set_option(const char* name, int value) { return opt_set(name, value); }
int se_debug_get_option(const char* name, int* value) { return opt_get(name, value); }
void se_debug_reset_options(void) { opt_reset(); }

// the ConvCall of se_gated_conv2d_ex for these arguments, chosen and named (no ctx, no device)
int se_debug_gconv_form(int cin, int cin1, int src1_is_vector, int cout, int k, int stride, int rate, int act, int upsample,
                        int B, int H, int W, int exec_flags, int net_id, char* out, size_t cap) {
  if (!out || cin <= 0 || cin1 < 0 || cout <= 0 || k <= 0 || stride <= 0 || rate <= 0 || B <= 0 || H <= 0 || W <= 0) return 1;
  const bool bf = (exec_flags & SE_FLAG_BF16) != 0;
  const int gran = bf ? 8 : 4;
  if (cin1 && ((cin % gran) || (cin1 % gran))) return 1;
  const LayerDef d = {"test", cin + cin1, cout, k, stride, rate, act, upsample};
  const bool raw = small_layer(d);
  if (raw && (k != 3 || cin != 12 || cin1 || (cout != 1 && cout != 3) || stride != 1 || rate != 1 || upsample)) return 1;
  if (!raw && (cout % 8)) return 1;
  const LayerFacts f = layer_facts(d, cin + cin1);       // chans: the identity
  if (!raw && f.cfg < 0) return 1;
  const int Cp = (cin + gran - 1) & ~(gran - 1);
  if (!raw && Cp + cin1 != f.CG[bf] * gran) return 1;
  const bool vec = cin1 && src1_is_vector;               // ... for which the entry point brings the fold scratch
  const ConvCall q = {d, f, B, H, W, Cp, cin1, cin1 ? (vec ? SRC2_VECTOR : SRC2_TENSOR) : SRC2_NONE, bf,
                      (exec_flags & SE_FLAG_LOW_LATENCY) != 0, (exec_flags & SE_FLAG_CONSERVATIVE) != 0, net_id, vec};
  const Choice ch = choose_form(q);
  const char* name = form_name(ch, q);
  if (!name) return 1;
  const std::string s = std::string(ch.fold ? "vecbias," : "") + name;
  if (s.size() + 1 > cap) return 1;
  memcpy(out, s.c_str(), s.size() + 1);
  return 0;
}

// ---- unit-test entry points (allocate scratch internally; synchronise the stream before freeing) ----
int se_gated_conv2d_ex(se_ctx* c, void* stream, const float* x, const float* x1, int x1_is_vector, const float* w_host,
                       const float* b_host, float* y, int B, int Cin, int Cin1, int H, int W, int Cout, int k, int stride,
                       int rate, int act, int upsample, int exec_flags) {
  if (!c || !x || !w_host || !b_host || !y) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCHK(c, hipSetDevice(c->device));
  begin_call(c, stream, exec_flags & (SE_FLAG_LOW_LATENCY | SE_FLAG_BF16));
  const bool bf = c->bf16;
  if (!x1) Cin1 = 0;
  if (x1 && ((Cin % 4) || (Cin1 % 4))) return fail(c, "two-source conv: channel counts must be multiples of 4");
  if (bf && x1 && ((Cin % 8) || (Cin1 % 8))) return fail(c, "two-source bf16 conv: channel counts must be multiples of 8");
  const int CinT = Cin + Cin1;
  Layer L;
  L.def = LayerDef{"test", CinT, Cout, k, stride, rate, act, upsample};
  const bool raw = small_layer(L.def);
  if (raw && (k != 3 || CinT != 12 || x1 || (Cout != 1 && Cout != 3) || stride != 1 || rate != 1 || upsample))
    return fail(c, "raw conv: only 3x3 12->{1,3}");
  if (!raw && (Cout % 8)) return fail(c, "gated conv needs Cout %% 8 == 0");
  L.w.assign(w_host, w_host + (size_t)Cout * CinT * k * k);
  L.b.assign(b_host, b_host + Cout);
  std::vector<int> chans(CinT);
  std::iota(chans.begin(), chans.end(), 0);
  if (pack_layer_images(L, chans, c->err)) return 1;
  const int Cp = bf ? (Cin + 7) & ~7 : (Cin + 3) & ~3;
  DevBuf xin, x1in, yout, vb_test;
  // launches on c->st read these buffers and the layer's images: every return drains the stream before they are freed
  struct Drain {
    se_ctx* c;
    ~Drain() {
      (void)hipStreamSynchronize(c->st);
      c->vbias_ws = nullptr; c->vec32 = nullptr;
    }
  } drain{c};
  HIPCHK(c, xin.alloc((size_t)B * H * W * Cp * 4));
  if (poison(c, xin, (size_t)B * H * W * Cp * 4, c->st)) return 1;
  int rc = (bf ? launch_nchw_to_nhwc16 : launch_nchw_to_nhwc)(x, xin, B, Cin, Cp, H, W, c->st) != hipSuccess;
  if (!rc && x1) {
    // second source of the virtual concat (editline_g.py:166-167,211): a tensor (B,Cin1,H,W) or a per-image vector (B,Cin1)
    const size_t n1 = x1_is_vector ? (size_t)B * Cin1 : (size_t)B * H * W * Cin1;
    HIPCHK(c, x1in.alloc(n1 * 4));
    if (poison(c, x1in, n1 * 4, c->st)) return 1;
    if (x1_is_vector && !bf) rc = hipMemcpyAsync(x1in, x1, n1 * 4, hipMemcpyDeviceToDevice, c->st) != hipSuccess;
    else if (x1_is_vector) rc = launch_nchw_to_nhwc16(x1, x1in, B, Cin1, Cin1, 1, 1, c->st) != hipSuccess;
    else rc = (bf ? launch_nchw_to_nhwc16 : launch_nchw_to_nhwc)(x1, x1in, B, Cin1, Cin1, H, W, c->st) != hipSuccess;
  }
  if (!rc && raw) {
    SmallConvParams sp;
    memset(&sp, 0, sizeof sp);
    sp.x = xin; sp.w = L.direct[bf]; sp.b = L.d_b; sp.B = B; sp.H = H; sp.W = W; sp.cout = Cout; sp.mode = 4;
    sp.bf16 = bf ? 1 : 0;
    sp.out_nchw = y;
    rc = launch_small_conv(sp, c->st) != hipSuccess;
  } else if (!rc) {
    const ConvShape sh = conv_shape(L.def, H, W);
    const int Gs = bf ? (Cout / 2 + 7) & ~7 : Cout / 2;
    HIPCHK(c, yout.alloc((size_t)B * sh.Ho * sh.Wo * Gs * 4));
    if (poison(c, yout, (size_t)B * sh.Ho * sh.Wo * Gs * 4, c->st)) return 1;
    if (x1in && x1_is_vector) {               // scratch of the folded vector source (the forwards take it from the workspace)
      HIPCHK(c, vb_test.alloc((size_t)B * 9 * 192 * 4));
      if (poison(c, vb_test, (size_t)B * 9 * 192 * 4, c->st)) return 1;
      c->vbias_ws = vb_test;
      c->vec32 = bf ? x1 : nullptr;           // bf16 mode: the caller's fp32 vector (x1in is its bf16 rounding)
    }
    rc = run_gconv(c, L, xin, Cp, x1in, Cin1, x1_is_vector, yout, B, H, W);
    if (!rc) rc = (bf ? launch_nhwc16_to_nchw : launch_nhwc_to_nchw)(yout, y, B, Cout / 2, Gs, sh.Ho, sh.Wo, c->st) != hipSuccess;
  }
  return rc;
}

int se_gated_conv2d(se_ctx* c, void* stream, const float* x, const float* w_host, const float* b_host, float* y, int B,
                    int Cin, int H, int W, int Cout, int k, int stride, int rate, int act, int upsample) {
  return se_gated_conv2d_ex(c, stream, x, nullptr, 0, w_host, b_host, y, B, Cin, 0, H, W, Cout, k, stride, rate, act,
                            upsample, 0);
}

int se_attention_ex(se_ctx* c, void* stream, const float* x, const float* mask_full, float* out, float* similar_out, int B,
                    int h, int w, int exec_flags) {
  if (!c || !x || !mask_full || !out) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (h < 4 || w < 4 || (h % 2) || (w % 2)) return fail(c, "attention: h, w must be even and >= 4");
  HIPCHK(c, hipSetDevice(c->device));
  begin_call(c, stream, exec_flags & SE_FLAG_BF16);
  const bool bf = c->bf16;
  const int R = (h / 2) * (w / 2), Rp = att_row_stride(R, true) + 64;
  // the refusal of run_attention, before anything is allocated: similar_out at a streaming size
  const bool streaming = att_streaming(h, w, bf, similar_out != nullptr);
  const int L = ((h - 4) / 2 + 1) * ((w - 4) / 2 + 1);
  if (streaming && similar_out)
    return fail(c, "attention: similar_out (the %d x %d score matrix) is not available on a %dx%d feature map: "
                   "it runs in the streaming form, which never forms it", L, L, h, w);
  // the R x R matrices E and P exist in the materialised form only (the streaming form's scratch is O(R))
  const size_t rr = streaming ? 0 : 2 * (size_t)B * R * Rp;
  const size_t bytes = ((size_t)B * h * w * 96 * 3 + rr + (size_t)B * Rp * (7 + 4 * 96) + 64 * 96 * B + 2 * (size_t)B * R + 9 * (size_t)(w / 2 + 72) + (size_t)B * (768 + (h / 2) * 384)) * 4 + (1 << 16);
  char* ws = nullptr;
  HIPCHK(c, hipMalloc(&ws, bytes));
  if (poison(c, ws, bytes, c->st)) { (void)hipStreamSynchronize(c->st); (void)hipFree(ws); return 1; }      // (what no block covers, too)
  c->arena.reset(ws, bytes, false);
  c->arena2.reset(nullptr, 0, false);
  Plan P(c, c->G, B);
  Act xin = P.alloc(h, w, 96), o = P.alloc(h, w, 96);
  int rc = P.rc;
  if (!rc) rc = (bf ? launch_nchw_to_nhwc16 : launch_nchw_to_nhwc)(x, xin.p, B, 96, 96, h, w, c->st) != hipSuccess;
  if (!rc) rc = run_attention(c, P, xin, mask_full, o, similar_out);
  if (!rc) rc = (bf ? launch_nhwc16_to_nchw : launch_nhwc_to_nchw)(o.p, out, B, 96, 96, h, w, c->st) != hipSuccess;
  (void)hipStreamSynchronize(c->st);
  (void)hipFree(ws);
  return rc;
}

int se_attention(se_ctx* c, void* stream, const float* x, const float* mask_full, float* out, float* similar_out, int B,
                 int h, int w) {
  return se_attention_ex(c, stream, x, mask_full, out, similar_out, B, h, w, 0);
}

// ---- the kernels between the convolutions: input packing, pooling, output conv (tests/test_gpu_glue.py) ----
int se_pack_inputs(se_ctx* c, void* stream, int net_id, const float* x, const float* x2, const float* mask, const float* mask2,
                   const float* guide, void* packed_out, void* style_out, int B, int H, int W, int flags, int exec_flags) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (B < 1 || H < 1 || W < 1) return fail(c, "pack: bad shape B=%d H=%d W=%d", B, H, W);
  if (net_id != SE_NET_M && net_id != SE_NET_G) return fail(c, "pack: net_id must be SE_NET_G or SE_NET_M");
  if (!x || !guide || !packed_out || (net_id == SE_NET_G && (!x2 || !mask || !mask2 || !style_out))) return fail(c, "null pointer argument");
  HIPCHK(c, hipSetDevice(c->device));
  begin_call(c, stream, exec_flags & SE_FLAG_BF16);
  // no scratch: the kernels write the caller's buffers directly, as they write the first conv's input in the forwards
  if (net_id == SE_NET_M) {      // plan_netM
    HIPCHK(c, (c->bf16 ? launch_pack_m16 : launch_pack_m)(x, guide, (float*)packed_out, B, H, W, c->st));
  } else {                       // plan_netG
    HIPCHK(c, (c->bf16 ? launch_pack_g16 : launch_pack_g)(x, x2, mask, mask2, guide, (float*)packed_out, (float*)style_out, B, H, W,
                                                          (flags & SE_FLAG_NO_MASK_CC) ? 1 : 0,
                                                          (flags & SE_FLAG_JOINT_TRAIN_INP) ? 1 : 0, c->st));
  }
  return 0;
}

int se_column_reduce(se_ctx* c, void* stream, const float* x, float* out, unsigned short* out_bf16, int B, int C, int H, int W,
                     int op, int exec_flags) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (!x || !out) return fail(c, "null pointer argument");
  if (B < 1 || C < 1 || H < 1 || W < 1) return fail(c, "column reduce: bad shape B=%d C=%d H=%d W=%d", B, C, H, W);
  if (op < 0 || op > 2) return fail(c, "column reduce: op must be 0 (max), 1 (mean) or 2 (rsqrt of the sum of squares)");
  const bool bf = (exec_flags & SE_FLAG_BF16) != 0;
  // what launch_colreduce refuses, before anything is allocated or enqueued
  if (C > 256 || C % (bf ? 8 : 4))
    return fail(c, "column reduce: C = %d must be a multiple of %d and at most 256", C, bf ? 8 : 4);
  if ((double)B * H * W * C * (bf ? 2 : 4) >= 2147483648.0) return fail(c, "column reduce: B H W C beyond the 32-bit byte range");
  HIPCHK(c, hipSetDevice(c->device));
  begin_call(c, stream, exec_flags & SE_FLAG_BF16);
  DevBuf xin, part;
  struct Drain {      // the launches on c->st read the scratch: every return drains the stream before it is freed
    se_ctx* c;
    ~Drain() { (void)hipStreamSynchronize(c->st); }
  } drain{c};
  const size_t xbytes = (size_t)B * H * W * C * (bf ? 2 : 4), pbytes = (size_t)B * COLREDUCE_SPLITS * C * 4;
  HIPCHK(c, xin.alloc(xbytes));
  HIPCHK(c, part.alloc(pbytes));
  if (poison(c, xin, xbytes, c->st) || poison(c, part, pbytes, c->st)) return 1;
  HIPCHK(c, (bf ? launch_nchw_to_nhwc16 : launch_nchw_to_nhwc)(x, xin, B, C, C, H, W, c->st));
  HIPCHK(c, launch_colreduce(xin, part, out, B, H * W, C, op, c->st, bf ? 1 : 0, (float*)out_bf16));
  return 0;
}

int se_output_conv(se_ctx* c, void* stream, const float* x, const float* w_host, const float* b_host, int B, int H, int W, int cout,
                   int mode, const se_output_conv_io* io, int no_mask_coarse, int packed, int exec_flags) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (!x || !w_host || !b_host || !io) return fail(c, "null pointer argument");
  if (B < 1 || H < 1 || W < 1) return fail(c, "output conv: bad shape B=%d H=%d W=%d", B, H, W);
  if (mode < 0 || mode > 3) return fail(c, "output conv: mode must be 0..3");
  if (cout != (mode == 0 ? 1 : 3)) return fail(c, "output conv: mode %d has %d output channels", mode, mode == 0 ? 1 : 3);
  // the pointers the kernel dereferences without a test
  if (mode == 0 && !io->out) return fail(c, "output conv: mode 0 writes `out`");
  if (mode == 2 && (!io->img || !io->mask || !io->xnow)) return fail(c, "output conv: mode 2 needs img, mask and xnow");
  if (mode == 3 && (io->composed || io->rgb8 || io->m8) && (!io->img || !io->mask))
    return fail(c, "output conv: the composite of mode 3 needs img and mask");
  HIPCHK(c, hipSetDevice(c->device));
  begin_call(c, stream, exec_flags & SE_FLAG_BF16);
  const bool bf = c->bf16;
  Layer L;
  L.def = LayerDef{"test", 12, cout, 3, 1, 1, ACT_NONE, 0};
  L.w.assign(w_host, w_host + (size_t)cout * 12 * 9);
  L.b.assign(b_host, b_host + cout);
  std::vector<int> chans(12);
  std::iota(chans.begin(), chans.end(), 0);
  if (pack_layer_images(L, chans, c->err)) return 1;
  DevBuf xin;
  struct Drain {      // the launches on c->st read xin and the layer's images: every return drains the stream before they are freed
    se_ctx* c;
    ~Drain() { (void)hipStreamSynchronize(c->st); }
  } drain{c};
  const int Cp = bf ? 16 : 12;
  const size_t xbytes = (size_t)B * H * W * Cp * (bf ? 2 : 4);
  HIPCHK(c, xin.alloc(xbytes));
  if (poison(c, xin, xbytes, c->st)) return 1;
  HIPCHK(c, (bf ? launch_nchw_to_nhwc16 : launch_nchw_to_nhwc)(x, xin, B, 12, Cp, H, W, c->st));
  SmallConvParams sp;      // filled as small() fills it
  memset(&sp, 0, sizeof sp);
  sp.x = xin; sp.w = L.direct[bf]; sp.b = L.d_b; sp.B = B; sp.H = H; sp.W = W; sp.cout = cout;
  sp.bf16 = bf ? 1 : 0;
  sp.mode = mode; sp.out_nchw = io->out; sp.hard = io->hard; sp.img = io->img; sp.mask = io->mask; sp.xnow = (float*)io->xnow;
  sp.composed = io->composed; sp.no_mask_coarse = no_mask_coarse ? 1 : 0;
  if (mode == 3) { sp.rgb8 = io->rgb8; sp.m8 = io->m8; }
  if (mode == 0) sp.lock = io->lock;
  if (packed) {
    const long packed_bs = 4l * H * W;
    if (mode == 0) sp.out_bs = packed_bs;
    if (mode == 3) { sp.mask_bs = packed_bs; sp.comp_bs = packed_bs; }
  }
  HIPCHK(c, launch_small_conv(sp, c->st));
  return 0;
}

}  // extern "C"
