// Host-only internals of libsketchedit_hip.so, shared by its host files (se_plan.hip, se_api.hip, se_api_window.hip,
// se_api_select.hip, se_api_move.hip, se_api_codec.hip, se_api_debug.hip): the context, the workspace arena, the error and entry helpers, and
// the few functions that one of those files defines and another calls.  Like se_dispatch.h it holds no __global__ code; it is
// not part of the C-ABI.
#pragma once
#include "../../include/sketchedit_hip.h"
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

namespace se {

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

}  // namespace se

struct se_ctx {
  int device = 0;
  std::mutex mu;
  std::string err;
  std::map<std::string, se::Layer> G, M;
  se::Layer wconv1_j4;      // G.wconv1 packed for a 4-channel input: with --joint_train_inp its guide channel is zero
  float* zeros = nullptr;   // zero page for out-of-bounds granules
  float* lut8 = nullptr;    // 256 floats: (v/255 - 0.5)/0.5, the dataset's normalisation of a uint8 value (se_dequantize_u8)
  se::Arena arena;          // workspace arena of the main branch
  se::Arena arena2;         // low-latency mode: arena of the concurrent side branch (disjoint region of the workspace)
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
  bool paired = false;             // the plan being made is one half of a paired pass (pair_rule): no inner fork, its own arena
  int half = 0;                    // ... which half: 0 on the caller's stream and the main arena, 1 on st_side and the side arena
  bool conservative = false;       // SE_FLAG_CONSERVATIVE of the running call: netM's 96 -> 192 layers on F(2x2,3x3)
  const se_netG_taps* taps = nullptr;      // se_netG_forward_taps: intermediate outputs of the running netG plan
  float* vbias_ws = nullptr;       // [B][9][192] scratch for the folded vector source of the next two-source layer (plan_netG)
  const float* vec32 = nullptr;    // bf16 mode: the fp32 copy of the vector source (the conv source itself is its bf16 rounding)
  unsigned char* rgb8 = nullptr;   // se_inference_u8: uint8 outputs written by the last kernel of the running call
  unsigned char* m8 = nullptr;
  se::Profiler prof;
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

namespace se {

extern thread_local std::string g_create_err;      // what a failed se_create said (se_api.hip; read by se_last_error(NULL))

inline int fail(se_ctx* c, const char* fmt, ...) {
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

inline int xcd_remap_enabled() { return opt(OPT_XCD_REMAP); }     // SE_XCD_REMAP=0 switches the XCD-aware tile order off (A/B measurements)

// Every raw-tile / Winograd / gather kernel addresses its source through a buffer resource with 32-bit BYTE offsets and uses
// byte offset 0x80000000 as the "outside the image -> hardware zero fill" sentinel, so a tensor one launch addresses must stay
// below 2^31 BYTES (the guards used to count elements).  The forwards never reach the limit: they split
// the batch into passes (batch_passes).  SE_TEST_OFFSET_LIMIT (se_debug_set_option only) lowers it so that the tests reach the
// split with a handful of small images.
inline long long addr_limit() {
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
inline int poison_byte() {
  const int v = opt(OPT_TEST_POISON);
  return v >= 1 && v <= 255 ? v : 0;
}
inline int poison(se_ctx* c, void* p, size_t bytes, hipStream_t st) {
  const int v = poison_byte();
  if (!v || !p || !bytes) return 0;
  HIPCHK(c, hipMemsetAsync(p, v, bytes, st));
  return 0;
}

inline bool aligned_to(const void* p, int a) { return ((uintptr_t)p & (uintptr_t)(a - 1)) == 0; }

inline size_t pad256(size_t n) { return (n + 255) & ~(size_t)255; }

// whether the byte ranges [a, a + an) and [b, b + bn) share a byte
inline bool overlaps(const void* a, size_t an, const void* b, size_t bn) {
  return (uintptr_t)a < (uintptr_t)b + bn && (uintptr_t)b < (uintptr_t)a + an;
}

inline int check_dims(se_ctx* c, int B, int H, int W) {
  if (B < 1 || H < 16 || W < 16 || (H % 8) || (W % 8)) return fail(c, "bad shape B=%d H=%d W=%d (H, W must be multiples of 8, >= 16)", B, H, W);
  return 0;
}

inline void begin_call(se_ctx* c, void* stream, int flags) {
  c->st = c->st_main = (hipStream_t)stream;
  c->dry = false;
  c->low_latency = (flags & SE_FLAG_LOW_LATENCY) != 0;
  c->bf16 = (flags & SE_FLAG_BF16) != 0;
  c->conservative = (flags & SE_FLAG_CONSERVATIVE) != 0;
  c->serial = c->prof.on;
  c->taps = nullptr;
  c->rgb8 = nullptr; c->m8 = nullptr;
  c->paired = false; c->half = 0;
  c->cur_net = SE_NET_G;       // per-op entry points run as netG layers whatever plan ran last; the plans set their own
  set_profiler(&c->prof);
}

// what every entry that plans a forward does once its arguments are checked (the mutex is held)
inline int forward_enter(se_ctx* c) {
  HIPCHK(c, hipSetDevice(c->device));
  c->serial = c->prof.on;      // profiler on: default mode planned on one stream (Plan::forked)
  c->fork2 = opt(OPT_FORK_DEFAULT) != 0;
  return 0;
}

// what an entry that launches without planning a forward does once its arguments are checked (the mutex is held)
inline int device_enter(se_ctx* c) {
  HIPCHK(c, hipSetDevice(c->device));
  set_profiler(&c->prof);
  return 0;
}

// ---- se_plan.hip: the layer tables, the conv launchers, the plans of netM / netG and how a forward's workspace is carved ----
extern const LayerDef G_LAYERS[], M_LAYERS[];
extern const int NG, NM;

int run_gconv(se_ctx* c, const Layer& L, const float* src0, int C0, const float* src1, int C1, int src1_vec, float* dst,
              int B, int Hin, int Win);

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
  Plan(se_ctx* c_, std::map<std::string, Layer>& n, int B_) : c(c_), net(n), B(B_), ar(home()) {}
  // the arena a plan starts in and returns to after a side branch: the main one, or the side one for the second half of a paired pass
  Arena* home() const { return c->paired && c->half ? &c->arena2 : &c->arena; }
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
    // A paired pass (pair_rule): each half allocates from its own arena only and is enqueued on its own stream, behind the fork
    // event of the pass, so the same ordering holds per half.
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
  // (a half of a paired pass is one chain on one stream: the side stream and arena belong to the other half)
  bool forked() const { return !c->paired && (c->low_latency || (c->fork2 && !c->serial)) && c->st_side; }
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

int plan_netM(se_ctx* c, const float* image, const float* sketch, float* mask_out, float* hard_out, float* maskim_out,
              int B, int H, int W, long packed_bs = 0, const unsigned char* lock = nullptr);
int plan_netG(se_ctx* c, const float* x, const float* x2, const float* mask, const float* mask2, const float* guide,
              float* coarse_out, float* fine_out, const float* soft_mask, float* composed_out, int B, int H, int W,
              int flags, long packed_bs = 0);
int att_row_stride(int R, bool bf);
bool att_streaming(int h, int w, bool bf, bool want_similar);
int run_attention(se_ctx* c, Plan& P, Act& x, const float* mask_full, Act& out, float* similar_nchw);
int pass_size(se_ctx* c, int B, int H, int W, int flags);
// Paired passes: whether a pass of `bb` images of the default mode runs as two half-batch chains, images
// [0, ceil(bb / 2)) on the caller's stream and the main arena, the rest on the side stream and the side arena, between one fork
// and one join.  Pure: the arguments and SE_PAIR_MIN_PIXELS (0: never).  A half runs the kernels a pass of its size runs, and
// which kernel a layer runs does not depend on the batch (se_dispatch.h), so an image's bits do not depend on the pairing.
inline bool pair_rule(int bb, int H, int W, int flags) {
  const int min_pixels = opt(OPT_PAIR_MIN_PIXELS);
  return !(flags & SE_FLAG_LOW_LATENCY) && bb >= 2 && min_pixels > 0 && (long long)bb * H * W >= min_pixels;
}
inline int pair_first(int bb) { return (bb + 1) / 2; }       // images of the first half
// ... and whether THIS call pairs: never while the profiler is on (c->serial: one stream, per-kernel durations) or with taps
inline bool pair_pass(const se_ctx* c, int bb, int H, int W, int flags) {
  return pair_rule(bb, H, W, flags) && !c->serial && !c->taps && c->st_side;
}
se_ctx::Peaks plan_peaks(se_ctx* c, int which, int B, int H, int W, int flags, bool want_maskim, bool pair = false);
int pair_fork(se_ctx* c, hipStream_t main);
void pair_half(se_ctx* c, int half);
int pair_join(se_ctx* c, hipStream_t main);
int carve(se_ctx* c, const se_ctx::Peaks& pk, void* ws, size_t ws_bytes, size_t tail);

// ---- se_api.hip: the resize resources of the ctx, and the forward that leaves uint8 (the window edits and fills end in it) ----
int rs_enter(se_ctx* c, hipStream_t st);
const se_ctx::ResampleTable* rs_table(se_ctx* c, int in, int out, int filter);
unsigned char* rs_scratch(se_ctx* c, size_t bytes);
int inference_u8_locked(se_ctx* c, void* stream, const float* image, const float* sketch, unsigned char* rgb_out,
                        unsigned char* mask_u8_out, void* ws, size_t ws_bytes, int B, int H, int W, int flags, int tail_planes,
                        const unsigned char* lock8 = nullptr);

// ---- se_api_window.hip: the se_window records of a call, checked and put into the ctx's ring (the encoders take windows too) ----
int win_check_records(se_ctx* c, const se_window* wins, int B, int hs, int ws, bool need_sketch);
const se_window* win_put(se_ctx* c, hipStream_t st, const se_window* wins, int B);

}  // namespace se
