// Host side of libsketchedit_hip.so behind the C-ABI declared in include/sketchedit_hip.h: the context and its weights, the
// forwards of netM / netG / inference with the hipGraph cache, the uint8 ends, and the Pillow-exact resize with its resources.
// The plans themselves: se_plan.hip; the context and what the host files share: se_host.h; weight images: se_pack.hip; the
// entries of the editing sessions: se_api_window.hip, se_api_select.hip, se_api_move.hip, se_api_codec.hip; profiler, switches and per-op
// entries: se_api_debug.hip.
#include "se_host.h"

using namespace se;

namespace se {

thread_local std::string g_create_err;

}  // namespace se

namespace {

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

}  // namespace

namespace se {

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

// The forward with the output quantisation of test.py:25-27 fused into its last kernel: the composite and the soft mask
// leave the device as uint8 only (a quarter of the fp32 bytes, no separate pass); the soft mask needed between netM and
// the final composite lives in the workspace.
// `tail_planes` fp32 (B,H,W) planes at the end of the workspace are the caller's; the soft and hard masks sit in front of them
// (`_locked` = the ctx's mutex is held; lock8 = the (B,H,W) lock plane of DESIGN.md 6g, or null)
int inference_u8_locked(se_ctx* c, void* stream, const float* image, const float* sketch, unsigned char* rgb_out,
                        unsigned char* mask_u8_out, void* ws, size_t ws_bytes, int B, int H, int W, int flags, int tail_planes,
                        const unsigned char* lock8) {
  flags &= ~(SE_FLAG_GRAPH | SE_FLAG_PACKED_OUT | SE_FLAG_RAW_FINE);
  const size_t plane = ((size_t)B * H * W * 4 + 255) & ~(size_t)255;
  const size_t tail = (2 + (size_t)tail_planes) * plane;
  if (ws_bytes < tail) return fail(c, "workspace too small: %zu bytes", ws_bytes);
  float* hard_all = (float*)((char*)ws + ws_bytes - tail + plane);
  float* soft_all = (float*)((char*)ws + ws_bytes - tail);
  const size_t HW = (size_t)H * W;
  const int nb = pass_size(c, B, H, W, flags);       // passes over image ranges beyond the kernels' 32-bit byte offsets
  if (!nb) return 1;
  if (poison(c, soft_all, 2 * plane, (hipStream_t)stream)) return 1;      // (the caller's tail planes are the caller's to fill)
  for (int p0 = 0; p0 < B; p0 += nb) {
    const int pb = std::min(nb, B - p0);
    // a paired pass (pair_rule): two half-batch chains, planned one after the other, on the two streams and arenas
    const bool pair = pair_pass(c, pb, H, W, flags);
    const se_ctx::Peaks pk = plan_peaks(c, 3, pb, H, W, flags, false, pair);
    if (carve(c, pk, ws, ws_bytes, tail)) return 1;
    if (pair && pair_fork(c, (hipStream_t)stream)) return 1;
    int rc = 0;
    for (int half = 0; half < (pair ? 2 : 1) && !rc; ++half) {
      const int b0 = p0 + (half ? pair_first(pb) : 0), bb = !pair ? pb : half ? pb - pair_first(pb) : pair_first(pb);
      const float *img = image + b0 * 3 * HW, *sk = sketch + b0 * HW;
      float *hard = hard_all + b0 * HW, *soft = soft_all + b0 * HW;
      begin_call(c, stream, flags);
      if (pair) pair_half(c, half);
      rc = plan_netM(c, img, sk, soft, hard, nullptr, bb, H, W, 0, lock8 ? lock8 + b0 * HW : nullptr);
      if (!rc) rc = carve(c, pk, ws, ws_bytes, tail);
      if (rc) break;
      c->rgb8 = rgb_out + b0 * 3 * HW; c->m8 = mask_u8_out ? mask_u8_out + b0 * HW : nullptr;
      rc = plan_netG(c, img, img, hard, hard, sk, nullptr, nullptr, soft, nullptr, bb, H, W, flags);
    }
    if (pair && pair_join(c, (hipStream_t)stream) && !rc) rc = 1;      // (joined after a failed half too: the streams stay ordered)
    if (rc) return rc;
  }
  return 0;
}

}  // namespace se

namespace {

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
                // ... and as the two half-batch chains se_inference makes of such a pass (pair_pass; se_netM_forward and
                // se_netG_forward never pair: the single chain above stays counted)
                if (pair_pass(c, bb, H, W, flags)) {
                  const se_ctx::Peaks pp = plan_peaks(c, 3, bb, H, W, flags, mi != 0, true);
                  if (pp.main + pp.side > peak) peak = pp.main + pp.side;
                }
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
  flags &= ~SE_FLAG_RAW_FINE;      // se_fill_window_u8 only
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
  for (int p0 = 0; p0 < B; p0 += nb) {
    const int pb = std::min(nb, B - p0);
    // A paired pass (pair_rule): images [p0, p0 + ceil(pb / 2)) as one netM -> netG chain on the caller's stream
    // and the main arena, the rest as another on the side stream and the side arena, between one fork and one join.  The host
    // plans and enqueues the halves one after the other, so the ctx's per-plan state is never live for both; what the halves
    // share on the device is read-only (inputs, weights), everything written is addressed per image or lives in the half's arena.
    const bool pair = pair_pass(c, pb, H, W, flags);
    const se_ctx::Peaks pk = plan_peaks(c, 3, pb, H, W, flags, maskim_out != nullptr, pair);
    if (carve(c, pk, ws, ws_bytes, plane)) return 1;
    if (pair && pair_fork(c, (hipStream_t)stream)) return 1;
    int rc = 0;
    for (int half = 0; half < (pair ? 2 : 1) && !rc; ++half) {
      const int b0 = p0 + (half ? pair_first(pb) : 0), bb = !pair ? pb : half ? pb - pair_first(pb) : pair_first(pb);
      const float *img = image + b0 * 3 * HW, *sk = sketch + b0 * HW;
      float *hard = hard_all + b0 * HW, *mk = mask_out + b0 * mask_bs;
      begin_call(c, stream, flags);
      if (pair) pair_half(c, half);
      rc = plan_netM(c, img, sk, mk, hard, maskim_out ? maskim_out + b0 * 3 * HW : nullptr, bb, H, W, packed_bs,     // editline2_model.py:339,346-347
                     lock8 ? lock8 + b0 * HW : nullptr);
      if (!rc) rc = carve(c, pk, ws, ws_bytes, plane);
      if (rc) break;
      // netG(inputs, inputs, mask_inpaint, mask_inpaint, line)  :366-368 ; composite with the soft mask :132
      rc = plan_netG(c, img, img, hard, hard, sk, coarse_out ? coarse_out + b0 * 3 * HW : nullptr, fine_out ? fine_out + b0 * 3 * HW : nullptr,
                     mk, composed_out + b0 * comp_bs, bb, H, W, flags, packed_bs);
    }
    if (pair && pair_join(c, (hipStream_t)stream) && !rc) rc = 1;      // (joined after a failed half too: the streams stay ordered)
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
  flags &= ~SE_FLAG_RAW_FINE;      // se_fill_window_u8 only
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
                           ws_bytes, B, H, W, flags & ~(SE_FLAG_GRAPH | SE_FLAG_RAW_FINE), lock_u8);
}

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
  if (device_enter(c)) return 1;
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
  if (device_enter(c)) return 1;
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

}  // extern "C"
