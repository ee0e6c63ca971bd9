// Measurement and test support behind include/sketchedit_hip.h: the in-library profiler's report, the developer switches, and
// the per-op entries the unit tests call (one gated conv, the attention, the kernels between the convolutions).
#include "se_host.h"
#include "se_s2poly.h"

using namespace se;

// ====================================================================================================
extern "C" {

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
// ... and one derived, read-only entry: "SE_PAIR_RULE:B,H,W,exec_flags" answers pair_rule (se_host.h) for a pass of B images --
// 1 two half-batch chains, 0 one chain -- from the arguments and SE_PAIR_MIN_PIXELS alone: no ctx, no device (the set of
// exported names is fixed; the query rides on the entry that reads the table the rule reads)
int se_debug_get_option(const char* name, int* value) {
  static const char q[] = "SE_PAIR_RULE:";
  if (name && value && !strncmp(name, q, sizeof q - 1)) {
    int B = 0, H = 0, W = 0, flags = 0, end = 0;
    if (sscanf(name + sizeof q - 1, "%d,%d,%d,%d%n", &B, &H, &W, &flags, &end) != 4 || name[sizeof q - 1 + end] || B < 1 || H < 1 || W < 1) return 1;
    *value = pair_rule(B, H, W, flags) ? 1 : 0;
    return 0;
  }
  // ... and two for the polyphase form (se_s2poly.h): an entry of its 1-D tables, and a float of the image its packer builds for
  // the probe layer of the header (built once per width and kept)
  static const char qt[] = "SE_S2POLY_TABLE:", qp[] = "SE_S2POLY_PACK:";
  if (name && value && !strncmp(name, qt, sizeof qt - 1)) {
    int q = -1, j = -1, end = 0;
    if (sscanf(name + sizeof qt - 1, "%d,%d%n", &q, &j, &end) != 2 || name[sizeof qt - 1 + end] || q < 0 || q > 4 || j < 0 || j > 6) return 1;
    *value = j == 0 ? s2poly_src_a(q) : j == 1 ? s2poly_src_b(q) : j < 5 ? s2poly_wcoef(q, j - 2) : s2poly_fold(q, j - 5);
    return 0;
  }
  if (name && value && !strncmp(name, qp, sizeof qp - 1)) {
    int cout = 0, end = 0;
    long long i = -1;
    if (sscanf(name + sizeof qp - 1, "%d,%lld%n", &cout, &i, &end) != 2 || name[sizeof qp - 1 + end] || (cout != 96 && cout != 192) || i < 0) return 1;
    static std::mutex mu;
    static std::vector<float> kept[2];
    std::lock_guard<std::mutex> lk(mu);
    std::vector<float>& all = kept[cout == 192];
    if (all.empty()) {
      auto probe = [](long long n) { return (float)((7919 * n) % 2053 - 1026) / 1024.f; };
      std::vector<float> w((size_t)cout * 48 * 9), b(cout), bias;
      for (size_t n = 0; n < w.size(); ++n) w[n] = probe((long long)n);
      for (int n = 0; n < cout; ++n) b[n] = probe(10007 + n);
      if (!s2poly_pack_host(w.data(), b.data(), cout, all, bias)) return 1;
      all.insert(all.end(), bias.begin(), bias.end());
    }
    if ((size_t)i >= all.size()) return 1;
    memcpy(value, &all[(size_t)i], sizeof(int));
    return 0;
  }
  return opt_get(name, value);
}
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
