// The editing sessions' window entries behind include/sketchedit_hip.h, sketchedit_feather.h and sketchedit_fill.h: the
// se_window records and their ring, window edits at the frame's and at a working size, locked regions, the feathered paste,
// fills of a painted region, the undo journal, and the sketch's tiles and strokes (kernels: se_window.hip, se_feather.hip,
// se_fill.hip).
#include "../../include/sketchedit_feather.h"
#include "../../include/sketchedit_fill.h"
#include "se_host.h"

using namespace se;

// ---- editing sessions: window edits of a resident frame (se_window.hip) ------------------------------
namespace se {

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

}  // namespace se

namespace {

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
    const size_t ln = (size_t)wins[i].Hi * wins[i].Wi;
    for (int j = 0; j < B; ++j)
      if (overlaps(locks[i], ln, wins[j].frame_u8, (size_t)wins[j].Hi * wins[j].Wi * 3)) return fail(c, "locks[%d] overlaps the frame of wins[%d]", i, j);
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

// ====================================================================================================
extern "C" {

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
  if (device_enter(c)) return 1;
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
// SE_FLAG_RAW_FINE in flags (se_fill_window_u8 alone lets it through): rgb8 is the quantised `fine`, uncomposed.
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
  flags &= ~(SE_FLAG_GRAPH | SE_FLAG_PACKED_OUT | SE_FLAG_RAW_FINE);
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
  for (int i = 0; i < B; ++i) {
    const unsigned char* k0 = keeps[i];
    const size_t kn = (size_t)wins[i].Hi * wins[i].Wi;
    for (int j = 0; j < B; ++j) {
      const size_t pn = (size_t)wins[j].Hi * wins[j].Wi;
      if (overlaps(k0, kn, wins[j].frame_u8, 3 * pn)) return fail(c, "keeps[%d] overlaps the frame of wins[%d]", i, j);
      if (overlaps(k0, kn, holes[j], pn)) return fail(c, "keeps[%d] overlaps holes[%d]", i, j);
      if (locks && locks[j] && overlaps(k0, kn, locks[j], pn)) return fail(c, "keeps[%d] overlaps locks[%d]", i, j);
      if (j <= i || !overlaps(k0, kn, keeps[j], pn)) continue;
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
    for (int j = 0; j < B; ++j) {
      if (overlaps(slots[i], bytes, wins[j].frame_u8, (size_t)wins[j].Hi * wins[j].Wi * 3)) return fail(c, "slots[%d] overlaps the frame of wins[%d]", i, j);
      if (j > i && overlaps(slots[i], bytes, slots[j], bytes)) return fail(c, "slots[%d] and slots[%d] overlap", i, j);
    }
  }
  if (swap && win_check_disjoint(c, wins, B, hs, ws)) return 1;
  if (device_enter(c)) return 1;
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
  if (device_enter(c)) return 1;
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
  if (overlaps(segs, (size_t)N * 5 * sizeof(int), sketch_out, (size_t)B * hs * ws)) return fail(c, "segs overlaps sketch_out");
  if (device_enter(c)) return 1;
  const hipStream_t st = (hipStream_t)stream;
  const se_window* d = win_put(c, st, recs.data(), 2 * B);
  if (!d) return 1;
  HIPCHK(c, launch_sketch_strokes(d, B, hs, ws, segs, nseg_sum, sketch_out, st));
  return 0;
}

}  // extern "C"
