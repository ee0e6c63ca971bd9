// The editing sessions' encoders behind include/sketchedit_png.h, sketchedit_jpg.h and sketchedit_jpg2.h: the host halves of
// the device PNG and JPEG encoders (kernels: se_png.hip, se_jpg.hip).
#include "../../include/sketchedit_png.h"
#include "../../include/sketchedit_jpg.h"
#include "../../include/sketchedit_jpg2.h"
#include "se_host.h"

using namespace se;

// ====================================================================================================
extern "C" {

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
  const size_t on = (size_t)B * cap, zn = (size_t)B * sizeof(unsigned long long);
  for (int i = 0; i < B; ++i) {
    const unsigned char* f = wins[i].frame_u8;
    const size_t fn = (size_t)wins[i].Hi * wins[i].Wi * 3;
    if (overlaps(out, on, f, fn)) return fail(c, "out overlaps the frame of wins[%d]", i);
    if (overlaps(sizes_out, zn, f, fn)) return fail(c, "sizes_out overlaps the frame of wins[%d]", i);
    if (overlaps(workspace, need, f, fn)) return fail(c, "workspace overlaps the frame of wins[%d]", i);
  }
  if (overlaps(out, on, workspace, need)) return fail(c, "out overlaps the workspace");
  if (overlaps(out, on, sizes_out, zn)) return fail(c, "out overlaps sizes_out");
  if (overlaps(sizes_out, zn, workspace, need)) return fail(c, "sizes_out overlaps the workspace");
  if (device_enter(c)) return 1;
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

struct Span { const void* p; size_t n; const char* name; };       // a byte range of the call, named for the refusal

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
  std::vector<Span> dst = {{out, (size_t)B * cap, "out"},
                           {sizes_out, (size_t)B * sizeof(unsigned long long), "sizes_out"},
                           {workspace, need, "the workspace"}};
  if (opt_) dst.push_back({tables_out, (size_t)B * SE_JPG_TABLE_RECORD_BYTES, "tables_out"});
  for (size_t i = 0; i < srcs.size(); ++i)
    for (const Span& d : dst)
      if (overlaps(d.p, d.n, srcs[i].p, srcs[i].n)) {
        char what[64];
        snprintf(what, sizeof what, src_fmt, (int)i);
        return fail(c, "%s overlaps %s", d.name, what);
      }
  for (size_t i = 0; i < dst.size(); ++i)
    for (size_t j = i + 1; j < dst.size(); ++j)
      if (overlaps(dst[i].p, dst[i].n, dst[j].p, dst[j].n)) return fail(c, "%s overlaps %s", dst[i].name, dst[j].name);
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
    srcs.push_back({wins[i].frame_u8, (size_t)wins[i].Hi * wins[i].Wi * 3, nullptr});
  if (jpg2_check(c, B, flags, out, cap, se_jpg2_bound(hs, ws, flags), sizes_out, tables_out, workspace, workspace_bytes, jpg2_need(L), srcs,
                 "the frame of wins[%d]"))
    return 1;
  if (device_enter(c)) return 1;
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
  const std::vector<Span> srcs = {{coef, (size_t)B * R * nblk * 128, nullptr}};
  if (jpg2_check(c, B, flags, out, cap, (size_t)R * jpg_row_bound(nblk, flags), sizes_out, tables_out, workspace, workspace_bytes, jpg2_need(L),
                 srcs, "coef"))
    return 1;
  if (device_enter(c)) return 1;
  const hipStream_t st = (hipStream_t)stream;
  void* blk[5];
  if (jpg2_blocks(c, workspace, L, st, blk)) return 1;
  return jpg2_code(c, B, R, nblk, flags, coef, blk, out, cap, sizes_out, tables_out, st);
}

}  // extern "C"
