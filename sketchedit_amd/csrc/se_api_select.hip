// The editing sessions' selection entries behind include/sketchedit_select.h, sketchedit_lasso.h, sketchedit_modify.h and
// sketchedit_outline.h: selection by colour, lasso selections and their algebra, the modification of a selection's shape, and the
// outline of a selection (kernels: se_select.hip, se_lasso.hip, se_modify.hip, se_outline.hip).
#include "../../include/sketchedit_select.h"
#include "../../include/sketchedit_lasso.h"
#include "../../include/sketchedit_modify.h"
#include "../../include/sketchedit_outline.h"
#include "se_host.h"

using namespace se;

// ====================================================================================================
extern "C" {

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
  if (overlaps(state_u8, n, frame_u8, 3 * n)) return fail(c, "state_u8 overlaps frame_u8");
  if (device_enter(c)) return 1;
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
  if (overlaps(changed_out, (size_t)passes * sizeof(unsigned), state_u8, (size_t)Hi * Wi)) return fail(c, "changed_out overlaps state_u8");
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
  if (overlaps(plane_out, n, state_u8, n)) return fail(c, "plane_out overlaps state_u8");
  if (device_enter(c)) return 1;
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
  if (edges && N > 0 && overlaps(edges, (size_t)N * 4 * sizeof(int), plane_out, (size_t)Hi * Wi)) return fail(c, "edges overlaps plane_out");
  if (device_enter(c)) return 1;
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
  if (out != a && overlaps(out, n, a, n)) return fail(c, "out overlaps a (it may be a itself)");
  if (b && out != b && overlaps(out, n, b, n)) return fail(c, "out overlaps b (it may be b itself)");
  if (device_enter(c)) return 1;
  HIPCHK(c, launch_plane_combine(a, b, Hi, Wi, op, out, (hipStream_t)stream));
  return 0;
}

// ---- modify a selection's shape (include/sketchedit_modify.h) ------------------------------------------------
// Every check on the host, then ONE launch that writes the caller's plane directly: no workspace, nothing for SE_TEST_POISON to
// fill.
int se_plane_modify_u8(se_ctx* c, void* stream, const unsigned char* plane, int Hi, int Wi, int op, int radius, unsigned char* out) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (lasso_check_plane(c, Hi, Wi)) return 1;
  if (op < SE_MODIFY_EXPAND || op > SE_MODIFY_SMOOTH) return fail(c, "bad op=%d (0 .. 2)", op);
  if (radius < 1 || radius > SE_MODIFY_MAX_RADIUS) return fail(c, "bad radius=%d (1 .. %d)", radius, SE_MODIFY_MAX_RADIUS);
  if (!plane) return fail(c, "null pointer argument: plane");
  if (!out) return fail(c, "null pointer argument: out");
  const size_t n = (size_t)Hi * Wi;
  if (overlaps(out, n, plane, n)) return fail(c, "out overlaps plane (a tile reads the halo its neighbours store: not in place)");
  if (device_enter(c)) return 1;
  HIPCHK(c, launch_plane_modify(plane, Hi, Wi, op, radius, out, (hipStream_t)stream));
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
  if (en && overlaps(edges_out, en, plane, pn)) return fail(c, "edges_out overlaps plane");
  if (overlaps(info_out, in, plane, pn)) return fail(c, "info_out overlaps plane");
  if (overlaps(workspace, need, plane, pn)) return fail(c, "workspace overlaps plane");
  if (en && overlaps(edges_out, en, info_out, in)) return fail(c, "edges_out overlaps info_out");
  if (en && overlaps(edges_out, en, workspace, need)) return fail(c, "edges_out overlaps the workspace");
  if (overlaps(info_out, in, workspace, need)) return fail(c, "info_out overlaps the workspace");
  if (device_enter(c)) return 1;
  const hipStream_t st = (hipStream_t)stream;
  if (poison(c, workspace, need, st)) return 1;
  int* cnt = (int*)workspace;
  HIPCHK(c, launch_outline_count(plane, Hi, Wi, cnt, st));
  HIPCHK(c, launch_outline_scan(cnt, Hi, Wi, cap, info_out, st));
  if (cap > 0) HIPCHK(c, launch_outline_emit(plane, Hi, Wi, cnt, edges_out, cap, st));
  return 0;
}

}  // extern "C"
