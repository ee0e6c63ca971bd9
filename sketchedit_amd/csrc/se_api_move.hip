// The editing sessions' move entries behind include/sketchedit_move.h: the drop of a lifted selection and the shift of its plane
// (kernels: se_move.hip); and behind include/sketchedit_warp.h the drop through an affine map and the warp
// of the plane (kernels: se_warp.hip); and behind include/sketchedit_filter.h the blur and the mosaic of a
// selection (kernels: se_filter.hip); and behind include/sketchedit_adjust.h the tone and colour of a selection,
// the histogram and the table made of it (kernels: se_adjust.hip); and behind include/sketchedit_blend.h the
// seamless drop (kernels: se_blend.hip); and behind include/sketchedit_canvas.h the canvas of a session
// (kernels: se_canvas.hip).
#include "../../include/sketchedit_adjust.h"
#include "../../include/sketchedit_blend.h"
#include "../../include/sketchedit_canvas.h"
#include "../../include/sketchedit_filter.h"
#include "../../include/sketchedit_move.h"
#include "../../include/sketchedit_warp.h"
#include "se_host.h"

using namespace se;

// ====================================================================================================
extern "C" {

// Every check on the host, then ONE launch that writes the caller's frame or plane directly: no workspace, nothing for
// SE_TEST_POISON to fill.
namespace {

// The frame's size.  What the launches take: plane_shift walks Hi Wi / 4 dwords, 256 to a workgroup, along grid.x (< 2^31
// workgroups); move_drop's grid is the destination rectangle's 64 x 16 tiles, at most (Wi + 63) / 64 along x and (Hi + 15) / 16
// along y, where a grid holds 65 535.
int move_check_frame(se_ctx* c, int Hi, int Wi) {
  if (Hi < 16 || Wi < 16) return fail(c, "bad Hi=%d Wi=%d (a frame is at least 16 x 16)", Hi, Wi);
  if ((Hi + 15) / 16 > 65535 || (long long)Hi * Wi / 1024 >= (1ll << 31))
    return fail(c, "move: Hi=%d Wi=%d is more than one launch takes", Hi, Wi);
  return 0;
}

// the box against the rectangle (ry0, rx0, rh, rw) that must hold it ...
int move_check_box(se_ctx* c, int by0, int bx0, int by1, int bx1, int ry0, int rx0, int rh, int rw, const char* holder) {
  if (by1 <= by0 || bx1 <= bx0) return fail(c, "bad box (%d, %d, %d, %d): a box (by0, bx0, by1, bx1) is half open and not empty", by0, bx0, by1, bx1);
  if (by0 < ry0 || bx0 < rx0 || by1 > ry0 + rh || bx1 > rx0 + rw)
    return fail(c, "the box (%d, %d, %d, %d) lies outside the %s (y0=%d x0=%d, %d x %d)", by0, bx0, by1, bx1, holder, ry0, rx0, rh, rw);
  return 0;
}

// ... the offset and the flip of a move ...
int move_check_offset(se_ctx* c, int dy, int dx, int flip) {
  if (dy < -SE_MOVE_MAX_OFFSET || dy > SE_MOVE_MAX_OFFSET) return fail(c, "bad dy=%d (|dy| <= %d)", dy, SE_MOVE_MAX_OFFSET);
  if (dx < -SE_MOVE_MAX_OFFSET || dx > SE_MOVE_MAX_OFFSET) return fail(c, "bad dx=%d (|dx| <= %d)", dx, SE_MOVE_MAX_OFFSET);
  if (flip < 0 || flip > 3) return fail(c, "bad flip=%d (0 .. 3)", flip);
  return 0;
}

// ... and the six values of a warp's inverse map (a host pointer)
int warp_check_map(se_ctx* c, const long long* m) {
  if (!m) return fail(c, "null pointer argument: m");
  static const char* const names[6] = {"ayy", "ayx", "ay0", "axy", "axx", "ax0"};
  for (int i = 0; i < 6; ++i) {
    const bool tr = i == 2 || i == 5;
    const long long lim = tr ? SE_WARP_MAX_TRANSLATION : (long long)SE_WARP_MAX_COEF;
    if (m[i] < -lim || m[i] > lim)
      return fail(c, "bad m: %s=%lld (a %s is at most %lld in magnitude)", names[i], m[i], tr ? "translation" : "coefficient", lim);
  }
  return 0;
}

// what every entry that takes a lift shares, in two steps: the frame, the lift and the box inside it ...
int lift_check_shape(se_ctx* c, const unsigned char* frame_u8, int Hi, int Wi, const unsigned char* lift, int ly0, int lx0, int lh, int lw,
                     const unsigned char* sel_u8, int by0, int bx0, int by1, int bx1) {
  if (!frame_u8) return fail(c, "null pointer argument: frame_u8");
  if (!lift) return fail(c, "null pointer argument: lift");
  if (!sel_u8) return fail(c, "null pointer argument: sel_u8");
  if (move_check_frame(c, Hi, Wi)) return 1;
  if (lh < 16 || lw < 16) return fail(c, "bad lift rectangle lh=%d lw=%d (a side is at least 16)", lh, lw);
  if (ly0 < 0 || lx0 < 0 || lh > Hi || lw > Wi || ly0 > Hi - lh || lx0 > Wi - lw)
    return fail(c, "the lift rectangle (ly0=%d lx0=%d, %d x %d) lies outside the frame (Hi=%d Wi=%d)", ly0, lx0, lh, lw, Hi, Wi);
  if (!aligned_to(lift, 16)) return fail(c, "lift must be 16-byte aligned");
  return move_check_box(c, by0, bx0, by1, bx1, ly0, lx0, lh, lw, "lift rectangle");
}

// ... and the lift and the planes against the frame's bytes
int lift_check_overlaps(se_ctx* c, const unsigned char* frame_u8, int Hi, int Wi, const unsigned char* lift, int lh, int lw,
                        const unsigned char* sel_u8, const unsigned char* lock_u8) {
  const size_t pn = (size_t)Hi * Wi, lpitch = ((size_t)3 * lw + 15) & ~(size_t)15, ln = (size_t)lh * lpitch;
  if (overlaps(lift, ln, frame_u8, 3 * pn)) return fail(c, "lift overlaps frame_u8");
  if (overlaps(sel_u8, pn, frame_u8, 3 * pn)) return fail(c, "sel_u8 overlaps frame_u8");
  if (lock_u8 && overlaps(lock_u8, pn, frame_u8, 3 * pn)) return fail(c, "lock_u8 overlaps frame_u8");
  return 0;
}

// what both filters share: the above, the amount and the feather; `grow` = the blur's radius (0 for the mosaic): the lift rectangle
// holds the box grown by it and clipped to the frame
int filter_check(se_ctx* c, const unsigned char* frame_u8, int Hi, int Wi, const unsigned char* lift, int ly0, int lx0, int lh, int lw,
                 const unsigned char* sel_u8, const unsigned char* lock_u8, int by0, int bx0, int by1, int bx1, int grow, int amount, int feather) {
  if (lift_check_shape(c, frame_u8, Hi, Wi, lift, ly0, lx0, lh, lw, sel_u8, by0, bx0, by1, bx1)) return 1;
  if (amount < SE_FILTER_MIN_AMOUNT || amount > SE_FILTER_MAX_AMOUNT)
    return fail(c, "bad amount=%d (%d .. %d, Q8)", amount, SE_FILTER_MIN_AMOUNT, SE_FILTER_MAX_AMOUNT);
  if (feather < 0 || feather > SE_FILTER_MAX_FEATHER) return fail(c, "bad feather=%d (0 .. %d)", feather, SE_FILTER_MAX_FEATHER);
  const int gy0 = by0 - grow > 0 ? by0 - grow : 0, gx0 = bx0 - grow > 0 ? bx0 - grow : 0;
  const int gy1 = by1 + grow < Hi ? by1 + grow : Hi, gx1 = bx1 + grow < Wi ? bx1 + grow : Wi;
  if (gy0 < ly0 || gx0 < lx0 || gy1 > ly0 + lh || gx1 > lx0 + lw)
    return fail(c, "the lift rectangle (ly0=%d lx0=%d, %d x %d) does not contain the box (%d, %d, %d, %d) grown by radius=%d and clipped to the frame",
                ly0, lx0, lh, lw, by0, bx0, by1, bx1, grow);
  return lift_check_overlaps(c, frame_u8, Hi, Wi, lift, lh, lw, sel_u8, lock_u8);
}

}  // namespace

int se_move_drop_u8(se_ctx* c, void* stream, unsigned char* frame_u8, int Hi, int Wi, const unsigned char* lift, int ly0, int lx0, int lh,
                    int lw, const unsigned char* sel_u8, const unsigned char* lock_u8, int by0, int bx0, int by1, int bx1, int dy, int dx,
                    int flip, int radius) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (lift_check_shape(c, frame_u8, Hi, Wi, lift, ly0, lx0, lh, lw, sel_u8, by0, bx0, by1, bx1)) return 1;
  if (move_check_offset(c, dy, dx, flip)) return 1;
  if (radius < 0 || radius > SE_MOVE_MAX_RADIUS) return fail(c, "bad radius=%d (0 .. %d)", radius, SE_MOVE_MAX_RADIUS);
  if (lift_check_overlaps(c, frame_u8, Hi, Wi, lift, lh, lw, sel_u8, lock_u8)) return 1;
  if (device_enter(c)) return 1;
  const int lpitch = (3 * lw + 15) & ~15;
  HIPCHK(c, launch_move_drop(frame_u8, Hi, Wi, lift, ly0, lx0, lw, lpitch, sel_u8, lock_u8, by0, bx0, by1, bx1, dy, dx, flip, radius,
                             (hipStream_t)stream));
  return 0;
}

size_t se_move_blend_u8_workspace_bytes(int box_h, int box_w) {
  if (box_h < 1 || box_w < 1 || box_h > SE_BLEND_MAX_SIDE || box_w > SE_BLEND_MAX_SIDE) return 0;
  return blend_workspace_bytes(box_h + 2, box_w + 2);
}

// The plain drop's checks, then the workspace's; the launches are a function of the rectangle's size alone (se_blend.hip).  The
// workspace is the one scratch region: SE_TEST_POISON fills it, and the kernels write every record in front of its first read.
int se_move_blend_u8(se_ctx* c, void* stream, unsigned char* frame_u8, int Hi, int Wi, const unsigned char* lift, int ly0, int lx0, int lh,
                     int lw, const unsigned char* sel_u8, const unsigned char* lock_u8, int by0, int bx0, int by1, int bx1, int dy, int dx,
                     int flip, void* workspace, size_t workspace_bytes) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (lift_check_shape(c, frame_u8, Hi, Wi, lift, ly0, lx0, lh, lw, sel_u8, by0, bx0, by1, bx1)) return 1;
  if (move_check_offset(c, dy, dx, flip)) return 1;
  if (by1 - by0 > SE_BLEND_MAX_SIDE || bx1 - bx0 > SE_BLEND_MAX_SIDE)
    return fail(c, "the box (%d, %d, %d, %d) has a side above %d", by0, bx0, by1, bx1, SE_BLEND_MAX_SIDE);
  if (lift_check_overlaps(c, frame_u8, Hi, Wi, lift, lh, lw, sel_u8, lock_u8)) return 1;
  if (!workspace) return fail(c, "null pointer argument: workspace");
  const size_t need = se_move_blend_u8_workspace_bytes(by1 - by0, bx1 - bx0), pn = (size_t)Hi * Wi;
  if (workspace_bytes < need) return fail(c, "workspace too small: %zu bytes, need %zu", workspace_bytes, need);
  if (!aligned_to(workspace, 16)) return fail(c, "workspace must be 16-byte aligned");
  const size_t ln = (size_t)lh * (((size_t)3 * lw + 15) & ~(size_t)15);
  if (overlaps(workspace, need, frame_u8, 3 * pn)) return fail(c, "workspace overlaps frame_u8");
  if (overlaps(workspace, need, lift, ln)) return fail(c, "workspace overlaps lift");
  if (overlaps(workspace, need, sel_u8, pn)) return fail(c, "workspace overlaps sel_u8");
  if (lock_u8 && overlaps(workspace, need, lock_u8, pn)) return fail(c, "workspace overlaps lock_u8");
  if (device_enter(c)) return 1;
  const hipStream_t st = (hipStream_t)stream;
  const int lpitch = (3 * lw + 15) & ~15;
  const bool lands = (by0 + dy > 0 ? by0 + dy : 0) < (by1 + dy < Hi ? by1 + dy : Hi) && (bx0 + dx > 0 ? bx0 + dx : 0) < (bx1 + dx < Wi ? bx1 + dx : Wi);
  if (lands && poison(c, workspace, need, st)) return 1;             // the whole box outside the frame: nothing is enqueued
  HIPCHK(c, launch_move_blend(frame_u8, Hi, Wi, lift, ly0, lx0, lh, lw, lpitch, sel_u8, lock_u8, by0, bx0, by1, bx1, dy, dx, flip, workspace, st));
  return 0;
}

int se_plane_shift_u8(se_ctx* c, void* stream, const unsigned char* sel_u8, int Hi, int Wi, int by0, int bx0, int by1, int bx1, int dy,
                      int dx, int flip, unsigned char* plane_out) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (!sel_u8) return fail(c, "null pointer argument: sel_u8");
  if (!plane_out) return fail(c, "null pointer argument: plane_out");
  if (move_check_frame(c, Hi, Wi)) return 1;
  if (move_check_box(c, by0, bx0, by1, bx1, 0, 0, Hi, Wi, "frame")) return 1;
  if (move_check_offset(c, dy, dx, flip)) return 1;
  const size_t pn = (size_t)Hi * Wi;
  if (overlaps(plane_out, pn, sel_u8, pn)) return fail(c, "plane_out overlaps sel_u8");
  if (device_enter(c)) return 1;
  HIPCHK(c, launch_plane_shift(sel_u8, Hi, Wi, by0, bx0, by1, bx1, dy, dx, flip, plane_out, (hipStream_t)stream));
  return 0;
}

// The canvas: out of place, every check on the host, ONE launch that writes every byte of `out`.  What the launch takes: canvas_map
// walks C Hn Wn / 4 < 2^29 dwords, 256 to a workgroup; canvas_turn's grid is at most 1024 x 512 tiles.
int se_canvas_u8(se_ctx* c, void* stream, const unsigned char* in, int Hi, int Wi, int C, unsigned char* out, int Hn, int Wn, int oy, int ox,
                     int orient, int pad_mode, unsigned pad_rgb) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (!out) return fail(c, "null pointer argument: out");
  if (C != 1 && C != 3) return fail(c, "bad C=%d (1: a plane, 3: a frame)", C);
  if (!in && C != 1) return fail(c, "null pointer argument: in (only a plane, C = 1, may be NULL)");
  if (orient < 0 || orient > 7) return fail(c, "bad orient=%d (0 .. 7)", orient);
  if (pad_mode != SE_CANVAS_EDGE && pad_mode != SE_CANVAS_REFLECT && pad_mode != SE_CANVAS_CONSTANT)
    return fail(c, "bad pad_mode=%d (SE_CANVAS_EDGE, _REFLECT or _CONSTANT)", pad_mode);
  if (Hi < 1 || Wi < 1 || Hi > SE_CANVAS_MAX_SIDE || Wi > SE_CANVAS_MAX_SIDE || (long long)C * Hi * Wi >= (1ll << 31))
    return fail(c, "bad Hi=%d Wi=%d (1 .. %d, C Hi Wi < 2^31)", Hi, Wi, SE_CANVAS_MAX_SIDE);
  if (Hn < 1 || Wn < 1 || Hn > SE_CANVAS_MAX_SIDE || Wn > SE_CANVAS_MAX_SIDE || (long long)C * Hn * Wn >= (1ll << 31))
    return fail(c, "bad Hn=%d Wn=%d (1 .. %d, C Hn Wn < 2^31)", Hn, Wn, SE_CANVAS_MAX_SIDE);
  if (oy < -SE_CANVAS_MAX_OFFSET || oy > SE_CANVAS_MAX_OFFSET) return fail(c, "bad oy=%d (|oy| <= %d)", oy, SE_CANVAS_MAX_OFFSET);
  if (ox < -SE_CANVAS_MAX_OFFSET || ox > SE_CANVAS_MAX_OFFSET) return fail(c, "bad ox=%d (|ox| <= %d)", ox, SE_CANVAS_MAX_OFFSET);
  if (in && overlaps(in, (size_t)C * Hi * Wi, out, (size_t)C * Hn * Wn)) return fail(c, "out overlaps in");
  if (device_enter(c)) return 1;
  HIPCHK(c, launch_canvas(in, Hi, Wi, C, out, Hn, Wn, oy, ox, orient, pad_mode, pad_rgb, (hipStream_t)stream));
  return 0;
}

int se_warp_drop_u8(se_ctx* c, void* stream, unsigned char* frame_u8, int Hi, int Wi, const unsigned char* lift, int ly0, int lx0, int lh,
                    int lw, const unsigned char* sel_u8, const unsigned char* lock_u8, int by0, int bx0, int by1, int bx1, int ry0, int rx0,
                    int rh, int rw, const long long* m) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (lift_check_shape(c, frame_u8, Hi, Wi, lift, ly0, lx0, lh, lw, sel_u8, by0, bx0, by1, bx1)) return 1;
  if (warp_check_map(c, m)) return 1;
  if (rh <= 0 || rw <= 0) return fail(c, "bad destination rectangle rh=%d rw=%d: it is not empty", rh, rw);
  if (ry0 < 0 || rx0 < 0 || rh > Hi || rw > Wi || ry0 > Hi - rh || rx0 > Wi - rw)
    return fail(c, "the destination rectangle (ry0=%d rx0=%d, %d x %d) lies outside the frame (Hi=%d Wi=%d)", ry0, rx0, rh, rw, Hi, Wi);
  if (lift_check_overlaps(c, frame_u8, Hi, Wi, lift, lh, lw, sel_u8, lock_u8)) return 1;
  if (device_enter(c)) return 1;
  const int lpitch = (3 * lw + 15) & ~15;
  HIPCHK(c, launch_warp_drop(frame_u8, Hi, Wi, lift, ly0, lx0, lw, lpitch, sel_u8, lock_u8, by0, bx0, by1, bx1, ry0, rx0, rh, rw, m,
                             (hipStream_t)stream));
  return 0;
}

int se_plane_warp_u8(se_ctx* c, void* stream, const unsigned char* sel_u8, int Hi, int Wi, int by0, int bx0, int by1, int bx1,
                     const long long* m, unsigned char* plane_out) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (!sel_u8) return fail(c, "null pointer argument: sel_u8");
  if (!plane_out) return fail(c, "null pointer argument: plane_out");
  if (move_check_frame(c, Hi, Wi)) return 1;
  if (move_check_box(c, by0, bx0, by1, bx1, 0, 0, Hi, Wi, "frame")) return 1;
  if (warp_check_map(c, m)) return 1;
  const size_t pn = (size_t)Hi * Wi;
  if (overlaps(plane_out, pn, sel_u8, pn)) return fail(c, "plane_out overlaps sel_u8");
  if (device_enter(c)) return 1;
  HIPCHK(c, launch_plane_warp(sel_u8, Hi, Wi, by0, bx0, by1, bx1, m, plane_out, (hipStream_t)stream));
  return 0;
}

int se_filter_blur_u8(se_ctx* c, void* stream, unsigned char* frame_u8, int Hi, int Wi, const unsigned char* lift, int ly0, int lx0, int lh,
                      int lw, const unsigned char* sel_u8, const unsigned char* lock_u8, int by0, int bx0, int by1, int bx1, const int* taps,
                      int radius, int amount, int feather) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (!taps) return fail(c, "null pointer argument: taps");
  if (radius < 1 || radius > SE_FILTER_MAX_RADIUS) return fail(c, "bad radius=%d (1 .. %d)", radius, SE_FILTER_MAX_RADIUS);
  long long sum = 0;
  for (int k = 0; k <= radius; ++k) {
    if (taps[k] < 0) return fail(c, "bad taps: taps[%d]=%d is negative", k, taps[k]);
    sum += k ? 2ll * taps[k] : (long long)taps[k];
  }
  if (sum != SE_FILTER_ONE) return fail(c, "bad taps: taps[0] + 2 (taps[1] + .. + taps[%d]) = %lld, not %d", radius, sum, SE_FILTER_ONE);
  if (filter_check(c, frame_u8, Hi, Wi, lift, ly0, lx0, lh, lw, sel_u8, lock_u8, by0, bx0, by1, bx1, radius, amount, feather)) return 1;
  if (device_enter(c)) return 1;
  const int lpitch = (3 * lw + 15) & ~15;
  HIPCHK(c, launch_filter_blur(frame_u8, Hi, Wi, lift, ly0, lx0, lw, lpitch, sel_u8, lock_u8, by0, bx0, by1, bx1, taps, radius, amount, feather,
                               (hipStream_t)stream));
  return 0;
}

int se_filter_mosaic_u8(se_ctx* c, void* stream, unsigned char* frame_u8, int Hi, int Wi, const unsigned char* lift, int ly0, int lx0, int lh,
                        int lw, const unsigned char* sel_u8, const unsigned char* lock_u8, int by0, int bx0, int by1, int bx1, int cell,
                        int amount, int feather) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (cell < 2 || cell > SE_FILTER_MAX_CELL) return fail(c, "bad cell=%d (2 .. %d)", cell, SE_FILTER_MAX_CELL);
  if (filter_check(c, frame_u8, Hi, Wi, lift, ly0, lx0, lh, lw, sel_u8, lock_u8, by0, bx0, by1, bx1, 0, amount, feather)) return 1;
  if (device_enter(c)) return 1;
  const int lpitch = (3 * lw + 15) & ~15;
  HIPCHK(c, launch_filter_mosaic(frame_u8, Hi, Wi, lift, ly0, lx0, lw, lpitch, sel_u8, lock_u8, by0, bx0, by1, bx1, cell, amount, feather,
                                 (hipStream_t)stream));
  return 0;
}

int se_adjust_u8(se_ctx* c, void* stream, unsigned char* frame_u8, int Hi, int Wi, const unsigned char* lift, int ly0, int lx0, int lh, int lw,
                 const unsigned char* sel_u8, const unsigned char* lock_u8, int by0, int bx0, int by1, int bx1, const unsigned char* lut,
                 const int* matrix, int amount, int feather) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (lift_check_shape(c, frame_u8, Hi, Wi, lift, ly0, lx0, lh, lw, sel_u8, by0, bx0, by1, bx1)) return 1;
  for (int k = 0; matrix && k < 12; ++k) {
    const int lim = k < 9 ? SE_ADJUST_MAX_COEF : SE_ADJUST_MAX_OFFSET;
    if (matrix[k] < -lim || matrix[k] > lim)
      return fail(c, "bad matrix: matrix[%d]=%d (%s at most %d in magnitude)", k, matrix[k], k < 9 ? "a coefficient is" : "an offset is", lim);
  }
  if (amount < 0 || amount > SE_ADJUST_ONE_AMOUNT) return fail(c, "bad amount=%d (0 .. %d, Q8)", amount, SE_ADJUST_ONE_AMOUNT);
  if (feather < 0 || feather > SE_ADJUST_MAX_FEATHER) return fail(c, "bad feather=%d (0 .. %d)", feather, SE_ADJUST_MAX_FEATHER);
  if (lift_check_overlaps(c, frame_u8, Hi, Wi, lift, lh, lw, sel_u8, lock_u8)) return 1;
  if (lut && overlaps(lut, 768, frame_u8, (size_t)3 * Hi * Wi)) return fail(c, "lut overlaps frame_u8");
  if (device_enter(c)) return 1;
  const int lpitch = (3 * lw + 15) & ~15;
  HIPCHK(c, launch_adjust(frame_u8, Hi, Wi, lift, ly0, lx0, lw, lpitch, sel_u8, lock_u8, by0, bx0, by1, bx1, lut, matrix, amount, feather,
                          (hipStream_t)stream));
  return 0;
}

size_t se_adjust_hist_u8_workspace_bytes(int Hi, int Wi) {
  if (Hi < 16 || Wi < 16) return 0;
  return (size_t)adjust_hist_groups(Hi, Wi) * 4096;
}

int se_adjust_hist_u8(se_ctx* c, void* stream, const unsigned char* frame_u8, int Hi, int Wi, const unsigned char* sel_u8, int by0, int bx0,
                      int by1, int bx1, unsigned int* hist, void* workspace, size_t workspace_bytes) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (!frame_u8) return fail(c, "null pointer argument: frame_u8");
  if (!hist) return fail(c, "null pointer argument: hist_dev");
  if (!workspace) return fail(c, "null pointer argument: workspace");
  if (move_check_frame(c, Hi, Wi)) return 1;
  if (move_check_box(c, by0, bx0, by1, bx1, 0, 0, Hi, Wi, "frame")) return 1;
  if (!aligned_to(hist, 4)) return fail(c, "hist_dev must be 4-byte aligned");
  const size_t need = se_adjust_hist_u8_workspace_bytes(Hi, Wi), pn = (size_t)Hi * Wi;
  if (workspace_bytes < need) return fail(c, "workspace too small: %zu bytes, need %zu", workspace_bytes, need);
  if (!aligned_to(workspace, 256)) return fail(c, "workspace must be 256-byte aligned");
  if (overlaps(hist, 4096, frame_u8, 3 * pn)) return fail(c, "hist_dev overlaps frame_u8");
  if (overlaps(workspace, need, frame_u8, 3 * pn)) return fail(c, "workspace overlaps frame_u8");
  if (overlaps(hist, 4096, workspace, need)) return fail(c, "hist_dev overlaps the workspace");
  if (sel_u8 && overlaps(hist, 4096, sel_u8, pn)) return fail(c, "hist_dev overlaps sel_u8");
  if (sel_u8 && overlaps(workspace, need, sel_u8, pn)) return fail(c, "workspace overlaps sel_u8");
  if (device_enter(c)) return 1;
  const hipStream_t st = (hipStream_t)stream;
  if (poison(c, workspace, need, st)) return 1;
  HIPCHK(c, launch_hist_tiles(frame_u8, Wi, sel_u8, by0, bx0, by1, bx1, (unsigned*)workspace, st));
  HIPCHK(c, launch_hist_sum((const unsigned*)workspace, adjust_hist_groups(by1 - by0, bx1 - bx0), hist, st));
  return 0;
}

int se_adjust_lut_u8(se_ctx* c, void* stream, const unsigned int* hist_src, const unsigned int* hist_ref, int mode, int which, int clip,
                     unsigned char* lut) {
  if (!c) return 1;
  std::lock_guard<std::mutex> lk(c->mu);
  if (!hist_src) return fail(c, "null pointer argument: hist_src_dev");
  if (!lut) return fail(c, "null pointer argument: lut_dev");
  if (mode != SE_ADJUST_STRETCH && mode != SE_ADJUST_EQUALIZE && mode != SE_ADJUST_MATCH) return fail(c, "bad mode=%d (SE_ADJUST_STRETCH, _EQUALIZE or _MATCH)", mode);
  if (which != SE_ADJUST_PER_CHANNEL && which != SE_ADJUST_LUMA) return fail(c, "bad which=%d (SE_ADJUST_PER_CHANNEL or _LUMA)", which);
  if (clip < 0 || clip > SE_ADJUST_MAX_CLIP) return fail(c, "bad clip=%d (0 .. %d per mille)", clip, SE_ADJUST_MAX_CLIP);
  if (mode == SE_ADJUST_MATCH && !hist_ref) return fail(c, "null pointer argument: hist_ref_dev (SE_ADJUST_MATCH takes a reference)");
  if (mode != SE_ADJUST_MATCH && hist_ref) return fail(c, "hist_ref_dev is for SE_ADJUST_MATCH only (mode=%d)", mode);
  if (!aligned_to(hist_src, 4)) return fail(c, "hist_src_dev must be 4-byte aligned");
  if (hist_ref && !aligned_to(hist_ref, 4)) return fail(c, "hist_ref_dev must be 4-byte aligned");
  if (overlaps(lut, 768, hist_src, 4096)) return fail(c, "lut_dev overlaps hist_src_dev");
  if (hist_ref && overlaps(lut, 768, hist_ref, 4096)) return fail(c, "lut_dev overlaps hist_ref_dev");
  if (device_enter(c)) return 1;
  HIPCHK(c, launch_adjust_lut(hist_src, hist_ref, mode, which, clip, lut, (hipStream_t)stream));
  return 0;
}

}  // extern "C"
