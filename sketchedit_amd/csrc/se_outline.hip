// The outline of a selection (the definition is stated in include/sketchedit_outline.h and in plain numpy in
// tests/outline_util.py): the boundary runs of the pixels a plane selects, as records in the lasso's edge format.  Three
// integer-only kernels, plain vector loads and stores, no atomics, nothing polled or spun on, any alignment of the plane and any
// Wi; no byte outside the plane is read, none outside the written records, the two info words and the workspace is written.  The
// launch boundary is the only synchronisation: count -> scan -> emit, on one stream.
//
//  tile (count / emit):  one wave = one 64 x 64 tile (ragged at the right and bottom edges), select_flood's staging: lanes along
//           x, one ballot per row, give lane y the row mask S_y (byte != 0) of its tile; the rows above and below the tile are two
//           more ballots (zero outside the frame), the columns left and right one ballot each with lanes along y.  Rows:
//           N_y = S_y & ~S_{y-1}, (S)_y = S_y & ~S_{y+1}, the neighbours' masks by wave shuffles.  Columns: the 64 x 64 bit matrix
//           is transposed by 64 ballots (lane x keeps column x, bit y), then E_x = C_x & ~C_{x+1}, W_x = C_x & ~C_{x-1}.  In every
//           mask m a run starts at the bits of m & ~(m << 1); a lane's runs are in bit order and the lanes in row (column)
//           order, which is the definition's order within a kind.
//           count: the four run counts of the tile (wave sums of popcounts) go to the workspace, cnt[4 tile + kind].
//           emit:  the same masks again; a run's global index is the scanned cnt[4 tile + kind] + the lane's exclusive prefix of
//           the popcounts + its rank among the lane's starts.  Records with index < cap are stored (one 16-byte store where
//           edges_out is 16-byte aligned, else four dwords); indices ascend within a lane, so it stops at the first >= cap.
//  scan:    ONE workgroup of 256: the exclusive scan of the n = 4 tiles <= 65 536 counts IN PLACE -- a thread owns a contiguous
//           chunk, sums it, the sums are scanned (wave shuffles, the four waves' totals through LDS), and the thread walks its
//           chunk again, reading each count before it stores the offset in its place -- and info_out = {total, min(total, cap)}.
#include "../../include/sketchedit_hip.h"
#include "../../include/sketchedit_outline.h"
#include "se_device.h"
#include "se_kernels.h"

#include <cstdint>

namespace se {

namespace {

typedef unsigned long long u64;

// inclusive prefix sum over the wave's 64 lanes
__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d *= 2) {
    const int o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  return v;
}

__device__ __forceinline__ int run_starts(u64 m) { return __popcll(m & ~(m << 1)); }

// the lane's runs of mask m (bits along the run's axis, tile origin t0 there; `fixed` = the frame row of an N / S run, the frame
// column of an E / W run), stored from global index g on while g < cap
template <int KIND>
__device__ __forceinline__ void emit_runs(u64 m, int fixed, int t0, long long g, int cap, int* __restrict__ out, bool al16) {
  u64 st = m & ~(m << 1);
  const int f = 4 * fixed;
  while (st != 0 && g < cap) {
    const int a = __ffsll((long long)st) - 1;
    st &= st - 1;
    const u64 r = ~(m >> a);                                           // (r == 0 only for a == 0 and a full mask)
    const int len = r ? __ffsll((long long)r) - 1 : 64;
    const int p0 = 4 * (t0 + a), p1 = 4 * (t0 + a + len);
    int4 rec;
    if (KIND == 0) rec = make_int4(p0, f, p1, f);                      // N
    else if (KIND == 1) rec = make_int4(p1, f + 4, p0, f + 4);         // S
    else if (KIND == 2) rec = make_int4(f + 4, p0, f + 4, p1);         // E
    else rec = make_int4(f, p1, f, p0);                                // W
    int* dst = out + 4 * (size_t)g;                                    // (g < cap <= 2^24: inside the caller's cap records)
    if (al16) {
      *(int4*)dst = rec;
    } else {
      dst[0] = rec.x; dst[1] = rec.y; dst[2] = rec.z; dst[3] = rec.w;
    }
    ++g;
  }
}

// EMIT false: cnt[4 tile + k] <- the tile's run counts.  EMIT true: cnt holds their exclusive scan; the records are stored.
template <bool EMIT>
__global__ void __launch_bounds__(64) outline_tile_kernel(const unsigned char* __restrict__ plane, int Hi, int Wi, int ntx, int* __restrict__ cnt,
                                                          int* __restrict__ out, int cap) {
  const int lane = threadIdx.x;
  const int tile = (int)blockIdx.x;
  const int ty0 = (tile / ntx) * 64, tx0 = (tile % ntx) * 64;
  const int th = min(64, Hi - ty0), tw = min(64, Wi - tx0);           // the tile's rows and columns (>= 1)
  const bool col = lane < tw;
  const unsigned char* base = plane + (size_t)ty0 * Wi + tx0;         // the tile's first byte
  // the tile: lane y keeps row y
  u64 S = 0;
#pragma unroll 8
  for (int y = 0; y < 64; ++y) {
    unsigned v = 0;
    if (y < th && col) v = base[(size_t)y * Wi + lane];
    const u64 s = __ballot(v != 0);
    if (lane == y) S = s;
  }
  // the halo, zero outside the frame: the rows above and below (lanes along x), the columns left and right (lanes along y)
  unsigned va = 0, vb = 0, vl = 0, vr = 0;
  if (ty0 > 0 && col) va = (base - Wi)[lane];
  if (ty0 + th < Hi && col) vb = base[(size_t)th * Wi + lane];        // (then th == 64)
  if (lane < th) {
    if (tx0 > 0) vl = base[(long)lane * Wi - 1];
    if (tx0 + tw < Wi) vr = base[(long)lane * Wi + tw];               // (then tw == 64)
  }
  const u64 Sa = __ballot(va != 0), Sb = __ballot(vb != 0), Cl = __ballot(vl != 0), Cr = __ballot(vr != 0);
  // rows: lanes >= th hold S = 0, so the row under a ragged tile's last is unselected as it is
  u64 up = __shfl_up(S, 1, 64), dn = __shfl_down(S, 1, 64);
  if (lane == 0) up = Sa;
  if (lane == 63) dn = Sb;
  const u64 mN = S & ~up, mS = S & ~dn;
  // columns: lane x keeps column x, bit y
  u64 C = 0;
#pragma unroll 8
  for (int x = 0; x < 64; ++x) {
    const u64 c = __ballot(((S >> x) & 1ull) != 0);
    if (lane == x) C = c;
  }
  u64 lf = __shfl_up(C, 1, 64), rt = __shfl_down(C, 1, 64);
  if (lane == 0) lf = Cl;
  if (lane == 63) rt = Cr;
  const u64 mE = C & ~rt, mW = C & ~lf;
  const int iN = wave_incl_scan(run_starts(mN), lane), iS = wave_incl_scan(run_starts(mS), lane);
  const int iE = wave_incl_scan(run_starts(mE), lane), iW = wave_incl_scan(run_starts(mW), lane);
  if (!EMIT) {
    if (lane == 63) {
      int* c = cnt + 4 * (size_t)tile;
      c[0] = iN; c[1] = iS; c[2] = iE; c[3] = iW;
    }
  } else {
    const int* c = cnt + 4 * (size_t)tile;
    const bool al16 = ((uintptr_t)out & 15) == 0;
    emit_runs<0>(mN, ty0 + lane, tx0, (long long)c[0] + iN - run_starts(mN), cap, out, al16);
    emit_runs<1>(mS, ty0 + lane, tx0, (long long)c[1] + iS - run_starts(mS), cap, out, al16);
    emit_runs<2>(mE, tx0 + lane, ty0, (long long)c[2] + iE - run_starts(mE), cap, out, al16);
    emit_runs<3>(mW, tx0 + lane, ty0, (long long)c[3] + iW - run_starts(mW), cap, out, al16);
  }
}

__global__ void __launch_bounds__(256) outline_scan_kernel(int* __restrict__ cnt, int n, int cap, int* __restrict__ info) {
  __shared__ int s_wave[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int per = (n + 255) / 256;
  const int i0 = min(n, tid * per), i1 = min(n, i0 + per);            // the thread's chunk
  int sum = 0;
  for (int i = i0; i < i1; ++i) sum += cnt[i];
  const int incl = wave_incl_scan(sum, lane);
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  int at = incl - sum, total = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    at += w < wave ? s_wave[w] : 0;
    total += s_wave[w];
  }
  for (int i = i0; i < i1; ++i) {
    const int v = cnt[i];
    cnt[i] = at;
    at += v;
  }
  if (tid == 0) {
    info[0] = total;
    info[1] = min(total, cap);
  }
}

}  // namespace

hipError_t launch_outline_count(const unsigned char* plane, int Hi, int Wi, int* cnt, hipStream_t st) {
  const int ntx = (Wi + 63) / 64, nty = (Hi + 63) / 64;
  // bytes: the plane read once with the halo's share, 16 bytes of counts per tile
  set_launch_cost(0.0, (double)Hi * Wi * (1.0 + 4.0 / 64.0) + 16.0 * ntx * nty, "outline_count");
  set_launch_grid((long)ntx * nty);
  ProfScope ps_(st, PL_OUTLINE_COUNT);
  hipLaunchKernelGGL(outline_tile_kernel<false>, dim3((unsigned)(ntx * nty)), dim3(64), 0, st, plane, Hi, Wi, ntx, cnt, (int*)nullptr, 0);
  return hipGetLastError();
}

hipError_t launch_outline_scan(int* cnt, int Hi, int Wi, int cap, int* info_out, hipStream_t st) {
  const int n = 4 * ((Wi + 63) / 64) * ((Hi + 63) / 64);
  // bytes: the counts read twice and written once
  set_launch_cost(0.0, 12.0 * n + 8.0, "outline_scan");
  set_launch_grid(1);
  ProfScope ps_(st, PL_OUTLINE_SCAN);
  hipLaunchKernelGGL(outline_scan_kernel, dim3(1), dim3(256), 0, st, cnt, n, cap, info_out);
  return hipGetLastError();
}

hipError_t launch_outline_emit(const unsigned char* plane, int Hi, int Wi, const int* offs, int* edges_out, int cap, hipStream_t st) {
  const int ntx = (Wi + 63) / 64, nty = (Hi + 63) / 64;
  // bytes: the plane read once with the halo's share; the records are data dependent (not counted)
  set_launch_cost(0.0, (double)Hi * Wi * (1.0 + 4.0 / 64.0) + 16.0 * ntx * nty, "outline_emit");
  set_launch_grid((long)ntx * nty);
  ProfScope ps_(st, PL_OUTLINE_EMIT);
  hipLaunchKernelGGL(outline_tile_kernel<true>, dim3((unsigned)(ntx * nty)), dim3(64), 0, st, plane, Hi, Wi, ntx, const_cast<int*>(offs), edges_out, cap);
  return hipGetLastError();
}

}  // namespace se
