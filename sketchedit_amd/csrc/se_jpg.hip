// The device JPEG encoder of the editing sessions (DESIGN.md sections 6k and 6l; the stream is defined in include/sketchedit_jpg.h
// and, for the flags, include/sketchedit_jpg2.h, and restated in tests/jpg_stream_util.py and tests/jpg2_stream_util.py): the
// hs x ws rectangle of a resident frame -> the entropy-coded segment of a baseline JPEG, one restart interval per row of MCUs.
// B requests per call, each with its own frame (se_window records of the ctx's table, as the journal reads them).  Without flags:
// 4:4:4, Annex K's tables, three launches (blocks, rows, finish).  SE_JPG_420 takes blocks420 for blocks; SE_JPG_OPTIMIZE puts
// hist and tables in front of rows.
//
//  blocks:    one wave per MCU, lane = pixel (y, x) of the 8 x 8 block.  The pixel (clamped to the rectangle: edge replication),
//             its Y, Cb, Cr; per component dct_store: the two passes of the integer DCT as 8 + 8 wave shuffles (lane (y, u) sums
//             over the lanes of its row, lane (v, u) over the lanes of its column), the quantiser, and the int16 coefficient
//             stored at its ZIGZAG index: coef[image][row][mcu][component][64].
//  blocks420: (SE_JPG_420) one wave per MCU of 16 x 16 pixels, lane = chroma sample (cy, cx).  The lane reads its 2 x 2 pixels
//             (clamped to the rectangle: rule 2'), keeps their four Y and sums their Cb and Cr: (sum + 1 + (cx & 1)) >> 2 (an MCU
//             starts at an even chroma column, so the column's parity is cx's).  Y block (by, bx): lane (y, x) takes pixel
//             (8 by + y, 8 bx + x) from lane (4 by + y / 2, 4 bx + x / 2) by four shuffles, one per position in the 2 x 2.  Six
//             dct_store.  coef[image][row][mcu][6][64].
//  hist:      (SE_JPG_OPTIMIZE) the walk of `rows` without the bits: a wave per block, a lane per zigzag index, its symbols into
//             4 x 256 LDS counters; one partial histogram per row of MCUs to the workspace.
//  tables:    (SE_JPG_OPTIMIZE) one wave per (image, alphabet): the rows' partials summed in row order; rule 5b by se_png.hip's
//             form (a rank sort by (count, symbol), the two-queue merge by one lane, depths by walking up, halving while a depth
//             exceeds 16); canonical codes as (code << 5) | length per symbol to the workspace; the record of 5e to tables_out.
//  rows:      one workgroup of 1024 lanes per row of MCUs of an image; the row's blocks (3 an MCU, 6 under SE_JPG_420) are walked
//             in tiles of 16, a wave per block, lane = zigzag index; the codes from Annex K's constants or, under
//             SE_JPG_OPTIMIZE, from the workspace.  Nothing in a row is sequential:
//               - lane 0 codes the DC difference against coefficient 0 of the previous block of its component, read directly
//                 (three blocks to the left; under SE_JPG_420 one, three or six by the block's place in its MCU; 0 for the row's
//                 first);
//               - the non-zero AC coefficients are one ballot; the run in front of a lane is its distance to the next lower set
//                 bit (bit 0 standing for the DC), so its token is (run >> 4) ZRL codes, the code of (run & 15, size) and the
//                 magnitude bits, in two parts: the ZRLs (at most 3 x 16 bits) and the code with its magnitude bits (at most
//                 16 + 11); lane 63 emits EOB if its coefficient is 0;
//               - bit offsets from a scan over the wave and then over the tile's blocks; the two parts are ORed into an LDS
//                 stage one behind the other, MSB first (a part can straddle three words); the open word is carried to the next
//                 tile;
//               - stuffing is a second compaction: a lane per whole staged word counts its FF bytes, a block scan gives the FFs
//                 before it, and the lane writes its 4 bytes at position + FFs before them, a 00 behind each FF;
//               - the padding with 1-bits, the last bytes and the row's marker go out by one lane; the row's size to the
//                 workspace.
//             AC coefficients and DC differences are clamped to what the tables have codes for (1023 and 2047), which only
//             se_jpg2_code_i16's own planes can exceed: the block kernels keep section 6k's ranges (sizes up to 10 and 11), so
//             from pixels the clamp never acts, and a clamp of the size instead would write the same bytes.
//  finish:    one workgroup per row: the row's offset (the sum of the sizes before it) and the copy of its slot to out + b cap
//             (dwords where the destination is aligned, bytes at both ends: no byte outside [0, size) is written); the last
//             row's workgroup writes the size.
//
// Every address is a function of the geometry alone, except the offsets inside a slot and inside out, which the sizes give and
// the bound covers (stage words, slot bytes and out bytes are checked against their capacity all the same).  Plain vector
// stores only, no inline assembly, no global atomics.
#include "../../include/sketchedit_jpg2.h"
#include "se_device.h"
#include "se_jpg_tables.h"
#include "se_kernels.h"

#include <cstdint>

namespace se {

namespace {

constexpr int JPG_T = 1024;                     // lanes of a row's workgroup
constexpr int JPG_TILE = JPG_T / 64;            // blocks of a tile: a wave each
constexpr int JPG_BITS_K = 22 + 63 * 26;        // the most bits of one block under Annex K's tables
constexpr int JPG_BITS_OPT = 27 + 63 * 26;      // ... under tables whose codes may all be 16 bits
constexpr int JPG_STAGE = (31 + JPG_TILE * JPG_BITS_OPT + 31) / 32 + 2;        // words of the stage: 31 carried bits + a tile, and two more
static_assert(JPG_STAGE <= JPG_T, "the flush has a lane per staged word");

// one 8 x 8 block: lane (y, x) holds sample v - 128 -> the quantised coefficient at the lane's zigzag index
__device__ __forceinline__ void dct_store(int v, int lane, const int* ax, const int* ay, int zz, int tb, int scale, short* dst) {
  const int x = lane & 7;
  int t = 0;                                    // lane (y, u = x): over the pixels of row y
#pragma unroll
  for (int i = 0; i < 8; ++i) t += ax[i] * __shfl(v, (lane & 56) + i, 64);
  const int t1 = (t + 512) >> 10;
  int s = 0;                                    // lane (v = y, u = x): over t1 of column u
#pragma unroll
  for (int i = 0; i < 8; ++i) s += ay[i] * __shfl(t1, i * 8 + x, 64);
  const int q = min(max(((int)JPG_BASE[tb][zz] * scale + 50) / 100, 1), 255);
  const int m = ((s < 0 ? -s : s) + (q << 15)) / (q << 16);
  dst[zz] = (short)(s < 0 ? -m : m);
}

__global__ void __launch_bounds__(256) jpg_blocks_kernel(const se_window* __restrict__ wins, int hs, int ws, int nbx, int scale,
                                                         short* __restrict__ coef) {
  const int lane = threadIdx.x & 63;
  const int mx = blockIdx.x * 4 + (threadIdx.x >> 6), my = blockIdx.y, b = blockIdx.z;
  if (mx >= nbx) return;                        // (wave-uniform; the kernel has no barrier)
  const se_window w = wins[b];
  const int y = lane >> 3, x = lane & 7;
  const int yy = min(my * 8 + y, hs - 1), xx = min(mx * 8 + x, ws - 1);       // rule 2: inside the rectangle
  const unsigned char* px = w.frame_u8 + ((size_t)(w.y0 + yy) * w.Wi + (w.x0 + xx)) * 3;
  const int R = px[0], G = px[1], Bl = px[2];
  int p[3];
  p[0] = (19595 * R + 38470 * G + 7471 * Bl + 32768) >> 16;
  p[1] = (-11059 * R - 21709 * G + 32768 * Bl + (128 << 16) + 32767) >> 16;
  p[2] = (32768 * R - 27439 * G - 5329 * Bl + (128 << 16) + 32767) >> 16;
  int ax[8], ay[8];                             // A[u = x][.] for the row pass, A[v = y][.] for the column pass
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    ax[i] = JPG_A[x * 8 + i];
    ay[i] = JPG_A[y * 8 + i];
  }
  const int zz = JPG_ZZ_OF[lane];
  short* dst = coef + (((size_t)b * gridDim.y + my) * nbx + mx) * 192;
#pragma unroll
  for (int c = 0; c < 3; ++c) dct_store(p[c] - 128, lane, ax, ay, zz, c ? 1 : 0, scale, dst + c * 64);
}

__global__ void __launch_bounds__(256) jpg2_blocks420_kernel(const se_window* __restrict__ wins, int hs, int ws, int nmx, int scale,
                                                             short* __restrict__ coef) {
  const int lane = threadIdx.x & 63;
  const int mx = blockIdx.x * 4 + (threadIdx.x >> 6), my = blockIdx.y, b = blockIdx.z;
  if (mx >= nmx) return;                        // (wave-uniform; the kernel has no barrier)
  const se_window w = wins[b];
  const int y = lane >> 3, x = lane & 7;        // the chroma sample, and the lane's place in every block
  int yv[4], cb = 0, cr = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int yy = min(my * 16 + 2 * y + (k >> 1), hs - 1), xx = min(mx * 16 + 2 * x + (k & 1), ws - 1);       // rule 2'
    const unsigned char* px = w.frame_u8 + ((size_t)(w.y0 + yy) * w.Wi + (w.x0 + xx)) * 3;
    const int R = px[0], G = px[1], Bl = px[2];
    yv[k] = (19595 * R + 38470 * G + 7471 * Bl + 32768) >> 16;
    cb += (-11059 * R - 21709 * G + 32768 * Bl + (128 << 16) + 32767) >> 16;
    cr += (32768 * R - 27439 * G - 5329 * Bl + (128 << 16) + 32767) >> 16;
  }
  const int bias = 1 + (x & 1);                 // rule 1'': the chroma column is 8 mx + x
  cb = (cb + bias) >> 2;
  cr = (cr + bias) >> 2;
  int ax[8], ay[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    ax[i] = JPG_A[x * 8 + i];
    ay[i] = JPG_A[y * 8 + i];
  }
  const int zz = JPG_ZZ_OF[lane];
  short* dst = coef + (((size_t)b * gridDim.y + my) * nmx + mx) * 384;
  const int k = (y & 1) * 2 + (x & 1);
#pragma unroll
  for (int blk = 0; blk < 4; ++blk) {
    const int src = ((blk >> 1) * 4 + (y >> 1)) * 8 + (blk & 1) * 4 + (x >> 1);
    const int v0 = __shfl(yv[0], src, 64), v1 = __shfl(yv[1], src, 64), v2 = __shfl(yv[2], src, 64), v3 = __shfl(yv[3], src, 64);
    dct_store((k == 0 ? v0 : k == 1 ? v1 : k == 2 ? v2 : v3) - 128, lane, ax, ay, zz, 0, scale, dst + blk * 64);
  }
  dct_store(cb - 128, lane, ax, ay, zz, 1, scale, dst + 256);
  dct_store(cr - 128, lane, ax, ay, zz, 1, scale, dst + 320);
}

// What lane `lane` of the wave of block `blk` emits.  c: its coefficient (the DC difference for lane 0), clamped to the ranges the
// tables have codes for; tb: 0 luminance, 1 chrominance.  Called by whole waves (a ballot); a wave that is not live passes c = 0.
struct LaneToken {
  int tb, size, run;       // run: the zeros in front of a non-zero AC coefficient
  unsigned mag;            // the magnitude bits
  bool dc, ac, eob;        // which of the three the lane emits (at most one)
};

__device__ __forceinline__ LaneToken lane_token(const short* __restrict__ cf_row, int blk, int nblk, int lane, int mode420) {
  LaneToken t;
  const bool live = blk < nblk;                 // (wave-uniform)
  const int pos = mode420 ? blk % 6 : blk % 3;
  t.tb = mode420 ? (pos >= 4 ? 1 : 0) : (pos ? 1 : 0);
  const int back = mode420 ? (pos == 0 ? 3 : pos < 4 ? 1 : 6) : 3;            // the previous block of this component
  int c = 0;
  if (live) {
    const short* cf = cf_row + (size_t)blk * 64;
    c = cf[lane];
    if (lane == 0 && blk >= back) c -= cf[-64 * back];
    const int lim = lane ? 1023 : 2047;
    c = min(max(c, -lim), lim);
  }
  const unsigned long long nz = __ballot(lane > 0 && c != 0);
  const int a = c < 0 ? -c : c;
  t.size = a ? 32 - __clz(a) : 0;
  t.mag = (unsigned)((c < 0 ? c - 1 : c) & ((1 << t.size) - 1));
  t.dc = live && lane == 0;
  t.ac = live && lane > 0 && c != 0;
  t.eob = live && lane == 63 && c == 0;
  const unsigned long long below = (nz | 1ull) & ((1ull << lane) - 1ull);
  t.run = lane ? lane - 1 - (63 - __clzll((long long)below)) : 0;
  return t;
}

__global__ void __launch_bounds__(JPG_T) jpg2_hist_kernel(const short* __restrict__ coef, int R, int nblk, int mode420,
                                                         unsigned* __restrict__ hist) {
  __shared__ unsigned s_hist[4][256];           // DC lum, AC lum, DC chr, AC chr
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t q = (size_t)blockIdx.y * R + blockIdx.x;
  const short* cf_row = coef + q * (size_t)nblk * 64;
  s_hist[tid >> 8][tid & 255] = 0u;
  __syncthreads();
  for (int base = 0; base < nblk; base += JPG_TILE) {
    const LaneToken t = lane_token(cf_row, base + wave, nblk, lane, mode420);
    if (t.dc) atomicAdd(&s_hist[2 * t.tb][t.size], 1u);
    if (t.ac) {
      atomicAdd(&s_hist[2 * t.tb + 1][((t.run & 15) << 4) | t.size], 1u);
      if (t.run >> 4) atomicAdd(&s_hist[2 * t.tb + 1][0xf0], (unsigned)(t.run >> 4));
    }
    if (t.eob) atomicAdd(&s_hist[2 * t.tb + 1][0], 1u);
  }
  __syncthreads();
  hist[q * 1024 + tid] = s_hist[tid >> 8][tid & 255];
}

constexpr int JPG_NSYM = 257;                    // 256 symbols and the one that is never emitted

__global__ void __launch_bounds__(64) jpg2_tables_kernel(const unsigned* __restrict__ hist, int R, unsigned* __restrict__ codes,
                                                         unsigned* __restrict__ tables_out) {
  __shared__ unsigned s_cnt[JPG_NSYM], s_lw[JPG_NSYM], s_iw[JPG_NSYM], s_blc[17], s_next[17], s_rec[68];
  __shared__ unsigned short s_ls[JPG_NSYM], s_parent[2 * JPG_NSYM];
  __shared__ unsigned char s_len[256];
  __shared__ int s_m, s_maxlen;
  const int lane = threadIdx.x, t = blockIdx.x, b = blockIdx.y;

  for (int s = lane; s < 256; s += 64) {        // rule 5a: the rows' partials, in row order
    const unsigned* h = hist + ((size_t)b * R * 4 + t) * 256 + s;
    unsigned c = 0u;
    for (int r = 0; r < R; ++r) c += h[(size_t)r * 1024];
    s_cnt[s] = c;
  }
  if (lane == 0) s_cnt[256] = 1u;
  for (;;) {                                    // rule 5b
    __syncthreads();
    for (int s = lane; s < 256; s += 64) s_len[s] = 0;
    if (lane < 17) s_blc[lane] = 0u;
    if (lane == 0) { s_m = 0; s_maxlen = 0; }
    __syncthreads();
    for (int s = lane; s < JPG_NSYM; s += 64) {
      const unsigned c = s_cnt[s];
      if (c) {
        int rank = 0;
        for (int j = 0; j < JPG_NSYM; ++j) {
          const unsigned cj = s_cnt[j];
          rank += (cj && (cj < c || (cj == c && j < s))) ? 1 : 0;
        }
        s_lw[rank] = c;
        s_ls[rank] = (unsigned short)s;
        atomicAdd(&s_m, 1);
      }
    }
    __syncthreads();
    const int m = s_m;                          // >= 2: a real symbol (every block has a DC and an EOB or a coefficient 63) and 256
    if (lane == 0) {
      int li = 0, ii = 0, ni = 0;               // heads of the leaf and the internal queue, internal nodes made
      for (int k = 0; k < m - 1; ++k) {
        int nd[2];
        unsigned wt[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          if (li < m && (ii >= ni || s_lw[li] <= s_iw[ii])) { nd[e] = li; wt[e] = s_lw[li]; ++li; }
          else { nd[e] = m + ii; wt[e] = s_iw[ii]; ++ii; }
        }
        s_iw[ni] = wt[0] + wt[1];
        s_parent[nd[0]] = s_parent[nd[1]] = (unsigned short)(m + ni);
        ++ni;
      }
    }
    __syncthreads();
    for (int i = lane; i < m; i += 64) {
      int d = 0;
      for (int node = i; node != 2 * m - 2; node = s_parent[node]) ++d;
      const int s = s_ls[i];
      atomicMax(&s_maxlen, d);
      if (s < 256) {
        s_len[s] = (unsigned char)min(d, 255);
        if (d <= 16) atomicAdd(&s_blc[d], 1u);
      }
    }
    __syncthreads();
    if (s_maxlen <= 16) break;                  // (block-uniform: nobody changes it before the barrier at the loop's head)
    for (int s = lane; s < 256; s += 64) {
      const unsigned c = s_cnt[s];
      if (c) s_cnt[s] = (c + 1u) >> 1;
    }
  }
  // rule 5c: the first code of every length, and the number of symbols with a shorter one (their place in the record)
  if (lane == 0) {
    unsigned code = 0u, before = 0u;
    for (int bits = 1; bits <= 16; ++bits) {
      const unsigned n = s_blc[bits];
      s_next[bits] = code;
      s_blc[bits] = (n << 16) | before;         // (at most 256 of either)
      before += n;
      code = (code + n) << 1;
    }
  }
  for (int i = lane; i < 68; i += 64) s_rec[i] = 0u;
  __syncthreads();
  unsigned char* rec = (unsigned char*)s_rec;
  if (lane < 16) rec[lane] = (unsigned char)(s_blc[lane + 1] >> 16);
  for (int s = lane; s < 256; s += 64) {
    const int l = s_len[s];
    unsigned e = 0u;
    if (l) {
      unsigned rank = 0u;
      for (int j = 0; j < s; ++j) rank += s_len[j] == l ? 1u : 0u;
      e = ((s_next[l] + rank) << 5) | (unsigned)l;
      rec[16 + (s_blc[l] & 0xffffu) + rank] = (unsigned char)s;              // (fewer than 256 real symbols lie before it)
    }
    codes[((size_t)b * 4 + t) * 256 + s] = e;
  }
  __syncthreads();
  for (int i = lane; i < 68; i += 64) tables_out[((size_t)b * 4 + t) * 68 + i] = s_rec[i];
}

__global__ void __launch_bounds__(JPG_T) jpg_rows_kernel(const short* __restrict__ coef, int R, int nblk, int mode420,
                                                         const unsigned* __restrict__ codes, unsigned* __restrict__ sizes,
                                                         unsigned char* __restrict__ slots, size_t slot_bytes) {
  __shared__ unsigned s_tab[4][256];            // (code << 5) | length per symbol: DC lum, AC lum, DC chr, AC chr
  __shared__ unsigned s_stage[JPG_STAGE];
  __shared__ int s_wsum[JPG_TILE], s_fsum[JPG_TILE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row = blockIdx.x, b = blockIdx.y;
  const size_t q = (size_t)b * R + row;
  const short* cf_row = coef + q * (size_t)nblk * 64;
  unsigned char* slot = slots + q * slot_bytes;

  s_tab[tid >> 8][tid & 255] = codes ? codes[(size_t)b * 1024 + tid] : 0u;
  for (int i = tid; i < JPG_STAGE; i += JPG_T) s_stage[i] = 0u;
  __syncthreads();
  if (!codes) {                                 // Annex K's
    if (tid < 2 * 162) {
      const int t = tid / 162, k = tid - t * 162;
      s_tab[2 * t + 1][JPG_AC_SYMBOLS[t][k]] = canonical(JPG_AC_COUNTS[t], k);
    } else if (tid >= 512 && tid < 512 + 24) {
      const int t = (tid - 512) / 12, k = (tid - 512) - t * 12;
      s_tab[2 * t][k] = canonical(JPG_DC_COUNTS[t], k);          // (the DC symbols are 0 .. 11 in code order)
    }
  }
  __syncthreads();

  unsigned obytes = 0;     // bytes of the slot written so far
  int cbits = 0;           // bits of the open word, s_stage[0]
  auto emit = [&](unsigned& at, unsigned v) {   // one byte and its stuffing
    if (at < slot_bytes) slot[at] = (unsigned char)v;
    ++at;
    if (v == 0xffu) {
      if (at < slot_bytes) slot[at] = 0;
      ++at;
    }
  };
  // the n <= 64 low bits of v at stream bit `at`, MSB first: bit i of the stream is bit 31 - (i & 31) of word i >> 5
  auto put = [&](int at, unsigned long long v, int n) {
    if (!n) return;
    const int wd = at >> 5, sh = at & 31;
    v <<= 64 - n;
    const unsigned w0 = (unsigned)(v >> (32 + sh)), w1 = (unsigned)(v >> sh), w2 = sh ? (unsigned)v << (32 - sh) : 0u;
    if (wd + 2 < JPG_STAGE) {
      if (w0) atomicOr(&s_stage[wd], w0);
      if (w1) atomicOr(&s_stage[wd + 1], w1);
      if (w2) atomicOr(&s_stage[wd + 2], w2);
    }
  };

  for (int base = 0; base < nblk; base += JPG_TILE) {
    const LaneToken t = lane_token(cf_row, base + wave, nblk, lane, mode420);
    unsigned long long za = 0ull, cb = 0ull;    // the ZRLs; the code and the magnitude bits
    int la = 0, lb = 0;
    if (t.dc) {
      const unsigned e = s_tab[2 * t.tb][t.size];
      cb = ((unsigned long long)(e >> 5) << t.size) | t.mag;
      lb = (int)(e & 31u) + t.size;
    } else if (t.ac) {
      const unsigned z = s_tab[2 * t.tb + 1][0xf0], e = s_tab[2 * t.tb + 1][((t.run & 15) << 4) | t.size];
      const int zl = (int)(z & 31u);
      for (int i = 0; i < (t.run >> 4); ++i) za = (za << zl) | (unsigned long long)(z >> 5);
      la = (t.run >> 4) * zl;
      cb = ((unsigned long long)(e >> 5) << t.size) | t.mag;
      lb = (int)(e & 31u) + t.size;
    } else if (t.eob) {
      const unsigned e = s_tab[2 * t.tb + 1][0];
      cb = (unsigned long long)(e >> 5);
      lb = (int)(e & 31u);
    }
    const int tl = la + lb;
    int x = tl;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int yv = __shfl_up(x, o, 64);
      if (lane >= o) x += yv;
    }
    if (lane == 63) s_wsum[wave] = x;
    __syncthreads();
    int pre = 0, tot = 0;
#pragma unroll
    for (int w2 = 0; w2 < JPG_TILE; ++w2) {
      const int sw = s_wsum[w2];
      pre += w2 < wave ? sw : 0;
      tot += sw;
    }
    {
      const int at = cbits + pre + x - tl;
      put(at, za, la);
      put(at + la, cb, lb);
    }
    __syncthreads();
    // the whole words of the stage -> the slot, stuffed; the open word -> s_stage[0]
    const int total = cbits + tot, fw = min(total >> 5, JPG_STAGE - 1);
    unsigned word = 0u;
    int nff = 0;
    if (tid < fw) {
      word = s_stage[tid];
#pragma unroll
      for (int i = 0; i < 4; ++i) nff += ((word >> (8 * i)) & 255u) == 255u ? 1 : 0;
    }
    int fx = nff;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int yv = __shfl_up(fx, o, 64);
      if (lane >= o) fx += yv;
    }
    if (lane == 63) s_fsum[wave] = fx;
    __syncthreads();
    int fpre = 0, ftot = 0;
#pragma unroll
    for (int w2 = 0; w2 < JPG_TILE; ++w2) {
      const int sw = s_fsum[w2];
      fpre += w2 < wave ? sw : 0;
      ftot += sw;
    }
    if (tid < fw) {
      unsigned at = obytes + 4u * (unsigned)tid + (unsigned)(fpre + fx - nff);
#pragma unroll
      for (int i = 3; i >= 0; --i) emit(at, (word >> (8 * i)) & 255u);
    }
    const unsigned open = s_stage[fw];
    __syncthreads();
    for (int i = tid; i < JPG_STAGE; i += JPG_T) s_stage[i] = i == 0 ? open : 0u;
    obytes += 4u * (unsigned)fw + (unsigned)ftot;
    cbits = total & 31;
  }
  // the open word padded with 1-bits to a byte, the marker, the size  (lane 0 wrote s_stage[0] itself)
  if (tid == 0) {
    const int nb = (cbits + 7) >> 3;
    const unsigned pad = cbits & 7 ? (0xffffffffu >> cbits) & (nb < 4 ? ~(0xffffffffu >> (8 * nb)) : 0xffffffffu) : 0u;
    const unsigned word = s_stage[0] | pad;
    unsigned at = obytes;
    for (int i = 0; i < nb; ++i) emit(at, (word >> (24 - 8 * i)) & 255u);
    if (row < R - 1) {
      if (at + 1 < slot_bytes) {
        slot[at] = 0xff;
        slot[at + 1] = (unsigned char)(0xd0 + (row & 7));
      }
      at += 2;
    }
    sizes[q] = at;
  }
}

__global__ void __launch_bounds__(256) jpg_finish_kernel(int R, const unsigned* __restrict__ sizes, const unsigned char* __restrict__ slots,
                                                         size_t slot_bytes, unsigned char* __restrict__ out, size_t cap,
                                                         unsigned long long* __restrict__ sizes_out) {
  __shared__ unsigned long long s_off;
  const int tid = threadIdx.x, r = blockIdx.x, b = blockIdx.y;
  const unsigned* sz = sizes + (size_t)b * R;
  if (tid == 0) s_off = 0ull;
  __syncthreads();
  {
    unsigned long long mine = 0ull;
    for (int i = tid; i < r; i += 256) mine += sz[i];
    if (mine) atomicAdd(&s_off, mine);
  }
  __syncthreads();
  const size_t off = (size_t)s_off, nbytes = sz[r];
  if (nbytes > slot_bytes || off + nbytes > cap) return;        // (the bound rules it out; block-uniform)
  unsigned char* dst = out + (size_t)b * cap + off;
  const unsigned char* src = slots + ((size_t)b * R + r) * slot_bytes;                   // 16-byte aligned
  const unsigned* src32 = (const unsigned*)src;
  const size_t head = min(nbytes, (size_t)((4 - ((uintptr_t)dst & 3)) & 3));
  const size_t nd = (nbytes - head) >> 2;
  if ((size_t)tid < head) dst[tid] = src[tid];
  for (size_t i = tid; i < nd; i += 256) {
    const size_t o = head + 4 * i;
    const int sh = (int)(o & 3) * 8;
    const unsigned lo = src32[o >> 2];
    *(unsigned*)(dst + o) = sh ? (lo >> sh) | (src32[(o >> 2) + 1] << (32 - sh)) : lo;   // (bytes o .. o + 3 < nbytes: inside the slot)
  }
  for (size_t i = head + 4 * nd + tid; i < nbytes; i += 256) dst[i] = src[i];
  if (r == R - 1 && tid == 0) sizes_out[b] = (unsigned long long)(off + nbytes);
}

}  // namespace

int jpg_rows(int hs, int flags) { return flags & SE_JPG_420 ? (hs + 15) / 16 : (hs + 7) / 8; }

int jpg_row_blocks(int ws, int flags) { return flags & SE_JPG_420 ? 6 * ((ws + 15) / 16) : 3 * ((ws + 7) / 8); }

size_t jpg_row_bound(int nblk, int flags) {
  return 2 * (((size_t)(flags & SE_JPG_OPTIMIZE ? JPG_BITS_OPT : JPG_BITS_K) * nblk + 7) / 8) + 2;
}

// a slot holds a row's bound, rounded up to 16 bytes
size_t jpg_slot_bytes(int nblk, int flags) { return (jpg_row_bound(nblk, flags) + 15) & ~(size_t)15; }

static int jpg_quality_scale(int quality) { return quality < 50 ? 5000 / quality : 200 - 2 * quality; }

hipError_t launch_jpg_blocks(const se_window* d_wins, int B, int hs, int ws, int quality, short* coef, hipStream_t st) {
  const int R = (hs + 7) / 8, nbx = (ws + 7) / 8;
  const double mcus = (double)B * R * nbx;
  // bytes: the pixels read, the coefficients written; flops: two passes of 8 multiply-adds per value
  set_launch_cost(mcus * 192.0 * 32.0, mcus * (192.0 + 384.0), "jpg_blocks");
  set_launch_grid((long)((nbx + 3) / 4) * R * B);
  ProfScope ps_(st, PL_JPG_BLOCKS);
  hipLaunchKernelGGL(jpg_blocks_kernel, dim3((unsigned)((nbx + 3) / 4), (unsigned)R, (unsigned)B), dim3(256), 0, st, d_wins, hs, ws, nbx,
                     jpg_quality_scale(quality), coef);
  return hipGetLastError();
}

hipError_t launch_jpg2_blocks420(const se_window* d_wins, int B, int hs, int ws, int quality, short* coef, hipStream_t st) {
  const int R = (hs + 15) / 16, nmx = (ws + 15) / 16;
  const double mcus = (double)B * R * nmx;
  // bytes: the pixels read, the coefficients written; flops: two passes of 8 multiply-adds per value
  set_launch_cost(mcus * 384.0 * 32.0, mcus * (768.0 + 768.0), "jpg2_blocks420");
  set_launch_grid((long)((nmx + 3) / 4) * R * B);
  ProfScope ps_(st, PL_JPG2_BLOCKS);
  hipLaunchKernelGGL(jpg2_blocks420_kernel, dim3((unsigned)((nmx + 3) / 4), (unsigned)R, (unsigned)B), dim3(256), 0, st, d_wins, hs, ws, nmx,
                     jpg_quality_scale(quality), coef);
  return hipGetLastError();
}

hipError_t launch_jpg2_hist(int B, int R, int nblk, int flags, const short* coef, unsigned* hist, hipStream_t st) {
  set_launch_cost(0.0, (double)B * R * (nblk * 128.0 + 4096.0), "jpg2_hist");
  set_launch_grid((long)R * B);
  ProfScope ps_(st, PL_JPG2_HIST);
  hipLaunchKernelGGL(jpg2_hist_kernel, dim3((unsigned)R, (unsigned)B), dim3(JPG_T), 0, st, coef, R, nblk, flags & SE_JPG_420 ? 1 : 0, hist);
  return hipGetLastError();
}

hipError_t launch_jpg2_tables(int B, int R, const unsigned* hist, unsigned* codes, unsigned char* tables_out, hipStream_t st) {
  set_launch_cost(0.0, (double)B * (R * 4096.0 + 4096.0 + 1088.0), "jpg2_tables");
  set_launch_grid(4L * B);
  ProfScope ps_(st, PL_JPG2_TABLES);
  hipLaunchKernelGGL(jpg2_tables_kernel, dim3(4u, (unsigned)B), dim3(64), 0, st, hist, R, codes, (unsigned*)tables_out);
  return hipGetLastError();
}

hipError_t launch_jpg_rows(int B, int R, int nblk, int flags, const short* coef, const unsigned* codes, unsigned* sizes,
                           unsigned char* slots, hipStream_t st) {
  // bytes: the coefficients read; the slots written (an upper bound: the raw pixels)
  set_launch_cost(0.0, (double)B * R * nblk * (128.0 + 64.0), "jpg_rows");
  set_launch_grid((long)R * B);
  ProfScope ps_(st, PL_JPG_ROWS);
  hipLaunchKernelGGL(jpg_rows_kernel, dim3((unsigned)R, (unsigned)B), dim3(JPG_T), 0, st, coef, R, nblk, flags & SE_JPG_420 ? 1 : 0, codes, sizes,
                     slots, jpg_slot_bytes(nblk, flags));
  return hipGetLastError();
}

hipError_t launch_jpg_finish(int B, int R, int nblk, size_t slot_bytes, const unsigned* sizes, const unsigned char* slots,
                             unsigned char* out, size_t cap, unsigned long long* sizes_out, hipStream_t st) {
  set_launch_cost(0.0, (double)B * R * nblk * 64.0 * 2.0, "jpg_finish");
  set_launch_grid((long)R * B);
  ProfScope ps_(st, PL_JPG_FINISH);
  hipLaunchKernelGGL(jpg_finish_kernel, dim3((unsigned)R, (unsigned)B), dim3(256), 0, st, R, sizes, slots, slot_bytes, out, cap, sizes_out);
  return hipGetLastError();
}

}  // namespace se
