// The device JPEG encoder of the editing sessions (the stream is defined in include/sketchedit_jpg.h and
// restated in tests/jpg_stream_util.py): the hs x ws rectangle of a resident frame -> the entropy-coded segment of a baseline
// JPEG, 4:4:4, Annex K's tables, one restart interval per row of MCUs.  B requests per call, each with its own frame (se_window
// records of the ctx's table, as the journal reads them).  Three launches:
//
//  blocks: one wave per MCU, lane = pixel (y, x) of the 8 x 8 block.  The pixel (clamped to the rectangle: edge replication),
//          its Y, Cb, Cr; per component the two passes of the integer DCT as 8 + 8 wave shuffles (lane (y, u) sums over the
//          lanes of its row, lane (v, u) over the lanes of its column), the quantiser, and the int16 coefficient stored at its
//          ZIGZAG index: coef[image][row][mcu][component][64].
//  rows:   one workgroup of 1024 lanes per row of MCUs of an image; the row's 3 ceil(ws / 8) blocks are walked in tiles of 16, a
//          wave per block, lane = zigzag index.  Nothing in a row is sequential:
//            - lane 0 codes the DC difference against coefficient 0 of the block three to the left, read directly (0 for the
//              row's first MCU);
//            - the non-zero AC coefficients are one ballot; the run in front of a lane is its distance to the next lower set
//              bit (bit 0 standing for the DC), so its token is (run >> 4) ZRL codes, the code of (run & 15, size) and the
//              magnitude bits: at most 3 * 11 + 16 + 10 = 59 bits in one 64-bit value; lane 63 emits EOB if its coefficient is 0;
//            - bit offsets from a scan over the wave and then over the tile's blocks; the bits are ORed into an LDS stage, MSB
//              first (a token can straddle three words); the open word is carried to the next tile;
//            - stuffing is a second compaction: a lane per whole staged word counts its FF bytes, a block scan gives the FFs
//              before it, and the lane writes its 4 bytes at position + FFs before them, a 00 behind each FF;
//            - the padding with 1-bits, the last bytes and the row's marker go out by one lane; the row's size to the workspace.
//  finish: one workgroup per row: the row's offset (the sum of the sizes before it) and the copy of its slot to out + b cap
//          (dwords where the destination is aligned, bytes at both ends: no byte outside [0, size) is written); the last row's
//          workgroup writes the size.
//
// Every address is a function of the geometry alone, except the offsets inside a slot and inside out, which the sizes give and
// the bound covers (stage words, slot bytes and out bytes are checked against their capacity all the same).  Plain vector
// stores only, no inline assembly.
#include "../../include/sketchedit_jpg.h"
#include "se_device.h"
#include "se_jpg_tables.h"
#include "se_kernels.h"

#include <cstdint>

namespace se {

namespace {

constexpr int JPG_T = 1024;                     // lanes of a row's workgroup
constexpr int JPG_TILE = JPG_T / 64;            // blocks of a tile: a wave each
constexpr int JPG_BLOCK_BITS = 22 + 63 * 26;    // the most bits of one block
constexpr int JPG_STAGE = (31 + JPG_TILE * JPG_BLOCK_BITS + 31) / 32 + 2;      // words of the stage: 31 carried bits + a tile, and two more

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
  for (int c = 0; c < 3; ++c) {
    const int v = p[c] - 128;
    int t = 0;                                  // lane (y, u = x): over the pixels of row y
#pragma unroll
    for (int i = 0; i < 8; ++i) t += ax[i] * __shfl(v, (lane & 56) + i, 64);
    const int t1 = (t + 512) >> 10;
    int s = 0;                                  // lane (v = y, u = x): over t1 of column u
#pragma unroll
    for (int i = 0; i < 8; ++i) s += ay[i] * __shfl(t1, i * 8 + x, 64);
    const int q = min(max(((int)JPG_BASE[c ? 1 : 0][zz] * scale + 50) / 100, 1), 255);
    const int m = ((s < 0 ? -s : s) + (q << 15)) / (q << 16);
    dst[c * 64 + zz] = (short)(s < 0 ? -m : m);
  }
}

__global__ void __launch_bounds__(JPG_T) jpg_rows_kernel(const short* __restrict__ coef, int R, int nblk, unsigned* __restrict__ sizes,
                                                         unsigned char* __restrict__ slots, size_t slot_bytes) {
  __shared__ unsigned s_ac[2][256], s_dc[2][12];               // (code << 5) | length per symbol, 0 where the table has none
  __shared__ unsigned s_stage[JPG_STAGE];
  __shared__ int s_wsum[JPG_TILE], s_fsum[JPG_TILE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row = blockIdx.x, b = blockIdx.y;
  const size_t q = (size_t)b * R + row;
  const short* cf_row = coef + q * (size_t)nblk * 64;
  unsigned char* slot = slots + q * slot_bytes;

  if (tid < 512) s_ac[tid >> 8][tid & 255] = 0u;
  for (int i = tid; i < JPG_STAGE; i += JPG_T) s_stage[i] = 0u;
  __syncthreads();
  if (tid < 2 * 162) {
    const int t = tid / 162, k = tid - t * 162;
    s_ac[t][JPG_AC_SYMBOLS[t][k]] = canonical(JPG_AC_COUNTS[t], k);
  } else if (tid >= 512 && tid < 512 + 24) {
    const int t = (tid - 512) / 12, k = (tid - 512) - t * 12;
    s_dc[t][k] = canonical(JPG_DC_COUNTS[t], k);                // (the DC symbols are 0 .. 11 in code order)
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

  for (int base = 0; base < nblk; base += JPG_TILE) {
    const int blk = base + wave;
    const bool live = blk < nblk;               // (wave-uniform)
    const int tb = blk % 3 ? 1 : 0;             // the tables: luminance for Y, chrominance for Cb and Cr
    int c = 0;
    if (live) {
      const short* cf = cf_row + (size_t)blk * 64;
      c = cf[lane];
      if (lane == 0 && blk >= 3) c -= cf[-192];                 // the DC of the previous block of this component
    }
    const unsigned long long nz = __ballot(lane > 0 && c != 0);
    const int a = c < 0 ? -c : c;
    const int size = min(a ? 32 - __clz(a) : 0, lane ? 10 : 11);                 // (the ranges of 6k; a clamp keeps the index in the table)
    const unsigned long long mag = (unsigned long long)((c < 0 ? c - 1 : c) & ((1 << size) - 1));
    unsigned long long bits = 0ull;
    int tl = 0;
    if (live) {
      if (lane == 0) {
        const unsigned e = s_dc[tb][size];
        bits = ((unsigned long long)(e >> 5) << size) | mag;
        tl = (int)(e & 31u) + size;
      } else if (c != 0) {
        const unsigned long long below = (nz | 1ull) & ((1ull << lane) - 1ull);
        const int run = lane - 1 - (63 - __clzll((long long)below));
        const unsigned z = s_ac[tb][0xf0], e = s_ac[tb][((run & 15) << 4) | size];
        const int zl = (int)(z & 31u), el = (int)(e & 31u);
        for (int i = 0; i < (run >> 4); ++i) bits = (bits << zl) | (unsigned long long)(z >> 5);
        bits = (((bits << el) | (unsigned long long)(e >> 5)) << size) | mag;
        tl = (run >> 4) * zl + el + size;
      } else if (lane == 63) {
        const unsigned e = s_ac[tb][0];
        bits = (unsigned long long)(e >> 5);
        tl = (int)(e & 31u);
      }
    }
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
    if (tl) {                                   // tl bits at stream bit `at`, MSB first: bit i of the stream is bit 31 - (i & 31) of word i >> 5
      const int at = cbits + pre + x - tl, wd = at >> 5, sh = at & 31;
      const unsigned long long v = bits << (64 - tl);
      const unsigned w0 = (unsigned)(v >> (32 + sh)), w1 = (unsigned)(v >> sh), w2 = sh ? (unsigned)v << (32 - sh) : 0u;
      if (wd + 2 < JPG_STAGE) {
        if (w0) atomicOr(&s_stage[wd], w0);
        if (w1) atomicOr(&s_stage[wd + 1], w1);
        if (w2) atomicOr(&s_stage[wd + 2], w2);
      }
    }
    __syncthreads();
    // the whole words of the stage -> the slot, stuffed; the open word -> s_stage[0]
    const int total = cbits + tot, fw = min(total >> 5, JPG_STAGE - 1);                     // (at most 831 by the block bound: a lane per word)
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

int jpg_rows(int hs) { return (hs + 7) / 8; }

int jpg_row_blocks(int ws) { return 3 * ((ws + 7) / 8); }

size_t jpg_row_bound(int ws) { return 2 * (((size_t)JPG_BLOCK_BITS * jpg_row_blocks(ws) + 7) / 8) + 2; }

// a slot holds a row's bound, rounded up to 16 bytes
size_t jpg_slot_bytes(int ws) { return (jpg_row_bound(ws) + 15) & ~(size_t)15; }

int jpg_quality_scale(int quality) { return quality < 50 ? 5000 / quality : 200 - 2 * quality; }

hipError_t launch_jpg_blocks(const se_window* d_wins, int B, int hs, int ws, int quality, short* coef, hipStream_t st) {
  const int R = jpg_rows(hs), nbx = (ws + 7) / 8;
  const double mcus = (double)B * R * nbx;
  // bytes: the pixels read, the coefficients written; flops: two passes of 8 multiply-adds per value
  set_launch_cost(mcus * 192.0 * 32.0, mcus * (192.0 + 384.0), "jpg_blocks");
  set_launch_grid((long)((nbx + 3) / 4) * R * B);
  ProfScope ps_(st, PL_JPG_BLOCKS);
  hipLaunchKernelGGL(jpg_blocks_kernel, dim3((unsigned)((nbx + 3) / 4), (unsigned)R, (unsigned)B), dim3(256), 0, st, d_wins, hs, ws, nbx,
                     jpg_quality_scale(quality), coef);
  return hipGetLastError();
}

hipError_t launch_jpg_rows(int B, int hs, int ws, const short* coef, unsigned* sizes, unsigned char* slots, hipStream_t st) {
  const int R = jpg_rows(hs), nblk = jpg_row_blocks(ws);
  // bytes: the coefficients read; the slots written (an upper bound: the raw pixels)
  set_launch_cost(0.0, (double)B * R * nblk * (128.0 + 64.0), "jpg_rows");
  set_launch_grid((long)R * B);
  ProfScope ps_(st, PL_JPG_ROWS);
  hipLaunchKernelGGL(jpg_rows_kernel, dim3((unsigned)R, (unsigned)B), dim3(JPG_T), 0, st, coef, R, nblk, sizes, slots, jpg_slot_bytes(ws));
  return hipGetLastError();
}

hipError_t launch_jpg_finish(int B, int hs, int ws, const unsigned* sizes, const unsigned char* slots, unsigned char* out, size_t cap,
                             unsigned long long* sizes_out, hipStream_t st) {
  const int R = jpg_rows(hs);
  set_launch_cost(0.0, (double)B * R * jpg_row_blocks(ws) * 64.0 * 2.0, "jpg_finish");
  set_launch_grid((long)R * B);
  ProfScope ps_(st, PL_JPG_FINISH);
  hipLaunchKernelGGL(jpg_finish_kernel, dim3((unsigned)R, (unsigned)B), dim3(256), 0, st, R, sizes, slots, jpg_slot_bytes(ws), out, cap, sizes_out);
  return hipGetLastError();
}

// the same kernel for rows of any geometry (se_jpg2.hip): R rows an image, slots of slot_bytes (16-byte aligned), nblk blocks a row
hipError_t launch_jpg_finish_rows(int B, int R, int nblk, size_t slot_bytes, const unsigned* sizes, const unsigned char* slots,
                                  unsigned char* out, size_t cap, unsigned long long* sizes_out, hipStream_t st) {
  set_launch_cost(0.0, (double)B * R * nblk * 64.0 * 2.0, "jpg_finish");
  set_launch_grid((long)R * B);
  ProfScope ps_(st, PL_JPG_FINISH);
  hipLaunchKernelGGL(jpg_finish_kernel, dim3((unsigned)R, (unsigned)B), dim3(256), 0, st, R, sizes, slots, slot_bytes, out, cap, sizes_out);
  return hipGetLastError();
}

}  // namespace se
