// The device PNG encoder of the editing sessions (the stream is defined in include/sketchedit_png.h and
// restated in tests/png_stream_util.py): the hs x ws rectangle of a resident frame -> the zlib stream of its PNG.  B requests per
// call, each with its own frame (se_window records of the ctx's table, as the journal reads them).  Three launches:
//
//  rows:    one wave per row of a rectangle: the two candidates' sums of |residual| and the row's filter type (1 SUB, 2 UP).
//  stripes: one workgroup of 1024 lanes per stripe of 32 rows.  The stripe's filtered bytes are never stored: a lane computes
//           the byte at stripe position p from the frame (p -> row and column, the row's type, one or two frame bytes).  The
//           stripe is walked twice in tiles of 1024 positions, a lane per position:
//             - run starts (byte != its predecessor) as one ballot word per wave, kept in LDS with 5 more words for the 320
//               positions behind the tile; a position's run start is the highest set bit at or below it (its own wave's
//               ballot, else the waves before, else the carry of the earlier tiles), so its index k in its run is known, and
//               the run's remaining length, capped at 258, is a find-first-set over at most 6 of those words;
//             - the token rule in closed form: k == 0 is a literal; with j = (k - 1) % 258, j >= 2 emits nothing (it lies
//               inside a match), j == 1 is a literal iff the run ends behind it (a tail of two), j == 0 is a match of
//               min(remaining, 258) if that is >= 3, else a literal;
//             - first walk: the histogram (LDS atomics) and the checksum parts s1 = sum v, s2 = sum (n - p) v;
//             - between the walks the code: a rank sort of the used symbols by (count, symbol), then the classic two-queue
//               merge by one lane (sorted leaves, internal nodes in the order they are made: the head with the smaller
//               (weight, id) is the minimum over all live nodes, a leaf winning a tie against an internal node, whose id is
//               larger) -- the tree of "remove the two smallest (weight, id)"; depths by walking up; deeper than 15: counts
//               (c + 1) >> 1 and again; canonical codes from the counts per length and a symbol's rank among its length;
//             - second walk: a block scan of the tokens' bit lengths, the bits ORed into an LDS stage (a token is at most
//               15 + 5 + 1 bits: two words), whole words flushed to the stripe's slot, the open word carried to the next tile.
//           The block header goes through the same stage first, end-of-block and the empty stored block last.
//  finish:  one workgroup per stripe: the stripe's offset (the sum of the sizes before it), the copy of its slot to out + b cap
//           (dwords where the destination is aligned, bytes at both ends: no byte outside [0, size) is written); the first
//           stripe's workgroup writes 78 01, the last one's the final block, the Adler-32 combined from the parts in 64-bit
//           arithmetic, and the size.
//
// Every address is a function of the geometry alone, except the offsets inside a slot and inside out, which the sizes give and
// the bound covers (slot words and out bytes are checked against their capacity all the same).  Plain vector stores only.
#include "../../include/sketchedit_png.h"
#include "se_device.h"
#include "se_kernels.h"

#include <cstdint>

namespace se {

namespace {

constexpr int PNG_ROWS = 32;                    // rows of a stripe
constexpr int PNG_T = 1024;                     // lanes of a stripe's workgroup = positions of a tile
constexpr int PNG_HALO = 320;                   // positions behind a tile whose run starts are kept: 5 ballot words >= 258
constexpr int PNG_WAVES = PNG_T / 64;
constexpr int PNG_MASKS = PNG_WAVES + PNG_HALO / 64;
constexpr int PNG_NSYM = 286, PNG_EOB = 256, PNG_MAXM = 258;
constexpr int PNG_STAGE = 680;                  // words of the stage: 31 carried bits + 1024 tokens of at most 21 bits, and one more
constexpr unsigned ADLER = 65521u;

// match length 3 .. 258 -> its symbol, the value and the number of its extra bits (RFC 1951 3.2.5, in closed form)
__device__ __forceinline__ void length_symbol(int len, int& sym, unsigned& extra, int& nb) {
  const int l = len - 3;
  if (len == PNG_MAXM) { sym = 285; extra = 0; nb = 0; return; }
  if (l < 8) { sym = 257 + l; extra = 0; nb = 0; return; }
  nb = (31 - __clz(l)) - 2;
  sym = 261 + 4 * nb + ((l >> nb) & 3);
  extra = (unsigned)l & ((1u << nb) - 1u);
}

__global__ void __launch_bounds__(256) png_rows_kernel(const se_window* __restrict__ wins, int B, int hs, int ws,
                                                       unsigned char* __restrict__ ftype) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= (long)B * hs) return;                // (wave-uniform; the kernel has no barrier)
  const int y = (int)(r % hs), b = (int)(r / hs);
  const se_window w = wins[b];
  const size_t pitch = (size_t)w.Wi * 3;
  const unsigned char* row = w.frame_u8 + ((size_t)(w.y0 + y) * w.Wi + w.x0) * 3;       // the row's bytes: [row, row + 3 ws)
  const int n = 3 * ws;
  int ssub = 0, sup = 0;
  for (int i = lane; i < n; i += 64) {
    const int cur = row[i];
    const int a = (cur - (i >= 3 ? (int)row[i - 3] : 0)) & 255, u = (cur - (y > 0 ? (int)(row - pitch)[i] : 0)) & 255;
    ssub += a >= 128 ? 256 - a : a;
    sup += u >= 128 ? 256 - u : u;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ssub += __shfl_down(ssub, o, 64);
    sup += __shfl_down(sup, o, 64);
  }
  if (lane == 0) ftype[r] = sup < ssub ? 2 : 1;
}

__global__ void __launch_bounds__(PNG_T) png_stripe_kernel(const se_window* __restrict__ wins, int hs, int ws, int S,
                                                           const unsigned char* __restrict__ ftype, unsigned* __restrict__ sizes,
                                                           unsigned* __restrict__ parts, unsigned char* __restrict__ slots,
                                                           size_t slot_bytes) {
  __shared__ unsigned short s_val[PNG_T + PNG_HALO + 1];        // the bytes at positions base - 1 .. base + T + HALO - 1
  __shared__ unsigned long long s_mask[PNG_MASKS];              // run starts of positions base .. base + T + HALO - 1
  __shared__ int s_wlast[PNG_WAVES], s_wsum[PNG_WAVES];
  __shared__ unsigned s_hist[PNG_NSYM], s_lw[PNG_NSYM], s_iw[PNG_NSYM], s_code[PNG_NSYM];
  __shared__ unsigned short s_ls[PNG_NSYM], s_parent[2 * PNG_NSYM];
  __shared__ unsigned char s_len[PNG_NSYM], s_ft[PNG_ROWS];
  __shared__ unsigned s_blc[16], s_next[16];
  __shared__ int s_m, s_maxlen;
  __shared__ unsigned s_stage[PNG_STAGE];
  __shared__ unsigned long long s_a1, s_a2;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = blockIdx.x, b = blockIdx.y;
  const se_window w = wins[b];
  const int ys = s * PNG_ROWS, rows = min(PNG_ROWS, hs - ys), rowlen = 1 + 3 * ws, n = rows * rowlen;
  const size_t pitch = (size_t)w.Wi * 3;
  const unsigned char* rect = w.frame_u8 + ((size_t)w.y0 * w.Wi + w.x0) * 3;
  unsigned* gout = (unsigned*)(slots + ((size_t)b * S + s) * slot_bytes);
  const unsigned slot_words = (unsigned)(slot_bytes >> 2);

  if (tid < rows) s_ft[tid] = ftype[(size_t)b * hs + ys + tid];
  if (tid < PNG_NSYM) s_hist[tid] = tid == PNG_EOB ? 1u : 0u;
  for (int i = tid; i < PNG_STAGE; i += PNG_T) s_stage[i] = 0u;
  if (tid == 0) { s_a1 = 0ull; s_a2 = 0ull; }
  __syncthreads();

  // the filtered byte at stripe position p, 0 <= p < n
  auto value_at = [&](int p) -> int {
    const int r = p / rowlen, c = p - r * rowlen, t = s_ft[r];
    if (c == 0) return t;
    const int i = c - 1, y = ys + r;
    const unsigned char* row = rect + (size_t)y * pitch;
    const int cur = row[i];
    const int pred = t == 1 ? (i >= 3 ? (int)row[i - 3] : 0) : (y > 0 ? (int)(row - pitch)[i] : 0);
    return (cur - pred) & 255;
  };
  // nbits (1 .. 32) of value at bit `at` of the stage
  auto put = [&](int at, unsigned value, int nbits) {
    const int wd = at >> 5, sh = at & 31;
    atomicOr(&s_stage[wd], value << sh);
    if (sh + nbits > 32) atomicOr(&s_stage[wd + 1], value >> (32 - sh));
  };
  unsigned wbase = 0;      // words of the slot written so far
  int cbits = 0;           // bits of the open word, s_stage[0]
  // `add` more bits are in the stage behind the cbits carried ones: its whole words -> the slot, the open one -> s_stage[0]
  auto flush = [&](int add) {
    __syncthreads();
    const int total = cbits + add, fw = total >> 5;
    if (tid < fw && wbase + (unsigned)tid < slot_words) gout[wbase + tid] = s_stage[tid];
    const unsigned open = s_stage[fw];
    __syncthreads();
    for (int i = tid; i < PNG_STAGE; i += PNG_T) s_stage[i] = i == 0 ? open : 0u;
    wbase += (unsigned)fw;
    cbits = total & 31;
  };

  unsigned long long a1 = 0ull, a2 = 0ull;
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 1) {
      // ---- the code (rule 4) ------------------------------------------------------------------------------------------------
      for (;;) {
        if (tid < PNG_NSYM) s_len[tid] = 0;
        if (tid < 16) s_blc[tid] = 0u;
        if (tid == 0) { s_m = 0; s_maxlen = 0; }
        __syncthreads();
        const unsigned c = tid < PNG_NSYM ? s_hist[tid] : 0u;
        if (c) {
          int rank = 0;
          for (int j = 0; j < PNG_NSYM; ++j) {
            const unsigned cj = s_hist[j];
            rank += (cj && (cj < c || (cj == c && j < tid))) ? 1 : 0;
          }
          s_lw[rank] = c;
          s_ls[rank] = (unsigned short)tid;
          atomicAdd(&s_m, 1);
        }
        __syncthreads();
        const int m = s_m;                        // >= 2: a stripe has a literal and end-of-block
        if (tid == 0) {
          int li = 0, ii = 0, ni = 0;             // heads of the leaf and the internal queue, internal nodes made
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
        if (tid < m) {
          int d = 0;
          for (int node = tid; node != 2 * m - 2; node = s_parent[node]) ++d;
          s_len[s_ls[tid]] = (unsigned char)min(d, 255);
          atomicMax(&s_maxlen, d);
          if (d <= 15) atomicAdd(&s_blc[d], 1u);
        }
        __syncthreads();
        if (s_maxlen <= 15) break;                // (block-uniform: nobody changes it before the barrier below)
        if (c) s_hist[tid] = (c + 1u) >> 1;
        __syncthreads();
      }
      if (tid == 0) {
        unsigned code = 0u;
        for (int bits = 1; bits <= 15; ++bits) {
          code = (code + (bits > 1 ? s_blc[bits - 1] : 0u)) << 1;
          s_next[bits] = code;
        }
      }
      __syncthreads();
      if (tid < PNG_NSYM) {
        const int l = s_len[tid];
        unsigned code = 0u;
        if (l) {
          int rank = 0;
          for (int j = 0; j < tid; ++j) rank += s_len[j] == l ? 1 : 0;
          code = __brev(s_next[l] + (unsigned)rank) >> (32 - l);          // a code goes out from its most significant bit
        }
        s_code[tid] = code;
      }
      // ---- the block header (rule 5): 17 + 19 * 3 + 287 * 4 = 1222 bits -------------------------------------------------------
      if (tid == 0) put(0, (2u << 1) | (29u << 3) | (0u << 8) | (15u << 13), 17);
      if (tid >= 3 && tid < 19) put(17 + 3 * tid, 4u, 3);                  // (the first three, symbols 16 - 18, are 0)
      if (tid < PNG_NSYM + 1) put(74 + 4 * tid, __brev(tid < PNG_NSYM ? (unsigned)s_len[tid] : 1u) >> 28, 4);
      flush(1222);
      __syncthreads();
    }
    int carry = 0;                                // the last run start of the tiles before this one
    for (int base = 0; base < n; base += PNG_T) {
      {
        const int p = base - 1 + tid;
        s_val[tid] = (unsigned short)(p < 0 ? 0x1ff : p < n ? value_at(p) : 0x100);      // position n starts a run: the end
        if (tid <= PNG_HALO) {
          const int q = base - 1 + PNG_T + tid;
          s_val[PNG_T + tid] = (unsigned short)(q < n ? value_at(q) : 0x100);
        }
      }
      __syncthreads();
      const int p = base + tid, v = s_val[tid + 1];
      const bool st = v != (int)s_val[tid];
      const unsigned long long bal = __ballot(st);
      if (lane == 0) {
        s_mask[wave] = bal;
        s_wlast[wave] = bal ? base + wave * 64 + 63 - __clzll(bal) : -1;
      }
      if (tid < PNG_HALO) {                       // (whole waves)
        const unsigned long long bh = __ballot(s_val[PNG_T + tid + 1] != s_val[PNG_T + tid]);
        if (lane == 0) s_mask[PNG_WAVES + wave] = bh;
      }
      __syncthreads();
      int last = carry, next_carry = carry;
      {
        const unsigned long long mine = bal & (~0ull >> (63 - lane));
        bool found = mine != 0ull;
        if (found) last = base + wave * 64 + 63 - __clzll(mine);
        bool cf = false;
        for (int w2 = PNG_WAVES - 1; w2 >= 0; --w2) {
          const int x = s_wlast[w2];
          if (x >= 0) {
            if (!cf) { next_carry = x; cf = true; }
            if (!found && w2 < wave) { last = x; found = true; }
          }
        }
      }
      carry = next_carry;
      // the token of this position: sym >= 0 a literal, mlen > 0 a match, neither: nothing
      int sym = -1, mlen = 0;
      if (p < n) {
        if (st) {
          sym = v;
        } else {
          const int j = (p - last - 1) % PNG_MAXM;
          const int q = tid + 1;
          if (j == 0) {
            int d = PNG_MAXM;                     // positions to the next run start, capped: the run's remaining length from p
            const int w0 = q >> 6;
            unsigned long long mk = s_mask[w0] & (~0ull << (q & 63));
            for (int e = 0; e < 6; ++e) {
              if (mk) { d = min(((w0 + e) << 6) + __ffsll((long long)mk) - 1 - tid, PNG_MAXM); break; }
              if (w0 + e + 1 >= PNG_MASKS) break;
              mk = s_mask[w0 + e + 1];
            }
            if (d >= 3) mlen = d; else sym = v;
          } else if (j == 1) {
            if ((s_mask[q >> 6] >> (q & 63)) & 1ull) sym = v;
          }
        }
      }
      if (pass == 0) {
        if (sym >= 0) {
          atomicAdd(&s_hist[sym], 1u);
        } else if (mlen) {
          int ls, nb;
          unsigned ex;
          length_symbol(mlen, ls, ex, nb);
          atomicAdd(&s_hist[ls], 1u);
        }
        if (p < n) {
          a1 += (unsigned long long)v;
          a2 += (unsigned long long)(n - p) * (unsigned long long)v;
        }
      } else {
        unsigned tb = 0u;
        int tl = 0;
        if (sym >= 0) {
          tb = s_code[sym];
          tl = s_len[sym];
        } else if (mlen) {
          int ls, nb;
          unsigned ex;
          length_symbol(mlen, ls, ex, nb);
          const int l0 = s_len[ls];
          tb = s_code[ls] | (ex << l0);           // the code, the extra bits, the distance code 0 (one bit)
          tl = l0 + nb + 1;
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
        for (int w2 = 0; w2 < PNG_WAVES; ++w2) {
          const int sw = s_wsum[w2];
          pre += w2 < wave ? sw : 0;
          tot += sw;
        }
        if (tl) put(cbits + pre + x - tl, tb, tl);
        flush(tot);
      }
    }
    if (pass == 0) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        a1 += __shfl_down(a1, o, 64);
        a2 += __shfl_down(a2, o, 64);
      }
      if (lane == 0) {
        atomicAdd(&s_a1, a1);
        atomicAdd(&s_a2, a2);
      }
      __syncthreads();
    }
  }
  // end-of-block, the empty stored block: 000, pad to a byte, 00 00 FF FF
  __syncthreads();
  if (tid == 0) {
    int at = cbits;
    put(at, s_code[PNG_EOB], s_len[PNG_EOB]);
    at = (at + s_len[PNG_EOB] + 3 + 7) & ~7;
    put(at, 0xffff0000u, 32);
    at += 32;
    s_m = at;
  }
  __syncthreads();
  const int endbits = s_m;                        // a multiple of 8, at most 31 + 15 + 3 + 7 + 32: three words
  if (tid < ((endbits + 31) >> 5) && wbase + (unsigned)tid < slot_words) gout[wbase + tid] = s_stage[tid];
  if (tid == 0) {
    const size_t q = (size_t)b * S + s;
    sizes[q] = wbase * 4u + (unsigned)(endbits >> 3);
    parts[2 * q] = (unsigned)(s_a1 % ADLER);
    parts[2 * q + 1] = (unsigned)(s_a2 % ADLER);
  }
}

__global__ void __launch_bounds__(256) png_finish_kernel(int hs, int ws, int S, const unsigned* __restrict__ sizes,
                                                         const unsigned* __restrict__ parts, const unsigned char* __restrict__ slots,
                                                         size_t slot_bytes, unsigned char* __restrict__ out, size_t cap,
                                                         unsigned long long* __restrict__ sizes_out) {
  __shared__ unsigned long long s_off;
  const int tid = threadIdx.x, s = blockIdx.x, b = blockIdx.y;
  const unsigned* sz = sizes + (size_t)b * S;
  if (tid == 0) s_off = 2ull;
  __syncthreads();
  {
    unsigned long long mine = 0ull;
    for (int i = tid; i < s; i += 256) mine += sz[i];
    if (mine) atomicAdd(&s_off, mine);
  }
  __syncthreads();
  const size_t off = (size_t)s_off, nbytes = sz[s];
  unsigned char* img = out + (size_t)b * cap;
  if (off + nbytes + 9 > cap) return;             // (the bound rules it out; block-uniform)
  unsigned char* dst = img + off;
  const unsigned char* src = slots + ((size_t)b * S + s) * slot_bytes;                   // 16-byte aligned; ceil(nbytes / 4) words written
  const unsigned* src32 = (const unsigned*)src;
  const size_t head = min(nbytes, (size_t)((4 - ((uintptr_t)dst & 3)) & 3));
  const size_t nd = (nbytes - head) >> 2;
  if ((size_t)tid < head) dst[tid] = src[tid];
  for (size_t i = tid; i < nd; i += 256) {
    const size_t o = head + 4 * i;
    const int sh = (int)(o & 3) * 8;
    const unsigned lo = src32[o >> 2];
    *(unsigned*)(dst + o) = sh ? (lo >> sh) | (src32[(o >> 2) + 1] << (32 - sh)) : lo;   // (bytes o .. o + 3 < nbytes: both words written)
  }
  for (size_t i = head + 4 * nd + tid; i < nbytes; i += 256) dst[i] = src[i];
  if (s == 0 && tid == 0) {
    img[0] = 0x78;
    img[1] = 0x01;
  }
  if (s == S - 1 && tid == 0) {
    const unsigned rowlen = 1u + 3u * (unsigned)ws;
    unsigned long long A = 1ull, Bv = 0ull;
    for (int i = 0; i < S; ++i) {
      const unsigned long long ni = (unsigned long long)min(PNG_ROWS, hs - i * PNG_ROWS) * rowlen;
      const size_t q = (size_t)b * S + i;
      Bv = (Bv + (ni % ADLER) * A + parts[2 * q + 1]) % ADLER;
      A = (A + parts[2 * q]) % ADLER;
    }
    unsigned char* t = dst + nbytes;
    t[0] = 0x01; t[1] = 0x00; t[2] = 0x00; t[3] = 0xff; t[4] = 0xff;
    t[5] = (unsigned char)(Bv >> 8); t[6] = (unsigned char)(Bv & 255u); t[7] = (unsigned char)(A >> 8); t[8] = (unsigned char)(A & 255u);
    sizes_out[b] = (unsigned long long)(off + nbytes + 9);
  }
}

}  // namespace

int png_stripes(int hs) { return (hs + PNG_ROWS - 1) / PNG_ROWS; }

size_t png_stripe_bound(size_t n) { return 159 + (15 * n + 7) / 8; }

// a slot holds the largest stripe's bound, rounded up to 16 bytes (the stage is flushed in whole words)
size_t png_slot_bytes(int ws) { return (png_stripe_bound((size_t)PNG_ROWS * (1 + 3 * (size_t)ws)) + 15) & ~(size_t)15; }

hipError_t launch_png_rows(const se_window* d_wins, int B, int hs, int ws, unsigned char* ftype, hipStream_t st) {
  const long rows = (long)B * hs;
  // bytes: every row read twice (as itself and as the row above), a type written per row
  set_launch_cost(0.0, (double)rows * (6.0 * ws + 1.0), "png_rows");
  set_launch_grid((rows + 3) / 4);
  ProfScope ps_(st, PL_PNG_ROWS);
  hipLaunchKernelGGL(png_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, d_wins, B, hs, ws, ftype);
  return hipGetLastError();
}

hipError_t launch_png_stripes(const se_window* d_wins, int B, int hs, int ws, const unsigned char* ftype, unsigned* sizes, unsigned* parts,
                              unsigned char* slots, hipStream_t st) {
  const int S = png_stripes(hs);
  // bytes: two walks, each reading a byte and its predictor; the slots written (an upper bound: the bytes themselves)
  set_launch_cost(0.0, (double)B * hs * (1.0 + 3.0 * ws) * 5.0, "png_stripes");
  set_launch_grid((long)S * B);
  ProfScope ps_(st, PL_PNG_STRIPES);
  hipLaunchKernelGGL(png_stripe_kernel, dim3((unsigned)S, (unsigned)B), dim3(PNG_T), 0, st, d_wins, hs, ws, S, ftype, sizes, parts, slots,
                     png_slot_bytes(ws));
  return hipGetLastError();
}

hipError_t launch_png_finish(int B, int hs, int ws, const unsigned* sizes, const unsigned* parts, const unsigned char* slots, unsigned char* out,
                             size_t cap, unsigned long long* sizes_out, hipStream_t st) {
  const int S = png_stripes(hs);
  set_launch_cost(0.0, (double)B * hs * (1.0 + 3.0 * ws) * 2.0, "png_finish");
  set_launch_grid((long)S * B);
  ProfScope ps_(st, PL_PNG_FINISH);
  hipLaunchKernelGGL(png_finish_kernel, dim3((unsigned)S, (unsigned)B), dim3(256), 0, st, hs, ws, S, sizes, parts, slots, png_slot_bytes(ws), out,
                     cap, sizes_out);
  return hipGetLastError();
}

}  // namespace se
