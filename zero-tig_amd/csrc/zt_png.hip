// Result PNGs of predict.py / evals.py encoded on the device (predict.py:57-61, 101-104: `Image.fromarray(..).save(.., "PNG")`):
// the quantised [H][W][3] uint8 frame becomes a finished zlib stream; the host only frames it as PNG chunks (CRC-32) and writes.
//   scanlines: filter type 4 (Paeth) on every row, neighbours outside the image are 0, the left neighbour is 3 bytes back.
//   blocks:    PNG_R rows = one dynamic-Huffman deflate block (BTYPE 2) of literals + end-of-block only (no LZ77 matching), with
//              its own canonical code of at most 15 bits, built by the workgroup that packs the block.  A non-final block is
//              followed by an empty stored block (bits 000, pad, 00 00 FF FF), so every block starts on a byte boundary and is
//              produced independently into a worst-case sized slot; a second kernel gathers the slots behind the zlib header.
//   header:    BFINAL, BTYPE = 2, HLIT = 0 (257 codes), HDIST = 0, HCLEN = 15; code-length-code lengths 0 for 16..18 and 4 for 0..15
//              (a complete 4-bit code: each of the 257 + 1 lengths that follow is its own 4-bit value, bit-reversed).
//   checksum:  Adler-32 from per-block integer partials a_k = sum d_i, b_k = sum (n_k - i) d_i, combined in block order.
//   mode 2:    the same scanlines, blocks, slots and gather; per block a second candidate tokenisation with run-length matches
//              (zlib's Z_RLE idea): a run is a maximal stretch of equal bytes inside the block (it may cross row ends, never the
//              block); its first byte is a literal, the other L - 1 bytes are cut from the run's start into chunks of 258; a chunk
//              of 3..258 bytes is one match (length, distance 1), a final chunk of 1 or 2 bytes is literals.  Its code covers the
//              286 literal/length symbols (HLIT = 29), length extra bits as in RFC 1951, one distance code of length 1 (HDIST = 0),
//              so its header is 116 bits longer.  The block is written that way only where its total bit count, header included,
//              is strictly smaller than the literal-only one; otherwise it is written exactly as mode 1 writes it.
// Bit fields are deposited into 32-bit words; words shared between threads receive disjoint fields through atomicAdd on
// zeroed memory (an OR, and deterministic).  Everything is integer: the same input gives the same bytes.
#include "zt_common.h"

namespace {

constexpr int PNG_T = 256;                   // threads per workgroup
constexpr int PNG_R = 8;                     // scanlines per deflate block
constexpr int PNG_SPT = 32;                   // symbols per thread and chunk of the packing loop
constexpr int PNG_CH = PNG_T * PNG_SPT;
constexpr int PNG_RUNW = PNG_SPT / 4 + 1;      // LDS words per staged run (odd stride)
constexpr int PNG_NSYM = 257;                // 256 literals + end-of-block
constexpr int PNG_EOB = 256;
constexpr int PNG_MAXLEN = 15;
constexpr int PNG_HDR_BITS = 3 + 5 + 5 + 4 + 19 * 3 + (PNG_NSYM + 1) * 4;      // 1106
constexpr int PNG_NLL = 286;                 // mode 2: literals, end-of-block and the 29 length symbols
constexpr int PNG_HDR_BITS_RLE = 3 + 5 + 5 + 4 + 19 * 3 + (PNG_NLL + 1) * 4;   // 1222
constexpr int PNG_MAXMATCH = 258;
constexpr unsigned PNG_ADLER_MOD = 65521u;

struct PngPlan {
  int nblk;
  long long row_bytes;                       // 1 + 3 W
  size_t slot_bytes;                         // capacity of one block's slot
  size_t off_slots, off_counts, off_adler;   // workspace offsets (filtered scanlines start at 0)
  size_t ws_bytes, out_bytes;
};

inline PngPlan png_plan(int H, int W) {
  PngPlan p;
  p.nblk = (H + PNG_R - 1) / PNG_R;
  p.row_bytes = 1 + 3LL * W;
  const long long nsym = (long long)PNG_R * p.row_bytes + 1;
  // header + 15 bits per symbol + stored-block tail, plus two words of slack for the zero fill; multiple of 16
  p.slot_bytes = (size_t)(((PNG_HDR_BITS + PNG_MAXLEN * nsym + 3 + 7) / 8 + 4 + 8 + 15) & ~15LL);
  p.off_slots = (size_t)(((long long)H * p.row_bytes + 15) & ~15LL);
  p.off_counts = p.off_slots + (size_t)p.nblk * p.slot_bytes;
  p.off_adler = (p.off_counts + (size_t)p.nblk * 4 + 15) & ~(size_t)15;
  p.ws_bytes = p.off_adler + (size_t)p.nblk * 16;
  p.out_bytes = (2 + (size_t)p.nblk * p.slot_bytes + 4 + 15) & ~(size_t)15;
  return p;
}

__device__ __forceinline__ unsigned png_bitrev(unsigned v, int n) {
  unsigned r = 0;
  for (int i = 0; i < n; ++i) {
    r = (r << 1) | (v & 1u);
    v >>= 1;
  }
  return r;
}

// add the n-bit field v at bit position `pos` of the zeroed word array (may straddle two words)
__device__ __forceinline__ void png_put(unsigned* words, long long pos, unsigned v, int n) {
  const long long w = pos >> 5;
  const int sh = (int)(pos & 31);
  atomicAdd(&words[w], v << sh);
  if (sh + n > 32) atomicAdd(&words[w + 1], v >> (32 - sh));
}

// Canonical Huffman code of at most 15 bits for the NS-bin histogram `hist` (LDS), by the whole workgroup: rank sort of the
// occurring symbols, the in-place minimum-redundancy construction of Moffat and Katajainen on the sorted counts (thread 0),
// lengths above 15 folded back until the Kraft sum is exactly 1 (thread 0), canonical codes in parallel.
// -> tab[s] = bit-reversed code | length << 16 (0 for symbols that do not occur).  A histogram with a single occurring symbol
// gets a second, unused one-bit code so that the code is complete.  Bins that are zero do not enter the construction: the code of
// a 257-symbol histogram padded to 286 bins is the code of the 257 bins.
template <int NS>
__device__ void png_build_code(const unsigned* hist, unsigned* tab) {
  __shared__ unsigned skey[NS];
  __shared__ unsigned short ssym[NS];
  __shared__ unsigned char slen[NS];
  __shared__ int ncodes[NS + 3];
  __shared__ unsigned next_code[PNG_MAXLEN + 1];
  __shared__ int nused_s;
  const int t = threadIdx.x;
  for (int s = t; s < NS; s += PNG_T) slen[s] = 0;
  if (t == 0) nused_s = 0;
  __syncthreads();
  for (int s = t; s < NS; s += PNG_T) {
    const unsigned h = hist[s];
    if (h) {
      int r = 0;
      for (int j = 0; j < NS; ++j) {
        const unsigned hj = hist[j];
        r += (hj != 0 && (hj < h || (hj == h && j < s))) ? 1 : 0;
      }
      skey[r] = h;
      ssym[r] = (unsigned short)s;
      atomicAdd(&nused_s, 1);
    }
  }
  __syncthreads();
  if (t == 0) {
    const int n = nused_s;
    for (int i = 0; i < NS + 3; ++i) ncodes[i] = 0;
    if (n == 1) {
      slen[ssym[0]] = 1;
      slen[ssym[0] == 0 ? 1 : 0] = 1;
      ncodes[1] = 2;
    } else if (n >= 2) {
      unsigned* A = skey;                    // ascending counts -> code lengths, in place
      A[0] += A[1];
      int root = 0, leaf = 2, next;
      for (next = 1; next < n - 1; ++next) {
        if (leaf >= n || A[root] < A[leaf]) {
          A[next] = A[root];
          A[root++] = (unsigned)next;
        } else {
          A[next] = A[leaf++];
        }
        if (leaf >= n || (root < next && A[root] < A[leaf])) {
          A[next] += A[root];
          A[root++] = (unsigned)next;
        } else {
          A[next] += A[leaf++];
        }
      }
      A[n - 2] = 0;
      for (next = n - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
      int avbl = 1, used = 0, dpth = 0;
      root = n - 2;
      next = n - 1;
      while (avbl > 0) {
        while (root >= 0 && (int)A[root] == dpth) {
          ++used;
          --root;
        }
        while (avbl > used) {
          A[next--] = (unsigned)dpth;
          --avbl;
        }
        avbl = 2 * used;
        ++dpth;
        used = 0;
      }
      for (int i = 0; i < n; ++i) ncodes[A[i]]++;          // depths are at most n - 1 < NS
      // length limit: fold the deeper leaves into level 15, then move leaves down until the Kraft sum is 2^15 / 2^15
      for (int i = PNG_MAXLEN + 1; i < NS + 3; ++i) {
        ncodes[PNG_MAXLEN] += ncodes[i];
        ncodes[i] = 0;
      }
      unsigned total = 0;
      for (int i = PNG_MAXLEN; i > 0; --i) total += (unsigned)ncodes[i] << (PNG_MAXLEN - i);
      while (total != (1u << PNG_MAXLEN)) {
        ncodes[PNG_MAXLEN]--;
        for (int i = PNG_MAXLEN - 1; i > 0; --i)
          if (ncodes[i]) {
            ncodes[i]--;
            ncodes[i + 1] += 2;
            break;
          }
        --total;
      }
      // the sorted order is ascending: the most frequent symbols take the shortest lengths
      int j = n;
      for (int i = 1; i <= PNG_MAXLEN; ++i)
        for (int l = ncodes[i]; l > 0; --l) slen[ssym[--j]] = (unsigned char)i;
    }
    unsigned code = 0;
    next_code[0] = 0;
    for (int l = 1; l <= PNG_MAXLEN; ++l) {
      code = (code + (unsigned)ncodes[l - 1]) << 1;
      next_code[l] = code;
    }
  }
  __syncthreads();
  for (int s = t; s < NS; s += PNG_T) {
    const int l = slen[s];
    unsigned v = 0;
    if (l) {
      unsigned c = next_code[l];
      for (int j = 0; j < s; ++j) c += (slen[j] == l) ? 1u : 0u;
      v = png_bitrev(c, l) | ((unsigned)l << 16);
    }
    tab[s] = v;
  }
  __syncthreads();
}

__device__ __forceinline__ int png_paeth(int a, int b, int c) {
  const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// length 3..258 -> literal/length symbol, number of extra bits and their value (RFC 1951, 3.2.5)
__device__ __forceinline__ void png_len_code(int L, int& sym, int& eb, unsigned& ev) {
  const int m = L - 3;
  if (L == PNG_MAXMATCH) {
    sym = 285, eb = 0, ev = 0;
  } else if (m < 8) {
    sym = 257 + m, eb = 0, ev = 0;
  } else {
    eb = 29 - __builtin_clz((unsigned)m);    // floor(log2 m) - 2
    sym = 261 + 4 * eb + ((m >> eb) & 3);
    ev = (unsigned)m & ((1u << eb) - 1u);
  }
}
__device__ __forceinline__ int png_len_extra(int sym) { return (sym < 265 || sym == 285) ? 0 : (sym - 261) >> 2; }

// Workgroup scan of one value per thread, sum or maximum (of unsigned, identity 0): shuffles inside a wave, the wave totals through
// `wtot` (PNG_T / 64 words of LDS); two barriers.  -> the value over the threads before this one; `total` over all of them.
template <bool MAX>
__device__ __forceinline__ unsigned png_scan_excl(unsigned v, unsigned* wtot, unsigned& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned x = __shfl(v, (lane - o) & 63);
    if (lane >= o) v = MAX ? max(v, x) : v + x;
  }
  const unsigned up = __shfl(v, (lane - 1) & 63);
  unsigned excl = lane > 0 ? up : 0u;
  if (lane == 63) wtot[wv] = v;
  __syncthreads();
  total = 0;
  for (int i = 0; i < PNG_T / 64; ++i) {
    const unsigned x = wtot[i];
    if (i < wv) excl = MAX ? max(excl, x) : excl + x;
    total = MAX ? max(total, x) : total + x;
  }
  __syncthreads();
  return excl;
}

// Positions [c0, c0 + PNG_CH) of the block's filtered bytes into the LDS stage with coalesced loads: thread t's run of PNG_SPT
// bytes lies at a stride of 9 words, so the runs are read without bank conflicts.  Ends with a barrier.
__device__ __forceinline__ void png_stage_chunk(const unsigned char* f, long long n, long long c0, unsigned* stage) {
  const int t = threadIdx.x;
  unsigned char* stb = reinterpret_cast<unsigned char*>(stage);
  for (int j = 0; j < PNG_SPT; ++j) {
    const int li = t + PNG_T * j;
    if (c0 + li < n) stb[(li / PNG_SPT) * (4 * PNG_RUNW) + (li % PNG_SPT)] = f[c0 + li];
  }
  __syncthreads();
}

// one thread's PNG_SPT positions of a packing chunk for the run tokenisation (the bytes stay in the LDS stage): the number of them
// inside the block, the byte before and the byte after (-1: none), and qprev = where the position before the first one stands in
// its run's chunk of 258, only read when the first byte continues the run.  With d = distance of the first position from its run
// start, qprev = (d - 1) % 258 - 1: that is -1 both when the position before is the run's first byte and when it is the 258th
// byte of a chunk (where 257 would be the plain value); png_rle_walk steps -1 and 257 alike to 0 on a byte that continues the run.
struct PngRun {
  int cnt, prev, look, qprev;
};

// Stages chunk c0 of the block's filtered bytes like the packing loop and finds every position's run start: a thread notes its
// last position that differs from the byte before it, a workgroup max-scan hands each thread the last such position before its
// own, `carry` the one of the chunks before.  The stage is read by png_rle_walk: a barrier has to follow before it is rewritten.
__device__ __forceinline__ void png_rle_chunk(const unsigned char* f, long long n, long long c0, unsigned* stage, unsigned* wtot,
                                              long long& carry, PngRun& u) {
  const int t = threadIdx.x;
  png_stage_chunk(f, n, c0, stage);
  const long long r0 = c0 + (long long)t * PNG_SPT;
  u.cnt = (int)max(0LL, min((long long)PNG_SPT, n - r0));
  u.prev = (u.cnt > 0 && r0 > 0) ? (int)f[r0 - 1] : -1;
  u.look = r0 + PNG_SPT < n ? (int)f[r0 + PNG_SPT] : -1;
  unsigned ls = 0;                           // 1 + chunk-relative index of the last run start among this thread's positions
  int pv = u.prev;
#pragma unroll 1
  for (int q = 0; q < PNG_SPT / 4; ++q) {
    const unsigned w = stage[t * PNG_RUNW + q];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = 4 * q + i, b = (int)((w >> (8 * i)) & 255u);
      if (j < u.cnt && b != pv) ls = (unsigned)(t * PNG_SPT + j + 1);
      pv = b;
    }
  }
  unsigned all;
  const unsigned before = png_scan_excl<true>(ls, wtot, all);
  const long long start = before ? c0 + before - 1 : carry;
  if (all) carry = c0 + all - 1;
  u.qprev = -1;
  if (u.cnt > 0 && (int)(stage[t * PNG_RUNW] & 255u) == u.prev) u.qprev = (int)((unsigned)(r0 - start - 1) % (unsigned)PNG_MAXMATCH) - 1;
}

// tokens of the thread's positions in order: emit(nlit, byte, 0) for one or two literals, emit(0, byte, length) for a match.  The
// token of a chunk comes from the chunk's last position: the 258th byte after the run's first, the last byte of the block, or
// the one before a different byte.
template <class F>
__device__ __forceinline__ void png_rle_walk(const unsigned* stage, const PngRun& u, F&& emit) {
  int q = u.qprev, pv = u.prev;
  const unsigned* run = stage + threadIdx.x * PNG_RUNW;
  unsigned w = run[0];
#pragma unroll 1
  for (int k = 0; k < PNG_SPT / 4; ++k) {
    const unsigned wn = run[k + 1];          // the ninth word of a run is padding: read, never used
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = 4 * k + i;
      if (j < u.cnt) {
        const int b = (int)((w >> (8 * i)) & 255u);
        const int nx = j + 1 < u.cnt ? (int)((i < 3 ? w >> (8 * i + 8) : wn) & 255u) : u.look;
        q = b != pv ? -1 : (q == PNG_MAXMATCH - 1 ? 0 : q + 1);
        if (q < 0) emit(1, b, 0);
        else if (q == PNG_MAXMATCH - 1 || nx != b) {
          if (q >= 2) emit(0, b, q + 1);
          else emit(q + 1, b, 0);
        }
        pv = b;
      }
    }
    w = wn;
  }
}

// the block's tokens of the run tokenisation behind its header, PNG_CH positions at a time like the literal-only packing: bit
// counts summed per thread, a workgroup scan for the bit offsets, fields (two literals: at most 30 bits, a match: at most
// 15 + 5 + 1) deposited through the 64-bit accumulator; end-of-block last
__device__ void png_pack_rle(const unsigned char* f, long long n, unsigned* words, const unsigned* tabb, unsigned* stage,
                             unsigned* wtot) {
  const int t = threadIdx.x;
  const long long nsym = n + 1;
  long long base = PNG_HDR_BITS_RLE, carry = 0;
  for (long long c0 = 0; c0 < nsym; c0 += PNG_CH) {
    PngRun u;
    png_rle_chunk(f, n, c0, stage, wtot, carry, u);
    const long long r0 = c0 + (long long)t * PNG_SPT;
    const bool eob = r0 <= n && n < r0 + PNG_SPT;
    unsigned nb = eob ? tabb[PNG_EOB] >> 16 : 0;
    png_rle_walk(stage, u, [&](int nlit, int b, int len) {
      if (len) {
        int sym, eb;
        unsigned ev;
        png_len_code(len, sym, eb, ev);
        nb += (tabb[sym] >> 16) + (unsigned)eb + 1u;
      } else {
        nb += (unsigned)nlit * (tabb[b] >> 16);
      }
    });
    unsigned chunk_bits;
    const long long start = base + png_scan_excl<false>(nb, wtot, chunk_bits);
    base += chunk_bits;
    long long w = start >> 5;
    int nacc = (int)(start & 31);
    unsigned long long acc = 0;
    bool first = true;
    auto put = [&](unsigned long long v, int nbits) {
      acc |= v << nacc;
      nacc += nbits;
      if (nacc >= 32) {
        if (first) atomicAdd(&words[w], (unsigned)acc);              // shared with the run before
        else words[w] = (unsigned)acc;                               // every bit of an interior word is this thread's
        first = false;
        acc >>= 32;
        nacc -= 32;
        ++w;
      }
    };
    png_rle_walk(stage, u, [&](int nlit, int b, int len) {
      if (len) {
        int sym, eb;
        unsigned ev;
        png_len_code(len, sym, eb, ev);
        const unsigned e = tabb[sym];
        const int l = (int)(e >> 16);
        put((unsigned long long)(e & 0xFFFFu) | ((unsigned long long)ev << l), l + eb + 1);   // distance code: one 0 bit
      } else {
        const unsigned e = tabb[b];
        const int l = (int)(e >> 16);
        const unsigned long long c = e & 0xFFFFu;
        put(nlit == 2 ? c | (c << l) : c, nlit * l);
      }
    });
    if (eob) put(tabb[PNG_EOB] & 0xFFFFu, (int)(tabb[PNG_EOB] >> 16));
    if (nb > 0 && nacc > 0) atomicAdd(&words[w], (unsigned)acc);
    __syncthreads();                                                 // the stage is rewritten by the next chunk
  }
}

// workgroup k: rows [k R, min(H, (k + 1) R)) -> filtered scanlines (workspace), histogram, code, packed deflate block in slot k,
// its byte count and Adler partials.  MODE 2 also counts the symbols of the run tokenisation, builds their code and packs the
// block with it where that is strictly shorter.
template <int MODE>
__global__ void __launch_bounds__(PNG_T) png_block_kernel(const unsigned char* __restrict__ src, int H, int W, unsigned char* filt,
                                                          unsigned char* slots, size_t slot_bytes, unsigned* __restrict__ counts,
                                                          unsigned long long* __restrict__ adler) {
  constexpr int NS = MODE == 2 ? PNG_NLL : PNG_NSYM;
  __shared__ unsigned hist[4][NS + 3];
  __shared__ unsigned tab[NS];
  __shared__ unsigned tabb[MODE == 2 ? PNG_NLL : 1];
  __shared__ unsigned long long red[2][PNG_T];
  __shared__ unsigned wtot[PNG_T / 64];
  __shared__ unsigned stage[PNG_T * PNG_RUNW];
  const int t = threadIdx.x, k = blockIdx.x;
  const long long rb = 1 + 3LL * W, rowpix = 3LL * W;
  const int y0 = k * PNG_R, rows = min(PNG_R, H - y0);
  const long long n = rows * rb;
  unsigned char* f = filt + (size_t)y0 * rb;

  for (int i = t; i < 4 * (NS + 3); i += PNG_T) (&hist[0][0])[i] = 0;
  __syncthreads();
  unsigned long long sa = 0, sb = 0;
  for (int r = 0; r < rows; ++r) {
    const int y = y0 + r;
    const unsigned char* row = src + (size_t)y * rowpix;
    for (long long c = t; c < rb; c += PNG_T) {
      int d = 4;
      if (c > 0) {
        const long long x = c - 1;
        const unsigned char* p = row + x;
        const int cur = p[0];
        const int a = x >= 3 ? p[-3] : 0;
        const int b = y > 0 ? p[-rowpix] : 0;
        const int cc = (y > 0 && x >= 3) ? p[-rowpix - 3] : 0;
        d = (cur - png_paeth(a, b, cc)) & 255;
      }
      const long long i = r * rb + c;
      f[i] = (unsigned char)d;
      atomicAdd(&hist[t >> 6][d], 1u);
      sa += (unsigned)d;
      sb += (unsigned long long)(n - i) * (unsigned)d;
    }
  }
  red[0][t] = sa;
  red[1][t] = sb;
  __syncthreads();
  for (int s = t; s < PNG_NSYM; s += PNG_T) hist[0][s] += hist[1][s] + hist[2][s] + hist[3][s];
  for (int s = PNG_T / 2; s > 0; s >>= 1) {
    if (t < s) {
      red[0][t] += red[0][t + s];
      red[1][t] += red[1][t + s];
    }
    __syncthreads();
  }
  if (t == 0) {
    hist[0][PNG_EOB] = 1;
    adler[2 * k] = red[0][0];
    adler[2 * k + 1] = red[1][0];
  }
  __threadfence();                           // the filtered bytes are read back below by other threads of this workgroup
  __syncthreads();
  png_build_code<NS>(hist[0], tab);

  // size of the block from the histogram: sum of count x length
  const long long nsym = n + 1;
  unsigned long long bits = 0;
  for (int s = t; s < PNG_NSYM; s += PNG_T) bits += (unsigned long long)hist[0][s] * (tab[s] >> 16);
  red[0][t] = bits;
  __syncthreads();
  for (int s = PNG_T / 2; s > 0; s >>= 1) {
    if (t < s) red[0][t] += red[0][t + s];
    __syncthreads();
  }
  const bool last = k == (int)gridDim.x - 1;
  long long end_bits = PNG_HDR_BITS + (long long)red[0][0];
  bool rle = false;
  if constexpr (MODE == 2) {
    // the other candidate: histogram of the run tokenisation, its code, its size with extra bits and one distance bit per match
    for (int i = t; i < 4 * (NS + 3); i += PNG_T) (&hist[0][0])[i] = 0;
    __syncthreads();
    long long carry = 0;
    for (long long c0 = 0; c0 < n; c0 += PNG_CH) {
      PngRun u;
      png_rle_chunk(f, n, c0, stage, wtot, carry, u);
      unsigned* h = hist[t >> 6];
      png_rle_walk(stage, u, [&](int nlit, int b, int len) {
        if (len) {
          int sym, eb;
          unsigned ev;
          png_len_code(len, sym, eb, ev);
          atomicAdd(&h[sym], 1u);
        } else {
          atomicAdd(&h[b], (unsigned)nlit);
        }
      });
      __syncthreads();                       // the stage is rewritten by the next chunk
    }
    unsigned long long nmatch = 0;
    for (int s = t; s < NS; s += PNG_T) {
      hist[0][s] += hist[1][s] + hist[2][s] + hist[3][s];
      if (s == PNG_EOB) hist[0][s] = 1;
      if (s > PNG_EOB) nmatch += hist[0][s];
    }
    red[1][t] = nmatch;
    __syncthreads();
    for (int s = PNG_T / 2; s > 0; s >>= 1) {
      if (t < s) red[1][t] += red[1][t + s];
      __syncthreads();
    }
    if (red[1][0] > 0) {                     // without a match the longer header alone decides
      png_build_code<NS>(hist[0], tabb);
      bits = 0;
      for (int s = t; s < NS; s += PNG_T)
        bits += (unsigned long long)hist[0][s] * ((tabb[s] >> 16) + (unsigned)png_len_extra(s) + (s > PNG_EOB ? 1u : 0u));
      red[0][t] = bits;
      __syncthreads();
      for (int s = PNG_T / 2; s > 0; s >>= 1) {
        if (t < s) red[0][t] += red[0][t + s];
        __syncthreads();
      }
      const long long rle_bits = PNG_HDR_BITS_RLE + (long long)red[0][0];
      if (rle_bits < end_bits) {
        rle = true;
        end_bits = rle_bits;
      }
    }
  }
  const long long nbytes = last ? (end_bits + 7) >> 3 : ((end_bits + 3 + 7) >> 3) + 4;
  unsigned* words = reinterpret_cast<unsigned*>(slots + (size_t)k * slot_bytes);
  const long long nwords = (nbytes + 3) / 4 + 1;
  for (long long w = t; w < nwords; w += PNG_T) words[w] = 0;
  __threadfence();
  __syncthreads();

  // header
  if (t == 0) {
    png_put(words, 0, (last ? 1u : 0u) | (2u << 1), 3);
    if (rle) png_put(words, 3, (unsigned)(PNG_NLL - 257), 5);         // HLIT = 29
    png_put(words, 13, 15u, 4);                                       // HDIST = 0 (and HLIT = 0 without matches) stay zero
    for (int i = 3; i < 19; ++i) png_put(words, 17 + 3 * i, 4u, 3);    // symbols 16, 17, 18 first: length 0
    counts[k] = (unsigned)nbytes;
    if (!last) png_put(words, (nbytes - 2) * 8, 0xFFFFu, 16);          // stored block: LEN = 0, NLEN = 0xFFFF
  }
  if (!rle)
    for (int s = t; s < PNG_NSYM; s += PNG_T) png_put(words, 74 + 4 * s, png_bitrev(tab[s] >> 16, 4), 4);   // distance length: 0

  if constexpr (MODE == 2) {
    if (rle) {
      for (int s = t; s < PNG_NLL; s += PNG_T) png_put(words, 74 + 4 * s, png_bitrev(tabb[s] >> 16, 4), 4);
      if (t == 0) png_put(words, 74 + 4 * PNG_NLL, png_bitrev(1u, 4), 4);   // the one distance code: length 1
      png_pack_rle(f, n, words, tabb, stage, wtot);
      return;
    }
  }

  // symbols, PNG_CH at a time: staged in LDS, lengths summed per thread, a workgroup scan for the bit offsets, codes deposited
  long long base = PNG_HDR_BITS;
  for (long long c0 = 0; c0 < nsym; c0 += PNG_CH) {
    png_stage_chunk(f, n, c0, stage);
    const long long r0 = c0 + (long long)t * PNG_SPT;
    const int cnt = (int)max(0LL, min((long long)PNG_SPT, nsym - r0));
    unsigned r[PNG_SPT / 4];
#pragma unroll
    for (int q = 0; q < PNG_SPT / 4; ++q) r[q] = stage[t * PNG_RUNW + q];
    unsigned nb = 0;
#pragma unroll
    for (int j = 0; j < PNG_SPT; ++j)
      if (j < cnt) nb += tab[r0 + j < n ? (r[j >> 2] >> (8 * (j & 3))) & 255u : (unsigned)PNG_EOB] >> 16;
    unsigned chunk_bits;
    const long long start = base + png_scan_excl<false>(nb, wtot, chunk_bits);
    base += chunk_bits;
    long long w = start >> 5;
    int nacc = (int)(start & 31);
    unsigned long long acc = 0;
    bool first = true;
#pragma unroll
    for (int j = 0; j < PNG_SPT; ++j) {
      if (j < cnt) {
        const unsigned e = tab[r0 + j < n ? (r[j >> 2] >> (8 * (j & 3))) & 255u : (unsigned)PNG_EOB];
        acc |= (unsigned long long)(e & 0xFFFFu) << nacc;
        nacc += (int)(e >> 16);
        if (nacc >= 32) {
          if (first) atomicAdd(&words[w], (unsigned)acc);              // shared with the run before
          else words[w] = (unsigned)acc;                               // every bit of an interior word is this thread's
          first = false;
          acc >>= 32;
          nacc -= 32;
          ++w;
        }
      }
    }
    if (cnt > 0 && nacc > 0) atomicAdd(&words[w], (unsigned)acc);
    __syncthreads();                                                   // the stage is rewritten by the next chunk
  }
}

// workgroup k copies slot k behind the zlib header and the blocks before it; the last one appends the Adler-32 and the size
__global__ void __launch_bounds__(PNG_T) png_gather_kernel(const unsigned char* __restrict__ slots, size_t slot_bytes,
                                                           const unsigned* __restrict__ counts,
                                                           const unsigned long long* __restrict__ adler, int H, int W,
                                                           unsigned char* __restrict__ out, unsigned* __restrict__ nbytes_out) {
  __shared__ unsigned long long red[PNG_T];
  const int t = threadIdx.x, k = blockIdx.x, nblk = gridDim.x;
  unsigned long long s = 0;
  for (int j = t; j < k; j += PNG_T) s += counts[j];
  red[t] = s;
  __syncthreads();
  for (int o = PNG_T / 2; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  const unsigned long long off = red[0];
  const unsigned char* sp = slots + (size_t)k * slot_bytes;
  unsigned char* dp = out + 2 + off;
  const long long n = counts[k];
  const long long head = min(n, (long long)((4 - ((uintptr_t)dp & 3)) & 3));
  const long long nw = (n - head) / 4;
  if (t < head) dp[t] = sp[t];
  for (long long wi = t; wi < nw; wi += PNG_T) {
    const long long i = head + 4 * wi;
    *reinterpret_cast<unsigned*>(dp + i) =
        (unsigned)sp[i] | ((unsigned)sp[i + 1] << 8) | ((unsigned)sp[i + 2] << 16) | ((unsigned)sp[i + 3] << 24);
  }
  for (long long i = head + 4 * nw + t; i < n; i += PNG_T) dp[i] = sp[i];
  if (t == 0 && k == 0) {
    out[0] = 0x78;                           // deflate, 32 KiB window
    out[1] = 0x01;                           // FCHECK, no preset dictionary, fastest
  }
  if (t == 0 && k == nblk - 1) {
    const unsigned long long rb = 1 + 3ULL * W;
    unsigned long long A = 1, B = 0;
    for (int j = 0; j < nblk; ++j) {
      const unsigned long long nj = (unsigned long long)min(PNG_R, H - j * PNG_R) * rb;
      B = (B + (nj % PNG_ADLER_MOD) * A + adler[2 * j + 1] % PNG_ADLER_MOD) % PNG_ADLER_MOD;
      A = (A + adler[2 * j] % PNG_ADLER_MOD) % PNG_ADLER_MOD;
    }
    unsigned char* e = dp + n;
    e[0] = (unsigned char)(B >> 8);
    e[1] = (unsigned char)B;
    e[2] = (unsigned char)(A >> 8);
    e[3] = (unsigned char)A;
    nbytes_out[0] = (unsigned)(2 + off + n + 4);
  }
}

__global__ void __launch_bounds__(PNG_T) png_code_lengths_kernel(const unsigned* __restrict__ hist, unsigned char* __restrict__ len) {
  __shared__ unsigned h[PNG_NSYM];
  __shared__ unsigned tab[PNG_NSYM];
  for (int s = threadIdx.x; s < PNG_NSYM; s += PNG_T) h[s] = hist[s];
  __syncthreads();
  png_build_code<PNG_NSYM>(h, tab);
  for (int s = threadIdx.x; s < PNG_NSYM; s += PNG_T) len[s] = (unsigned char)(tab[s] >> 16);
}

}  // namespace

extern "C" int zt_png_sizes(int H, int W, size_t* ws_bytes, size_t* out_bytes) {
  ZT_REQUIRE(H > 0 && W > 0 && ws_bytes && out_bytes);
  const PngPlan p = png_plan(H, W);
  ZT_REQUIRE(p.out_bytes < (1ULL << 32));    // the byte count is a 32-bit device scalar
  *ws_bytes = p.ws_bytes;
  *out_bytes = p.out_bytes;
  return ZT_OK;
}

extern "C" int zt_png_encode_u8_mode(const unsigned char* src, int H, int W, int mode, void* ws, size_t ws_bytes, unsigned char* out,
                                     size_t out_bytes, unsigned* nbytes, hipStream_t stream) {
  ZT_REQUIRE(src && ws && out && nbytes && H > 0 && W > 0 && (mode == 1 || mode == 2));
  const PngPlan p = png_plan(H, W);
  ZT_REQUIRE(p.out_bytes < (1ULL << 32) && ws_bytes >= p.ws_bytes && out_bytes >= p.out_bytes);
  ZT_REQUIRE(((uintptr_t)ws & 15) == 0 && ((uintptr_t)out & 3) == 0);
  unsigned char* base = static_cast<unsigned char*>(ws);
  unsigned* counts = reinterpret_cast<unsigned*>(base + p.off_counts);
  unsigned long long* adler = reinterpret_cast<unsigned long long*>(base + p.off_adler);
  if (mode == 2)
    hipLaunchKernelGGL(png_block_kernel<2>, dim3(p.nblk), dim3(PNG_T), 0, stream, src, H, W, base, base + p.off_slots, p.slot_bytes, counts,
                       adler);
  else
    hipLaunchKernelGGL(png_block_kernel<1>, dim3(p.nblk), dim3(PNG_T), 0, stream, src, H, W, base, base + p.off_slots, p.slot_bytes, counts,
                       adler);
  hipLaunchKernelGGL(png_gather_kernel, dim3(p.nblk), dim3(PNG_T), 0, stream, (const unsigned char*)(base + p.off_slots), p.slot_bytes,
                     (const unsigned*)counts, (const unsigned long long*)adler, H, W, out, nbytes);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}

extern "C" int zt_png_encode_u8(const unsigned char* src, int H, int W, void* ws, size_t ws_bytes, unsigned char* out, size_t out_bytes,
                                unsigned* nbytes, hipStream_t stream) {
  return zt_png_encode_u8_mode(src, H, W, 1, ws, ws_bytes, out, out_bytes, nbytes, stream);
}

extern "C" int zt_png_code_lengths(const unsigned* hist257, unsigned char* len257, hipStream_t stream) {
  ZT_REQUIRE(hist257 && len257);
  hipLaunchKernelGGL(png_code_lengths_kernel, dim3(1), dim3(PNG_T), 0, stream, hist257, len257);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}
