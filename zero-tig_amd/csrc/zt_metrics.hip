// Evaluation metrics of evals.py on the device: SSIM (evals.py:87, skimage structural_similarity on the two uint8 frames) and
// histogram matching of the output to the ground truth (evals.py:100-103, skimage exposure.match_histograms with its default
// channel_axis=None: ALL three channels pooled into one distribution).
//   SSIM: 7x7 uniform window, sample covariance (49/48), data_range 255, 3-pixel border cropped before the mean, so only windows
//         that lie wholly inside the image count.  Window sums are exact integers; S and its reduction are fp64 in a fixed order.
//   match_histograms: out = interp(rank(src) / N, template CDF, template levels).  rank = number of source values <= v, found
//         by an LSD radix sort of the order-preserving 32-bit keys (8-bit digits, 4 passes, keys only) and an upper-bound search.
#include "zt_common.h"

namespace {

// ================================================================ SSIM ====================================================
constexpr int SS_TH = 32;                 // output rows per workgroup
constexpr int SS_TW = 64;                 // output columns per workgroup
constexpr int SS_IH = SS_TH + 6;          // staged input rows
constexpr int SS_RD = 18;                 // staged dwords per input row (72 bytes >= 64 + 6)

// quantised bytes of 4 consecutive pixels of row gy starting at column gx (zeros outside the image: such pixels only reach
// outputs that are masked)
__device__ __forceinline__ unsigned ssim_stage4(const float* __restrict__ p, int gy, int gx, int H, int W, bool vec) {
  if (gy >= H || gx >= W) return 0u;
  const float* r = p + (size_t)gy * W + gx;
  if (vec && gx + 3 < W) {
    const float4 v = *reinterpret_cast<const float4*>(r);
    return (unsigned)zt_quant_u8(v.x, 1) | ((unsigned)zt_quant_u8(v.y, 1) << 8) | ((unsigned)zt_quant_u8(v.z, 1) << 16) |
           ((unsigned)zt_quant_u8(v.w, 1) << 24);
  }
  unsigned o = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (gx + k < W) o |= (unsigned)zt_quant_u8(r[k], 1) << (8 * k);
  return o;
}

// grid (tiles x, tiles y, 3 channels); workgroup = 32 x 64 outputs.  Phase 1 stages the quantised bytes of both frames
// (38 x 70 window of inputs), phase 2 forms the horizontal 7-tap sums of x, y, xx, yy, xy with a running sum over 8 outputs per
// thread, phase 3 the vertical 7-tap sums over 8 outputs per thread, S in fp64 and the block's partial sum.
__global__ void __launch_bounds__(256) ssim_tile_kernel(const float* __restrict__ a, const float* __restrict__ b, int H, int W, int vec,
                                                        double* __restrict__ partial) {
  __shared__ unsigned xa[SS_IH * SS_RD], ya[SS_IH * SS_RD];
  __shared__ uint4 hs[SS_IH * SS_TW];                  // {sx | sy << 16, sxx, syy, sxy}: 7 * 255 < 2^16, 7 * 255^2 < 2^19
  __shared__ double red[256];
  const int t = threadIdx.x;
  const int tx0 = blockIdx.x * SS_TW, ty0 = blockIdx.y * SS_TH;
  const size_t plane = (size_t)blockIdx.z * H * W;

  for (int it = t; it < SS_IH * SS_RD; it += 256) {
    const int r = it / SS_RD, g = it - r * SS_RD;
    xa[it] = ssim_stage4(a + plane, ty0 + r, tx0 + 4 * g, H, W, vec != 0);
    ya[it] = ssim_stage4(b + plane, ty0 + r, tx0 + 4 * g, H, W, vec != 0);
  }
  __syncthreads();

  for (int it = t; it < SS_IH * (SS_TW / 8); it += 256) {
    const int r = it >> 3, c0 = (it & 7) * 8;
    unsigned wx[4], wy[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      wx[k] = xa[r * SS_RD + (c0 >> 2) + k];
      wy[k] = ya[r * SS_RD + (c0 >> 2) + k];
    }
    int px[14], py[14];
#pragma unroll
    for (int k = 0; k < 14; ++k) {
      px[k] = (int)((wx[k >> 2] >> (8 * (k & 3))) & 255u);
      py[k] = (int)((wy[k >> 2] >> (8 * (k & 3))) & 255u);
    }
    int sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      sx += px[k]; sy += py[k]; sxx += px[k] * px[k]; syy += py[k] * py[k]; sxy += px[k] * py[k];
    }
#pragma unroll
    for (int o = 0; o < 8; ++o) {
      hs[r * SS_TW + c0 + o] = make_uint4((unsigned)sx | ((unsigned)sy << 16), (unsigned)sxx, (unsigned)syy, (unsigned)sxy);
      if (o < 7) {
        sx += px[o + 7] - px[o]; sy += py[o + 7] - py[o];
        sxx += px[o + 7] * px[o + 7] - px[o] * px[o];
        syy += py[o + 7] * py[o + 7] - py[o] * py[o];
        sxy += px[o + 7] * py[o + 7] - px[o] * py[o];
      }
    }
  }
  __syncthreads();

  const int col = t & 63, r0 = (t >> 6) * 8;
  const int gx = tx0 + col;
  int sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    const uint4 v = hs[(r0 + k) * SS_TW + col];
    sx += (int)(v.x & 0xFFFFu); sy += (int)(v.x >> 16); sxx += (int)v.y; syy += (int)v.z; sxy += (int)v.w;
  }
  const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0), cov_norm = 49.0 / 48.0;
  double acc = 0.0;
#pragma unroll
  for (int o = 0; o < 8; ++o) {
    if (gx < W - 6 && ty0 + r0 + o < H - 6) {
      const double ux = (double)sx / 49.0, uy = (double)sy / 49.0;
      const double vx = cov_norm * ((double)sxx / 49.0 - ux * ux);
      const double vy = cov_norm * ((double)syy / 49.0 - uy * uy);
      const double vxy = cov_norm * ((double)sxy / 49.0 - ux * uy);
      acc += ((2.0 * ux * uy + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2));
    }
    if (o < 7) {
      const uint4 p = hs[(r0 + o + 7) * SS_TW + col], m = hs[(r0 + o) * SS_TW + col];
      sx += (int)(p.x & 0xFFFFu) - (int)(m.x & 0xFFFFu);
      sy += (int)(p.x >> 16) - (int)(m.x >> 16);
      sxx += (int)p.y - (int)m.y; syy += (int)p.z - (int)m.z; sxy += (int)p.w - (int)m.w;
    }
  }
  red[t] = acc;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (t < k) red[t] += red[t + k];
    __syncthreads();
  }
  if (t == 0) partial[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = red[0];
}

// one workgroup: per channel, thread t adds partials t, t + 256, ... in index order, then the same tree as above
__global__ void __launch_bounds__(256) ssim_final_kernel(const double* __restrict__ partial, int per_channel, double npix,
                                                         double* __restrict__ out) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  double mean3 = 0.0;
  for (int c = 0; c < 3; ++c) {
    double s = 0.0;
    for (int i = t; i < per_channel; i += 256) s += partial[(size_t)c * per_channel + i];
    red[t] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
      if (t < k) red[t] += red[t + k];
      __syncthreads();
    }
    if (t == 0) mean3 += red[0] / npix;
    __syncthreads();
  }
  if (t == 0) out[0] = mean3 / 3.0;
}

// ======================================================= histogram matching ================================================
constexpr int HM_TILE = 4096;             // keys per workgroup and pass (256 threads x 16)

// order-preserving key of a finite float; -0.0 ranks equal to +0.0
__device__ __forceinline__ unsigned hm_key(unsigned u) {
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// exclusive prefix of v over the 256 threads of the workgroup (and the total).  wsum: 4 LDS words; the caller puts a
// __syncthreads() between two uses of the same wsum.
__device__ __forceinline__ unsigned hm_block_scan(unsigned v, unsigned* wsum, unsigned& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned up = __shfl(inc, (lane - d) & 63);
    if (lane >= d) inc += up;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  unsigned off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const unsigned s = wsum[w];
    if (w < wave) off += s;
    tot += s;
  }
  total = tot;
  return off + inc - v;
}

// four consecutive elements i..i+3 of the pass input as keys (0xFFFFFFFF past the end).  F32: the input is the fp32 source.
template <bool F32>
__device__ __forceinline__ void hm_load4(const unsigned* __restrict__ in, unsigned i, unsigned n, unsigned (&k)[4]) {
  if (i + 3 < n) {
    const uint4 v = *reinterpret_cast<const uint4*>(in + i);
    k[0] = v.x; k[1] = v.y; k[2] = v.z; k[3] = v.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) k[j] = i + j < n ? in[i + j] : (F32 ? 0x7FFFFFFFu : 0xFFFFFFFFu);
  }
  if (F32) {
#pragma unroll
    for (int j = 0; j < 4; ++j) k[j] = hm_key(k[j]);      // the padding 0x7FFFFFFF maps to 0xFFFFFFFF
  }
}

// hist[digit][tile] = number of keys of the tile whose digit (bits shift..shift+7) has that value
template <bool F32>
__global__ void __launch_bounds__(256) hm_digit_hist_kernel(const unsigned* __restrict__ in, unsigned n, int shift, unsigned ntiles,
                                                            unsigned* __restrict__ hist) {
  __shared__ unsigned h[256];
  const unsigned t = threadIdx.x, base = blockIdx.x * (unsigned)HM_TILE;
  h[t] = 0u;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned i = base + (unsigned)j * 1024u + t * 4u;
    unsigned k[4];
    hm_load4<F32>(in, i, n, k);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (i + e < n) atomicAdd(&h[(k[e] >> shift) & 255u], 1u);
  }
  __syncthreads();
  hist[(size_t)t * ntiles + blockIdx.x] = h[t];
}

// one workgroup per digit: hist[digit][*] -> its exclusive prefix over the tiles, tot[digit] = the row's sum
__global__ void __launch_bounds__(256) hm_row_scan_kernel(unsigned* __restrict__ hist, unsigned ntiles, unsigned* __restrict__ tot) {
  __shared__ unsigned wsum[4];
  unsigned* row = hist + (size_t)blockIdx.x * ntiles;
  unsigned carry = 0;
  for (unsigned c0 = 0; c0 < ntiles; c0 += 256u) {
    const unsigned i = c0 + threadIdx.x;
    const unsigned v = i < ntiles ? row[i] : 0u;
    unsigned total;
    const unsigned ex = hm_block_scan(v, wsum, total);
    if (i < ntiles) row[i] = carry + ex;
    carry += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) tot[blockIdx.x] = carry;
}

// padded LDS index of tile slot i: a thread's 16 consecutive slots start 17 words apart
__device__ __forceinline__ unsigned hm_pad(unsigned i) { return i + (i >> 4); }

// stable scatter of one tile by the digit at `shift`: the tile is sorted by that digit in LDS (eight stable one-bit splits, each
// a workgroup prefix sum), then every key goes to (digits below it, all tiles) + (its digit, earlier tiles) + (its place among
// the tile's keys of that digit)
template <bool F32>
__global__ void __launch_bounds__(256) hm_scatter_kernel(const unsigned* __restrict__ in, unsigned* __restrict__ outk, unsigned n, int shift,
                                                         unsigned ntiles, const unsigned* __restrict__ hist,
                                                         const unsigned* __restrict__ tot) {
  __shared__ unsigned keys[HM_TILE + HM_TILE / 16];
  __shared__ unsigned dbase[256], dstart[256];
  __shared__ unsigned wsum[4];
  const unsigned t = threadIdx.x, base = blockIdx.x * (unsigned)HM_TILE;
  const unsigned nvalid = n - base < (unsigned)HM_TILE ? n - base : (unsigned)HM_TILE;
  unsigned total;
  const unsigned below = hm_block_scan(tot[t], wsum, total);
  dbase[t] = below + hist[(size_t)t * ntiles + blockIdx.x];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned li = (unsigned)j * 1024u + t * 4u;
    unsigned k[4];
    hm_load4<F32>(in, base + li, n, k);
#pragma unroll
    for (int e = 0; e < 4; ++e) keys[hm_pad(li + e)] = k[e];
  }
  __syncthreads();
  for (int bit = shift; bit < shift + 8; ++bit) {
    unsigned k[16];
    unsigned zeros = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      k[j] = keys[t * 17u + j];
      zeros += 1u - ((k[j] >> bit) & 1u);
    }
    unsigned Z;
    unsigned zpos = hm_block_scan(zeros, wsum, Z);       // its barrier also ends the reads above
    unsigned opos = Z + t * 16u - zpos;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const unsigned one = (k[j] >> bit) & 1u;
      const unsigned pos = one ? opos : zpos;
      keys[hm_pad(pos)] = k[j];
      opos += one;
      zpos += 1u - one;
    }
    __syncthreads();
  }
  // the padding keys (all ones, last in the tile before the sort) stay behind every real key: slots [0, nvalid) are the real ones
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const unsigned i = (unsigned)j * 256u + t;
    const unsigned d = (keys[hm_pad(i)] >> shift) & 255u;
    if (i == 0u || ((keys[hm_pad(i - 1u)] >> shift) & 255u) != d) dstart[d] = i;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const unsigned i = (unsigned)j * 256u + t;
    if (i < nvalid) {
      const unsigned k = keys[hm_pad(i)];
      const unsigned d = (k >> shift) & 255u;
      outk[dbase[d] + (i - dstart[d])] = k;
    }
  }
}

// 256-bin histogram of the quantised template (np.round(x * 255)); thist is zeroed by the launcher; integer atomics only
__global__ void __launch_bounds__(256) hm_tmpl_hist_kernel(const float* __restrict__ tmpl, long long m, unsigned* __restrict__ thist) {
  __shared__ unsigned h[256];
  h[threadIdx.x] = 0u;
  __syncthreads();
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < m; i += (long long)gridDim.x * 256)
    atomicAdd(&h[zt_quant_u8(tmpl[i], 1)], 1u);
  __syncthreads();
  if (h[threadIdx.x] != 0u) atomicAdd(&thist[threadIdx.x], h[threadIdx.x]);
}

// occupied levels of the template: tq[j] = cumulative count / M, tv[j] = level / 255 as ToTensor forms it; nlev[0] = L
__global__ void __launch_bounds__(256) hm_tmpl_table_kernel(const unsigned* __restrict__ thist, long long m, unsigned* __restrict__ nlev,
                                                            double* __restrict__ tq, double* __restrict__ tv) {
  __shared__ unsigned wsum[4];
  const unsigned t = threadIdx.x;
  const unsigned c = thist[t];
  unsigned total, L;
  const unsigned cum = hm_block_scan(c, wsum, total) + c;
  __syncthreads();
  const unsigned j = hm_block_scan(c != 0u ? 1u : 0u, wsum, L);
  if (c != 0u) {
    tq[j] = (double)cum / (double)m;
    tv[j] = (double)__fdiv_rn((float)t, 255.0f);
  }
  if (t == 0) nlev[0] = L;
}

// out = interp(cnt / N, tq, tv) with cnt = number of sorted keys <= the element's key (fixed-length binary descents)
__device__ __forceinline__ float hm_apply_one(unsigned ubits, const unsigned* __restrict__ sorted, unsigned n, int steps, unsigned L,
                                              const double* stq, const double* stv) {
  const unsigned key = hm_key(ubits);
  unsigned cnt = 0;
  for (int s = steps - 1; s >= 0; --s) {
    const unsigned np = cnt + (1u << s);
    if (np <= n && sorted[np - 1u] <= key) cnt = np;
  }
  const double q = (double)cnt / (double)n;
  unsigned jc = 0;                                       // number of table entries with tq <= q
#pragma unroll
  for (int s = 8; s >= 0; --s) {
    const unsigned np = jc + (1u << s);
    if (np <= L && stq[np - 1u] <= q) jc = np;
  }
  double r;
  if (jc == 0u) r = stv[0];
  else if (jc == L) r = stv[L - 1u];
  else {
    const unsigned j = jc - 1u;
    r = ((stv[j + 1u] - stv[j]) / (stq[j + 1u] - stq[j])) * (q - stq[j]) + stv[j];
  }
  return (float)r;
}

__global__ void __launch_bounds__(256) hm_apply_kernel(const unsigned* __restrict__ src, const unsigned* __restrict__ sorted, unsigned n,
                                                       int steps, const unsigned* __restrict__ nlev, const double* __restrict__ tq,
                                                       const double* __restrict__ tv, float* __restrict__ out) {
  __shared__ double stq[256], stv[256];
  const unsigned L = nlev[0];
  stq[threadIdx.x] = threadIdx.x < L ? tq[threadIdx.x] : 0.0;
  stv[threadIdx.x] = threadIdx.x < L ? tv[threadIdx.x] : 0.0;
  __syncthreads();
  const unsigned i = (blockIdx.x * 256u + threadIdx.x) * 4u;
  if (i >= n) return;
  if (i + 3u < n) {
    const uint4 v = *reinterpret_cast<const uint4*>(src + i);
    float4 o;
    o.x = hm_apply_one(v.x, sorted, n, steps, L, stq, stv);
    o.y = hm_apply_one(v.y, sorted, n, steps, L, stq, stv);
    o.z = hm_apply_one(v.z, sorted, n, steps, L, stq, stv);
    o.w = hm_apply_one(v.w, sorted, n, steps, L, stq, stv);
    *reinterpret_cast<float4*>(out + i) = o;
  } else {
    for (unsigned e = i; e < n; ++e) out[e] = hm_apply_one(src[e], sorted, n, steps, L, stq, stv);
  }
}

template <bool F32>
int hm_sort_pass(const unsigned* in, unsigned* outk, unsigned n, int shift, unsigned ntiles, unsigned* hist, unsigned* tot,
                 hipStream_t stream) {
  hipLaunchKernelGGL(hm_digit_hist_kernel<F32>, dim3(ntiles), dim3(256), 0, stream, in, n, shift, ntiles, hist);
  ZT_LAUNCH_CHECK();
  hipLaunchKernelGGL(hm_row_scan_kernel, dim3(256), dim3(256), 0, stream, hist, ntiles, tot);
  ZT_LAUNCH_CHECK();
  hipLaunchKernelGGL(hm_scatter_kernel<F32>, dim3(ntiles), dim3(256), 0, stream, in, outk, n, shift, ntiles, (const unsigned*)hist,
                     (const unsigned*)tot);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}

}  // namespace

extern "C" int zt_ssim_u8_f32(const float* a, const float* b, int H, int W, double* partial, int npartial, double* out,
                              hipStream_t stream) {
  ZT_REQUIRE(a && b && partial && out && H >= 7 && W >= 7 && H <= (1 << 20) && W <= (1 << 20));
  const int ntx = zt_cdiv(W - 6, SS_TW), nty = zt_cdiv(H - 6, SS_TH);
  ZT_REQUIRE((long long)ntx * nty * 3 <= (long long)npartial);
  const int vec = (W % 4 == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0) ? 1 : 0;
  hipLaunchKernelGGL(ssim_tile_kernel, dim3(ntx, nty, 3), dim3(256), 0, stream, a, b, H, W, vec, partial);
  ZT_LAUNCH_CHECK();
  hipLaunchKernelGGL(ssim_final_kernel, dim3(1), dim3(256), 0, stream, (const double*)partial, ntx * nty,
                     (double)(H - 6) * (double)(W - 6), out);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}

extern "C" int zt_match_histograms_f32(const float* src, long long n, const float* tmpl, long long m, float* out, void* scratch,
                                       size_t scratch_bytes, hipStream_t stream) {
  ZT_REQUIRE(src && tmpl && out && scratch && n > 0 && m > 0 && n <= 0x7FFF0000LL && m <= 0x7FFF0000LL);
  ZT_REQUIRE((((uintptr_t)src | (uintptr_t)out | (uintptr_t)scratch) & 15) == 0);
  const unsigned N = (unsigned)n, ntiles = (unsigned)zt_cdivl(n, HM_TILE);
  const size_t nr = ((size_t)n + 3) & ~(size_t)3;
  ZT_REQUIRE(scratch_bytes >= 8 * nr + 1024 * (size_t)ntiles + 8192);
  unsigned* keysA = (unsigned*)scratch;
  unsigned* keysB = keysA + nr;
  unsigned* hist = keysB + nr;
  unsigned* tot = hist + 256 * (size_t)ntiles;
  unsigned* thist = tot + 256;
  unsigned* nlev = thist + 256;
  double* tq = (double*)(nlev + 4);
  double* tv = tq + 256;

  hipError_t e = hipMemsetAsync(thist, 0, 256 * sizeof(unsigned), stream);
  if (e != hipSuccess) return (int)e;
  const unsigned tblk = (unsigned)(zt_cdivl(m, 4096) < 1024 ? zt_cdivl(m, 4096) : 1024);
  hipLaunchKernelGGL(hm_tmpl_hist_kernel, dim3(tblk), dim3(256), 0, stream, tmpl, m, thist);
  ZT_LAUNCH_CHECK();
  hipLaunchKernelGGL(hm_tmpl_table_kernel, dim3(1), dim3(256), 0, stream, (const unsigned*)thist, m, nlev, tq, tv);
  ZT_LAUNCH_CHECK();

  int rc;
  if ((rc = hm_sort_pass<true>((const unsigned*)src, keysA, N, 0, ntiles, hist, tot, stream)) != ZT_OK) return rc;
  if ((rc = hm_sort_pass<false>(keysA, keysB, N, 8, ntiles, hist, tot, stream)) != ZT_OK) return rc;
  if ((rc = hm_sort_pass<false>(keysB, keysA, N, 16, ntiles, hist, tot, stream)) != ZT_OK) return rc;
  if ((rc = hm_sort_pass<false>(keysA, keysB, N, 24, ntiles, hist, tot, stream)) != ZT_OK) return rc;

  int steps = 0;
  while ((1ull << steps) <= (unsigned long long)N) ++steps;          // ceil(log2(N + 1))
  hipLaunchKernelGGL(hm_apply_kernel, dim3((unsigned)zt_cdivl(zt_cdivl(n, 4), 256)), dim3(256), 0, stream, (const unsigned*)src,
                     (const unsigned*)keysB, N, steps, (const unsigned*)nlev, (const double*)tq, (const double*)tv, out);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}
