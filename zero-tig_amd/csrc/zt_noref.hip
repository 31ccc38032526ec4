// No-reference grading of evals.py --noref 1: everything is read off ONE object, the 256 x 256 joint histogram of the
// 8-bit lightness L = max(R, G, B) of the input frame (rows, La) and of the enhanced frame (columns, Lb) on a sample grid.
//   zt_lightness_joint_hist_f32: the histogram.  Every workgroup counts its share of the samples in a private table in LDS (65536
//         counters of 16 bits, two to a dword, 128 KB) and then adds its non-zero counters to the table in memory.
//   zt_noref_from_hist: the 2-D cumulative sum of the table and from it the lightness order error, the marginals' first moments,
//         the clipped counts and the two entropies, in one workgroup.
// Integer sums throughout (the entropies: fp64 in level order), so the same frames give the same bits.
#include "zt_common.h"

namespace {

constexpr int NR_THREADS = 1024;
constexpr int NR_BINS = 65536;
constexpr unsigned NR_CAP = 65532;        // samples per workgroup: a multiple of 4 (16-byte loads) and at most 65535, so that a
                                          // 16-bit counter can neither wrap nor carry into the other half of its dword

__device__ __forceinline__ unsigned nr_light(float r, float g, float b) {
  return (unsigned)max(max(zt_quant_u8(r, 1), zt_quant_u8(g, 1)), zt_quant_u8(b, 1));
}

__device__ __forceinline__ void nr_count(unsigned* lh, unsigned la, unsigned lb) {
  const unsigned bin = la * 256u + lb;
  atomicAdd(&lh[bin >> 1], 1u << (16u * (bin & 1u)));
}

// grid: ceil(ns / NR_CAP) workgroups, workgroup g takes samples [g * NR_CAP, (g + 1) * NR_CAP).  VEC: the full grid (sample s is
// pixel s) with W % 4 == 0 and 16-byte aligned frames.  Otherwise sample (i, j) of the Hs x Ws grid is the pixel
// at row ((2i + 1) H) / (2 Hs), column ((2j + 1) W) / (2 Ws); `full` (Hs == H and Ws == W) skips the two divisions.
template <bool VEC>
__global__ void __launch_bounds__(NR_THREADS) nr_hist_kernel(const float* __restrict__ a, const float* __restrict__ b, int H, int W,
                                                             int Hs, int Ws, int full, unsigned long long ns, unsigned* __restrict__ hist) {
  __shared__ uint4 lh4[NR_BINS / 8];
  unsigned* lh = reinterpret_cast<unsigned*>(lh4);
  const unsigned t = threadIdx.x;
  for (unsigned d = t; d < NR_BINS / 8; d += NR_THREADS) lh4[d] = make_uint4(0u, 0u, 0u, 0u);
  __syncthreads();

  const unsigned long long s0 = (unsigned long long)blockIdx.x * NR_CAP;
  const unsigned long long s1 = s0 + NR_CAP < ns ? s0 + NR_CAP : ns;
  const size_t plane = (size_t)H * W;
  if (VEC) {
    for (unsigned long long s = s0 + 4ull * t; s < s1; s += 4ull * NR_THREADS) {
      const float4 ar = *reinterpret_cast<const float4*>(a + s), ag = *reinterpret_cast<const float4*>(a + plane + s),
                   ab = *reinterpret_cast<const float4*>(a + 2 * plane + s);
      const float4 br = *reinterpret_cast<const float4*>(b + s), bg = *reinterpret_cast<const float4*>(b + plane + s),
                   bb = *reinterpret_cast<const float4*>(b + 2 * plane + s);
      nr_count(lh, nr_light(ar.x, ag.x, ab.x), nr_light(br.x, bg.x, bb.x));
      nr_count(lh, nr_light(ar.y, ag.y, ab.y), nr_light(br.y, bg.y, bb.y));
      nr_count(lh, nr_light(ar.z, ag.z, ab.z), nr_light(br.z, bg.z, bb.z));
      nr_count(lh, nr_light(ar.w, ag.w, ab.w), nr_light(br.w, bg.w, bb.w));
    }
  } else {
    for (unsigned long long s = s0 + t; s < s1; s += NR_THREADS) {
      size_t p = (size_t)s;
      if (!full) {
        const unsigned long long i = s / (unsigned)Ws, j = s - i * (unsigned)Ws;
        const unsigned long long row = ((2 * i + 1) * (unsigned)H) / (2ull * (unsigned)Hs);
        const unsigned long long col = ((2 * j + 1) * (unsigned)W) / (2ull * (unsigned)Ws);
        p = (size_t)(row * (unsigned)W + col);
      }
      nr_count(lh, nr_light(a[p], a[plane + p], a[2 * plane + p]), nr_light(b[p], b[plane + p], b[2 * plane + p]));
    }
  }
  __syncthreads();

  for (unsigned d = t; d < NR_BINS / 8; d += NR_THREADS) {
    const uint4 v = lh4[d];
    if ((v.x | v.y | v.z | v.w) == 0u) continue;
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (w[k] & 0xFFFFu) atomicAdd(&hist[8 * d + 2 * k], w[k] & 0xFFFFu);
      if (w[k] >> 16) atomicAdd(&hist[8 * d + 2 * k + 1], w[k] >> 16);
    }
  }
}

__device__ __forceinline__ uint4 nr_add4(uint4 a, uint4 b) { return make_uint4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// One workgroup of 16 waves.  Wave w owns rows 16w .. 16w + 15 of the table, lane l columns 4l .. 4l + 3.  The column sums of the
// bands above give the wave its starting column totals; per row it adds the row to them and takes their inclusive scan over the
// 256 columns (4 in the lane, 64 lanes by shuffles): that is row x of C, the 2-D cumulative sum.  C[x][255] = R[x] and C[255][y]
// = K[y], so the marginals need no pass of their own.  S_loe = sum Hist (R + K - 2 C) = sum_x ha R + sum_y hb K - 2 sum Hist C.
__global__ void __launch_bounds__(NR_THREADS) nr_reduce_kernel(const unsigned* __restrict__ hist, long long* __restrict__ out_i,
                                                               double* __restrict__ out_f) {
  __shared__ uint4 band[16][64];
  __shared__ unsigned rc[256], kc[256];
  __shared__ unsigned long long acc[4];           // sum Hist C, sum ha R + hb K, S_a, S_b
  __shared__ double term[2][256];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const uint4* h4 = reinterpret_cast<const uint4*>(hist);
  if (t < 4) acc[t] = 0ull;

  uint4 cc = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
  for (int k = 0; k < 16; ++k) cc = nr_add4(cc, h4[(wave * 16 + k) * 64 + lane]);
  band[wave][lane] = cc;
  __syncthreads();
  cc = make_uint4(0u, 0u, 0u, 0u);
  for (int w = 0; w < wave; ++w) cc = nr_add4(cc, band[w][lane]);

  unsigned long long hc = 0ull;
#pragma unroll 2
  for (int k = 0; k < 16; ++k) {
    const uint4 row = h4[(wave * 16 + k) * 64 + lane];   // a second read (L2) instead of 64 registers held across the barrier
    cc = nr_add4(cc, row);
    const unsigned p0 = cc.x, p1 = p0 + cc.y, p2 = p1 + cc.z, p3 = p2 + cc.w;
    unsigned inc = p3;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned up = __shfl(inc, (lane - d) & 63);
      if (lane >= d) inc += up;
    }
    const unsigned base = inc - p3;
    hc += (unsigned long long)row.x * (base + p0) + (unsigned long long)row.y * (base + p1) +
          (unsigned long long)row.z * (base + p2) + (unsigned long long)row.w * (base + p3);
    if (lane == 63) rc[wave * 16 + k] = inc;
    if (wave == 15 && k == 15) {
      kc[4 * lane] = base + p0;
      kc[4 * lane + 1] = base + p1;
      kc[4 * lane + 2] = base + p2;
      kc[4 * lane + 3] = base + p3;
    }
  }
  if (hc) atomicAdd(&acc[0], hc);
  __syncthreads();

  if (t < 256) {
    const unsigned ha = rc[t] - (t ? rc[t - 1] : 0u), hb = kc[t] - (t ? kc[t - 1] : 0u);
    const double ns = (double)rc[255];
    atomicAdd(&acc[1], (unsigned long long)ha * rc[t] + (unsigned long long)hb * kc[t]);
    atomicAdd(&acc[2], (unsigned long long)ha * (unsigned)t);
    atomicAdd(&acc[3], (unsigned long long)hb * (unsigned)t);
    const double pa = (double)ha / ns, pb = (double)hb / ns;
    term[0][t] = ha ? pa * log2(pa) : 0.0;
    term[1][t] = hb ? pb * log2(pb) : 0.0;
  }
  __syncthreads();

  if (lane == 0 && wave < 2) {                    // the entropies: 256 terms in level order, one lane each
    double e = 0.0;
    for (int l = 0; l < 256; ++l) e -= term[wave][l];
    out_f[wave] = e;
  }
  if (t == 128) {
    out_i[0] = (long long)rc[255];
    out_i[1] = (long long)(acc[1] - 2ull * acc[0]);
    out_i[2] = (long long)acc[2];
    out_i[3] = (long long)acc[3];
    out_i[4] = (long long)(kc[255] - kc[254]);
    out_i[5] = (long long)kc[0];
  }
}

}  // namespace

extern "C" int zt_lightness_joint_hist_f32(const float* a, const float* b, int H, int W, int Hs, int Ws, unsigned* hist,
                                           hipStream_t stream) {
  ZT_REQUIRE(a && b && hist && H >= 1 && W >= 1 && Hs >= 1 && Ws >= 1 && H <= (1 << 20) && W <= (1 << 20));
  ZT_REQUIRE((unsigned long long)Hs * (unsigned long long)Ws < (1ull << 32));
  ZT_REQUIRE((((uintptr_t)a | (uintptr_t)b | (uintptr_t)hist) & 3) == 0);
  const unsigned long long ns = (unsigned long long)Hs * (unsigned long long)Ws;
  const int full = (Hs == H && Ws == W) ? 1 : 0;
  const bool vec = full && W % 4 == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0;
  hipError_t e = hipMemsetAsync(hist, 0, NR_BINS * sizeof(unsigned), stream);
  if (e != hipSuccess) return (int)e;
  // the grid follows from the cap, not from the CU count: the flush costs a workgroup one global atomic per bin it has filled, so
  // fewer, fuller workgroups win (32 at 1080p measured 3 x faster on dark frames than 512)
  const unsigned nwg = (unsigned)((ns + NR_CAP - 1) / NR_CAP);
  if (vec)
    hipLaunchKernelGGL(nr_hist_kernel<true>, dim3(nwg), dim3(NR_THREADS), 0, stream, a, b, H, W, Hs, Ws, full, ns, hist);
  else
    hipLaunchKernelGGL(nr_hist_kernel<false>, dim3(nwg), dim3(NR_THREADS), 0, stream, a, b, H, W, Hs, Ws, full, ns, hist);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}

extern "C" int zt_noref_from_hist(const unsigned* hist, long long* out_i, double* out_f, hipStream_t stream) {
  ZT_REQUIRE(hist && out_i && out_f);
  ZT_REQUIRE(((uintptr_t)hist & 15) == 0 && (((uintptr_t)out_i | (uintptr_t)out_f) & 7) == 0);
  hipLaunchKernelGGL(nr_reduce_kernel, dim3(1), dim3(NR_THREADS), 0, stream, hist, out_i, out_f);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}
