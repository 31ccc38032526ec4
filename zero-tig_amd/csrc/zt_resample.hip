// Float resize of a decoded frame (train.py / predict.py --y4m_size): one pass of Pillow's ImagingResample for mode F
// (src/libImaging/Resample.c, ImagingResampleHorizontal_32bpc / Vertical_32bpc) over planar fp32 [C][H][W]:
//   ss = 0.0; for t < count: ss = ss + (double)src[first + t] * coef[o][t]; dst = (float)ss
// The multiply and the add are separate double operations in tap order (-ffp-contract=off, no fma), so the result is the one
// Pillow's C loop gives; the double coefficients and the bounds come from the host (zero-tig_amd/ingest.py:pil_bicubic_tables_f64).
// Unlike the 8-bit resampler of zt_ingest.hip nothing is rounded to a byte between the passes, so it works at every bit depth.
// Bandwidth-bound: one thread per output element, consecutive threads on consecutive x in both passes.  The vertical pass is fully
// coalesced and its tap loop is wave-uniform (one output row per block row); in the horizontal pass neighbouring threads read
// overlapping windows of one source row, which the L1 / L2 serve.  The tables (9 taps x 1920 x 8 B = 138 KB at 3840 -> 1920) stay in
// L2.  No LDS, no atomics, 64-bit element offsets.
#include "zt_common.h"

namespace {

__device__ __forceinline__ float resample_store(double ss, int clamp01) {
  const float v = (float)ss;
  return clamp01 ? fminf(fmaxf(v, 0.f), 1.f) : v;
}

// rows: src [C][H][Wi] -> dst [C][H][Wo]; grid (ceil(Wo / 256), H, C)
__global__ void __launch_bounds__(256) resample_rows_kernel(const float* __restrict__ src, float* __restrict__ dst, int H, int Wi, int Wo,
                                                            const double* __restrict__ coef, const int* __restrict__ bounds, int ksize,
                                                            int clamp01) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= Wo) return;
  const long long row = (long long)blockIdx.z * H + blockIdx.y;
  const int first = max(bounds[2 * x], 0), n = min(min(bounds[2 * x + 1], ksize), Wi - first);   // a bad table never reads outside
  const double* k = coef + (long long)x * ksize;
  const float* s = src + row * Wi + first;
  double ss = 0.0;
  for (int t = 0; t < n; ++t) ss = ss + (double)s[t] * k[t];
  dst[row * Wo + x] = resample_store(ss, clamp01);
}

// columns: src [C][Hi][W] -> dst [C][Ho][W]; grid (ceil(W / 256), Ho, C)
__global__ void __launch_bounds__(256) resample_cols_kernel(const float* __restrict__ src, float* __restrict__ dst, int Hi, int Ho, int W,
                                                            const double* __restrict__ coef, const int* __restrict__ bounds, int ksize,
                                                            int clamp01) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= W) return;
  const int y = blockIdx.y;
  const int first = max(bounds[2 * y], 0), n = min(min(bounds[2 * y + 1], ksize), Hi - first);
  const double* k = coef + (long long)y * ksize;
  const float* s = src + ((long long)blockIdx.z * Hi + first) * W + x;
  double ss = 0.0;
  for (int t = 0; t < n; ++t) ss = ss + (double)s[(long long)t * W] * k[t];
  dst[((long long)blockIdx.z * Ho + y) * W + x] = resample_store(ss, clamp01);
}

}  // namespace

extern "C" int zt_resample_planar_f32(const float* src, float* dst, int C, int Hi, int Wi, int No, int axis, const double* coef,
                                      const int* bounds, int ksize, int clamp01, hipStream_t stream) {
  ZT_REQUIRE(src && dst && coef && bounds && src != dst && C > 0 && Hi > 0 && Wi > 0 && No > 0 && (axis == 0 || axis == 1) && ksize >= 1);
  ZT_REQUIRE(C <= 65535 && Hi <= 65535 && No <= 65535);          // grid.y / grid.z
  if (axis == 1) {
    hipLaunchKernelGGL(resample_rows_kernel, dim3(zt_cdiv(No, 256), Hi, C), dim3(256), 0, stream, src, dst, Hi, Wi, No, coef, bounds,
                       ksize, clamp01 ? 1 : 0);
  } else {
    hipLaunchKernelGGL(resample_cols_kernel, dim3(zt_cdiv(Wi, 256), No, C), dim3(256), 0, stream, src, dst, Hi, No, Wi, coef, bounds,
                       ksize, clamp01 ? 1 : 0);
  }
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}
