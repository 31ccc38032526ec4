// LPIPS (VGG16, lpips 0.1) of evals.py:73-80, 92-98 on the device.
//   zt_conv3x3_wide_bf16: the wide-channel 3x3 convolution of VGG's blocks 2-5 (Cin 64..512, Cout 128..512): an implicit GEMM
//       with M = pixels, N = Cout, K = 9 * Cin, built like a GEMM (128 x 128 tile, two barriers per K stage), see below.
//   zt_lpips_prep:     planar fp32 image in [0,1] -> nhwc (8-channel pitch) with the [-1,1] mapping and the scaling layer folded in
//   zt_maxpool2_nhwc:  2x2 / 2 max pool (floor), 16-byte accesses
//   zt_lpips_layer:    one tap's distance: unit-normalise both feature vectors of a pixel, weighted squared difference, mean
#include "zt_conv.h"

namespace {

// ======================================================= wide 3x3 convolution ==============================================
// Workgroup = 256 threads = 4 waves, output tile = (8 rows x 16 columns) pixels x 128 couts; waves 2 x 2, each 4 rows x 64 couts
// = acc[4 pixel rows][4 cout tiles] of 16x16 MFMA results.  K runs over 64-channel chunks; per chunk the 10 x 18 halo tile is
// staged ONCE and re-used by the nine taps; the weights of the chunk are staged one kernel row (3 taps x 128 couts x 64 channels
// = 48 KB) at a time, so a workgroup holds 72 KB of LDS and two of them share a CU: one computes while the other waits for its
// LDS-DMA at the barrier.  Both images are filled by 16-byte global_load_lds, lane-linear, with the XOR swizzle applied to the
// SOURCE address: a pixel / cout row is 128 bytes = 8 slots of 8 channels, logical slot s is stored at slot s ^ f(row), f chosen
// so that the 16 rows one ds_read_b128 phase touches fall into 16 different 16-byte bank groups.
// The MFMA's A operand is the WEIGHTS (rows = couts) and B the pixels: D then holds 4 consecutive couts of one pixel per lane.
// MFMA row r of cout tile q reads cout 32 (q >> 1) + 8 (r >> 2) + 4 (q & 1) + (r & 3), so the tiles q, q + 1 of a lane together are 8
// consecutive couts: one 16-byte bf16 store, no transposition through LDS.
constexpr int WC_TH = 8, WC_TW = 16;                    // output tile
constexpr int WC_IR = WC_TH + 2, WC_IC = WC_TW + 2;     // halo tile
constexpr int WC_KC = 64;                               // channels per chunk
constexpr int WC_NC = 128;                              // couts per workgroup
constexpr int WC_XSLOTS = 6 * 256;                      // 16-byte slots of the halo image (10 * 18 * 8 = 1440 used)
constexpr int WC_WSLOTS = 3 * WC_NC * 8;                // one kernel row of weights
constexpr int WC_NXI = WC_XSLOTS / 256, WC_NWI = WC_WSLOTS / 256;

struct WideArgs {
  const zt_bf16* x;
  const zt_bf16* w;
  const float* bias;
  zt_bf16* y;
  int N, H, W, Cin, ldx, CoutP, ldk, ldy, tilesY, relu;
};

__device__ __forceinline__ int wc_fx(int p) { return (p >> 1) & 7; }                            // halo pixels: 16 consecutive rows per read
__device__ __forceinline__ int wc_fw(int co) { return (((co >> 3) & 3) << 1) | ((co >> 1) & 1); }  // couts 8a + 4h + b, a, b = 0..3

__global__ void __launch_bounds__(256, 2) conv3x3_wide_bf16_kernel(WideArgs a) {
  __shared__ __attribute__((aligned(16))) zt_bf16 smem[(WC_XSLOTS + WC_WSLOTS) * 8];
  zt_bf16* const xs = smem;
  zt_bf16* const ws = smem + WC_XSLOTS * 8;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 1, wc = wave & 1;
  const int l15 = lane & 15, l4 = lane >> 4;
  int ty = blockIdx.y, n = 0;
  if (a.N > 1) {
    n = ty / a.tilesY;
    ty -= n * a.tilesY;
  }
  const int oy0 = ty * WC_TH, ox0 = blockIdx.x * WC_TW, co0 = blockIdx.z * WC_NC;

  // staging geometry, chunk invariant.  Slot e = i * 256 + tid: row (pixel / cout) = e >> 3 = 32 i + (tid >> 3), physical slot
  // tid & 7; 32 i does not reach the bits f() looks at, so the logical slot is the same for every i.
  const int r0 = tid >> 3;
  const int sx = (tid & 7) ^ wc_fx(r0), sw = (tid & 7) ^ wc_fw(r0);
  int x_off[WC_NXI];
#pragma unroll
  for (int i = 0; i < WC_NXI; ++i) {
    const int p = 32 * i + r0;
    const int hy = p / WC_IC, hx = p - hy * WC_IC;
    const int gy = oy0 - 1 + hy, gx = ox0 - 1 + hx;
    const bool in = p < WC_IR * WC_IC && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
    x_off[i] = in ? ((n * a.H + gy) * a.W + gx) * a.ldx + 8 * sx : -1;
  }
  const int w_off = (co0 + r0) * a.ldk + 8 * sw;        // + (tap * CoutP + 32 (i & 3)) * ldk + c0
  const int w_tap = a.CoutP * a.ldk;

  zt_f32x4 acc[4][4];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[m][q] = (zt_f32x4){0.f, 0.f, 0.f, 0.f};

  // fragment addresses (elements): weights row of this lane per cout tile, halo pixel of this lane for output row m, tap (0, 0)
  int wrow[4], wsw[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int co = wc * 64 + (q >> 1) * 32 + 8 * (l15 >> 2) + 4 * (q & 1) + (l15 & 3);
    wrow[q] = co * WC_KC;
    wsw[q] = wc_fw(co);
  }
  const int p00 = (wr * 4) * WC_IC + l15;

  for (int c0 = 0; c0 < a.Cin; c0 += WC_KC) {
#pragma unroll 1
    for (int ky = 0; ky < 3; ++ky) {
      __syncthreads();                                  // every wave is done reading the images that are replaced now
      if (ky == 0) {
#pragma unroll
        for (int i = 0; i < WC_NXI; ++i) {
          const void* src = x_off[i] >= 0 ? (const void*)(a.x + (unsigned)(x_off[i] + c0)) : (const void*)&zt_zero_chunk;
          zt_glds16(src, xs + (i * 4 + wave) * 512);
        }
      }
      const zt_bf16* wsrc = a.w + (unsigned)(w_off + ky * 3 * w_tap + c0);
#pragma unroll
      for (int i = 0; i < WC_NWI; ++i)
        zt_glds16(wsrc + (unsigned)((i >> 2) * w_tap + (i & 3) * 32 * a.ldk), ws + (i * 4 + wave) * 512);
      __syncthreads();                                  // drains the LDS-DMA (vmcnt) of every wave
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          zt_s16x8 fw[4], fp[4];
#pragma unroll
          for (int q = 0; q < 4; ++q)
            fw[q] = *reinterpret_cast<const zt_s16x8*>(ws + kx * (WC_NC * WC_KC) + wrow[q] + (((kk * 4 + l4) ^ wsw[q]) << 3));
#pragma unroll
          for (int m = 0; m < 4; ++m) {
            const int p = p00 + (m + ky) * WC_IC + kx;
            fp[m] = *reinterpret_cast<const zt_s16x8*>(xs + p * WC_KC + (((kk * 4 + l4) ^ wc_fx(p)) << 3));
          }
#pragma unroll
          for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[m][q] = zt_mfma_bf16(fw[q], fp[m], acc[m][q]);
        }
      }
    }
  }

  // epilogue: lane = pixel column l15, couts co0 + 64 wc + 32 g + 8 l4 + [0, 8) for g = 0, 1
  const int ox = ox0 + l15;
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const int co = co0 + wc * 64 + g * 32 + 8 * l4;
    float b[8];
    if (a.bias) {
      const float4 b0 = *reinterpret_cast<const float4*>(a.bias + co), b1 = *reinterpret_cast<const float4*>(a.bias + co + 4);
      b[0] = b0.x; b[1] = b0.y; b[2] = b0.z; b[3] = b0.w; b[4] = b1.x; b[5] = b1.y; b[6] = b1.z; b[7] = b1.w;
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) b[k] = 0.f;
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int oy = oy0 + wr * 4 + m;
      float v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        v[k] = acc[m][2 * g + (k >> 2)][k & 3] + b[k];
        if (a.relu) v[k] = fmaxf(v[k], 0.f);
      }
      if (oy < a.H && ox < a.W) zt_st8(a.y + ((size_t)(n * a.H + oy) * a.W + ox) * a.ldy + co, v);
    }
  }
}

// ======================================================= prep / pool =======================================================
// x = (a - 0.5) * 2 (evals.py cvt_array2tensor), then lpips' ScalingLayer (x - shift) / scale; channels 3..7 zero
template <typename T>
__global__ void __launch_bounds__(256) lpips_prep_kernel(const float* __restrict__ src, T* __restrict__ dst, int HW) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= HW) return;
  const float shift[3] = {-.030f, -.088f, -.188f}, scale[3] = {.458f, .448f, .450f};
  float v[8];
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = __fdiv_rn(__fsub_rn(__fmul_rn(__fsub_rn(src[(size_t)c * HW + i], 0.5f), 2.f), shift[c]), scale[c]);
#pragma unroll
  for (int c = 3; c < 8; ++c) v[c] = 0.f;
  T* d = dst + (size_t)i * 8;
  if constexpr (sizeof(T) == 2) {
    zt_st8(d, v);
  } else {
    ZtIO<T>::st4(d, make_float4(v[0], v[1], v[2], v[3]));
    ZtIO<T>::st4(d + 4, make_float4(v[4], v[5], v[6], v[7]));
  }
}

// one thread per output pixel and group of 4 (fp32) / 8 (bf16) channels
template <typename T, int V>
__global__ void __launch_bounds__(256) maxpool2_kernel(const T* __restrict__ x, T* __restrict__ y, int ldx, int ldy, int H, int W,
                                                       int Ho, int Wo, int CG, long long total) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int cg = (int)(e % CG);
  const long long p = e / CG;
  const int ox = (int)(p % Wo);
  const long long t = p / Wo;
  const int oy = (int)(t % Ho), n = (int)(t / Ho);
  const T* s = x + (((size_t)n * H + 2 * oy) * W + 2 * ox) * ldx + cg * V;
  float m[V];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const T* q = s + ((size_t)(k >> 1) * W + (k & 1)) * ldx;
    float v[V];
    if constexpr (V == 8) {
      zt_ld8(q, v);
    } else {
      const float4 f = ZtIO<T>::ld4(q);
      v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
    }
#pragma unroll
    for (int j = 0; j < V; ++j) m[j] = k == 0 ? v[j] : fmaxf(m[j], v[j]);
  }
  T* d = y + (((size_t)n * Ho + oy) * Wo + ox) * ldy + cg * V;
  if constexpr (V == 8) zt_st8(d, m);
  else ZtIO<T>::st4(d, make_float4(m[0], m[1], m[2], m[3]));
}

// ======================================================= distance of one tap ===============================================
// G = C / 8 lanes share a pixel (8 channels of both maps per lane, in registers): the two squared norms are reduced over the
// group by shuffles, then every lane forms its 8 terms w_c (fa_c / (|fa| + 1e-10) - fb_c / (|fb| + 1e-10))^2 in fp32 and adds
// them to its own fp64 sum.  Workgroup: fixed tree over the 256 sums -> partial[block]; lpips_final_kernel adds the partials in
// index order.  No atomics: same input, same bits.
template <typename T>
__device__ __forceinline__ void lp_ld8(const T* p, float (&f)[8]) {
  if constexpr (sizeof(T) == 2) {
    zt_ld8(p, f);
  } else {
    const float4 u = ZtIO<T>::ld4(p), v = ZtIO<T>::ld4(p + 4);
    f[0] = u.x; f[1] = u.y; f[2] = u.z; f[3] = u.w; f[4] = v.x; f[5] = v.y; f[6] = v.z; f[7] = v.w;
  }
}

template <typename T>
__global__ void __launch_bounds__(256) lpips_layer_kernel(const T* __restrict__ fa, const T* __restrict__ fb, int lda, int ldb,
                                                          long long npix, int C, const float* __restrict__ w,
                                                          double* __restrict__ partial) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  const int G = C >> 3, ppb = 256 / G;                    // lanes per pixel (8..64), pixels per workgroup and round
  const int sub = t % G, pl = t / G;
  float wv[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) wv[k] = w[sub * 8 + k];
  double acc = 0.0;
  const long long rounds = (npix + (long long)ppb * gridDim.x - 1) / ((long long)ppb * gridDim.x);
  for (long long r = 0; r < rounds; ++r) {              // every lane runs every round: the shuffles need the whole wave
    const long long p = (r * gridDim.x + blockIdx.x) * ppb + pl;
    const bool ok = p < npix;
    float va[8], vb[8];
    if (ok) {
      lp_ld8(fa + (size_t)p * lda + sub * 8, va);
      lp_ld8(fb + (size_t)p * ldb + sub * 8, vb);
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) va[k] = vb[k] = 0.f;
    }
    float sa = 0.f, sb = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      sa = fmaf(va[k], va[k], sa);
      sb = fmaf(vb[k], vb[k], sb);
    }
    for (int d = G >> 1; d > 0; d >>= 1) {
      sa += __shfl_xor(sa, d);
      sb += __shfl_xor(sb, d);
    }
    const float na = sqrtf(sa) + 1e-10f, nb = sqrtf(sb) + 1e-10f;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float d = __fsub_rn(__fdiv_rn(va[k], na), __fdiv_rn(vb[k], nb));
      s = fmaf(wv[k] * d, d, s);
    }
    acc += (double)s;
  }
  red[t] = acc;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (t < k) red[t] += red[t + k];
    __syncthreads();
  }
  if (t == 0) partial[blockIdx.x] = red[0];
}

__global__ void __launch_bounds__(256) lpips_final_kernel(const double* __restrict__ partial, int n, double npix, double* __restrict__ out) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int i = t; i < n; i += 256) s += partial[i];
  red[t] = s;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (t < k) red[t] += red[t + k];
    __syncthreads();
  }
  if (t == 0) out[0] = red[0] / npix;
}

}  // namespace

extern "C" int zt_conv3x3_wide_bf16(const void* x, int ldx, int N, int H, int W, int Cin, const void* w, int CoutP, int ldk,
                                    const float* bias, void* y, int ldy, int Cout, int relu, hipStream_t stream) {
  ZT_REQUIRE(x && w && y && N >= 1 && H >= 1 && W >= 1);
  ZT_REQUIRE(Cin >= WC_KC && Cin % WC_KC == 0 && Cout >= WC_NC && Cout % WC_NC == 0 && CoutP >= Cout && ldk >= Cin && ldx >= Cin && ldy >= Cout);
  ZT_REQUIRE(ldx % 8 == 0 && ldk % 8 == 0 && ldy % 8 == 0);
  ZT_REQUIRE((((uintptr_t)x | (uintptr_t)w | (uintptr_t)y) & 15) == 0 && (!bias || ((uintptr_t)bias & 15) == 0));
  // 32-bit element offsets in the staging code
  ZT_REQUIRE((long long)N * H * W * ldx < 0x7FFFFFFFll && 9ll * CoutP * ldk < 0x7FFFFFFFll);
  WideArgs a;
  a.x = (const zt_bf16*)x; a.w = (const zt_bf16*)w; a.bias = bias; a.y = (zt_bf16*)y;
  a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.ldx = ldx; a.CoutP = CoutP; a.ldk = ldk; a.ldy = ldy; a.relu = relu;
  a.tilesY = zt_cdiv(H, WC_TH);
  ZT_REQUIRE((long long)a.tilesY * N <= 65535 && Cout / WC_NC <= 65535);
  hipLaunchKernelGGL(conv3x3_wide_bf16_kernel, dim3(zt_cdiv(W, WC_TW), a.tilesY * N, Cout / WC_NC), dim3(256), 0, stream, a);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}

extern "C" int zt_lpips_prep(const float* src, void* dst, int dt, int H, int W, hipStream_t stream) {
  ZT_REQUIRE(src && dst && H >= 1 && W >= 1 && (dt == 0 || dt == 1) && ((uintptr_t)dst & 15) == 0 && (long long)H * W < 0x7FFFFFFFll);
  const int HW = H * W;
  if (dt) hipLaunchKernelGGL(lpips_prep_kernel<zt_bf16>, dim3(zt_cdiv(HW, 256)), dim3(256), 0, stream, src, (zt_bf16*)dst, HW);
  else hipLaunchKernelGGL(lpips_prep_kernel<float>, dim3(zt_cdiv(HW, 256)), dim3(256), 0, stream, src, (float*)dst, HW);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}

extern "C" int zt_maxpool2_nhwc(const void* x, int dt, int ldx, int N, int H, int W, int C, void* y, int ldy, hipStream_t stream) {
  const int V = dt ? 8 : 4;
  ZT_REQUIRE(x && y && (dt == 0 || dt == 1) && N >= 1 && H >= 2 && W >= 2 && C >= V && C % V == 0 && ldx >= C && ldy >= C);
  ZT_REQUIRE(ldx % V == 0 && ldy % V == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0);
  const int Ho = H / 2, Wo = W / 2, CG = C / V;
  const long long total = (long long)N * Ho * Wo * CG;
  ZT_REQUIRE(zt_cdivl(total, 256) < 0x7FFFFFFFll);
  const dim3 grid((unsigned)zt_cdivl(total, 256));
  if (dt) hipLaunchKernelGGL((maxpool2_kernel<zt_bf16, 8>), grid, dim3(256), 0, stream, (const zt_bf16*)x, (zt_bf16*)y, ldx, ldy, H, W, Ho, Wo, CG, total);
  else hipLaunchKernelGGL((maxpool2_kernel<float, 4>), grid, dim3(256), 0, stream, (const float*)x, (float*)y, ldx, ldy, H, W, Ho, Wo, CG, total);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}

extern "C" int zt_lpips_layer(const void* fa, int lda, const void* fb, int ldb, int dt, long long npix, int C, const float* w,
                              double* partial, int npartial, double* out, hipStream_t stream) {
  ZT_REQUIRE(fa && fb && w && partial && out && (dt == 0 || dt == 1) && npix >= 1 && npartial >= 1);
  ZT_REQUIRE((C == 64 || C == 128 || C == 256 || C == 512) && lda >= C && ldb >= C);
  const int al = dt ? 8 : 4;
  ZT_REQUIRE(lda % al == 0 && ldb % al == 0 && (((uintptr_t)fa | (uintptr_t)fb) & 15) == 0);
  const int ppb = 256 / (C / 8);
  long long nblk = zt_cdivl(npix, (long long)ppb * 4);      // about four pixels per lane group and workgroup
  if (nblk > npartial) nblk = npartial;
  if (nblk > 2048) nblk = 2048;
  if (dt) hipLaunchKernelGGL(lpips_layer_kernel<zt_bf16>, dim3((unsigned)nblk), dim3(256), 0, stream, (const zt_bf16*)fa, (const zt_bf16*)fb, lda, ldb, npix, C, w, partial);
  else hipLaunchKernelGGL(lpips_layer_kernel<float>, dim3((unsigned)nblk), dim3(256), 0, stream, (const float*)fa, (const float*)fb, lda, ldb, npix, C, w, partial);
  ZT_LAUNCH_CHECK();
  hipLaunchKernelGGL(lpips_final_kernel, dim3(1), dim3(256), 0, stream, (const double*)partial, (int)nblk, (double)npix, out);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}
