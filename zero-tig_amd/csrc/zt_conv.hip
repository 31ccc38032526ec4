// bf16 convolution entry points: argument checks and the choice of kernel family (conv2d_bf16_impl), and the weight repacks.
// The kernels live in one file per family: zt_conv_tiled.hip (tiled implicit GEMM, the RAFT pair kernels), zt_conv_ws.hip
// (persistent, weights in LDS), zt_conv_rs.hip (persistent, weights in registers), zt_conv_thin.hip (1x1 streaming kernels);
// the exact fp32 family is zt_conv_f32.hip, the weight gradients zt_wgrad.hip.  zt_conv.h holds what they share.
#include "zt_conv.h"
#include <stdlib.h>

namespace {

// all weight repacks of a step (forward and data-gradient operator of every layer) in one launch: entry = blockIdx.y
constexpr int ZT_MAXREP = 24;
struct RepackTable {
  const float* src[ZT_MAXREP];
  zt_bf16* dst[ZT_MAXREP];
  int Cout[ZT_MAXREP], Cin[ZT_MAXREP], K[ZT_MAXREP], CoutP[ZT_MAXREP], ldk[ZT_MAXREP], tflip[ZT_MAXREP];
};

__global__ void __launch_bounds__(256) repack_w_bf16_multi_kernel(RepackTable t) {
  const int en = blockIdx.y;
  const int Cout = t.Cout[en], Cin = t.Cin[en], KH = t.K[en], KW = t.K[en], CoutP = t.CoutP[en], ldk = t.ldk[en];
  const int total = Cout * Cin * KH * KW;
  for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
    const int kx = idx % KW, ky = (idx / KW) % KH, ci = (idx / (KW * KH)) % Cin, co = idx / (KW * KH * Cin);
    const zt_bf16 v = zt_f2bf(t.src[en][idx]);
    if (!t.tflip[en]) t.dst[en][((size_t)(ky * KW + kx) * CoutP + co) * ldk + ci] = v;
    else t.dst[en][((size_t)((KH - 1 - ky) * KW + (KW - 1 - kx)) * CoutP + ci) * ldk + co] = v;
  }
}

// torch fp32 [Cout][Cin][KH][KW] -> bf16 [tap][CoutP][ldk] (input channel fastest); transpose_flip: the data-gradient operator
__global__ void __launch_bounds__(256) repack_w_bf16_kernel(const float* __restrict__ src, zt_bf16* __restrict__ dst, int Cout,
                                                            int Cin, int KH, int KW, int CoutP, int ldk, int co_off,
                                                            int transpose_flip, int total) {
  int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  int kx = idx % KW;
  int ky = (idx / KW) % KH;
  int ci = (idx / (KW * KH)) % Cin;
  int co = idx / (KW * KH * Cin);
  zt_bf16 v = zt_f2bf(src[idx]);
  if (!transpose_flip) dst[((size_t)(ky * KW + kx) * CoutP + co_off + co) * ldk + ci] = v;
  else dst[((size_t)((KH - 1 - ky) * KW + (KW - 1 - kx)) * CoutP + co_off + ci) * ldk + co] = v;
}

}  // namespace

// variant: 0 = choose by problem size, 1 = force the persistent weight-stationary kernel, 2 = force the tiled kernel,
// 3 = force the register-stationary kernel
struct BnBwdFuse {             // zt_conv3x3_dgrad_bn_sums_bf16: the previous block's pre-activation and BatchNorm constants
  const void* zprev;
  int ldz;
  const float *scale, *shift, *mean;
};

static int conv2d_bf16_impl(const void* x, const void* x2, int csplit, int ldx, int ldx2, int N, int H, int W, int Cin,
                            const void* w, int CoutP, int ldk, const float* bias, void* y, int ldy, int out_mode,
                            int Cout, int KH, int KW, int stride, int padH, int padW, int act, float alpha,
                            const void* aux, int ldaux, int epi, int variant, void* y2, int ldy2, int esplit, hipStream_t stream,
                            float* stats = nullptr, const BnBwdFuse* bnb = nullptr) {
  ZT_REQUIRE(x && w && y && N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && out_mode >= 0 && out_mode <= 2);
  ZT_REQUIRE(epi >= 0 && epi <= 6 && (epi < 4 || (out_mode == 0 && variant == 2)) && (epi != 4 || (y2 && esplit > 0 && esplit < Cout)));
  ZT_REQUIRE(ldx % 8 == 0 && ldk % 8 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)w & 15) == 0);
  ZT_REQUIRE(!x2 || (csplit % HCK == 0 && ldx2 % 8 == 0 && ((uintptr_t)x2 & 15) == 0));
  ZT_REQUIRE(epi == 0 || aux);
  ConvArgsH a;
  a.x = (const zt_bf16*)x; a.x2 = (const zt_bf16*)x2; a.w = (const zt_bf16*)w; a.bias = bias; a.aux = (const zt_bf16*)aux; a.y = y;
  a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.ldx = ldx; a.ldx2 = ldx2; a.csplit = csplit;
  a.Ho = (H + 2 * padH - KH) / stride + 1;
  a.Wo = (W + 2 * padW - KW) / stride + 1;
  a.Cout = Cout; a.CoutP = CoutP; a.ldk = ldk; a.ldy = ldy; a.ldaux = ldaux;
  a.padH = padH; a.padW = padW; a.act = act; a.epi = epi; a.out_mode = out_mode; a.alpha = alpha;
  a.y2 = (zt_bf16*)y2; a.ldy2 = ldy2; a.esplit = esplit; a.stats = stats;
  a.zprev = nullptr; a.ldz = 0; a.bn_scale = a.bn_shift = a.bn_mean = nullptr;
  if (bnb) { a.zprev = (const zt_bf16*)bnb->zprev; a.ldz = bnb->ldz; a.bn_scale = bnb->scale; a.bn_shift = bnb->shift; a.bn_mean = bnb->mean; }
  ZT_REQUIRE(variant >= 0 && variant <= 3 && a.Ho > 0 && a.Wo > 0);
  // 32-bit element offsets in the staging code
  ZT_REQUIRE((long long)N * H * W * (ldx > ldx2 ? ldx : ldx2) < 0x7FFFFFFFll && (long long)KH * KW * CoutP * ldk < 0x7FFFFFFFll);
  a.tilesY = zt_cdiv(a.Ho, TH);
  int c16 = (Cout + 15) / 16;
  int NT = c16 >= 4 ? ((c16 % 4 == 0) ? 4 : (c16 % 3 == 0 ? 3 : 4)) : c16;
  // small feature maps (RAFT at 1/8 resolution): narrower tiles / fewer channels per workgroup so that >= ~2 workgroups per CU exist
  int MT = 2;
  long long wgs = (long long)zt_cdiv(a.Wo, 32) * a.tilesY * N * zt_cdiv(c16, NT);
  if (wgs < 512 || stride == 2) MT = 1;
  if (MT == 1 && NT == 4 && (long long)zt_cdiv(a.Wo, 16) * a.tilesY * N * zt_cdiv(c16, NT) < 512 && c16 % 2 == 0) NT = 2;
  // 32 couts per workgroup keep every tap's weights of a chunk resident next to the pixel tile (one staging + two barriers per chunk
  // instead of one per kernel row): -65 us over the RAFT encoders' 64-channel 180 x 320 layers (tools/bench_raft.py)
  if (NT == 4 && c16 % 2 == 0 && stride == 1) NT = 2;
  // full-resolution stride-1 layers of the enhancement nets: persistent weight-stationary kernel
  const bool ws_ok = N == 1 && stride == 1 && KH == KW && (KH == 1 || KH == 3) && padH == KH / 2 && padW == KW / 2 && Cin <= 64 && !x2;
  ZT_REQUIRE(variant != 1 || ws_ok);
  // thin-output 1x1 layers with planar fp32 output: streaming kernel
  if (variant == 0 && N == 1 && KH == 1 && KW == 1 && stride == 1 && padH == 0 && padW == 0 && !x2 && Cout <= 8 && out_mode == 1 &&
      epi == 0 && Cin % 8 == 0 && Cin <= 64 && ldk >= Cin && CoutP >= Cout) {
    zt_launch_conv1x1_thinout(a, stream);
    ZT_LAUNCH_CHECK();
    return ZT_OK;
  }
  // thin-input 1x1 layers: streaming kernel
  if (variant == 0 && N == 1 && KH == 1 && KW == 1 && stride == 1 && padH == 0 && padW == 0 && !x2 && Cin <= 8 && ldx == 8 && ldk == 8 &&
      out_mode == 0 && act <= 2 && Cout % 8 == 0 && CoutP >= Cout && ldy % 8 == 0 && ((uintptr_t)y & 15) == 0 &&
      (!aux || (ldaux % 8 == 0 && ((uintptr_t)aux & 15) == 0))) {
    zt_launch_conv1x1_thin(a, stream);
    ZT_LAUNCH_CHECK();
    return ZT_OK;
  }
  // register-stationary kernel: 3x3, bf16 nhwc output, 48 or 64 couts, input channels <= 16, 33..48 (Cout 48) or 49..64 (Cout 64)
  const bool rs_ok = ws_ok && KH == 3 && out_mode == 0 && act <= 2 && alpha == 1.f && ldy % 8 == 0 && ((uintptr_t)y & 15) == 0 &&
                     (!aux || (ldaux % 8 == 0 && ((uintptr_t)aux & 15) == 0)) && ldx >= 8 &&
                     ((Cout == 64 && (Cin <= 16 || Cin == 56 || Cin == 64)) || (Cout == 48 && (Cin <= 16 || Cin == 40 || Cin == 48)));
  ZT_REQUIRE(variant != 3 || rs_ok);
  if (stats && !(rs_ok && variant == 3)) return ZT_EINVAL;      // fused statistics exist in the register-stationary kernel only
  if (rs_ok && (variant == 3 || (variant == 0 && (long long)zt_cdiv(a.Wo, TW) * zt_cdiv(a.Ho, 8) >= 1024))) {
    int rcp = zt_launch_conv_rs(a, stream);
    if (rcp) return rcp;
    ZT_LAUNCH_CHECK();
    return ZT_OK;
  }
  if (variant != 2 && ws_ok && (variant == 1 || (long long)zt_cdiv(a.Wo, TW) * zt_cdiv(a.Ho, 8) >= 1024)) {
    a.tilesX = zt_cdiv(a.Wo, TW);
    int CCH = Cin <= 32 ? 1 : 2;
    int rcw = zt_launch_conv_ws(a, KH, NT, CCH, stream);
    if (rcw) return rcw;
    ZT_LAUNCH_CHECK();
    return ZT_OK;
  }
  a.tilesX = zt_cdiv(a.Wo, 16 * MT);
  int rc = zt_launch_conv_tiled(a, KH, KW, stride, MT, NT, stream);
  if (rc) return rc;
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}

extern "C" int zt_conv2d_nhwc_bf16_variant(const void* x, const void* x2, int csplit, int ldx, int ldx2, int N, int H, int W, int Cin,
                                           const void* w, int CoutP, int ldk, const float* bias, void* y, int ldy, int out_mode,
                                           int Cout, int KH, int KW, int stride, int padH, int padW, int act, float alpha,
                                           const void* aux, int ldaux, int epi, int variant, hipStream_t stream) {
  ZT_REQUIRE(epi >= 0 && epi <= 3);
  return conv2d_bf16_impl(x, x2, csplit, ldx, ldx2, N, H, W, Cin, w, CoutP, ldk, bias, y, ldy, out_mode, Cout, KH, KW, stride, padH, padW,
                          act, alpha, aux, ldaux, epi, variant, nullptr, 0, 0, stream);
}

extern "C" int zt_conv2d_nhwc_bf16_ex(const void* x, const void* x2, int csplit, int ldx, int ldx2, int N, int H, int W, int Cin,
                                      const void* w, int CoutP, int ldk, const float* bias, void* y, int ldy, int out_mode,
                                      int Cout, int KH, int KW, int stride, int padH, int padW, int act, float alpha,
                                      const void* aux, int ldaux, int epi, void* y2, int ldy2, int esplit, hipStream_t stream) {
  return conv2d_bf16_impl(x, x2, csplit, ldx, ldx2, N, H, W, Cin, w, CoutP, ldk, bias, y, ldy, out_mode, Cout, KH, KW, stride, padH, padW,
                          act, alpha, aux, ldaux, epi, epi >= 4 ? 2 : 0, y2, ldy2, esplit, stream);
}

extern "C" int zt_chan_stats_nhwc(const void* x, int dt, int ldx, int N, int HW, int C, int nblk, float* partial, hipStream_t stream);

extern "C" int zt_conv3x3_bn_stats_bf16(const void* x, int ldx, int H, int W, int Cin, const void* w, int CoutP, int ldk, const float* bias,
                                        void* y, int ldy, int Cout, float* stats, int stats_blocks, hipStream_t stream) {
  ZT_REQUIRE(x && w && y && stats && stats_blocks == 512 && Cout % 8 == 0);
  hipError_t e = hipMemsetAsync(stats, 0, sizeof(float) * (size_t)stats_blocks * 2 * Cout, stream);
  if (e != hipSuccess) return (int)e;
  const char* mt = getenv("ZT_STATS_FUSE_MIN_TILES");          // tests force the fused kernel onto small images
  const long long min_tiles = mt ? atoll(mt) : 1024;
  const bool fused = Cout == 64 && (Cin == 56 || Cin == 64) && ldx >= 8 && ldy % 8 == 0 && ((uintptr_t)y & 15) == 0 &&
                     (long long)zt_cdiv(W, TW) * zt_cdiv(H, 8) >= min_tiles;
  if (fused)
    return conv2d_bf16_impl(x, nullptr, 0, ldx, 0, 1, H, W, Cin, w, CoutP, ldk, bias, y, ldy, 0, Cout, 3, 3, 1, 1, 1, 0, 1.f, nullptr, 0, 0, 3,
                            nullptr, 0, 0, stream, stats);
  int rc = conv2d_bf16_impl(x, nullptr, 0, ldx, 0, 1, H, W, Cin, w, CoutP, ldk, bias, y, ldy, 0, Cout, 3, 3, 1, 1, 1, 0, 1.f, nullptr, 0, 0, 0,
                            nullptr, 0, 0, stream);
  if (rc) return rc;
  const int HW = H * W;
  int nblk = HW / 64 < 1 ? 1 : (HW / 64 > stats_blocks ? stats_blocks : HW / 64);
  return zt_chan_stats_nhwc(y, 1, ldy, 1, HW, Cout, nblk, stats, stream);
}

extern "C" int zt_conv3x3_dgrad_bn_sums_bf16(const void* dz, int lddz, int H, int W, const void* wT, int CoutP, int ldk, void* df, int lddf,
                                             const void* res, int ldres, const void* zprev, int ldz, const float* bn_scale,
                                             const float* bn_shift, const float* bn_mean, float* stats, int stats_blocks, hipStream_t stream) {
  ZT_REQUIRE(dz && wT && df && res && zprev && bn_scale && bn_shift && bn_mean && stats && stats_blocks == 512);
  ZT_REQUIRE(ldz % 8 == 0 && ((uintptr_t)zprev & 15) == 0 && (long long)zt_cdiv(W, TW) * zt_cdiv(H, 4) >= 1);
  hipError_t e = hipMemsetAsync(stats, 0, sizeof(float) * (size_t)stats_blocks * 2 * 64, stream);      // rows beyond the launch's workgroups stay zero
  if (e != hipSuccess) return (int)e;
  BnBwdFuse b = {zprev, ldz, bn_scale, bn_shift, bn_mean};
  return conv2d_bf16_impl(dz, nullptr, 0, lddz, 0, 1, H, W, 64, wT, CoutP, ldk, nullptr, df, lddf, 0, 64, 3, 3, 1, 1, 1, 0, 1.f, res, ldres, 3, 3, nullptr, 0,
                          0, stream, stats, &b);
}

extern "C" int zt_conv2d_nhwc_bf16(const void* x, const void* x2, int csplit, int ldx, int ldx2, int N, int H, int W, int Cin,
                                   const void* w, int CoutP, int ldk, const float* bias, void* y, int ldy, int out_mode, int Cout,
                                   int KH, int KW, int stride, int padH, int padW, int act, float alpha, const void* aux,
                                   int ldaux, int epi, hipStream_t stream) {
  return zt_conv2d_nhwc_bf16_variant(x, x2, csplit, ldx, ldx2, N, H, W, Cin, w, CoutP, ldk, bias, y, ldy, out_mode, Cout, KH, KW,
                                     stride, padH, padW, act, alpha, aux, ldaux, epi, 0, stream);
}

extern "C" int zt_repack_conv_weights_bf16_multi(int n, const void* const* src, void* const* dst, const int* Cout, const int* Cin,
                                                 const int* K, const int* CoutP, const int* ldk, const int* transpose_flip,
                                                 hipStream_t stream) {
  ZT_REQUIRE(n >= 1 && n <= ZT_MAXREP && src && dst && Cout && Cin && K && CoutP && ldk && transpose_flip);
  RepackTable t;
  int maxtotal = 0;
  for (int i = 0; i < ZT_MAXREP; ++i) {
    const int j = i < n ? i : 0;
    ZT_REQUIRE(src[j] && dst[j] && CoutP[j] % 16 == 0 && ldk[j] % 8 == 0);
    t.src[i] = (const float*)src[j]; t.dst[i] = (zt_bf16*)dst[j]; t.Cout[i] = Cout[j]; t.Cin[i] = Cin[j]; t.K[i] = K[j];
    t.CoutP[i] = CoutP[j]; t.ldk[i] = ldk[j]; t.tflip[i] = transpose_flip[j];
    const int total = Cout[j] * Cin[j] * K[j] * K[j];
    if (i < n && total > maxtotal) maxtotal = total;
  }
  int gx = zt_cdiv(maxtotal, 256);
  hipLaunchKernelGGL(repack_w_bf16_multi_kernel, dim3(gx > 64 ? 64 : gx, n), dim3(256), 0, stream, t);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}

extern "C" int zt_repack_conv_weight_bf16(const float* src, void* dst, int Cout, int Cin, int KH, int KW, int CoutP, int ldk,
                                          int co_off, int transpose_flip, hipStream_t stream) {
  ZT_REQUIRE(src && dst && CoutP % 16 == 0 && ldk % 8 == 0);
  int total = Cout * Cin * KH * KW;
  hipLaunchKernelGGL(repack_w_bf16_kernel, dim3(zt_cdiv(total, 256)), dim3(256), 0, stream, src, (zt_bf16*)dst, Cout, Cin, KH, KW,
                     CoutP, ldk, co_off, transpose_flip, total);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}
