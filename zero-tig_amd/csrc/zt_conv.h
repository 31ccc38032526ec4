// Internal header of the convolution sources (zt_conv.hip, zt_conv_*.hip, zt_wgrad.hip; not installed): the bf16 argument block,
// the tile constants and the few device helpers that more than one kernel family uses, and the per-family launchers that the
// dispatcher in zt_conv.hip calls.  One translation unit per kernel family: editing a kernel rebuilds its own file only.
#pragma once
#include "zt_common.h"

constexpr int TH = 4, TW = 32;          // output rows of a tiled workgroup / tile width of the tiled fp32, ws and rs kernels

__device__ __forceinline__ float apply_act(float v, int act) {
  switch (act) {
    case 1: return fmaxf(v, 0.f);
    case 2: return v > 0.f ? v : 0.2f * v;
    case 3: return 1.f / (1.f + expf(-v));
    case 4: return tanhf(v);
    case 5: return fminf(fmaxf(1.f / (1.f + expf(-v)), 0.0001f), 1.f);
    default: return v;
  }
}

// =====================================================================================================================
// bf16 throughput mode: activations and weights are bf16 in HBM, accumulation fp32 (v_mfma_f32_16x16x32_bf16, 16x the
// fp32 matrix rate).  Same tiling as the fp32 kernels; the K step is 32 channels, both operands are read from LDS with
// one ds_read_b128 per fragment ([pixel][40] / [cout][40] bf16 rows: 80-byte pitch -> conflict free).
// Weights: [tap][CoutP16][ldk] with the input channel fastest (ldk = Cin rounded to 8, zero padded).
// =====================================================================================================================
struct ConvArgsH {
  const zt_bf16* x;
  const zt_bf16* x2;
  const zt_bf16* w;
  const float* bias;
  const zt_bf16* aux;
  void* y;
  int N, H, W, Cin, ldx, ldx2, csplit;
  int Ho, Wo, Cout, CoutP, ldk, ldy, ldaux;
  int padH, padW;
  int act, epi, out_mode;      // out_mode: 0 bf16 nhwc, 1 fp32 planar, 2 fp32 nhwc
  float alpha;
  int tilesX, tilesY;
  zt_bf16* y2;                 // epi 4: second destination (r * h), channels [esplit, Cout) go there
  int ldy2, esplit;
  float* stats;                // conv_rs STATS: per-workgroup (sum, sum of squares) of the stored outputs, [grid][2][Cout]
  // conv_rs BSTATS (data gradient + residual of an Enhancer block): the BatchNorm backward sums of the PREVIOUS block, whose output
  // gradient this launch produces -- g = out * [bn_scale * zprev + bn_shift > 0]; stats[grid][2][Cout] = (sum g, sum g (zprev - bn_mean))
  const zt_bf16* zprev;
  int ldz;
  const float* bn_scale;
  const float* bn_shift;
  const float* bn_mean;
};

constexpr int HCK = 32;                 // channel granularity of a two-part (split) input

namespace {
__device__ const uint4 zt_zero_chunk = {0u, 0u, 0u, 0u};        // LDS-DMA source of the halo's out-of-image pixels
}  // namespace

__device__ __forceinline__ zt_f32x4 zt_mfma_bf16_k16(zt_s16x4 a, zt_s16x4 b, zt_f32x4 c) {
  // D = A(16x16) * B(16x16) + C: lane l holds A[row l&15][k = 4(l>>4)+j], B[k = 4(l>>4)+j][col l&15], j = 0..3
  return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0);
}

// ---- per-family launchers (hidden: not part of the library's ABI).  Each returns 0 or ZT_EINVAL when no instantiation takes
// the problem; the caller checks the launch.
#define ZT_HIDDEN __attribute__((visibility("hidden")))
// zt_conv_tiled.hip: tilesX / tilesY set by the caller for 16 * MT-pixel tiles
ZT_HIDDEN int zt_launch_conv_tiled(const ConvArgsH& a, int KH, int KW, int stride, int MT, int NT, hipStream_t stream);
// zt_conv_ws.hip: K in {1, 3}; tilesX set by the caller, tilesY by the launcher (8-row tiles)
ZT_HIDDEN int zt_launch_conv_ws(ConvArgsH& a, int K, int NT, int CCH, hipStream_t stream);
// zt_conv_rs.hip: sets tilesX / tilesY
ZT_HIDDEN int zt_launch_conv_rs(ConvArgsH& a, hipStream_t stream);
// zt_conv_thin.hip: the 1x1 streaming kernels (thin fp32 planar output / thin input)
ZT_HIDDEN int zt_launch_conv1x1_thinout(const ConvArgsH& a, hipStream_t stream);
ZT_HIDDEN int zt_launch_conv1x1_thin(const ConvArgsH& a, hipStream_t stream);
// zt_wgrad.hip: the slab reduction shared by the fp32 and bf16 weight gradients
ZT_HIDDEN int zt_launch_wgrad_reduce(const float* slab, int nslab, int ntap, int CT16, int NT16, float* grad_w, int Cout, int Cin,
                                     int accumulate, float* grad_b, hipStream_t stream);

extern "C" int zt_conv2d_nhwc_bf16(const void* x, const void* x2, int csplit, int ldx, int ldx2, int N, int H, int W, int Cin,
                                   const void* w, int CoutP, int ldk, const float* bias, void* y, int ldy, int out_mode, int Cout,
                                   int KH, int KW, int stride, int padH, int padW, int act, float alpha, const void* aux,
                                   int ldaux, int epi, hipStream_t stream);
