#include "zt_conv.h"
#include <stdlib.h>

namespace {

// ---- persistent, weight-stationary variant for the full-resolution enhancement / denoising layers (stride 1, K in {1,3},
// Cin <= 64): each workgroup (8 waves = 8 output rows x 32 columns) loads ALL its weights into LDS once and then walks
// pixel tiles grid-stride; the next tile's halo is prefetched into registers while the MFMAs of the current one run
// (two barriers per tile).  LDS rows are [pixel | cout][CCH*32 + 8] bf16 (144 B or 80 B pitch: conflict-free b128 reads).
template <int K, int NT, int CCH, int PTH>
__global__ void __launch_bounds__(64 * PTH) conv_ws_bf16_kernel(ConvArgsH a, int ntiles) {
  constexpr int NTHR = 64 * PTH;
  constexpr int CP = CCH == 2 ? 80 : 48;       // 160 B / 96 B row pitch: conflict-free ds_read_b128 (brute-forced over lane groups)
  constexpr int IR = PTH + K - 1, IC = TW + K - 1;
  constexpr int NPF = (IR * IC * CCH * 4 + NTHR - 1) / NTHR;     // 16-byte prefetch registers per thread
  constexpr int XS_HALO = IR * IC * CP, XS_STAGE = PTH * TW * (NT * 16 + 8);      // halo tile / output staging share xs
  __shared__ __attribute__((aligned(16))) zt_bf16 ws[K * K * NT * 16 * CP];
  __shared__ __attribute__((aligned(16))) zt_bf16 xs[XS_HALO > XS_STAGE ? XS_HALO : XS_STAGE];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, l4 = lane >> 4;
  const int co0 = blockIdx.y * (NT * 16);
  constexpr int pad = (K - 1) / 2;

  for (int e = tid; e < K * K * NT * 16 * CCH * 4; e += NTHR) {
    int q = e % (CCH * 4);
    int r = e / (CCH * 4);
    int co = r % (NT * 16), tap = r / (NT * 16);
    int c = q * 8;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (c < a.ldk && co0 + co < a.CoutP) v = *reinterpret_cast<const uint4*>(a.w + ((size_t)tap * a.CoutP + co0 + co) * a.ldk + c);
    *reinterpret_cast<uint4*>(ws + (tap * NT * 16 + co) * CP + c) = v;
  }

  // the halo element a thread fetches is the same for every tile: precompute its (row, col, channel) once
  uint4 pf[NPF];
  int pf_iy[NPF], pf_ix[NPF], pf_c[NPF];
#pragma unroll
  for (int i = 0; i < NPF; ++i) {
    int e = tid + i * NTHR;
    int q = e % (CCH * 4), p = e / (CCH * 4);
    pf_iy[i] = e < IR * IC * CCH * 4 ? p / IC : -100000;       // out-of-range slots never pass the bounds test
    pf_ix[i] = p % IC;
    pf_c[i] = q * 8;
  }
  auto prefetch = [&](int tile) {
    const int tx = tile % a.tilesX, ty = tile / a.tilesX;
    const int gy0 = ty * PTH - pad, gx0 = tx * TW - pad;
#pragma unroll
    for (int i = 0; i < NPF; ++i) {
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      const int gy = gy0 + pf_iy[i], gx = gx0 + pf_ix[i], c = pf_c[i];
      if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W && c < a.Cin) {
        v = *reinterpret_cast<const uint4*>(a.x + ((size_t)gy * a.W + gx) * a.ldx + c);
        if (c + 8 > a.Cin) {
          zt_bf16 tmp[8];
          __builtin_memcpy(tmp, &v, 16);
          for (int j = 0; j < 8; ++j)
            if (c + j >= a.Cin) tmp[j] = 0;
          __builtin_memcpy(&v, tmp, 16);
        }
      }
      pf[i] = v;
    }
  };

  int tile = blockIdx.x;
  if (tile < ntiles) prefetch(tile);
  // de-phase neighbouring workgroups by ~half a tile so that HBM reads, MFMA work and HBM writes of different CUs interleave
  // instead of the whole chip moving through the same phase in lock-step (speed only; no correctness dependence)
  if (blockIdx.x & 1) {
    __builtin_amdgcn_s_sleep(127);
    __builtin_amdgcn_s_sleep(127);
  }
  for (; tile < ntiles; tile += gridDim.x) {
#pragma unroll
    for (int i = 0; i < NPF; ++i) {
      int e = tid + i * NTHR;
      if (e < IR * IC * CCH * 4) *reinterpret_cast<uint4*>(xs + (e / (CCH * 4)) * CP + (e % (CCH * 4)) * 8) = pf[i];
    }
    __syncthreads();
    const int next = tile + gridDim.x;
    if (next < ntiles) prefetch(next);

    zt_f32x4 acc[2][NT];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int q = 0; q < NT; ++q) acc[m][q] = (zt_f32x4){0.f, 0.f, 0.f, 0.f};
    // software-pipelined over the K*K*CCH (tap, channel-half) steps: the fragments of step i+1 are in flight while the
    // MFMAs of step i issue.  Weights are the A operand, pixels the B operand: D[row = cout 4*(lane>>4)+j][col = pixel
    // lane&15], i.e. every lane ends up with 4 CONSECUTIVE output channels of one pixel (8-byte staging writes below).
    constexpr int NSTEP = K * K * CCH;
    zt_s16x8 av[2][2], bv[2][NT];
    const zt_bf16* xb = xs + (wave * IC + l15) * CP + 8 * l4;
    const zt_bf16* wb = ws + l15 * CP + 8 * l4;
#define ZT_LOADF(buf, step)                                                                                         \
  {                                                                                                                 \
    constexpr int tap_ = (step) / CCH, kc_ = (step) % CCH, ky_ = tap_ / K, kx_ = tap_ % K;                          \
    _Pragma("unroll") for (int m = 0; m < 2; ++m) av[buf][m] =                                                      \
        *reinterpret_cast<const zt_s16x8*>(xb + (ky_ * IC + m * 16 + kx_) * CP + kc_ * 32);                         \
    _Pragma("unroll") for (int q = 0; q < NT; ++q) bv[buf][q] =                                                     \
        *reinterpret_cast<const zt_s16x8*>(wb + (tap_ * NT * 16 + q * 16) * CP + kc_ * 32);                         \
  }
    ZT_LOADF(0, 0)
    zt_static_for<0, NSTEP>([&](auto step_c) {
      constexpr int step = decltype(step_c)::value;
      constexpr int cur = step & 1;
      if constexpr (step + 1 < NSTEP) ZT_LOADF(cur ^ 1, step + 1)
      __builtin_amdgcn_sched_barrier(0);      // keep the next step's LDS reads ahead of this step's MFMAs (hipcc re-serialises them otherwise)
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int q = 0; q < NT; ++q) acc[m][q] = zt_mfma_bf16(bv[cur][q], av[cur][m], acc[m][q]);
      __builtin_amdgcn_sched_barrier(0);
    });
#undef ZT_LOADF

    const int tx = tile % a.tilesX, ty = tile / a.tilesX;
    const int oy = ty * PTH + wave, ox0 = tx * TW;
    if (a.out_mode == 0) {
      // bf16 nhwc output: transpose the accumulators through LDS (wave-private slice of the halo buffer) so that global
      // traffic is 16 bytes per lane (2-byte stores are store-issue bound: ~15x slower on this layer)
      constexpr int OP = NT * 16 + 8;                      // staging row pitch (elements)
      __syncthreads();                                      // every wave is done reading xs
      zt_bf16* st = xs + wave * (TW * OP);
      // none / ReLU / LeakyReLU(0.2) are max(v, slope*v) with slope 1 / 0 / 0.2: branch-free on the hot path (a runtime switch
      // expanded over the 32 accumulators blew up the code size and the instruction cache); other activations go the slow way.
      const bool simple_act = a.act <= 2;
      const float slope = a.act == 0 ? 1.f : (a.act == 1 ? 0.f : 0.2f);
#pragma unroll
      for (int q = 0; q < NT; ++q) {
        const int cb = co0 + q * 16 + l4 * 4;
        float bj[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bj[j] = (a.bias && cb + j < a.Cout) ? a.bias[cb + j] : 0.f;
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          float v[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            v[j] = a.alpha * (acc[m][q][j] + bj[j]);
            v[j] = fmaxf(v[j], slope * v[j]);
          }
          if (!simple_act) {
#pragma unroll 1
            for (int j = 0; j < 4; ++j) v[j] = apply_act(a.alpha * (acc[m][q][j] + bj[j]), a.act);
          }
          uint2 pk;
          pk.x = zt_f2bf2(v[0], v[1]);
          pk.y = zt_f2bf2(v[2], v[3]);
          *reinterpret_cast<uint2*>(st + (m * 16 + l15) * OP + q * 16 + l4 * 4) = pk;
        }
      }
      // same wave wrote and reads: LDS ops of one wave complete in order, so no workgroup barrier is needed; the wave barrier
      // only pins the compiler's (and the test emulator's) ordering of the two phases
      __builtin_amdgcn_wave_barrier();
      if (oy < a.Ho) {
        for (int e = lane; e < TW * NT * 2; e += 64) {
          const int p = e / (NT * 2), c8 = (e % (NT * 2)) * 8;
          const int ox = ox0 + p, co = co0 + c8;
          if (ox < a.Wo && co < a.Cout) {
            uint4 v = *reinterpret_cast<const uint4*>(st + p * OP + c8);
            const size_t pix = (size_t)oy * a.Wo + ox;
            if (a.epi) {
              uint4 u = *reinterpret_cast<const uint4*>(a.aux + pix * a.ldaux + co);
              zt_bf16 tv[8], tu[8];
              __builtin_memcpy(tv, &v, 16);
              __builtin_memcpy(tu, &u, 16);
#pragma unroll
              for (int k = 0; k < 8; ++k) {
                float fv = zt_bf2f(tv[k]), fu = zt_bf2f(tu[k]);
                if (a.epi == 1) fv *= (fu > 0.f ? 1.f : 0.2f);
                else if (a.epi == 2) fv *= (fu > 0.f ? 1.f : 0.f);
                else fv += fu;
                tv[k] = zt_f2bf(fv);
              }
              __builtin_memcpy(&v, tv, 16);
            }
            zt_bf16* dst = (zt_bf16*)a.y + pix * a.ldy + co;
            if (co + 8 <= a.Cout) *reinterpret_cast<uint4*>(dst) = v;
            else {
              zt_bf16 tv[8];
              __builtin_memcpy(tv, &v, 16);
              for (int k = 0; k < 8 && co + k < a.Cout; ++k) dst[k] = tv[k];
            }
          }
        }
      }
    } else if (oy < a.Ho) {
#pragma unroll
      for (int q = 0; q < NT; ++q) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int co = co0 + q * 16 + l4 * 4 + j;
          if (co < a.Cout) {
            const float b = a.bias ? a.bias[co] : 0.f;
#pragma unroll
            for (int m = 0; m < 2; ++m) {
              const int ox = ox0 + m * 16 + l15;
              if (ox < a.Wo) {
                float v = apply_act(a.alpha * (acc[m][q][j] + b), a.act);
                const size_t pix = (size_t)oy * a.Wo + ox;
                if (a.epi) {
                  float u = zt_bf2f(a.aux[pix * a.ldaux + co]);
                  if (a.epi == 1) v *= (u > 0.f ? 1.f : 0.2f);
                  else if (a.epi == 2) v *= (u > 0.f ? 1.f : 0.f);
                  else v += u;
                }
                if (a.out_mode == 1) ((float*)a.y)[(size_t)co * a.ldy + pix] = v;
                else ((float*)a.y)[pix * a.ldy + co] = v;
              }
            }
          }
        }
      }
    }
    __syncthreads();
  }
}

template <int K>
int launch_conv_ws(ConvArgsH& a, int NT, int CCH, int pth, hipStream_t stream) {
  int c16 = (a.Cout + 15) / 16;
  a.tilesY = zt_cdiv(a.Ho, pth);
  int ntiles = a.tilesX * a.tilesY;
  // LDS per workgroup decides how many are co-resident per CU (phases of different workgroups overlap HBM reads, MFMA and stores)
  int cp = CCH == 2 ? 80 : 48;
  int lds = 2 * (K * K * NT * 16 * cp + (pth + K - 1) * (TW + K - 1) * cp);
  int per_cu = 160 * 1024 / (lds + 1024);
  per_cu = per_cu < 1 ? 1 : (per_cu > 4 ? 4 : per_cu);
  int gx = ntiles < 256 * per_cu ? ntiles : 256 * per_cu;
  if (const char* e = getenv("ZT_CONV_BLOCKS")) gx = atoi(e) > 0 && atoi(e) < gx ? atoi(e) : gx;      // test hook: fewer workgroups, deeper tile loops
  dim3 grid(gx, (c16 + NT - 1) / NT), block(64 * pth);
#define ZT_WS(nt, cch)                                                                               \
  hipLaunchKernelGGL((conv_ws_bf16_kernel<K, nt, cch, 8>), grid, block, 0, stream, a, ntiles);      \
  return 0
  if (CCH == 1) {
    if (NT == 1) { ZT_WS(1, 1); }
    if (NT == 2) { ZT_WS(2, 1); }
    if (NT == 3) { ZT_WS(3, 1); }
    ZT_WS(4, 1);
  }
  if (NT == 1) { ZT_WS(1, 2); }
  if (NT == 2) { ZT_WS(2, 2); }
  if (NT == 3) { ZT_WS(3, 2); }
  ZT_WS(4, 2);
#undef ZT_WS
}

}  // namespace

int zt_launch_conv_ws(ConvArgsH& a, int K, int NT, int CCH, hipStream_t stream) {
  // 8-row tiles, all couts per workgroup: the best of the (rows, couts) configurations measured
  return K == 3 ? launch_conv_ws<3>(a, NT, CCH, 8, stream) : launch_conv_ws<1>(a, NT, CCH, 8, stream);
}
