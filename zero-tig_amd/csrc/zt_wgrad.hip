// bf16 weight gradients (register-staged and LDS-DMA forms) and the slab reductions that finish every weight gradient, fp32
// and bf16: each workgroup of a partial pass writes one slab, the reduce kernels sum the slabs in a fixed order.
#include "zt_conv.h"
#include <stdlib.h>

namespace {

// grad_w[co][ci][ky][kx] (+)= sum_slabs slab[s][tap][ci][co]; grad_b[co] (+)= sum_slabs slab[s][bias tail].  32 slab
// elements (co fastest -> coalesced) x 8 slab groups per workgroup, eight loads in flight per thread; fixed summation order
// (deterministic).
__global__ void __launch_bounds__(256) wgrad_reduce_kernel(const float* __restrict__ slab, int nslab, int ntap, int CT16,
                                                           int NT16, float* __restrict__ grad, int Cout, int Cin,
                                                           int accumulate, float* __restrict__ grad_b) {
  __shared__ float sh[256];
  const int ex = threadIdx.x & 31, sg = threadIdx.x >> 5;
  const int e = blockIdx.x * 32 + ex;
  const int nw = ntap * CT16 * NT16;
  const int total = nw + NT16;
  float s = 0.f;
  if (e < total) {
    const size_t stride = (size_t)total;
    for (int k = sg; k < nslab; k += 64) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (k + 8 * j < nslab) ? slab[(size_t)(k + 8 * j) * stride + e] : 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) s += v[j];
    }
  }
  sh[threadIdx.x] = s;
  __syncthreads();
  if (sg == 0 && e < total) {
    s = (((sh[ex] + sh[32 + ex]) + (sh[64 + ex] + sh[96 + ex])) + ((sh[128 + ex] + sh[160 + ex]) + (sh[192 + ex] + sh[224 + ex])));
    if (e < nw) {
      int co = e % NT16;
      int ci = (e / NT16) % CT16;
      int tap = e / (NT16 * CT16);
      if (co < Cout && ci < Cin) {
        size_t o = ((size_t)co * Cin + ci) * ntap + tap;
        grad[o] = accumulate ? grad[o] + s : s;
      }
    } else if (grad_b) {
      int co = e - nw;
      if (co < Cout) grad_b[co] = accumulate ? grad_b[co] + s : s;
    }
  }
}

// One launch for ALL layers of a backward pass: segment s = blockIdx.y sums the slabs that every weight-gradient call of one layer
// appended to that layer's slab region (the three Denoise invocations, the three shared Enhancer blocks) and writes the layer's
// grad_w / grad_b.  Same per-element arithmetic as wgrad_reduce_kernel (fixed order: bit-reproducible); replaces 23 launches of
// ~9 us each per training step.
constexpr int ZT_MAXSEG = 16;
struct ReduceTable {
  const float* slab[ZT_MAXSEG];
  float* gw[ZT_MAXSEG];
  float* gb[ZT_MAXSEG];
  int nslab[ZT_MAXSEG], ntap[ZT_MAXSEG], CT16[ZT_MAXSEG], NT16[ZT_MAXSEG], Cout[ZT_MAXSEG], Cin[ZT_MAXSEG];
  int accumulate;
};

__global__ void __launch_bounds__(256) wgrad_reduce_multi_kernel(ReduceTable t) {
  __shared__ float sh[256];
  const int sgm = blockIdx.y;
  const float* __restrict__ slab = t.slab[sgm];
  const int nslab = t.nslab[sgm], ntap = t.ntap[sgm], CT16 = t.CT16[sgm], NT16 = t.NT16[sgm], Cout = t.Cout[sgm], Cin = t.Cin[sgm];
  const int ex = threadIdx.x & 31, sg = threadIdx.x >> 5;
  const int e = blockIdx.x * 32 + ex;
  const int nw = ntap * CT16 * NT16;
  const int total = nw + NT16;
  if (blockIdx.x * 32 >= total) return;                         // uniform: this segment is shorter than the longest one
  float s = 0.f;
  if (e < total) {
    const size_t stride = (size_t)total;
    for (int k = sg; k < nslab; k += 64) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (k + 8 * j < nslab) ? slab[(size_t)(k + 8 * j) * stride + e] : 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) s += v[j];
    }
  }
  sh[threadIdx.x] = s;
  __syncthreads();
  if (sg == 0 && e < total) {
    s = (((sh[ex] + sh[32 + ex]) + (sh[64 + ex] + sh[96 + ex])) + ((sh[128 + ex] + sh[160 + ex]) + (sh[192 + ex] + sh[224 + ex])));
    if (e < nw) {
      const int co = e % NT16, ci = (e / NT16) % CT16, tap = e / (NT16 * CT16);
      if (co < Cout && ci < Cin) {
        const size_t o = ((size_t)co * Cin + ci) * ntap + tap;
        t.gw[sgm][o] = t.accumulate ? t.gw[sgm][o] + s : s;
      }
    } else if (t.gb[sgm]) {
      const int co = e - nw;
      if (co < Cout) t.gb[sgm][co] = t.accumulate ? t.gb[sgm][co] + s : s;
    }
  }
}

// ---- bf16 weight gradient.  K = pixels: the MFMA needs 8 consecutive PIXELS per lane for one channel, i.e. the
// transpose of the NHWC tile; ds_read_b64_tr_b16 delivers exactly that from a [pixel][channel] LDS image, so staging is a
// plain 16-byte copy and tap shifts are row shifts (alignment preserved).
struct WgradArgsH {
  const zt_bf16* x;
  const zt_bf16* dz;
  float* slab;
  int H, W, Cin, ldx, Cout, lddz;
  int tilesX, ntiles;
  const zt_bf16* mask;         // MASK: dz is taken as dz * [mask > 0] (the ReLU that follows the layer, folded in)
  int ldmask;
};

constexpr int HTW = 32;                 // tile = HTH rows x 32 pixels; HTH = 2 * NW (4 or 8): 8-wave workgroups keep twice the bytes in flight

// NW waves per workgroup share the (tap, ci-tile) pairs; 8 for the 64x64 layer so that accumulators + staging registers stay <= 128
template <int KH, int KW, int CT, int NT, int NW, bool MASK = false>
__global__ void __launch_bounds__(NW * 64, 1) wgrad_mfma_bf16_kernel(WgradArgsH a) {
  constexpr int NTHR = NW * 64, HTH = NW;
  constexpr int IR = HTH + KH - 1, IC = HTW + KW - 1;
  constexpr int CIP = CT * 16 + 8, COP = NT * 16 + 8;
  constexpr int NPAIR = KH * KW * CT;
  constexpr int PPW = (NPAIR + NW - 1) / NW;
  constexpr int padH = (KH - 1) / 2, padW = (KW - 1) / 2;
  __shared__ __attribute__((aligned(16))) zt_bf16 xs[IR * IC * CIP];
  __shared__ __attribute__((aligned(16))) zt_bf16 zs[HTH * HTW * COP];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, g8 = (lane >> 4) * 8;
  const int trq = l15 >> 2, trp = (l15 & 3) * 4;       // this lane's row / column quad inside a transposing 4x16 block

  zt_f32x4 acc[PPW][NT];
#pragma unroll
  for (int p = 0; p < PPW; ++p)
#pragma unroll
    for (int q = 0; q < NT; ++q) acc[p][q] = (zt_f32x4){0.f, 0.f, 0.f, 0.f};
  constexpr int NPART = NTHR / (NT * 16);
  const int bco = tid % (NT * 16), bpart = tid / (NT * 16);
  float bsum = 0.f;

  // global -> registers -> LDS staging, software-pipelined: the next tile's loads are issued before this tile's MFMAs and land
  // while they run.  Loads are unconditional (clamped addresses); image borders and channel tails are masked when written.
  constexpr int NXL = (IR * IC * CT * 2 + NTHR - 1) / NTHR, NZL = (HTH * HTW * NT * 2 + NTHR - 1) / NTHR;
  uint4 px[NXL], pz[NZL], pm[MASK ? NZL : 1];
  auto relu_keep = [](unsigned g, unsigned m) {                  // two packed bf16: keep g where the activation m is > 0
    const unsigned lo = ((m & 0x8000u) == 0u && (m & 0x7FFFu) != 0u) ? 0xFFFFu : 0u;
    const unsigned hi = ((m & 0x80000000u) == 0u && (m & 0x7FFF0000u) != 0u) ? 0xFFFF0000u : 0u;
    return g & (lo | hi);
  };
  auto chan_mask = [](uint4 v, int nv, bool in) {               // keep the first nv (of 8) bf16 lanes
    const unsigned m0 = nv >= 2 ? ~0u : (nv == 1 ? 0xFFFFu : 0u), m1 = nv >= 4 ? ~0u : (nv == 3 ? 0xFFFFu : 0u);
    const unsigned m2 = nv >= 6 ? ~0u : (nv == 5 ? 0xFFFFu : 0u), m3 = nv >= 8 ? ~0u : (nv == 7 ? 0xFFFFu : 0u);
    v.x = in ? (v.x & m0) : 0u;
    v.y = in ? (v.y & m1) : 0u;
    v.z = in ? (v.z & m2) : 0u;
    v.w = in ? (v.w & m3) : 0u;
    return v;
  };
  // Interior tiles (halo inside the image, full channel octets: ~95 % of the tiles at 1080p) take a uniform fast path without the
  // per-slot clamps, bounds tests and channel masks (no extra registers: the slot's pixel / channel decomposition is recomputed).
  // (thin-input variants, CT == 1, measured 10-20 % slower with the extra path: they keep the general one)
  constexpr bool FASTP = CT >= 3;
  const bool x_plain = FASTP && a.Cin == CT * 16 && a.ldx >= CT * 16, z_plain = FASTP && a.Cout == NT * 16 && a.lddz >= NT * 16 && (!MASK || a.ldmask >= NT * 16);
  auto tile_interior = [&](int oy0, int ox0) {
    return FASTP && oy0 - padH >= 0 && oy0 - padH + IR <= a.H && ox0 - padW >= 0 && ox0 - padW + IC <= a.W && oy0 + HTH <= a.H && ox0 + HTW <= a.W;
  };
  auto load_tile = [&](int tile) {
    const int oy0 = (tile / a.tilesX) * HTH, ox0 = (tile % a.tilesX) * HTW;
    const bool fast = tile_interior(oy0, ox0);                  // uniform
    if (fast && x_plain) {
      const zt_bf16* xb = a.x + (unsigned)(((oy0 - padH) * a.W + ox0 - padW) * a.ldx);
#pragma unroll
      for (int i = 0; i < NXL; ++i) {
        int e = tid + i * NTHR;
        e = e < IR * IC * CT * 2 ? e : 0;                       // slots beyond the tile re-read slot 0 (never written)
        const int c8 = e % (CT * 2), p = e / (CT * 2);
        px[i] = *reinterpret_cast<const uint4*>(xb + (unsigned)(((p / IC) * a.W + p % IC) * a.ldx + c8 * 8));
      }
    } else {
#pragma unroll
      for (int i = 0; i < NXL; ++i) {
        const int e = tid + i * NTHR;
        const int c8 = e % (CT * 2), p = e / (CT * 2);
        int gy = oy0 - padH + p / IC, gx = ox0 - padW + p % IC;
        gy = gy < 0 ? 0 : (gy >= a.H ? a.H - 1 : gy);
        gx = gx < 0 ? 0 : (gx >= a.W ? a.W - 1 : gx);
        const int c = c8 * 8 + 8 <= a.ldx ? c8 * 8 : 0;
        px[i] = *reinterpret_cast<const uint4*>(a.x + (unsigned)((gy * a.W + gx) * a.ldx + c));
      }
    }
    if (fast && z_plain) {
      const unsigned zo = (unsigned)((oy0 * a.W + ox0) * a.lddz), mo = MASK ? (unsigned)((oy0 * a.W + ox0) * a.ldmask) : 0u;
#pragma unroll
      for (int i = 0; i < NZL; ++i) {
        int e = tid + i * NTHR;
        e = e < HTH * HTW * NT * 2 ? e : 0;
        const int c8 = e % (NT * 2), p = e / (NT * 2);
        const int rel = (p / HTW) * a.W + p % HTW;
        pz[i] = *reinterpret_cast<const uint4*>(a.dz + zo + (unsigned)(rel * a.lddz + c8 * 8));
        if constexpr (MASK) pm[i] = *reinterpret_cast<const uint4*>(a.mask + mo + (unsigned)(rel * a.ldmask + c8 * 8));
      }
    } else {
#pragma unroll
      for (int i = 0; i < NZL; ++i) {
        const int e = tid + i * NTHR;
        const int c8 = e % (NT * 2), p = e / (NT * 2);
        int gy = oy0 + p / HTW, gx = ox0 + p % HTW;
        gy = gy >= a.H ? a.H - 1 : gy;
        gx = gx >= a.W ? a.W - 1 : gx;
        const int c = c8 * 8 + 8 <= a.lddz ? c8 * 8 : 0;
        pz[i] = *reinterpret_cast<const uint4*>(a.dz + (unsigned)((gy * a.W + gx) * a.lddz + c));
        if constexpr (MASK) {
          const int cm = c8 * 8 + 8 <= a.ldmask ? c8 * 8 : 0;
          pm[i] = *reinterpret_cast<const uint4*>(a.mask + (unsigned)((gy * a.W + gx) * a.ldmask + cm));
        }
      }
    }
  };
  auto write_tile = [&](int tile) {
    const int oy0 = (tile / a.tilesX) * HTH, ox0 = (tile % a.tilesX) * HTW;
    const bool fast = tile_interior(oy0, ox0);                  // uniform
#pragma unroll
    for (int i = 0; i < NXL; ++i) {
      const int e = tid + i * NTHR;
      const int c8 = e % (CT * 2), p = e / (CT * 2);
      if (fast && x_plain) {
        if (e < IR * IC * CT * 2) *reinterpret_cast<uint4*>(xs + p * CIP + c8 * 8) = px[i];
      } else {
        const int gy = oy0 - padH + p / IC, gx = ox0 - padW + p % IC;
        const bool in = gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
        if (e < IR * IC * CT * 2) *reinterpret_cast<uint4*>(xs + p * CIP + c8 * 8) = chan_mask(px[i], a.Cin - c8 * 8, in);
      }
    }
#pragma unroll
    for (int i = 0; i < NZL; ++i) {
      const int e = tid + i * NTHR;
      const int c8 = e % (NT * 2), p = e / (NT * 2);
      uint4 g = pz[i];
      if constexpr (MASK) {
        g.x = relu_keep(g.x, pm[i].x);
        g.y = relu_keep(g.y, pm[i].y);
        g.z = relu_keep(g.z, pm[i].z);
        g.w = relu_keep(g.w, pm[i].w);
      }
      if (fast && z_plain) {
        if (e < HTH * HTW * NT * 2) *reinterpret_cast<uint4*>(zs + p * COP + c8 * 8) = g;
      } else {
        const int gy = oy0 + p / HTW, gx = ox0 + p % HTW;
        const bool in = gy < a.H && gx < a.W;
        if (e < HTH * HTW * NT * 2) *reinterpret_cast<uint4*>(zs + p * COP + c8 * 8) = chan_mask(g, a.Cout - c8 * 8, in);
      }
    }
  };

  if ((int)blockIdx.x < a.ntiles) load_tile(blockIdx.x);
  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    __syncthreads();
    write_tile(tile);
    __syncthreads();
    if (tile + (int)gridDim.x < a.ntiles) load_tile(tile + gridDim.x);
    if (bpart < NPART)
      for (int p = bpart; p < HTH * HTW; p += NPART) bsum += zt_bf2f(zs[p * COP + bco]);
    // per-wave (tap, ci-tile) pairs: branch-free (a wave without a pair in the last round recomputes the final pair into an
    // accumulator that is never written out), A fragments double-buffered and pinned ahead of the previous pair's MFMAs
    int aoff[PPW];
#pragma unroll
    for (int pi = 0; pi < PPW; ++pi) {
      int pr = wave + NW * pi;
      pr = pr < NPAIR ? pr : NPAIR - 1;
      const int tap = pr / CT, cit = pr - tap * CT;
      const int ky = tap / KW, kx = tap - ky * KW;
      aoff[pi] = (ky * IC + kx + g8 + trq) * CIP + cit * 16 + trp;
    }
    // Rows in blocks of four, fully unrolled inside a block: one flat software pipeline over the 4 * PPW (row, pair) steps.  The
    // A fragments (transposed x reads) run LA = 3 steps ahead of the MFMAs that consume them and the B fragments (dz) of a row
    // are requested one row earlier, across the row and block boundaries (indices clamped at the tile's end): with one step of
    // look-ahead inside a row and the B reads at the head of every row the 128+ clocks of LDS latency were exposed five-plus
    // times per row.
    constexpr int RB = 4, NS = RB * PPW, AD = 4, LA = 3;
    static_assert(HTH % RB == 0 && NS % AD == 0, "block geometry");
    zt_s16x4 alo[AD], ahi[AD];
    zt_s16x8 bv[2][NT];
    auto load_a = [&](auto bc, int row, auto pc) {
      constexpr int bi = decltype(bc)::value, pi = decltype(pc)::value;
      const zt_bf16* xr = xs + (row < HTH ? row : HTH - 1) * IC * CIP;
      alo[bi] = zt_lds_read_tr16(xr + aoff[pi]);
      ahi[bi] = zt_lds_read_tr16(xr + aoff[pi] + 4 * CIP);
    };
    auto load_b = [&](auto bc, int row) {
      constexpr int bi = decltype(bc)::value;
      const int rr = row < HTH ? row : HTH - 1;
#pragma unroll
      for (int q = 0; q < NT; ++q) {
        zt_s16x4 lo = zt_lds_read_tr16(zs + (rr * HTW + g8 + trq) * COP + q * 16 + trp);
        zt_s16x4 hi = zt_lds_read_tr16(zs + (rr * HTW + g8 + 4 + trq) * COP + q * 16 + trp);
        bv[bi][q] = (zt_s16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      }
    };
    load_b(ZtIdx<0>{}, 0);
    zt_static_for<0, LA>([&](auto sc) {
      constexpr int st = decltype(sc)::value;
      load_a(ZtIdx<st % AD>{}, st / PPW, ZtIdx<st % PPW>{});
    });
#pragma unroll 1
    for (int r0 = 0; r0 < HTH; r0 += RB) {
      zt_static_for<0, NS>([&](auto sc) {
        constexpr int st = decltype(sc)::value;
        constexpr int rl = st / PPW, pi = st % PPW, cur = st % AD;
        if constexpr (pi == 0) load_b(ZtIdx<(rl + 1) & 1>{}, r0 + rl + 1);          // next row's dz fragments (RB is even)
        {
          constexpr int nx = st + LA;                                                 // may run into the next block: row r0 + RB + ..
          load_a(ZtIdx<nx % AD>{}, r0 + nx / PPW, ZtIdx<nx % PPW>{});
        }
        __builtin_amdgcn_sched_barrier(0);
        zt_s16x8 av = (zt_s16x8){alo[cur][0], alo[cur][1], alo[cur][2], alo[cur][3], ahi[cur][0], ahi[cur][1], ahi[cur][2], ahi[cur][3]};
#pragma unroll
        for (int q = 0; q < NT; ++q) acc[pi][q] = zt_mfma_bf16(av, bv[rl & 1][q], acc[pi][q]);
        __builtin_amdgcn_sched_barrier(0);
      });
    }
  }
  float* out = a.slab + (size_t)blockIdx.x * (KH * KW * CT * 16 * NT * 16 + NT * 16);
  const int l4 = lane >> 4;
#pragma unroll
  for (int pi = 0; pi < PPW; ++pi) {
    const int pr = wave + NW * pi;
    if (pr < NPAIR) {
      const int tap = pr / CT, cit = pr - tap * CT;
#pragma unroll
      for (int q = 0; q < NT; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          out[((size_t)tap * CT * 16 + cit * 16 + l4 * 4 + j) * (NT * 16) + q * 16 + l15] = acc[pi][q][j];
    }
  }
  __syncthreads();
  float* fz = reinterpret_cast<float*>(zs);                 // HTH*HTW*COP bf16 >= NPART*NT16 floats
  if (bpart < NPART) fz[bpart * (NT * 16) + bco] = bsum;
  __syncthreads();
  if (tid < NT * 16) {
    float sum = 0.f;
    for (int k = 0; k < NPART; ++k) sum += fz[k * (NT * 16) + tid];
    out[KH * KW * CT * 16 * NT * 16 + tid] = sum;
  }
}

// ---- 64 -> 64 3x3 weight gradient (Enhancer conv.0: 3 launches per step), LDS-DMA form.
// Same MFMA decomposition as wgrad_mfma_bf16_kernel<3,3,4,4,8> (8 waves share the 36 (tap, ci-tile) pairs of an 8-row x 32-pixel
// tile; K = pixels through ds_read_b64_tr_b16), but
//  * both operand tiles go global -> LDS by DMA (`global_load_lds_dwordx4`): no staging registers, no ds_write pass, nothing of the
//    staging in any wave's instruction stream except the ~10 DMA issues per wave and tile;
//  * TWO tile buffers (2 x (10 x 34 + 8 x 32) pixels x 128 B = 149 KB): tile k+1 lands while tile k's MFMA loop runs, ONE barrier
//    per tile;
//  * pixel rows are exactly 128 B (a DMA destination is lane-linear, so rows cannot be padded) and XOR-swizzled at 32-byte (ci-tile)
//    granularity by s(col) = bit1(col) | bit3(col) << 1 -- applied to the SOURCE address of the DMA and to the read address.  A
//    transposing read's 32-lane half covers pixels {c..c+3, c+8..c+11} x 32 B: unswizzled these are 4-way bank conflicts on 128-B
//    rows (and 41 % of the LDS cycles on the former 144-byte-pitch image); with the swizzle every read is conflict-free (brute force
//    over all kx / ci-tile / row / half: DESIGN section 5);
//  * the bias gradient (column sums of dz) is an MFMA with an all-ones A fragment in the pair slot that wave 4 had idle (36 pairs
//    over 8 waves) instead of 32 two-byte LDS reads + adds per thread and tile;
//  * XCD-aware banded tile order as in conv_rs, so a tile's halo rows / columns are in its XCD's L2.
// Requires Cin == Cout == 64 and channel strides >= 64 (multiples of 8).
// CH = 48 (Denoise_1/2 conv2, six launches per step; round 3): the same kernel on 96-byte pixel rows.  A lane-linear DMA image cannot
// be padded and 6 chunks per pixel cannot be XOR-swizzled, so the transposing reads keep a 2-way conflict ({c..c+3} against
// {c+8..c+11}: every pitch from 96 to 208 bytes gives 2-way, brute force) -- the loop is VALU / MFMA bound, not LDS bound.  27 pairs
// over 8 waves: 4 slots per wave, the bias sums in wave 3's spare one.
constexpr int WG64_IR = 10, WG64_IC = 34;

template <int CH>
__device__ __forceinline__ int wg64_swz(int col) { return CH == 64 ? (((col >> 1) & 1) | (((col >> 3) & 1) << 1)) : 0; }

// CHX != CHZ (round 3): the thin-input first layers of Denoise_1/2 (Cin 3 / 12 in 8- / 16-channel pixels -> 48): one ci-tile, 9 pairs;
// the x image has 16- or 32-byte pixels (a transposing read of an 8-channel pixel takes its upper 8 "channels" from the next pixel:
// rows >= Cin of the product, which the slab reduction ignores, like the buffer's padding lanes).  Purely DMA / HBM bound.
template <int CHX, int CHZ>
__global__ void __launch_bounds__(512, 1) wgrad64_dma_bf16_kernel(WgradArgsH a) {
  static_assert((CHX == 64 && CHZ == 64) || (CHX == 48 && CHZ == 48) || ((CHX == 8 || CHX == 16) && CHZ == 48), "built shapes");
  constexpr int NW = 8, NTHR = 512, HTH = 8, IR = WG64_IR, IC = WG64_IC, CT = CHX >= 16 ? CHX / 16 : 1, NT = CHZ / 16;
  constexpr int CKX = CHX / 8, CKZ = CHZ / 8;
  constexpr int NPAIR = 9 * CT, PPW = (NPAIR + NW - 1) / NW;
  constexpr int WG64_XE = (IR * IC * CHX + 16 + 511) / 512 * 512, WG64_ZE = HTH * HTW * CHZ;       // x image + 32 B of slack, whole 1-KB pieces
  constexpr int NGX = (IR * IC * CKX + NTHR - 1) / NTHR, NGZ = (HTH * HTW * CKZ + NTHR - 1) / NTHR;    // DMA wave-instructions per wave and tile
  static_assert(HTH * HTW * CKZ % 64 == 0, "dz image = whole wave-instructions");
  __shared__ __attribute__((aligned(16))) zt_bf16 smem[2 * (WG64_XE + WG64_ZE)];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, g8 = (lane >> 4) * 8;
  const int trq = l15 >> 2, trp = (l15 & 3) * 4;

  // XCD-aware tile order (see conv_rs): workgroup b runs on XCD b % 8; an XCD's run of tiles walks bands of 4 tile rows column-major
  const int G = gridDim.x;
  const int pb = (G % 8 == 0) ? ((int)blockIdx.x % 8) * (G / 8) + (int)blockIdx.x / 8 : (int)blockIdx.x;
  const int tilesY = a.ntiles / a.tilesX;
  auto tile_xy = [&](int idx, int& ty, int& tx) {
    const int band = idx / (4 * a.tilesX), r = idx - band * 4 * a.tilesX;
    const int rows = tilesY - band * 4 < 4 ? tilesY - band * 4 : 4;
    tx = r / rows;
    ty = band * 4 + r - tx * rows;
  };

  // DMA slot e = 64 (8 i + wave) + lane -> pixel e >> 3 of the tile image (row-major), PHYSICAL 16-byte chunk e & 7, which receives
  // the logical chunk (e & 7) ^ (s(col) << 1): the swizzle sits on the source address (a DMA destination is lane-linear).  The
  // slot's source offset relative to the tile origin is tile-invariant: computed once (interior tiles: one 64-bit add per DMA;
  // the inner loop is VALU-issue bound -- 2.9 VALU per MFMA in the first build of this kernel -- so per-tile index arithmetic counts)
  int xoff[NGX], zoff[NGZ];
#pragma unroll
  for (int i = 0; i < NGX; ++i) {
    const int e = (i * NW + wave) * 64 + lane;
    const int p = e / CKX, row = p / IC, col = p - row * IC;
    xoff[i] = (row * a.W + col) * a.ldx + (((e - p * CKX) ^ (wg64_swz<CHX>(col) << 1)) * 8);
  }
#pragma unroll
  for (int i = 0; i < NGZ; ++i) {
    const int e = (i * NW + wave) * 64 + lane;
    const int p = e / CKZ, row = p / HTW, col = p - row * HTW;
    zoff[i] = (row * a.W + col) * a.lddz + (((e - p * CKZ) ^ (wg64_swz<CHZ>(col) << 1)) * 8);
  }
  auto dma_tile = [&](int idx, int buf) {
    int ty, tx;
    tile_xy(idx, ty, tx);
    const int oy0 = ty * HTH, ox0 = tx * HTW;
    zt_bf16* xb = smem + buf * (WG64_XE + WG64_ZE);
    zt_bf16* zb = xb + WG64_XE;
    if (oy0 - 1 >= 0 && oy0 - 1 + IR <= a.H && ox0 - 1 >= 0 && ox0 - 1 + IC <= a.W) {      // uniform: interior tile (~95 % at 1080p)
      const zt_bf16* xo = a.x + (unsigned)(((oy0 - 1) * a.W + ox0 - 1) * a.ldx);
      const zt_bf16* zo = a.dz + (unsigned)((oy0 * a.W + ox0) * a.lddz);
#pragma unroll
      for (int i = 0; i < NGX; ++i)
        if ((i * NW + NW) * 64 <= IR * IC * CKX || (i * NW + wave) * 64 + lane < IR * IC * CKX) ZT_GLDS16_HIDDEN(xo + xoff[i], xb + (i * NW + wave) * 512);
#pragma unroll
      for (int i = 0; i < NGZ; ++i)
        if ((i * NW + NW) * 64 <= HTH * HTW * CKZ || (i * NW + wave) * 64 < HTH * HTW * CKZ) ZT_GLDS16_HIDDEN(zo + zoff[i], zb + (i * NW + wave) * 512);
      return;
    }
    int ln = lane;
    ZT_OPAQUE(ln);                                              // border tiles: slot geometry recomputed, out-of-image pixels read zeros
#pragma unroll
    for (int i = 0; i < NGX; ++i) {
      const int e = (i * NW + wave) * 64 + ln;
      const int p = e / CKX, row = p / IC, col = p - row * IC;
      const int cj = (e - p * CKX) ^ (wg64_swz<CHX>(col) << 1);
      const int gy = oy0 - 1 + row, gx = ox0 - 1 + col;
      const bool in = gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
      const int gyc = gy < 0 ? 0 : (gy >= a.H ? a.H - 1 : gy), gxc = gx < 0 ? 0 : (gx >= a.W ? a.W - 1 : gx);
      const void* src = in ? (const void*)(a.x + (unsigned)((gyc * a.W + gxc) * a.ldx + cj * 8)) : (const void*)&zt_zero_chunk;
      if ((i * NW + NW) * 64 <= IR * IC * CKX || e < IR * IC * CKX) ZT_GLDS16_HIDDEN(src, xb + (i * NW + wave) * 512);
    }
#pragma unroll
    for (int i = 0; i < NGZ; ++i) {
      const int e = (i * NW + wave) * 64 + ln;
      const int p = e / CKZ, row = p / HTW, col = p - row * HTW;
      const int cj = (e - p * CKZ) ^ (wg64_swz<CHZ>(col) << 1);
      const int gy = oy0 + row, gx = ox0 + col;
      const bool in = gy < a.H && gx < a.W;
      const int gyc = gy >= a.H ? a.H - 1 : gy, gxc = gx >= a.W ? a.W - 1 : gx;
      const void* src = in ? (const void*)(a.dz + (unsigned)((gyc * a.W + gxc) * a.lddz + cj * 8)) : (const void*)&zt_zero_chunk;
      if ((i * NW + NW) * 64 <= HTH * HTW * CKZ || (i * NW + wave) * 64 < HTH * HTW * CKZ) ZT_GLDS16_HIDDEN(src, zb + (i * NW + wave) * 512);
    }
  };

  zt_f32x4 acc[PPW][NT];
#pragma unroll
  for (int p = 0; p < PPW; ++p)
#pragma unroll
    for (int q = 0; q < NT; ++q) acc[p][q] = (zt_f32x4){0.f, 0.f, 0.f, 0.f};

  // per-lane fragment offsets (elements) inside a tile buffer: pair slot pi -> (tap, ci-tile); pairs 36..39 do not exist: wave 4's
  // spare slot carries the bias sums (A = ones), the spare slots of waves 5..7 recompute pair 35 into a discarded accumulator
  int alo[PPW], ahi[PPW];
#pragma unroll
  for (int pi = 0; pi < PPW; ++pi) {
    int pr = wave + NW * pi;
    pr = pr < NPAIR ? pr : NPAIR - 1;
    const int tap = pr / CT, cit = pr - tap * CT;
    const int ky = tap / 3, kx = tap - ky * 3;
    const int c0 = kx + g8 + trq, c1 = c0 + 4;
    alo[pi] = (ky * IC + c0) * CHX + ((cit ^ wg64_swz<CHX>(c0)) * 16) + trp;
    ahi[pi] = (ky * IC + c1) * CHX + ((cit ^ wg64_swz<CHX>(c1)) * 16) + trp;
  }
  int blo[NT], bhi[NT];
  {
    const int c0 = g8 + trq, c1 = c0 + 4;
#pragma unroll
    for (int q = 0; q < NT; ++q) {
      blo[q] = WG64_XE + c0 * CHZ + ((q ^ wg64_swz<CHZ>(c0)) * 16) + trp;
      bhi[q] = WG64_XE + c1 * CHZ + ((q ^ wg64_swz<CHZ>(c1)) * 16) + trp;
    }
  }
  const bool ones_slot = wave == NPAIR % NW;                     // uniform: the first wave whose last pair slot is spare = bias column sums
  const zt_s16x8 ones = {0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};     // bf16 1.0

  const int n_my = pb < a.ntiles ? (a.ntiles - 1 - pb) / G + 1 : 0;
  if (n_my > 0) dma_tile(pb, 0);
  for (int k = 0; k < n_my; ++k) {
    ZT_WAIT_HIDDEN_DMA();             // this wave's pieces of tile k have landed ...
    __syncthreads();                  // ... and so have everyone else's; every wave has left tile k-1's loop (its buffer is free)
    // (a stagger -- waves 4..7 issuing their DMAs a quarter of the MFMA loop later, under their SIMD partner's MFMAs -- measured
    // no gain: 144.1 vs 143.9 us, profiles/r03_wgrad64_*; all eight issue at the head of the tile)
    if (k + 1 < n_my) dma_tile(pb + (k + 1) * G, (k + 1) & 1);
    // this tile's per-lane read addresses, once: everything below them is a compile-time row offset (ds_read immediate)
    const zt_bf16* tb = smem + (k & 1) * (WG64_XE + WG64_ZE);
    const zt_bf16 *pal[PPW], *pah[PPW], *pbl[NT], *pbh[NT];
#pragma unroll
    for (int pi = 0; pi < PPW; ++pi) {
      pal[pi] = tb + alo[pi];
      pah[pi] = tb + ahi[pi];
    }
#pragma unroll
    for (int q = 0; q < NT; ++q) {
      pbl[q] = tb + blo[q];
      pbh[q] = tb + bhi[q];
    }
    // ONE flat, fully unrolled software pipeline over the 8 rows x 5 pair slots: A fragments LA steps ahead of the MFMAs that
    // consume them, a row's B fragments one row ahead; steps past the tile's end re-read the last row (results unused)
    constexpr int NS = HTH * PPW, AD = 4, LA = 3;
    zt_s16x4 fal[AD], fah[AD];
    zt_s16x8 bv[2][NT];
    auto load_a = [&](auto bc, auto rc, auto pc) {
      constexpr int bi = decltype(bc)::value, pi = decltype(pc)::value;
      constexpr int row = decltype(rc)::value < HTH ? decltype(rc)::value : HTH - 1;
      fal[bi] = zt_lds_read_tr16(pal[pi] + row * IC * CHX);
      fah[bi] = zt_lds_read_tr16(pah[pi] + row * IC * CHX);
    };
    auto load_b = [&](auto bc, auto rc) {
      constexpr int bi = decltype(bc)::value;
      constexpr int row = decltype(rc)::value < HTH ? decltype(rc)::value : HTH - 1;
#pragma unroll
      for (int q = 0; q < NT; ++q) {
        const zt_s16x4 lo = zt_lds_read_tr16(pbl[q] + row * HTW * CHZ);
        const zt_s16x4 hi = zt_lds_read_tr16(pbh[q] + row * HTW * CHZ);
        bv[bi][q] = (zt_s16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      }
    };
    load_b(ZtIdx<0>{}, ZtIdx<0>{});
    zt_static_for<0, LA>([&](auto sc) {
      constexpr int st = decltype(sc)::value;
      load_a(ZtIdx<st % AD>{}, ZtIdx<st / PPW>{}, ZtIdx<st % PPW>{});
    });
    zt_static_for<0, NS>([&](auto sc) {
      constexpr int st = decltype(sc)::value;
      constexpr int row = st / PPW, pi = st % PPW, cur = st % AD;
      if constexpr (pi == 0) load_b(ZtIdx<(row + 1) & 1>{}, ZtIdx<row + 1>{});
      {
        constexpr int nx = st + LA;
        load_a(ZtIdx<nx % AD>{}, ZtIdx<nx / PPW>{}, ZtIdx<nx % PPW>{});
      }
      __builtin_amdgcn_sched_barrier(0);
      zt_s16x8 av = (zt_s16x8){fal[cur][0], fal[cur][1], fal[cur][2], fal[cur][3], fah[cur][0], fah[cur][1], fah[cur][2], fah[cur][3]};
      if constexpr (pi == PPW - 1) av = ones_slot ? ones : av;
#pragma unroll
      for (int q = 0; q < NT; ++q) acc[pi][q] = zt_mfma_bf16(av, bv[row & 1][q], acc[pi][q]);
      __builtin_amdgcn_sched_barrier(0);
    });
  }
  // slab of this workgroup: [tap][ci CT*16][co CHZ] + [co CHZ] (same layout as wgrad_mfma_bf16_kernel)
  float* out = a.slab + (size_t)blockIdx.x * (9 * CT * 16 * CHZ + CHZ);
  const int l4 = lane >> 4;
#pragma unroll
  for (int pi = 0; pi < PPW; ++pi) {
    const int pr = wave + NW * pi;
    if (pr < NPAIR) {
      const int tap = pr / CT, cit = pr - tap * CT;
#pragma unroll
      for (int q = 0; q < NT; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) out[((size_t)tap * CT * 16 + cit * 16 + l4 * 4 + j) * CHZ + q * 16 + l15] = acc[pi][q][j];
    }
  }
  if (ones_slot && l4 == 0) {          // every row of the ones product holds the column sums: row 0 (lanes 0..15, register 0)
#pragma unroll
    for (int q = 0; q < NT; ++q) out[9 * CT * 16 * CHZ + q * 16 + l15] = acc[PPW - 1][q][0];
  }
}

// ZT_WGRAD_DMA=0 selects the register-staged kernels where an LDS-DMA form exists (A/B: tests, tools/bench_wgrad.py).  Read on
// every call: the tests switch it inside one process.
static bool wgrad_dma_enabled() {
  const char* e = getenv("ZT_WGRAD_DMA");
  return !e || atoi(e) != 0;
}

// the 48 -> 48 3x3 layers take the DMA form too
static bool wgrad48_dma(int K, int Cin, int Cout, int ldx, int lddz) {
  return wgrad_dma_enabled() && K == 3 && Cin == 48 && Cout == 48 && ldx >= 48 && lddz >= 48 && ldx % 8 == 0 && lddz % 8 == 0;
}

// ... and the thin-input 3x3 layers with 48 couts whose pixels are exactly 8 or 16 channels wide (Denoise_1/2 conv1)
static bool wgrad_thin48_dma(int K, int Cin, int Cout, int ldx, int lddz, const void* mask) {
  return wgrad_dma_enabled() && !mask && K == 3 && Cout == 48 && (ldx == 8 || ldx == 16) && Cin <= ldx && lddz >= 48 && lddz % 8 == 0;
}

template <int KH, int KW>
int launch_wgrad_h(const WgradArgsH& a, int CT, int NT, int nblk, hipStream_t stream) {
  dim3 grid(nblk);
#define ZT_WG(ct, nt, nw) hipLaunchKernelGGL((wgrad_mfma_bf16_kernel<KH, KW, ct, nt, nw>), grid, dim3(nw * 64), 0, stream, a); return 0
  if (CT == 1 && NT == 3) {
    if (wgrad_thin48_dma(KH, a.Cin, a.Cout, a.ldx, a.lddz, a.mask)) {
      if (a.ldx == 8) hipLaunchKernelGGL((wgrad64_dma_bf16_kernel<8, 48>), grid, dim3(512), 0, stream, a);
      else hipLaunchKernelGGL((wgrad64_dma_bf16_kernel<16, 48>), grid, dim3(512), 0, stream, a);
      return 0;
    }
    ZT_WG(1, 3, 4);
  }
  if (CT == 1 && NT == 4) {
    if (a.mask) {
      hipLaunchKernelGGL((wgrad_mfma_bf16_kernel<KH, KW, 1, 4, 4, true>), grid, dim3(256), 0, stream, a);
      return 0;
    }
    ZT_WG(1, 4, 4);
  }
  if (a.mask) return ZT_EINVAL;                                  // the folded ReLU mask exists for the thin-input 64-cout layer only
  if (CT == 3 && NT == 3) {
    if (wgrad48_dma(KH, a.Cin, a.Cout, a.ldx, a.lddz)) {          // 8-row tiles, one workgroup per CU (ntiles / nblk sized for it by the caller)
      hipLaunchKernelGGL((wgrad64_dma_bf16_kernel<48, 48>), grid, dim3(512), 0, stream, a);
      return 0;
    }
    ZT_WG(3, 3, 4);
  }
  if (CT == 3 && NT == 1) { ZT_WG(3, 1, 4); }
  if (CT == 4 && NT == 4) {
    if (wgrad_dma_enabled() && KH == 3 && KW == 3 && a.Cin == 64 && a.Cout == 64 && a.ldx >= 64 && a.lddz >= 64 && a.ldx % 8 == 0 && a.lddz % 8 == 0 &&
        a.ntiles % a.tilesX == 0) {
      hipLaunchKernelGGL((wgrad64_dma_bf16_kernel<64, 64>), grid, dim3(512), 0, stream, a);
      return 0;
    }
    ZT_WG(4, 4, 8);
  }
  if (CT == 4 && NT == 1) { ZT_WG(4, 1, 4); }
#undef ZT_WG
  return ZT_EINVAL;
}

}  // namespace

int zt_launch_wgrad_reduce(const float* slab, int nslab, int ntap, int CT16, int NT16, float* grad_w, int Cout, int Cin,
                           int accumulate, float* grad_b, hipStream_t stream) {
  const int total = ntap * CT16 * NT16 + NT16;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(zt_cdiv(total, 32)), dim3(256), 0, stream, slab, nslab, ntap, CT16, NT16, grad_w,
                     Cout, Cin, accumulate, grad_b);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}

// partial pass: every workgroup writes one slab ([tap][ci16][co16] weights + [co16] bias column sums); -> number of slabs
static int wgrad_partial_bf16(const void* x, int ldx, const void* dz, int lddz, int H, int W, int Cin, int Cout, int KH, int KW,
                              float* slab, size_t slab_bytes, const void* relu_mask, int ldmask, int* nslab_out, hipStream_t stream) {
  ZT_REQUIRE(x && dz && slab && ldx % 8 == 0 && lddz % 8 == 0);
  ZT_REQUIRE(!relu_mask || (ldmask % 8 == 0 && ((uintptr_t)relu_mask & 15) == 0 && KH == 3 && Cin <= 16 && Cout == 64));
  ZT_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)dz & 15) == 0);
  int CT = (Cin + 15) / 16, NT = (Cout + 15) / 16;
  WgradArgsH a;
  a.x = (const zt_bf16*)x; a.dz = (const zt_bf16*)dz; a.slab = slab; a.H = H; a.W = W; a.Cin = Cin; a.ldx = ldx; a.Cout = Cout;
  a.lddz = lddz; a.mask = (const zt_bf16*)relu_mask; a.ldmask = ldmask;
  a.tilesX = zt_cdiv(W, HTW);
  const bool nw8 = (CT == 4 && NT == 4) ||
                   (CT == 3 && NT == 3 && KW == KH && wgrad48_dma(KH, Cin, Cout, ldx, lddz)) ||
                   (CT == 1 && NT == 3 && KW == KH && wgrad_thin48_dma(KH, Cin, Cout, ldx, lddz, relu_mask));
  a.ntiles = a.tilesX * zt_cdiv(H, nw8 ? 8 : 4);      // tile rows = waves of the variant (launch_wgrad_h)
  size_t per = ((size_t)KH * KW * CT * 16 * NT * 16 + NT * 16) * sizeof(float);
  // the 8-wave variant runs one workgroup per CU: 256 slabs keep every CU busy and halve its slab traffic (measured 280 -> 266 us);
  // the 4-wave variants co-reside two or three per CU
  int want = nw8 ? 256 : 512;
  if (const char* e = getenv("ZT_WGRAD_BLOCKS")) want = atoi(e) > 0 ? atoi(e) : want;      // tuning hook
  int nblk = a.ntiles < want ? a.ntiles : want;
  if ((size_t)nblk * per > slab_bytes) nblk = (int)(slab_bytes / per);
  ZT_REQUIRE(nblk >= 1);
  int rc = ZT_EINVAL;
  if (KH == 3 && KW == 3) rc = launch_wgrad_h<3, 3>(a, CT, NT, nblk, stream);
  else if (KH == 1 && KW == 1) rc = launch_wgrad_h<1, 1>(a, CT, NT, nblk, stream);
  if (rc) return rc;
  *nslab_out = nblk;
  return ZT_OK;
}

extern "C" int zt_conv2d_wgrad_nhwc_bf16(const void* x, int ldx, const void* dz, int lddz, int H, int W, int Cin, int Cout,
                                         int KH, int KW, float* slab, size_t slab_bytes, float* grad_w, float* grad_b,
                                         int accumulate, const void* relu_mask, int ldmask, hipStream_t stream) {
  ZT_REQUIRE(grad_w);
  int nblk = 0;
  int rc = wgrad_partial_bf16(x, ldx, dz, lddz, H, W, Cin, Cout, KH, KW, slab, slab_bytes, relu_mask, ldmask, &nblk, stream);
  if (rc) return rc;
  int CT = (Cin + 15) / 16, NT = (Cout + 15) / 16;
  return zt_launch_wgrad_reduce(slab, nblk, KH * KW, CT * 16, NT * 16, grad_w, Cout, Cin, accumulate, grad_b, stream);
}

extern "C" int zt_conv2d_wgrad_partial_bf16(const void* x, int ldx, const void* dz, int lddz, int H, int W, int Cin, int Cout, int KH,
                                            int KW, float* slab, size_t slab_bytes, const void* relu_mask, int ldmask, int* nslab_out,
                                            hipStream_t stream) {
  ZT_REQUIRE(nslab_out);
  int rc = wgrad_partial_bf16(x, ldx, dz, lddz, H, W, Cin, Cout, KH, KW, slab, slab_bytes, relu_mask, ldmask, nslab_out, stream);
  if (rc) return rc;
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}

extern "C" int zt_wgrad_reduce_multi_f32(int nseg, const void* const* slab, const int* nslab, const int* Cin, const int* Cout,
                                         const int* K, void* const* grad_w, void* const* grad_b, int accumulate, hipStream_t stream) {
  ZT_REQUIRE(nseg >= 1 && nseg <= ZT_MAXSEG && slab && nslab && Cin && Cout && K && grad_w && grad_b);
  ReduceTable t;
  int maxtotal = 0;
  for (int i = 0; i < ZT_MAXSEG; ++i) {
    const int j = i < nseg ? i : 0;
    ZT_REQUIRE(slab[j] && grad_w[j] && nslab[j] >= 1);
    t.slab[i] = (const float*)slab[j]; t.gw[i] = (float*)grad_w[j]; t.gb[i] = (float*)grad_b[j];
    t.nslab[i] = nslab[j]; t.ntap[i] = K[j] * K[j]; t.CT16[i] = (Cin[j] + 15) / 16 * 16; t.NT16[i] = (Cout[j] + 15) / 16 * 16;
    t.Cout[i] = Cout[j]; t.Cin[i] = Cin[j];
    const int total = t.ntap[i] * t.CT16[i] * t.NT16[i] + t.NT16[i];
    if (i < nseg && total > maxtotal) maxtotal = total;
  }
  t.accumulate = accumulate;
  hipLaunchKernelGGL(wgrad_reduce_multi_kernel, dim3(zt_cdiv(maxtotal, 32), nseg), dim3(256), 0, stream, t);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}
