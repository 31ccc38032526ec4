// ---- register-stationary persistent kernel for the full-resolution 3x3 layers (stride 1, bf16 nhwc output, 48 or 64 couts).
// The LDS-fed kernels (zt_conv_tiled.hip, zt_conv_ws.hip) are LDS-bandwidth bound (0.75 fragment reads per MFMA against the 0.5 that 128 B/clk sustains), so
// here the WEIGHTS LIVE IN REGISTERS for the whole launch (persistent workgroups, two per CU, <= 162 VGPRs of A fragments per
// wave) and LDS only carries pixels: a wave owns two adjacent output rows, so every pixel fragment it reads from the 4 halo
// rows feeds both rows (ky and ky-1) -- 0.17-0.33 reads per MFMA.  What LDS capacity that frees goes to double-buffering the
// halo (next tile's global loads fly during this tile's MFMAs and are written to the other buffer at its end) and the output
// staging (tile k-1's 16-byte global stores, with the fused mask / residual epilogue, are issued inside tile k's MFMA loop).
// One barrier per tile.  128-byte pixel rows are XOR-swizzled by (halo column & 7): conflict-free ds_read_b128 for every tap.
// Channel tails use the K=16 MFMA (48 = 32 + 16, and the thin 3/9/12-channel inputs are a single K=16 chunk).
#include "zt_conv.h"
#include <stdlib.h>

namespace {

// wave w of 4: row pair w >> 1; COSPLIT: couts [NQ*16*(w&1), +NQ*16) of 2*NQ*16, both 16-pixel halves (NM == 2)
//                               else   : all NQ*16 couts, 16-pixel half (w & 1) (NM == 1)
// RT = tile rows = waves per workgroup = 4: two independent workgroups per CU with one staging buffer each, so that one
// workgroup's epilogue / barrier / DMA issue overlaps the other's MFMA loop
// STATS: the train-mode BatchNorm that follows the layer (model.py:62) needs the per-channel sum and sum of squares of the output
// over all pixels: they are accumulated from the staged (bf16-rounded, i.e. exactly the stored) values in the store phase --
// per-thread over its chunks, butterfly over the 8 lanes of a wave that own the same channel octet, then into a per-wave LDS
// table owned lane by lane (no atomics: fixed summation order, bit-reproducible) -- and written once per workgroup at the end;
// zt_norm_finalize_f32 reduces the [grid][2][Cout] partials.  Replaces a separate 265 MB read pass per Enhancer block.
template <int NQ, int NM, bool COSPLIT, int C32, int C16, bool EPI, bool STATS = false>
__global__ void __launch_bounds__(256, 2) conv_rs_bf16_kernel(ConvArgsH a, int ntiles) {
  static_assert(!STATS || !EPI || COSPLIT, "backward statistics ride in the 64-cout data-gradient variant (aux fetched by the store phase)");
  constexpr bool BSTATS = STATS && EPI;                         // BatchNorm-backward sums instead of forward statistics
  constexpr int RT = 4, NTHR = 64 * RT;
  // fused aux operand (activation mask / residual): read in accumulator layout (8 bytes per lane and 16x16 block) half a loop
  // ahead (AUXD: 48 couts); with 64 couts (144 VGPRs of weights) that spills, so there the aux chunk is fetched by the store phase
  // at the start of the next tile, where no accumulator is live (AUXS; the other workgroup of the CU covers the exposed latency)
  constexpr bool AUXD = EPI && !COSPLIT, AUXS = EPI && COSPLIT;
  constexpr int IR = RT + 2, IC = TW + 2;
  constexpr int KC = C32 * 32 + C16 * 16;                       // input channels staged per pixel
  constexpr int PE = KC > 32 ? 64 : (KC > 16 ? 32 : 16);        // LDS elements per pixel; only the 128-byte rows need the swizzle
  constexpr bool SWZ = PE == 64;
  constexpr int NCHK = PE / 8;                                  // 16-byte chunks per pixel
  constexpr bool GLDS = PE == 64;                               // full 128-byte rows go global -> LDS by DMA: no staging registers
  constexpr int NPF = GLDS ? 1 : (IR * IC * NCHK + NTHR - 1) / NTHR;
  constexpr int NGL = (IR * IC * 8 + NTHR - 1) / NTHR;                // LDS-DMA wave-instructions per wave and tile
  constexpr int CW = (COSPLIT ? 2 : 1) * NQ * 16;               // couts of the layer (== a.Cout)
  constexpr int CH8 = CW / 8;
  constexpr bool SWZO = CW == 64;
  constexpr int NOUT = RT * TW * CH8 / NTHR;
  static_assert(RT * TW * CH8 % NTHR == 0 && NTHR % NCHK == 0, "tile geometry");
  __shared__ __attribute__((aligned(16))) zt_bf16 xs[2][IR * IC * PE];
  __shared__ __attribute__((aligned(16))) zt_bf16 st[RT * TW * CW];
  __shared__ float bias_s[CW];
  __shared__ __attribute__((aligned(16))) float stat_s[STATS ? RT * 2 * CW : 4];      // [wave][octet][sum 8 | sumsq 8]
  __shared__ __attribute__((aligned(16))) float bn_s[BSTATS ? 3 * CW : 4];             // BSTATS: [scale | shift | mean][channel]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, l4 = lane >> 4;
  const int rp = wave >> 1, sel = wave & 1;
  if constexpr (STATS) {
    for (int e = tid; e < RT * 2 * CW; e += NTHR) stat_s[e] = 0.f;
  }
  if constexpr (BSTATS) {
    for (int e = tid; e < 3 * CW; e += NTHR) bn_s[e] = e < CW ? a.bn_scale[e] : (e < 2 * CW ? a.bn_shift[e - CW] : a.bn_mean[e - 2 * CW]);
  }
  const int q0 = COSPLIT ? sel * NQ : 0, m0 = COSPLIT ? 0 : sel;

  if (tid < CW) bias_s[tid] = a.bias ? a.bias[tid] : 0.f;

  // A fragments: weights [tap][CoutP][ldk], this wave's couts, all taps and channel chunks -- resident for the whole launch
  zt_s16x8 w32[9][C32 > 0 ? C32 : 1][NQ];
  zt_s16x4 w16[9][NQ];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap)
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const zt_bf16* wr = a.w + ((size_t)tap * a.CoutP + (q0 + q) * 16 + l15) * a.ldk;
#pragma unroll
      for (int c = 0; c < C32; ++c) {
        const int kk = c * 32 + l4 * 8;
        w32[tap][c][q] = kk < a.ldk ? *reinterpret_cast<const zt_s16x8*>(wr + kk) : (zt_s16x8){0, 0, 0, 0, 0, 0, 0, 0};
      }
      if (C16) {
        const int kk = C32 * 32 + l4 * 4;
        w16[tap][q] = kk < a.ldk ? *reinterpret_cast<const zt_s16x4*>(wr + kk) : (zt_s16x4){0, 0, 0, 0};
      }
    }

  // XCD-aware tile order: workgroup b runs on XCD b % 8, so within every round of gridDim tiles XCD x takes the x-th run of
  // gridDim / 8 consecutive indices, and indices walk the image in bands of 4 tile rows, column-major inside a band: an XCD's
  // 32 tiles of a round form an 8 x 4 block whose interior halos are shared in that XCD's L2 instead of re-fetched from HBM.
  const int G = gridDim.x;
  const int pb = (G % 8 == 0) ? ((int)blockIdx.x % 8) * (G / 8) + (int)blockIdx.x / 8 : (int)blockIdx.x;
  const int n_my = pb < ntiles ? (ntiles - 1 - pb) / G + 1 : 0;
  // the (ty, tx) of this workgroup's k-th tile: computed once into a small LDS table (the divisions are ~40 instructions and
  // three phases per tile need the coordinates), recomputed only beyond the table
  constexpr int TTAB = 256;
  __shared__ int tile_s[TTAB];
  auto tile_calc = [&](int k, int& ty, int& tx) {
    const int idx = pb + k * G;
    const int band = idx / (4 * a.tilesX), r = idx - band * 4 * a.tilesX;
    const int rows = a.tilesY - band * 4 < 4 ? a.tilesY - band * 4 : 4;
    tx = r / rows;
    ty = band * 4 + r - tx * rows;
  };
  for (int k = tid; k < n_my && k < TTAB; k += NTHR) {
    int ty, tx;
    tile_calc(k, ty, tx);
    tile_s[k] = (ty << 16) | tx;
  }
  auto tile_xy = [&](int k, int& ty, int& tx) {
    if (k < TTAB) {
      const int v = __builtin_amdgcn_readfirstlane(tile_s[k]);
      ty = v >> 16;
      tx = v & 0xFFFF;
    } else {
      tile_calc(k, ty, tx);
    }
  };

  // halo slot e = tid + NTHR i -> pixel e / NCHK (row-major in the IR x IC halo), chunk e % NCHK == tid % NCHK for every i
  uint4 pf[NPF];
  const int hq = tid & (NCHK - 1);
  const int hq8 = hq * 8 + 8 <= a.ldx ? hq * 8 : a.ldx - 8;     // never read past the pixel's channels; masked below
  // LDS-DMA form: wave-instruction (RT i + wave) fills positions [64 (RT i + wave), +64) of the linear image; position e holds
  // pixel e / 8, logical chunk (e % 8) ^ (column & 7) -- the swizzle is applied to the source address.  Needs Cin % 8 == 0.
  // Interior tiles (the halo lies inside the image: ~95 % of them) take a precomputed per-slot offset relative to the tile
  // origin -- one add per DMA; border tiles recompute the clamped / zero-filled addresses.  The offsets cost NGL registers,
  // which the EPI instantiations do not have: they always take the general path.
  constexpr bool FASTSLOT = GLDS && !EPI;
  int soff[FASTSLOT ? NGL : 1];
  if constexpr (FASTSLOT) {
#pragma unroll
    for (int i = 0; i < NGL; ++i) {
      const int e = (i * RT + wave) * 64 + lane;
      const int p = e >> 3, col = p % IC;
      const int cj = (e & 7) ^ (col & 7);
      soff[i] = cj * 8 < a.Cin ? ((p / IC) * a.W + col) * a.ldx + cj * 8 : -1;       // -1: channel chunk beyond Cin -> zeros
    }
  }
  auto glds_halo = [&](int k) {
    int ty, tx;
    tile_xy(k, ty, tx);
    const int gy0 = ty * RT - 1, gx0 = tx * TW - 1;
    zt_bf16* xb = xs[k & 1];
    if constexpr (FASTSLOT) {
      if (gy0 >= 0 && gy0 + IR <= a.H && gx0 >= 0 && gx0 + IC <= a.W) {
        const zt_bf16* base = a.x + (unsigned)((gy0 * a.W + gx0) * a.ldx);
#pragma unroll
        for (int i = 0; i < NGL; ++i) {
          const void* src = soff[i] >= 0 ? (const void*)(base + soff[i]) : (const void*)&zt_zero_chunk;
          if (i * NTHR + NTHR - 1 < IR * IC * 8 || (i * RT + wave) * 64 + lane < IR * IC * 8) zt_glds16(src, xb + (i * RT + wave) * 512);
        }
        return;
      }
    }
    int ln = lane;
    ZT_OPAQUE(ln);                                              // recompute the slot geometry per tile instead of keeping it in registers
    if constexpr (!FASTSLOT && !BSTATS) {                       // (BSTATS: the second code path costs it two spilled registers)
      // EPI instantiations: interior tiles without the precomputed offsets -- the same address as the general path minus its
      // clamps, bounds tests and selects (35 -> ~12 vector instructions per DMA; the kernel is issue-co-limited, section 5)
      if (gy0 >= 0 && gy0 + IR <= a.H && gx0 >= 0 && gx0 + IC <= a.W) {
        const zt_bf16* base = a.x + (unsigned)((gy0 * a.W + gx0) * a.ldx);
#pragma unroll
        for (int i = 0; i < NGL; ++i) {
          const int e = (i * RT + wave) * 64 + ln;
          const int p = e >> 3, row = p / IC, col = p - row * IC;
          const int cj = (e & 7) ^ (col & 7);
          const void* src = cj * 8 < a.Cin ? (const void*)(base + (unsigned)((row * a.W + col) * a.ldx + cj * 8)) : (const void*)&zt_zero_chunk;
          if (i * NTHR + NTHR - 1 < IR * IC * 8 || e < IR * IC * 8) zt_glds16(src, xb + (i * RT + wave) * 512);
        }
        return;
      }
    }
#pragma unroll
    for (int i = 0; i < NGL; ++i) {
      const int e = (i * RT + wave) * 64 + ln;
      const int p = e >> 3, col = p % IC;
      const int cj = (e & 7) ^ (col & 7);
      const int gy = gy0 + p / IC, gx = gx0 + col;
      const bool in = gy >= 0 && gy < a.H && gx >= 0 && gx < a.W && cj * 8 < a.Cin;
      const int gyc = gy < 0 ? 0 : (gy >= a.H ? a.H - 1 : gy), gxc = gx < 0 ? 0 : (gx >= a.W ? a.W - 1 : gx);
      const int cc = cj * 8 + 8 <= a.ldx ? cj * 8 : 0;
      const zt_bf16* s1 = a.x + (unsigned)((gyc * a.W + gxc) * a.ldx + cc);
      const void* src = in ? (const void*)s1 : (const void*)&zt_zero_chunk;
      if (i * NTHR + NTHR - 1 < IR * IC * 8 || e < IR * IC * 8) zt_glds16(src, xb + (i * RT + wave) * 512);
    }
  };
  auto load_halo = [&](int k) {
    if constexpr (GLDS) {
      glds_halo(k);
      return;
    }
    int ty, tx;
    tile_xy(k, ty, tx);
    const int gy0 = ty * RT - 1, gx0 = tx * TW - 1;
#pragma unroll
    for (int i = 0; i < NPF; ++i) {
      const int p = (tid + i * NTHR) / NCHK;
      int gy = gy0 + p / IC, gx = gx0 + p % IC;                 // out-of-image slots read a clamped address, zeroed when written
      gy = gy < 0 ? 0 : (gy >= a.H ? a.H - 1 : gy);
      gx = gx < 0 ? 0 : (gx >= a.W ? a.W - 1 : gx);
      pf[i] = *reinterpret_cast<const uint4*>(a.x + (unsigned)((gy * a.W + gx) * a.ldx + hq8));
    }
  };
  auto write_halo = [&](int k) {
    if constexpr (GLDS) return;
    int ty, tx;
    tile_xy(k, ty, tx);
    const int gy0 = ty * RT - 1, gx0 = tx * TW - 1;
    const int nv = a.Cin - hq * 8;                              // valid channels of this thread's chunk: padding lanes are not trusted
    const unsigned k0 = nv >= 2 ? ~0u : (nv == 1 ? 0xFFFFu : 0u), k1 = nv >= 4 ? ~0u : (nv == 3 ? 0xFFFFu : 0u);
    const unsigned k2 = nv >= 6 ? ~0u : (nv == 5 ? 0xFFFFu : 0u), k3 = nv >= 8 ? ~0u : (nv == 7 ? 0xFFFFu : 0u);
    zt_bf16* xb = xs[k & 1];
#pragma unroll
    for (int i = 0; i < NPF; ++i) {
      const int e = tid + i * NTHR, p = e / NCHK, col = p % IC;
      const int gy = gy0 + p / IC, gx = gx0 + col;
      const bool in = gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
      uint4 v = pf[i];
      v.x = in ? (v.x & k0) : 0u;
      v.y = in ? (v.y & k1) : 0u;
      v.z = in ? (v.z & k2) : 0u;
      v.w = in ? (v.w & k3) : 0u;
      if (e < IR * IC * NCHK) *reinterpret_cast<uint4*>(xb + p * PE + ((SWZ ? (hq ^ (col & 7)) : hq) * 8)) = v;
    }
  };

  // staged outputs of tile k -> global: chunk e = tid + NTHR i -> pixel e / CH8 of the 4 x 32 tile, couts 8 (e % CH8)..+8.
  // AUXS: the aux chunks (and the BatchNorm pre-activations of BSTATS) of tile k straight from global, 16 bytes per lane, all in
  // flight -- issued BEFORE the next halo's DMAs: vector-memory operations complete in order, so the store phase's wait for these
  // loads would otherwise also wait for the whole halo that was issued in front of them (a full HBM round trip per tile)
  // (BSTATS keeps 32 registers of operands per lane: holding them across the DMA address arithmetic spills, and a scratch reload
  // is itself a vector-memory operation behind the DMAs -- there the loads stay inside the store phase, behind the halo issue)
  constexpr bool AUXE = AUXS && !BSTATS;
  static_assert(!AUXE || NOUT == 4, "hidden aux loads are waited for four at a time");
  zt_u32x4 uxe[AUXE ? NOUT : 1];
  auto aux_fetch = [&](int k) {
    int ty, tx;
    tile_xy(k, ty, tx);
    const int oy0 = ty * RT, ox0 = tx * TW;
#pragma unroll
    for (int i = 0; i < NOUT; ++i) {
      const int e = tid + i * NTHR, pl = e / CH8, ch = e % CH8;
      int oy = oy0 + pl / TW, ox = ox0 + pl % TW;
      oy = oy >= a.Ho ? a.Ho - 1 : oy;
      ox = ox >= a.Wo ? a.Wo - 1 : ox;
      ZT_HIDDEN_LD16(uxe[AUXE ? i : 0], a.aux + (unsigned)((oy * a.Wo + ox) * a.ldaux + ch * 8));
    }
  };
  auto store_tile = [&](int k) {
    int ty, tx;
    tile_xy(k, ty, tx);
    const int oy0 = ty * RT, ox0 = tx * TW;
    const zt_bf16* sb = st;
    const float neg = a.epi == 1 ? 0.2f : 0.f;
    uint4 v[NOUT], ux[BSTATS ? NOUT : 1], zx[BSTATS ? NOUT : 1];
    float ssum[STATS ? 8 : 1], ssq[STATS ? 8 : 1];
    if constexpr (STATS) {
#pragma unroll
      for (int c = 0; c < 8; ++c) ssum[c] = ssq[c] = 0.f;
    }
    if constexpr (AUXE) {
      // aux_fetch(k) was issued before load_halo(k + 2).  When that halo issue followed (GLDS && k + 2 < n_my), its NGL DMAs (the
      // last of which a wave may skip) are the only vector-memory operations behind the aux loads and may stay in flight: the
      // tied wait is vmcnt(NGL - 1).  Otherwise nothing was issued behind them and a full drain precedes the tied wait.
      // (one register-tied wait on every path -- two alternatives would meet in copies of the still pending registers; the drain
      // is a separate, untied statement in front of it)
      if (!(GLDS && k + 2 < n_my)) ZT_WAIT_HIDDEN_DMA();
      ZT_HIDDEN_WAIT4(GLDS ? NGL - 1 : 0, uxe[0], uxe[AUXE ? 1 : 0], uxe[AUXE ? 2 : 0], uxe[AUXE ? 3 : 0]);
    }
    if constexpr (BSTATS) {                                     // aux chunks + pre-activations straight from global (16 bytes per lane), all in flight
#pragma unroll
      for (int i = 0; i < NOUT; ++i) {
        const int e = tid + i * NTHR, pl = e / CH8, ch = e % CH8;
        int oy = oy0 + pl / TW, ox = ox0 + pl % TW;
        oy = oy >= a.Ho ? a.Ho - 1 : oy;
        ox = ox >= a.Wo ? a.Wo - 1 : ox;
        ux[BSTATS ? i : 0] = *reinterpret_cast<const uint4*>(a.aux + (unsigned)((oy * a.Wo + ox) * a.ldaux + ch * 8));
        zx[BSTATS ? i : 0] = *reinterpret_cast<const uint4*>(a.zprev + (unsigned)((oy * a.Wo + ox) * a.ldz + ch * 8));
      }
    }
#pragma unroll
    for (int i = 0; i < NOUT; ++i) {
      const int e = tid + i * NTHR, pl = e / CH8, ch = e % CH8;
      v[i] = *reinterpret_cast<const uint4*>(sb + pl * CW + ((SWZO ? (ch ^ (pl & 7)) : ch) * 8));
    }
#pragma unroll
    for (int i = 0; i < NOUT; ++i) {
      const int e = tid + i * NTHR, pl = e / CH8, ch = e % CH8;
      const int oy = oy0 + pl / TW, ox = ox0 + pl % TW;
      uint4 o = v[i];
      if (AUXS) {
        uint4 u;
        if constexpr (BSTATS) u = ux[BSTATS ? i : 0];
        else u = make_uint4(uxe[AUXE ? i : 0].x, uxe[AUXE ? i : 0].y, uxe[AUXE ? i : 0].z, uxe[AUXE ? i : 0].w);
        const unsigned vv[4] = {o.x, o.y, o.z, o.w}, uu[4] = {u.x, u.y, u.z, u.w};
        unsigned oo[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float f0 = zt_u2f(vv[j] << 16), f1 = zt_u2f(vv[j] & 0xFFFF0000u);
          const float g0 = zt_u2f(uu[j] << 16), g1 = zt_u2f(uu[j] & 0xFFFF0000u);
          if (a.epi == 3) { f0 += g0; f1 += g1; }
          else { f0 *= (g0 > 0.f ? 1.f : neg); f1 *= (g1 > 0.f ? 1.f : neg); }
          oo[j] = zt_f2bf2(f0, f1);
        }
        o = make_uint4(oo[0], oo[1], oo[2], oo[3]);
      }
      if (oy < a.Ho && ox < a.Wo) *reinterpret_cast<uint4*>((zt_bf16*)a.y + (unsigned)((oy * a.Wo + ox) * a.ldy + ch * 8)) = o;
      if constexpr (STATS && !BSTATS) {
        if (oy < a.Ho && ox < a.Wo) {
          const unsigned ow[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float f0 = zt_u2f(ow[j] << 16), f1 = zt_u2f(ow[j] & 0xFFFF0000u);
            ssum[2 * j] += f0;
            ssum[2 * j + 1] += f1;
            ssq[2 * j] += f0 * f0;
            ssq[2 * j + 1] += f1 * f1;
          }
        }
      }
      if constexpr (BSTATS) {
        // the stored (bf16-rounded) gradient of the previous block's output, masked by that block's ReLU, summed plain and against
        // its centred pre-activation: what zt_bn_bwd_reduce computes in a pass of its own over the same two tensors
        if (oy < a.Ho && ox < a.Wo) {
          const unsigned ow[4] = {o.x, o.y, o.z, o.w};
          const uint4 zq = zx[BSTATS ? i : 0];
          const unsigned zw[4] = {zq.x, zq.y, zq.z, zq.w};
          const float4 sa = *reinterpret_cast<const float4*>(bn_s + ch * 8), sb2 = *reinterpret_cast<const float4*>(bn_s + ch * 8 + 4);
          const float4 ha = *reinterpret_cast<const float4*>(bn_s + CW + ch * 8), hb = *reinterpret_cast<const float4*>(bn_s + CW + ch * 8 + 4);
          const float4 ma = *reinterpret_cast<const float4*>(bn_s + 2 * CW + ch * 8), mb = *reinterpret_cast<const float4*>(bn_s + 2 * CW + ch * 8 + 4);
          const float scv[8] = {sa.x, sa.y, sa.z, sa.w, sb2.x, sb2.y, sb2.z, sb2.w}, shv[8] = {ha.x, ha.y, ha.z, ha.w, hb.x, hb.y, hb.z, hb.w};
          const float muv[8] = {ma.x, ma.y, ma.z, ma.w, mb.x, mb.y, mb.z, mb.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float f0 = zt_u2f(ow[j] << 16), f1 = zt_u2f(ow[j] & 0xFFFF0000u);
            const float z0 = zt_u2f(zw[j] << 16), z1 = zt_u2f(zw[j] & 0xFFFF0000u);
            const float g0 = z0 * scv[2 * j] + shv[2 * j] > 0.f ? f0 : 0.f, g1 = z1 * scv[2 * j + 1] + shv[2 * j + 1] > 0.f ? f1 : 0.f;
            ssum[2 * j] += g0;
            ssum[2 * j + 1] += g1;
            ssq[2 * j] += g0 * (z0 - muv[2 * j]);
            ssq[2 * j + 1] += g1 * (z1 - muv[2 * j + 1]);
          }
        }
      }
    }
    if constexpr (STATS) {
      // chunk e = tid + NTHR i has channel octet tid % 8 for every i: lanes l, l^8, l^16, l^32 of a wave share it
      // Reduce-scatter over those 8 lanes instead of a full butterfly: every stage hands HALF of the still-live values to the
      // partner and keeps the sums of the other half (8 + 4 + 2 = 14 cross-lane moves instead of 48); each lane ends up owning 2 of
      // the octet's 16 sums -- index 8 (lane>>5 & 1) + 4 (lane>>4 & 1) + 2 (lane>>3 & 1) + {0, 1} -- and adds them to its own two
      // slots of the per-wave table (fixed order: bit-reproducible).
      const bool h5 = lane & 32, h4 = lane & 16, h3 = lane & 8;
      float k8[8], k4[4], k2[2];
#pragma unroll
      for (int c = 0; c < 8; ++c) k8[c] = (h5 ? ssq[c] : ssum[c]) + __shfl_xor(h5 ? ssum[c] : ssq[c], 32);
#pragma unroll
      for (int c = 0; c < 4; ++c) k4[c] = (h4 ? k8[c + 4] : k8[c]) + __shfl_xor(h4 ? k8[c] : k8[c + 4], 16);
#pragma unroll
      for (int c = 0; c < 2; ++c) k2[c] = (h3 ? k4[c + 2] : k4[c]) + __shfl_xor(h3 ? k4[c] : k4[c + 2], 8);
      float* t = stat_s + (wave * CH8 + (lane & 7)) * 16 + (h5 ? 8 : 0) + (h4 ? 4 : 0) + (h3 ? 2 : 0);
      t[0] += k2[0];
      t[1] += k2[1];
    }
  };

  __syncthreads();                                              // tile table and bias visible
  if (n_my > 0) {
    load_halo(0);
    write_halo(0);
  }
  __syncthreads();

  const float slope = a.act == 0 ? 1.f : (a.act == 1 ? 0.f : 0.2f);     // none / ReLU / LeakyReLU(0.2) == max(v, slope*v)
  // lane part of the pixel fragment address for kx = 0..2 (halo row and 16-pixel half are immediate offsets)
  int xoff32[3][C32 > 0 ? C32 : 1], xoff16[3];
#pragma unroll
  for (int kx = 0; kx < 3; ++kx) {
    const int col = l15 + kx;                                   // + 16 m: does not change col & 7
#pragma unroll
    for (int c = 0; c < C32; ++c) xoff32[kx][c] = col * PE + (SWZ ? (((c * 4 + l4) ^ (col & 7)) * 8) : (c * 32 + l4 * 8));
    xoff16[kx] = col * PE + (SWZ ? (((C32 * 4 + (l4 >> 1)) ^ (col & 7)) * 8 + (l4 & 1) * 4) : (C32 * 32 + l4 * 4));
  }

  for (int k = 0; k < n_my; ++k) {
    const zt_bf16* xb = xs[k & 1] + ((2 * rp) * IC + m0 * 16) * PE;
    zt_f32x4 acc[2][NM][NQ];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int m = 0; m < NM; ++m)
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[r][m][q] = *reinterpret_cast<const zt_f32x4*>(&bias_s[(q0 + q) * 16 + l4 * 4]);   // bias

    // the hidden aux loads of tile k-1 go out BEFORE the halo DMAs of tile k+1: store_tile's vmcnt(NGL - 1) counts on this order
    if constexpr (AUXE) {
      if (k >= 1) aux_fetch(k - 1);
    }
    if (k + 1 < n_my) load_halo(k + 1);
    // (`n_my > 1` follows from k >= 1; with the bare test hipcc's allocation of the BSTATS instantiation, which sits at 256 VGPRs,
    // puts 4 registers into scratch inside the tile loop -- check -Rpass-analysis=kernel-resource-usage after touching this)
    if (k >= 1 && n_my > 1) store_tile(k - 1);
    ZT_LDS_BARRIER();                                           // single staging buffer: every wave has read tile k-1 before tile k is staged
    uint2 au[AUXD ? 2 : 1][AUXD ? NM : 1][AUXD ? NQ : 1];       // AUXD: this lane's aux values, in accumulator layout

    // steps: halo row h (0..3) x kx x channel chunk; each step's fragments serve output rows r with ky = h - r in [0, 2]
    constexpr int NCK = C32 + C16;
    constexpr int NSTEP = 4 * 3 * NCK;
    zt_s16x8 xa[2][NM];
    zt_s16x4 xt[2][NM];
#define ZT_LOADX(bufi, step)                                                                                          \
  {                                                                                                                   \
    constexpr int h_ = (step) / (3 * NCK), kx_ = ((step) / NCK) % 3, c_ = (step) % NCK;                               \
    _Pragma("unroll") for (int m = 0; m < NM; ++m) {                                                                  \
      if constexpr (c_ < C32) xa[bufi][m] = *reinterpret_cast<const zt_s16x8*>(xb + (h_ * IC + m * 16) * PE + xoff32[kx_][c_ < C32 ? c_ : 0]); \
      else xt[bufi][m] = *reinterpret_cast<const zt_s16x4*>(xb + (h_ * IC + m * 16) * PE + xoff16[kx_]);              \
    }                                                                                                                 \
  }
    ZT_LOADX(0, 0)
    zt_static_for<0, NSTEP>([&](auto step_c) {
      constexpr int step = decltype(step_c)::value;
      constexpr int cur = step & 1;
      constexpr int h = step / (3 * NCK), kx = (step / NCK) % 3, c = step % NCK;
      if constexpr (step + 1 < NSTEP) ZT_LOADX(cur ^ 1, step + 1)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int ky = h - r;
        if (ky >= 0 && ky <= 2) {
#pragma unroll
          for (int m = 0; m < NM; ++m)
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
              if constexpr (c < C32) acc[r][m][q] = zt_mfma_bf16(w32[ky * 3 + kx][c < C32 ? c : 0][q], xa[cur][m], acc[r][m][q]);
              else acc[r][m][q] = zt_mfma_bf16_k16(w16[ky * 3 + kx][q], xt[cur][m], acc[r][m][q]);
            }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (AUXD && step == NSTEP / 2 - 1) {            // aux in accumulator layout: half a loop of latency cover
        int ty, tx;
        tile_xy(k, ty, tx);
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
          for (int m = 0; m < NM; ++m) {
            int oy = ty * RT + 2 * rp + r, ox = tx * TW + (m0 + m) * 16 + l15;
            oy = oy >= a.Ho ? a.Ho - 1 : oy;
            ox = ox >= a.Wo ? a.Wo - 1 : ox;
            const zt_bf16* ap = a.aux + (unsigned)((oy * a.Wo + ox) * a.ldaux + q0 * 16 + l4 * 4);
#pragma unroll
            for (int q = 0; q < NQ; ++q) au[AUXD ? r : 0][AUXD ? m : 0][AUXD ? q : 0] = *reinterpret_cast<const uint2*>(ap + q * 16);
          }
      }
    });
#undef ZT_LOADX
    if (k + 1 < n_my) write_halo(k + 1);

    // accumulators -> staging (bias, alpha, activation, bf16): lane holds couts 4 l4 .. +3 of 16-cout block q for pixel l15
    zt_bf16* sb = st;
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int m = 0; m < NM; ++m)
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          const int cb = (q0 + q) * 16 + l4 * 4;
          float v[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = acc[r][m][q][j];
          // alpha == 1 on this path (rs_ok): hipcc had if-converted `if (alpha != 1) v *= alpha` into 2 packed multiplies + 4 selects
          // per 4 values, executed always; and fmaxf() on MFMA outputs costs a canonicalising v_max per operand -- ZT_VMAX is the bare
          // instruction.  The epilogue is the largest share of this VALU-issue co-limited kernel's 2.7 VALU per MFMA (section 5).
          if (a.act) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = ZT_VMAX(v[j], slope * v[j]);
          }
          if constexpr (AUXD) {                                 // fused epilogue on the fp32 values: one rounding
            const uint2 u = au[AUXD ? r : 0][AUXD ? m : 0][AUXD ? q : 0];
            const float g[4] = {zt_u2f(u.x << 16), zt_u2f(u.x & 0xFFFF0000u), zt_u2f(u.y << 16), zt_u2f(u.y & 0xFFFF0000u)};
            const float neg = a.epi == 1 ? 0.2f : 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = a.epi == 3 ? v[j] + g[j] : v[j] * (g[j] > 0.f ? 1.f : neg);
          }
          uint2 pk;
          pk.x = zt_f2bf2(v[0], v[1]);
          pk.y = zt_f2bf2(v[2], v[3]);
          const int pl = (2 * rp + r) * TW + (m0 + m) * 16 + l15;
          const int ch = cb >> 3;
          *reinterpret_cast<uint2*>(sb + pl * CW + ((SWZO ? (ch ^ (pl & 7)) : ch) * 8) + (cb & 4)) = pk;
        }
    __syncthreads();
  }
  if (n_my > 0) {
    if constexpr (AUXE) aux_fetch(n_my - 1);
    store_tile(n_my - 1);
  }
  if constexpr (STATS) {
    __syncthreads();
    if (tid < 2 * CW) {                                         // stats[block][0: sum | 1: sum of squares][channel]
      const int which = tid / CW, c = tid % CW;
      float t = 0.f;
#pragma unroll
      for (int w = 0; w < RT; ++w) t += stat_s[(w * CH8 + (c >> 3)) * 16 + which * 8 + (c & 7)];
      a.stats[(size_t)blockIdx.x * 2 * CW + tid] = t;
    }
  }
}

}  // namespace

int zt_launch_conv_rs(ConvArgsH& a, hipStream_t stream) {
  a.tilesX = zt_cdiv(a.Wo, TW);
  a.tilesY = zt_cdiv(a.Ho, 4);
  const int ntiles = a.tilesX * a.tilesY;
  int gx = ntiles < 512 ? ntiles : 512;                        // two 4-wave workgroups per CU
  if (const char* e = getenv("ZT_CONV_BLOCKS")) gx = atoi(e) > 0 && atoi(e) < gx ? atoi(e) : gx;      // test hook: fewer workgroups, deeper tile loops
  dim3 grid(gx), block(256);
  const int kc = a.Cin <= 16 ? 0 : (a.Cin > 48 ? 2 : 1);       // 0: one K=16 chunk, 1: 32 + 16, 2: 32 + 32
  if (a.stats) {                                                // fused BatchNorm statistics: the 64 -> 64 layer
    if (!(a.Cout == 64 && kc == 2 && (!a.epi || (a.epi == 3 && a.zprev)))) return ZT_EINVAL;
    if (a.epi) hipLaunchKernelGGL((conv_rs_bf16_kernel<2, 2, true, 2, 0, true, true>), grid, block, 0, stream, a, ntiles);      // data gradient + residual + BN-backward sums
    else hipLaunchKernelGGL((conv_rs_bf16_kernel<2, 2, true, 2, 0, false, true>), grid, block, 0, stream, a, ntiles);           // forward + BN statistics
    return 0;
  }
#define ZT_RS(nq, nm, cs, c32, c16)                                                                                  \
  {                                                                                                                  \
    if (a.epi) hipLaunchKernelGGL((conv_rs_bf16_kernel<nq, nm, cs, c32, c16, true>), grid, block, 0, stream, a, ntiles); \
    else hipLaunchKernelGGL((conv_rs_bf16_kernel<nq, nm, cs, c32, c16, false>), grid, block, 0, stream, a, ntiles);  \
    return 0;                                                                                                        \
  }
  if (a.Cout == 64 && kc == 2) ZT_RS(2, 2, true, 2, 0)
  if (a.Cout == 64 && kc == 0) ZT_RS(2, 2, true, 0, 1)
  if (a.Cout == 48 && kc == 1) ZT_RS(3, 1, false, 1, 1)
  if (a.Cout == 48 && kc == 0) ZT_RS(3, 1, false, 0, 1)
#undef ZT_RS
  return ZT_EINVAL;
}
