// bf16 tiled implicit-GEMM convolution: every geometry the persistent kernels do not take (all RAFT layers, strided and 7x7
// layers, small maps), plus the motion-encoder pair kernels that run two such problems in one launch.
#include "zt_conv.h"

namespace {

// bf16 throughput mode: the activation result is rounded to bf16 (3 significant digits) right away, so the hardware
// exp / rcp (1 ulp-ish) replace the ~25-instruction libm expansions -- per element of the issue-bound small-map epilogues
__device__ __forceinline__ float apply_act_fast(float v, int act) {
  switch (act) {
    case 1: return fmaxf(v, 0.f);
    case 2: return v > 0.f ? v : 0.2f * v;
    case 3: return __builtin_amdgcn_rcpf(1.f + __expf(-v));
    case 4: return 1.f - 2.f * __builtin_amdgcn_rcpf(__expf(2.f * v) + 1.f);
    case 5: return fminf(fmaxf(__builtin_amdgcn_rcpf(1.f + __expf(-v)), 0.0001f), 1.f);
    default: return v;
  }
}

// ALL: every tap's weights of the current channel chunk fit in LDS next to the input tile -> 2 barriers per chunk;
// otherwise weights are staged per kernel row (7x7).  MT = 16-pixel MFMA tiles per wave along x (1 for small feature maps).
// CH2 = 32-channel MFMA K-steps per staged chunk: 2 (64 channels, 160-byte rows) halves the barrier / staging rounds of the
// latency-bound small-map layers whose Cin is a multiple of 64.
// PD = chunks of global loads in flight (register slots).  The small RAFT maps (45 x 80) are a serial chain of short kernels whose
// MFMA work per chunk (~0.2 us) cannot cover a global latency (~1-2 us): with PD = 3 nearly the whole K range is requested
// before the first MFMA instead of one latency being exposed per chunk.
template <int KH, int KW, int S, int NT, int MT, bool ALL, int CH2, int PD>
__device__ __forceinline__ void conv_mfma_bf16_body(const ConvArgsH& a, const int block_y) {
  static_assert(ALL || PD == 1, "per-row weight groups are staged inside the chunk");
  constexpr int KCH = 32 * CH2, KCHP = CH2 == 2 ? 80 : 48, CPP = 4 * CH2;      // channels / LDS pitch / 16-byte chunks per pixel
  constexpr int TWm = 16 * MT;
  constexpr int IR = (TH - 1) * S + KH, IC = (TWm - 1) * S + KW;
  constexpr int TG = ALL ? KH * KW : KW;          // taps staged together
  constexpr int NG = ALL ? 1 : KH;
  constexpr int XS_ELEMS = IR * IC * KCHP, WS_ELEMS = TG * NT * 16 * KCHP;      // XS_ELEMS * 2 bytes is a multiple of 16 (KCHP is)
  __shared__ __attribute__((aligned(16))) zt_bf16 smem[XS_ELEMS + WS_ELEMS];    // pixel tile | weight tile; the fp32 epilogue re-uses both
  zt_bf16* const xs = smem;
  zt_bf16* const ws = smem + XS_ELEMS;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // grid = (tile columns, cout groups, tile rows x images): no integer divisions in the (issue-bound) prologue
  const int tx = blockIdx.x;
  int ty = blockIdx.z, n = 0;
  if (a.N > 1) {
    n = ty / a.tilesY;
    ty -= n * a.tilesY;
  }
  const int co0 = block_y * (NT * 16);
  const int oy0 = ty * TH, ox0 = tx * TWm;
  const int gy0 = oy0 * S - a.padH, gx0 = ox0 * S - a.padW;
  const int l15 = lane & 15, l4 = lane >> 4;

  zt_f32x4 acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int q = 0; q < NT; ++q) acc[m][q] = (zt_f32x4){0.f, 0.f, 0.f, 0.f};

  // global -> registers -> LDS, software-pipelined over the 32-channel chunks: all loads of a chunk are issued together
  // (clamped addresses, no branches; borders and ragged channel tails are masked when written) and the NEXT chunk's loads are
  // issued before this chunk's MFMAs, so one global latency is exposed per launch rather than several per chunk.
  constexpr int NWS = (TG * NT * 16 * CPP + 255) / 256;
  constexpr int NXS = (IR * IC * CPP + 255) / 256;
  static_assert(256 % CPP == 0, "a thread's channel octet is the same for all of its staging slots");
  uint4 wv[PD][NWS], xv[PD][NXS];
  // Chunk-invariant slot geometry, computed ONCE: the per-chunk staging code is then a handful of adds per 16-byte slot.  (With
  // the index arithmetic inside the chunk loop these kernels issued ~1200 scalar + vector ALU instructions per 20 MFMAs and
  // were issue-bound on it: every small-map RAFT layer took 11-16 us whatever its FLOP count.)
  const int q8 = (tid % CPP) * 8;                               // this thread's channel octet within a chunk (all slots)
  int x_src1[NXS], x_src2[NXS], x_lds[NXS];
  unsigned x_in[NXS];
#pragma unroll
  for (int i = 0; i < NXS; ++i) {
    const int e = tid + i * 256, p = e / CPP;
    const int gy = gy0 + p / IC, gx = gx0 + p % IC;
    const int gyc = gy < 0 ? 0 : (gy >= a.H ? a.H - 1 : gy), gxc = gx < 0 ? 0 : (gx >= a.W ? a.W - 1 : gx);
    const int pix = (n * a.H + gyc) * a.W + gxc;
    x_src1[i] = pix * a.ldx + q8;
    x_src2[i] = pix * a.ldx2 + q8;
    x_lds[i] = e < IR * IC * CPP ? p * KCHP + q8 : -1;
    x_in[i] = (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) ? ~0u : 0u;
  }
  int w_src[NWS], w_lds[NWS];
  unsigned w_ok[NWS];
#pragma unroll
  for (int i = 0; i < NWS; ++i) {
    const int e = tid + i * 256, r = e / CPP;
    const int co = r % (NT * 16), tl = r / (NT * 16);
    const int tlc = tl < TG ? tl : TG - 1;                      // padding slots (never written) stay inside the weight array
    const int cor = co0 + co < a.CoutP ? co0 + co : a.CoutP - 1;
    w_src[i] = (tlc * a.CoutP + cor) * a.ldk + q8;
    w_lds[i] = e < TG * NT * 16 * CPP ? (tl * NT * 16 + co) * KCHP + q8 : -1;
    w_ok[i] = co0 + co < a.CoutP ? ~0u : 0u;
  }
  const int w_grp_stride = TG * a.CoutP * a.ldk;
  // uniform fast-path flags: a tile whose halo lies inside the image needs no zero fill, a workgroup whose couts all exist no
  // weight mask; full channel chunks need no tail masks.  Slots below the last one are in range for every thread (compile time).
  const bool x_interior = gy0 >= 0 && gy0 + IR <= a.H && gx0 >= 0 && gx0 + IC <= a.W;
  const bool w_all = co0 + NT * 16 <= a.CoutP;
  constexpr bool X_LAST_PARTIAL = (IR * IC * CPP) % 256 != 0, W_LAST_PARTIAL = (TG * NT * 16 * CPP) % 256 != 0;
  auto load_w = [&](auto sl, int c0, int grp) {
    constexpr int d = decltype(sl)::value;
    const int add = c0 + grp * w_grp_stride;
    const bool ragged = c0 + KCH > a.ldk;                       // uniform: only a ragged last chunk needs the channel clamp
#pragma unroll
    for (int i = 0; i < NWS; ++i) {
      int off = w_src[i] + add;
      if (ragged) off = c0 + q8 < a.ldk ? off : off - (c0 + q8);
      wv[d][i] = *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(a.w) + 2u * (unsigned)off);
    }
  };
  auto write_w = [&](auto sl, int c0) {
    constexpr int d = decltype(sl)::value;
    const bool plain = w_all && c0 + KCH <= a.ldk && c0 < a.Cin;         // uniform
    const unsigned cok = (c0 + q8 < a.ldk && c0 < a.Cin) ? ~0u : 0u;   // beyond the weight row / a padding chunk: zeros
#pragma unroll
    for (int i = 0; i < NWS; ++i) {
      uint4 v = wv[d][i];
      if (!plain) {
        const unsigned m = w_ok[i] & cok;
        v.x &= m; v.y &= m; v.z &= m; v.w &= m;
      }
      if (!(W_LAST_PARTIAL && i == NWS - 1) || w_lds[i] >= 0) *reinterpret_cast<uint4*>(ws + w_lds[i]) = v;
    }
  };
  auto load_x = [&](auto sl, int c0) {
    constexpr int d = decltype(sl)::value;
    const bool second = a.x2 != nullptr && c0 >= a.csplit;
    const zt_bf16* src = second ? a.x2 : a.x;
    const int ld = second ? a.ldx2 : a.ldx;
    const int cbase = second ? c0 - a.csplit : c0;
    const bool ragged = cbase + KCH > ld;
#pragma unroll
    for (int i = 0; i < NXS; ++i) {
      int off = (second ? x_src2[i] : x_src1[i]) + cbase;
      if (ragged) off = cbase + q8 < ld ? off : off - (cbase + q8);
      xv[d][i] = *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(src) + 2u * (unsigned)off);
    }
  };
  auto write_x = [&](auto sl, int c0) {
    constexpr int d = decltype(sl)::value;
    const bool second = a.x2 != nullptr && c0 >= a.csplit;
    const int cbase = second ? c0 - a.csplit : c0;
    const int climit = second ? a.Cin - a.csplit : (a.x2 ? a.csplit : a.Cin);
    const bool full = cbase + KCH <= climit;                      // uniform: no channel tail in this chunk
    const int nv = climit - (cbase + q8);                         // valid channels of this thread's octet (ragged tail / beyond the input)
    const unsigned m0 = nv >= 2 ? ~0u : (nv == 1 ? 0xFFFFu : 0u), m1 = nv >= 4 ? ~0u : (nv == 3 ? 0xFFFFu : 0u);
    const unsigned m2 = nv >= 6 ? ~0u : (nv == 5 ? 0xFFFFu : 0u), m3 = nv >= 8 ? ~0u : (nv == 7 ? 0xFFFFu : 0u);
#pragma unroll
    for (int i = 0; i < NXS; ++i) {
      uint4 v = xv[d][i];
      if (!(full && x_interior)) {
        if (full) {
          v.x &= x_in[i]; v.y &= x_in[i]; v.z &= x_in[i]; v.w &= x_in[i];
        } else {
          v.x &= x_in[i] & m0;
          v.y &= x_in[i] & m1;
          v.z &= x_in[i] & m2;
          v.w &= x_in[i] & m3;
        }
      }
      if (!(X_LAST_PARTIAL && i == NXS - 1) || x_lds[i] >= 0) *reinterpret_cast<uint4*>(xs + x_lds[i]) = v;
    }
  };

  // Chunk loop.  Every load is issued UNCONDITIONALLY (chunk index clamped to the last one; the channel range is padded to a
  // multiple of PD chunks whose padding chunks are staged as zeros): with `if (more)` around the prefetch the compiler lost
  // count of the outstanding loads and put s_waitcnt vmcnt(0) in front of every LDS write, i.e. one full memory latency per
  // chunk however deep the prefetch (1.6-2.6 us per chunk on the 45 x 80 maps; measured with tools/bench_small.py).
  float bias_q[NT];                                             // requested now: the K loop hides the latency the epilogue used to expose
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int co = co0 + q * 16 + l15;
    bias_q[q] = (a.bias && co < a.Cout) ? a.bias[co] : 0.f;
  }
  const int nch = (a.Cin + KCH - 1) / KCH;
  const int last_c0 = (nch - 1) * KCH;
  if (nch > 0) {
    zt_static_for<0, PD>([&](auto sl) {
      constexpr int d = decltype(sl)::value;
      const int c0 = d * KCH <= last_c0 ? d * KCH : last_c0;
      load_x(sl, c0);
      load_w(sl, c0, 0);
    });
  }
  // fragment reads run LA (tap, channel-half) steps ahead of the MFMAs that consume them (LDS latency ~100+ clocks against
  // MT*NT*16 clocks of MFMA per step; the compiler's own schedule waited for each step's reads right before its MFMAs)
  constexpr int NSTEP = TG * CH2;
  constexpr int LA = NSTEP > 2 ? 2 : 1;
  const zt_bf16* xfrag = xs + ((wave * S) * IC + l15 * S) * KCHP + 8 * l4;
  const zt_bf16* wfrag = ws + l15 * KCHP + 8 * l4;
  const int ngroups = (nch + PD - 1) / PD;
#pragma unroll 1
  for (int g = 0; g < ngroups; ++g) {
    zt_static_for<0, PD>([&](auto sl) {
      constexpr int d = decltype(sl)::value;
      const int c0 = (g * PD + d) * KCH;                          // >= Cin: a padding chunk (staged as zeros)
      __syncthreads();
      write_x(sl, c0);
      write_w(sl, c0);
      __syncthreads();
      const int cn = c0 + PD * KCH <= last_c0 ? c0 + PD * KCH : last_c0;
      load_x(sl, cn);
      if (ALL) load_w(sl, cn, 0);                                 // single tap group: its weights are prefetched as well
#pragma unroll 1
      for (int grp = 0; grp < NG; ++grp) {
        if (grp > 0) {                                            // per-kernel-row weight groups (7x7): staged inside the chunk
          __syncthreads();
          load_w(sl, c0, grp);
          write_w(sl, c0);
          __syncthreads();
        }
        zt_s16x8 fa[LA + 1][MT], fb[LA + 1][NT];
        auto loadf = [&](auto bc, auto sc) {
          constexpr int bi = decltype(bc)::value, step = decltype(sc)::value;
          constexpr int tl = step / CH2, kc = step % CH2;
          const int ky = ALL ? tl / KW : grp, kx = ALL ? tl % KW : tl;
#pragma unroll
          for (int m = 0; m < MT; ++m)
            fa[bi][m] = *reinterpret_cast<const zt_s16x8*>(xfrag + (ky * IC + m * 16 * S + kx) * KCHP + kc * 32);
#pragma unroll
          for (int q = 0; q < NT; ++q)
            fb[bi][q] = *reinterpret_cast<const zt_s16x8*>(wfrag + (tl * NT * 16 + q * 16) * KCHP + kc * 32);
        };
        zt_static_for<0, LA>([&](auto sc) { loadf(ZtIdx<decltype(sc)::value % (LA + 1)>{}, sc); });
        zt_static_for<0, NSTEP>([&](auto sc) {
          constexpr int step = decltype(sc)::value;
          constexpr int cur = step % (LA + 1);
          if constexpr (step + LA < NSTEP) loadf(ZtIdx<(step + LA) % (LA + 1)>{}, ZtIdx<step + LA>{});
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int q = 0; q < NT; ++q) acc[m][q] = zt_mfma_bf16(fa[cur][m], fb[cur][q], acc[m][q]);
          __builtin_amdgcn_sched_barrier(0);
        });
      }
      if (!ALL) load_w(sl, cn, 0);
    });
  }

  const int oy = oy0 + wave;
  // fp32 nhwc output without a fused operand (the all-pairs correlation volume, corr.py:52-60: 52 MB at 1080p): the accumulator
  // layout gives every lane 4-byte stores 64 bytes apart; transposed through LDS each lane writes 16 contiguous bytes of a
  // pixel's cout run instead.  Wave-private slice of the (now idle) pixel / weight staging buffers.
  constexpr int SP = NT * 16 + 4;                               // staging row pitch in floats
  constexpr bool CAN_STAGE = 4 * 16 * MT * SP * 4 <= (XS_ELEMS + WS_ELEMS) * 2;
  if constexpr (CAN_STAGE) {
    if (a.out_mode == 2 && a.epi == 0 && a.ldy % 4 == 0) {      // uniform
      __syncthreads();                                          // every wave is done with the operand tiles
      float* stg = reinterpret_cast<float*>(smem) + wave * (16 * MT * SP);
#pragma unroll
      for (int q = 0; q < NT; ++q)
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            stg[(m * 16 + l4 * 4 + j) * SP + q * 16 + l15] = apply_act_fast(a.alpha * (acc[m][q][j] + bias_q[q]), a.act);
      __builtin_amdgcn_wave_barrier();                          // same wave writes and reads (LDS ops of a wave complete in order)
      if (oy < a.Ho) {
        constexpr int C4 = NT * 4;                              // 16-byte chunks per pixel
        for (int e = lane; e < 16 * MT * C4; e += 64) {
          const int p = e / C4, c4 = e - p * C4;
          const int ox = ox0 + p, co = co0 + c4 * 4;
          if (ox < a.Wo && co < a.Cout) {
            const float4 v = *reinterpret_cast<const float4*>(stg + p * SP + c4 * 4);
            float* dst = (float*)a.y + ((size_t)(n * a.Ho + oy) * a.Wo + ox) * a.ldy + co;
            if (co + 4 <= a.Cout) *reinterpret_cast<float4*>(dst) = v;
            else {
              const float t[4] = {v.x, v.y, v.z, v.w};
              for (int k = 0; k < 4 && co + k < a.Cout; ++k) dst[k] = t[k];
            }
          }
        }
      }
      return;
    }
  }
  // bf16 nhwc output without a fused operand (most RAFT layers): same transposition, bf16 -- one 16-byte store per lane instead of
  // eight 2-byte stores that each touch four 32-byte pieces of different lines (the epilogue was ~3 us of every small-map launch:
  // DESIGN.md section 5, full launch against a launch without epilogue)
  constexpr int SPH = NT * 16 + 8;                              // staging row pitch in bf16 elements (16-byte multiple)
  if constexpr (4 * 16 * MT * SPH * 2 <= (XS_ELEMS + WS_ELEMS) * 2) {
    if (a.out_mode == 0 && a.epi == 0 && a.ldy % 8 == 0 && (((uintptr_t)a.y) & 15) == 0) {      // uniform
      __syncthreads();
      zt_bf16* stg = smem + wave * (16 * MT * SPH);
#pragma unroll
      for (int q = 0; q < NT; ++q)
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            stg[(m * 16 + l4 * 4 + j) * SPH + q * 16 + l15] = zt_f2bf(apply_act_fast(a.alpha * (acc[m][q][j] + bias_q[q]), a.act));
      __builtin_amdgcn_wave_barrier();
      if (oy < a.Ho) {
        constexpr int C8 = NT * 2;                              // 16-byte chunks per pixel
        for (int e = lane; e < 16 * MT * C8; e += 64) {
          const int p = e / C8, c8 = e - p * C8;
          const int ox = ox0 + p, co = co0 + c8 * 8;
          if (ox < a.Wo && co < a.Cout) {
            const uint4 v = *reinterpret_cast<const uint4*>(stg + p * SPH + c8 * 8);
            zt_bf16* dst = (zt_bf16*)a.y + ((size_t)(n * a.Ho + oy) * a.Wo + ox) * a.ldy + co;
            if (co + 8 <= a.Cout) *reinterpret_cast<uint4*>(dst) = v;
            else {
              zt_bf16 t[8];
              __builtin_memcpy(t, &v, 16);
              for (int k = 0; k < 8 && co + k < a.Cout; ++k) dst[k] = t[k];
            }
          }
        }
      }
      return;
    }
  }
  // bf16 nhwc output with a fused operand (residual add, ReLU masks, the two GRU fusions): activated values staged in fp32 so the
  // arithmetic is the scalar path's; operands and results move as 16-byte chunks of 8 channels
  if constexpr (CAN_STAGE) {
    const bool al = a.ldy % 8 == 0 && (((uintptr_t)a.y) & 15) == 0 && a.ldaux % 8 == 0 && (((uintptr_t)a.aux) & 15) == 0 &&
                    (a.epi != 4 || (a.ldy2 % 8 == 0 && a.esplit % 8 == 0 && (((uintptr_t)a.y2) & 15) == 0));
    if (a.out_mode == 0 && a.epi != 0 && al) {                   // uniform
      __syncthreads();
      float* stg = reinterpret_cast<float*>(smem) + wave * (16 * MT * SP);
#pragma unroll
      for (int q = 0; q < NT; ++q)
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            stg[(m * 16 + l4 * 4 + j) * SP + q * 16 + l15] = apply_act_fast(a.alpha * (acc[m][q][j] + bias_q[q]), a.act);
      __builtin_amdgcn_wave_barrier();
      if (oy < a.Ho) {
        constexpr int C8 = NT * 2;
        for (int e = lane; e < 16 * MT * C8; e += 64) {
          const int p = e / C8, c8 = e - p * C8;
          const int ox = ox0 + p, co = co0 + c8 * 8;
          if (ox >= a.Wo || co >= a.Cout) continue;
          const size_t pix = (size_t)(n * a.Ho + oy) * a.Wo + ox;
          const float4 va = *reinterpret_cast<const float4*>(stg + p * SP + c8 * 8);
          const float4 vb = *reinterpret_cast<const float4*>(stg + p * SP + c8 * 8 + 4);
          const float v[8] = {va.x, va.y, va.z, va.w, vb.x, vb.y, vb.z, vb.w};
          const bool second = a.epi == 4 && co >= a.esplit;     // the r half of [z | r]
          const bool whole = co + 8 <= a.Cout;
          const zt_bf16* up = a.aux + pix * a.ldaux + (second ? co - a.esplit : co);
          zt_bf16* dst = second ? a.y2 + pix * a.ldy2 + (co - a.esplit) : (zt_bf16*)a.y + pix * a.ldy + co;
          const bool need_u = a.epi != 4 || second;
          auto combine = [&](float r, float uf, float hf) {
            if (a.epi == 4) return second ? r * uf : r;
            if (a.epi == 5) return (1.f - uf) * hf + uf * r;
            if (a.epi == 1) return r * (uf > 0.f ? 1.f : 0.2f);
            if (a.epi == 2) return r * (uf > 0.f ? 1.f : 0.f);
            if (a.epi == 6) return fmaxf(r + uf, 0.f);          // ResidualBlock: relu(x + y) (extractor.py:56)
            return r + uf;
          };
          if (whole) {                                          // registers only: no indexed local arrays (they would go to scratch)
            uint4 uq = make_uint4(0, 0, 0, 0), hq = make_uint4(0, 0, 0, 0), oq;
            if (need_u) uq = *reinterpret_cast<const uint4*>(up);
            if (a.epi == 5) hq = *reinterpret_cast<const uint4*>(dst);
            const unsigned uw[4] = {uq.x, uq.y, uq.z, uq.w}, hw[4] = {hq.x, hq.y, hq.z, hq.w};
            unsigned ow[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const float lo = combine(v[2 * k], zt_u2f(uw[k] << 16), zt_u2f(hw[k] << 16));
              const float hi = combine(v[2 * k + 1], zt_u2f(uw[k] & 0xffff0000u), zt_u2f(hw[k] & 0xffff0000u));
              ow[k] = zt_f2bf2(lo, hi);
            }
            oq = make_uint4(ow[0], ow[1], ow[2], ow[3]);
            *reinterpret_cast<uint4*>(dst) = oq;
          } else {
#pragma unroll
            for (int k = 0; k < 8; ++k)
              if (co + k < a.Cout)
                dst[k] = zt_f2bf(combine(v[k], need_u ? zt_bf2f(up[k]) : 0.f, a.epi == 5 ? zt_bf2f(dst[k]) : 0.f));
          }
        }
      }
      return;
    }
  }
  if (oy >= a.Ho) return;
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int co = co0 + q * 16 + l15;
    if (co >= a.Cout) continue;
    const float b = bias_q[q];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int ox = ox0 + m * 16 + l4 * 4 + j;
        if (ox >= a.Wo) continue;
        float v = apply_act_fast(a.alpha * (acc[m][q][j] + b), a.act);
        const size_t pix = (size_t)(n * a.Ho + oy) * a.Wo + ox;
        if (a.epi == 4 || a.epi == 5) {       // SepConvGRU fusions (update.py:42-58), bf16 nhwc only
          zt_bf16* yb = (zt_bf16*)a.y;
          if (a.epi == 4) {     // [z | r] = sigmoid(conv): z is stored, r leaves as r * h
            if (co < a.esplit) yb[pix * a.ldy + co] = zt_f2bf(v);
            else a.y2[pix * a.ldy2 + co - a.esplit] = zt_f2bf(v * zt_bf2f(a.aux[pix * a.ldaux + co - a.esplit]));
          } else {              // q = tanh(conv): h = (1 - z) * h + z * q in place (aux = z)
            const float z = zt_bf2f(a.aux[pix * a.ldaux + co]), hv = zt_bf2f(yb[pix * a.ldy + co]);
            yb[pix * a.ldy + co] = zt_f2bf((1.f - z) * hv + z * v);
          }
          continue;
        }
        if (a.epi) {
          float u = zt_bf2f(a.aux[pix * a.ldaux + co]);
          if (a.epi == 1) v *= (u > 0.f ? 1.f : 0.2f);
          else if (a.epi == 2) v *= (u > 0.f ? 1.f : 0.f);
          else v += u;
          if (a.epi == 6) v = fmaxf(v, 0.f);
        }
        if (a.out_mode == 1) ((float*)a.y)[((size_t)n * a.Cout + co) * a.ldy + (size_t)oy * a.Wo + ox] = v;
        else if (a.out_mode == 2) ((float*)a.y)[pix * a.ldy + co] = v;
        else ((zt_bf16*)a.y)[pix * a.ldy + co] = zt_f2bf(v);
      }
    }
  }
}

template <int KH, int KW, int S, int NT, int MT, bool ALL, int CH2, int PD>
__global__ void __launch_bounds__(256) conv_mfma_bf16_kernel(ConvArgsH a) {
  conv_mfma_bf16_body<KH, KW, S, NT, MT, ALL, CH2, PD>(a, (int)blockIdx.y);
}

// TWO independent convolutions of the same kernel instantiation and the same map in ONE launch: cout groups [0, ysplit) of the
// grid's y axis run problem a0, the rest a1 (RAFT's motion encoder: convc2 || convf2, update.py:91-94 -- the small-map layers are
// bound by their fixed launch + prologue + epilogue cost, and neither of the two fills the chip on its own)
template <int KH, int KW, int S, int NT, int MT, bool ALL, int CH2, int PD>
__global__ void __launch_bounds__(256) conv_mfma_bf16_pair_kernel(ConvArgsH a0, ConvArgsH a1, int ysplit) {
  const bool first = (int)blockIdx.y < ysplit;                    // uniform
  // by value: through a reference to `first ? a0 : a1` hipcc keeps both argument blocks in scratch and indexes them (312 bytes per
  // lane, 14 -> 25 us per launch); the copy is scalar selects, field by field
  const ConvArgsH a = first ? a0 : a1;
  conv_mfma_bf16_body<KH, KW, S, NT, MT, ALL, CH2, PD>(a, first ? (int)blockIdx.y : (int)blockIdx.y - ysplit);
}

// ... and of two DIFFERENT instantiations (same map, 16-pixel tiles): convc1 (1x1, 324 -> 256) || convf1 (7x7, 2 -> 128), the two
// heads of the motion encoder (update.py:89, 91).  Each body has its own static LDS tile; a workgroup uses one of them.
template <int KH1, int KW1, int NT1, bool ALL1, int CH21, int PD1, int KH2, int KW2, int NT2, bool ALL2, int CH22, int PD2>
__global__ void __launch_bounds__(256) conv_mfma_bf16_pair2_kernel(ConvArgsH a0, ConvArgsH a1, int ysplit) {
  if ((int)blockIdx.y < ysplit) conv_mfma_bf16_body<KH1, KW1, 1, NT1, 1, ALL1, CH21, PD1>(a0, (int)blockIdx.y);
  else conv_mfma_bf16_body<KH2, KW2, 1, NT2, 1, ALL2, CH22, PD2>(a1, (int)blockIdx.y - ysplit);
}

template <int KH, int KW, int S, int MT>
int launch_conv_h(const ConvArgsH& a, int NT, hipStream_t stream) {
  dim3 block(256);
  int c16 = (a.Cout + 15) / 16;
  if ((long long)a.tilesY * a.N > 65535) return ZT_EINVAL;
  dim3 grid(a.tilesX, (c16 + NT - 1) / NT, a.tilesY * a.N);
  constexpr int IRc = (TH - 1) * S + KH, ICc = (16 * MT - 1) * S + KW;
  // 64-channel chunks where every chunk is full: Cin (and the split point of a two-part input) multiples of 64
  const bool wide = a.Cin % 64 == 0 && (!a.x2 || a.csplit % 64 == 0);
  // latency-bound launches (about two workgroups per CU or fewer, several channel chunks): two chunks of loads in flight
  const bool deep = MT == 1 && (long long)grid.x * grid.y * grid.z <= 1024 && a.Cin > 64;
#define ZT_CH(nt)                                                                                             \
  {                                                                                                           \
    constexpr bool all1 = (KH * KW * nt * 16 + IRc * ICc) * 48 * 2 <= 72 * 1024;                              \
    constexpr bool all2 = (KH * KW * nt * 16 + IRc * ICc) * 80 * 2 <= 64 * 1024;                              \
    constexpr bool fits2 = all2;              /* only while >= 2 workgroups still fit a CU: larger tiles lose more than they gain */ \
    if constexpr (fits2) {                                                                                    \
      if (wide) {                                                                                             \
        if constexpr (MT == 1) {                                                                              \
          if (deep) {                                                                                         \
            hipLaunchKernelGGL((conv_mfma_bf16_kernel<KH, KW, S, nt, MT, all2, 2, 2>), grid, block, 0, stream, a); \
            break;                                                                                            \
          }                                                                                                   \
        }                                                                                                     \
        hipLaunchKernelGGL((conv_mfma_bf16_kernel<KH, KW, S, nt, MT, all2, 2, 1>), grid, block, 0, stream, a); \
        break;                                                                                                \
      }                                                                                                       \
    }                                                                                                         \
    if constexpr (MT == 1 && all1) {                                                                          \
      if (deep) {                                                                                             \
        hipLaunchKernelGGL((conv_mfma_bf16_kernel<KH, KW, S, nt, MT, all1, 1, 2>), grid, block, 0, stream, a); \
        break;                                                                                                \
      }                                                                                                       \
    }                                                                                                         \
    hipLaunchKernelGGL((conv_mfma_bf16_kernel<KH, KW, S, nt, MT, all1, 1, 1>), grid, block, 0, stream, a);    \
  }
  switch (NT) {
    case 1: ZT_CH(1) break;
    case 2: ZT_CH(2) break;
    case 3: ZT_CH(3) break;
    default: ZT_CH(4) break;
  }
#undef ZT_CH
  return 0;
}

}  // namespace

int zt_launch_conv_tiled(const ConvArgsH& a, int KH, int KW, int stride, int MT, int NT, hipStream_t stream) {
  // stride 1: 32- or 16-pixel tiles (MT = 2 / 1); stride 2 always runs 16-pixel tiles (conv2d_bf16_impl)
#define ZT_GEO1(kh, kw) \
  if (KH == kh && KW == kw && stride == 1) return MT == 2 ? launch_conv_h<kh, kw, 1, 2>(a, NT, stream) : launch_conv_h<kh, kw, 1, 1>(a, NT, stream);
#define ZT_GEO2(kh, kw) \
  if (KH == kh && KW == kw && stride == 2 && MT == 1) return launch_conv_h<kh, kw, 2, 1>(a, NT, stream);
  ZT_GEO1(3, 3) ZT_GEO2(3, 3) ZT_GEO1(1, 1) ZT_GEO2(1, 1) ZT_GEO1(1, 5) ZT_GEO1(5, 1) ZT_GEO1(7, 7) ZT_GEO2(7, 7)
#undef ZT_GEO1
#undef ZT_GEO2
  return ZT_EINVAL;
}

// motion-encoder pairs (see conv_mfma_bf16_pair_kernel / _pair2_kernel): square kernels KA, KB (pad K / 2, stride 1), bf16 nhwc in / out,
// same map and activation.  Falls back to two launches when the two problems do not take the kernel instantiations built here.
extern "C" int zt_conv2d_pair_nhwc_bf16(const void* xA, int ldxA, int CinA, const void* wA, int CoutPA, int ldkA, const float* biasA, void* yA,
                                        int ldyA, int CoutA, int KA, const void* xB, int ldxB, int CinB, const void* wB, int CoutPB, int ldkB,
                                        const float* biasB, void* yB, int ldyB, int CoutB, int KB, int N, int H, int W, int act, hipStream_t stream) {
  auto single = [&]() {
    int rc = zt_conv2d_nhwc_bf16(xA, nullptr, 0, ldxA, 0, N, H, W, CinA, wA, CoutPA, ldkA, biasA, yA, ldyA, 0, CoutA, KA, KA, 1, KA / 2, KA / 2, act, 1.f,
                                 nullptr, 0, 0, stream);
    if (rc) return rc;
    return zt_conv2d_nhwc_bf16(xB, nullptr, 0, ldxB, 0, N, H, W, CinB, wB, CoutPB, ldkB, biasB, yB, ldyB, 0, CoutB, KB, KB, 1, KB / 2, KB / 2, act, 1.f,
                               nullptr, 0, 0, stream);
  };
  ZT_REQUIRE(xA && xB && wA && wB && yA && yB);
  const int tilesY = zt_cdiv(H, TH), tilesX = zt_cdiv(W, 16);
  const int gA = zt_cdiv(zt_cdiv(CoutA, 16), 2), gB = zt_cdiv(zt_cdiv(CoutB, 16), 2);
  // common conditions of the small-map instantiations (conv2d_bf16_impl in zt_conv.hip / launch_conv_h): NT = 2 (32 couts per workgroup), MT = 1
  const bool small = N == 1 && CoutA % 32 == 0 && CoutB % 32 == 0 && CoutA >= 64 && CoutB >= 64 &&
                     (long long)zt_cdiv(W, 32) * tilesY * zt_cdiv(CoutA / 16, 2) < 512 && (long long)zt_cdiv(W, 32) * tilesY * zt_cdiv(CoutB / 16, 2) < 512 &&
                     (long long)tilesX * tilesY * (gA + gB) <= 1024 && ldxA % 8 == 0 && ldxB % 8 == 0 && ldyA % 8 == 0 && ldyB % 8 == 0 && tilesY <= 65535;
  // (3x3, 3x3): both wide (64-channel chunks) and deep (two chunks in flight); (1x1, 7x7): 32-channel chunks, 1x1 deep, 7x7 per-row weights
  const bool p33 = small && KA == 3 && KB == 3 && CinA % 64 == 0 && CinB % 64 == 0 && CinA > 64 && CinB > 64;
  const bool p17 = small && KA == 1 && KB == 7 && CinA % 64 != 0 && CinA > 64 && CinB <= 8;
  if (!p33 && !p17) return single();
  ConvArgsH a[2];
  const void* xs[2] = {xA, xB};
  const void* ws[2] = {wA, wB};
  const float* bs[2] = {biasA, biasB};
  void* ys[2] = {yA, yB};
  const int ldx[2] = {ldxA, ldxB}, Cin[2] = {CinA, CinB}, CoutP[2] = {CoutPA, CoutPB}, ldk[2] = {ldkA, ldkB}, ldy[2] = {ldyA, ldyB}, Cout[2] = {CoutA, CoutB};
  const int Ks[2] = {KA, KB};
  for (int i = 0; i < 2; ++i) {
    ConvArgsH& c = a[i];
    c.x = (const zt_bf16*)xs[i]; c.x2 = nullptr; c.w = (const zt_bf16*)ws[i]; c.bias = bs[i]; c.aux = nullptr; c.y = ys[i];
    c.N = N; c.H = H; c.W = W; c.Cin = Cin[i]; c.ldx = ldx[i]; c.ldx2 = 0; c.csplit = 0;
    c.Ho = H; c.Wo = W; c.Cout = Cout[i]; c.CoutP = CoutP[i]; c.ldk = ldk[i]; c.ldy = ldy[i]; c.ldaux = 0;
    c.padH = Ks[i] / 2; c.padW = Ks[i] / 2; c.act = act; c.epi = 0; c.out_mode = 0; c.alpha = 1.f;
    c.tilesX = tilesX; c.tilesY = tilesY; c.y2 = nullptr; c.ldy2 = 0; c.esplit = 0; c.stats = nullptr;
    c.zprev = nullptr; c.ldz = 0; c.bn_scale = c.bn_shift = c.bn_mean = nullptr;
    ZT_REQUIRE(((uintptr_t)c.x & 15) == 0 && ((uintptr_t)c.w & 15) == 0 && c.ldk % 8 == 0 && ((uintptr_t)c.y & 15) == 0);
  }
  const dim3 grid(tilesX, gA + gB, tilesY);
  if (p33) hipLaunchKernelGGL((conv_mfma_bf16_pair_kernel<3, 3, 1, 2, 1, true, 2, 2>), grid, dim3(256), 0, stream, a[0], a[1], gA);
  else hipLaunchKernelGGL((conv_mfma_bf16_pair2_kernel<1, 1, 2, true, 1, 2, 7, 7, 2, false, 1, 1>), grid, dim3(256), 0, stream, a[0], a[1], gA);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}
