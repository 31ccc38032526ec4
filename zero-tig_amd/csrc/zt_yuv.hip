// Raw video in and out of predict.py (--y4m_in / --y4m_out, --y4m_out_depth): planar Y'CbCr of 8 bits, or of B = 9, 10, 12, 14 or
// 16 bits (tags C420p10 ... C444p16), <-> RGB with chroma resampling, on the device.
// A frame is the YUV4MPEG2 payload: plane Y [H][W], then U, then V ([H/2][W/2] for 4:2:0, [H][W/2] for 4:2:2, [H][W] for 4:4:4),
// contiguous uint8, or little-endian uint16 with the value in the low B bits; a deep sample above m = 2^B - 1 is read as m.
// The arithmetic is integer and fixed, so the result is the same on every machine.  One definition, two scales:
//              samples           RGB levels L      coefficients round(c 2^S)   accumulator          mid       top
//   8 bits     uint8             0..255            S = 14                      int                  128       255
//   deep       min(uint16, m)    0..65535          S = 20                      int64 (peak 2^41)    2^(B-1)   m
//   decode  chroma upsampled to full resolution as an integer carrying a factor of 16 (horizontal weights sum to 4: centre siting
//           (3, 1) towards the nearer neighbour, left siting 4 / (2, 2); vertical weights (3, 1) for 4:2:0, 4 otherwise; clamped
//           at the plane's edges), y = 16 CY (Y - yo), u = U16 - 16 mid, v = V16 - 16 mid,
//           R = clip((y + CRV v + 2^(S+3)) >> (S+4)), G = clip((y - CGU u - CGV v + 2^(S+3)) >> (S+4)), B = clip((y + CBU u + 2^(S+3)) >> (S+4)),
//           clipped to 0..L; 8 bits store the level (uint8 HWC) or its ToTensor table entry, deep float(level) / 65535.f (an IEEE division)
//   encode  level = zt_quantize_u8_hwc mode 0 for 8 bits, deep x > 0 ? (x < 1 ? (int)(x * 65535.f + 0.5f) : 65535) : 0 (NaN -> 0; a
//           float32 multiply, then a float32 add); Y = yo + ((CYR R + CYG G + CYB B + 2^(S-1)) >> S); chroma from the integer RGB
//           sums over the sample's footprint (box for centre siting, [1, 2, 1] for left siting, both rows for 4:2:0; weight total 2^sh):
//           U = mid + ((CUR Rs + CUG Gs + CUB Bs + 2^(S-1+sh)) >> (S+sh)), V alike; every plane clipped to 0..top.
// The coefficients (matrix, range and depth folded in) are computed by the host in double precision (zero-tig_amd/y4m.py) and
// travel as kernel arguments: no colour constant lives here.  The deep ones arrive as 64-bit values, every one of them fits 32 bits
// (the largest, CBU at 9 bits, is below 2^29), and every other factor is below 2^21, so each product is one 32 x 32 -> 64 bit multiply.
// Kernels of a few MB, HBM-bound: a thread owns a 2 x 8 luma patch, so every chroma sample is loaded (decode) or made (encode)
// once; with W % 8 == 0 and 16-byte aligned pointers every access is 4, 8 or 16 bytes wide along the row, any other width takes
// single-sample accesses with the same arithmetic.  No atomics, no scratch; the only LDS is the 256-entry ToTensor table of the
// fused 8-bit decode.  Every result is clamped BEFORE its shift (offsets folded into the accumulator), and packed words are built
// by OR from values already clamped to the sample's width: the note at clip_shr.
#include "zt_common.h"

namespace {

typedef long long i64;

struct DecCoef { int yo, cy, crv, cgu, cgv, cbu; };
struct EncCoef { int yo, cyr, cyg, cyb, cur, cug, cub, cvr, cvg, cvb; };
struct DecCoefDeep : DecCoef { int m, mid16; };
struct EncCoefDeep : EncCoef { int m, mid; };

// What differs between the depths: T the sample, Acc the accumulator, S the coefficient precision, LMAX the top RGB level, PER the
// samples of a 32-bit word, LUT whether the fp32 decode goes through the table in LDS; top and mid of the planes (mid16 = 16 mid,
// the scale of the decode's chroma), the clamp of a sample that was read, the quantiser of the encode, and what the decode keeps
// of a level until its store (Out, out) and stores (value).
struct Px8 {
  typedef unsigned char T;
  typedef int Acc;
  typedef DecCoef Dec;
  typedef EncCoef Enc;
  static constexpr int S = 14, LMAX = 255, PER = 4;
  static constexpr bool LUT = true;
  template <class K> static __device__ __forceinline__ int top(const K&) { return 255; }
  static __device__ __forceinline__ int mid(const Enc&) { return 128; }
  static __device__ __forceinline__ int mid16(const Dec&) { return 2048; }
  static __device__ __forceinline__ int sample(int v, int) { return v; }
  static __device__ __forceinline__ int quant(float x) { return zt_quant_u8(x, 0); }
  typedef int Out;                                    // the level, looked up at the store
  static __device__ __forceinline__ int out(int c) { return c; }
  static __device__ __forceinline__ float value(int c, const float* lut) { return lut[c]; }
};

struct PxDeep {
  typedef unsigned short T;
  typedef i64 Acc;
  typedef DecCoefDeep Dec;
  typedef EncCoefDeep Enc;
  static constexpr int S = 20, LMAX = 65535, PER = 2;
  static constexpr bool LUT = false;
  template <class K> static __device__ __forceinline__ int top(const K& k) { return k.m; }
  static __device__ __forceinline__ int mid(const Enc& k) { return k.mid; }
  static __device__ __forceinline__ int mid16(const Dec& k) { return k.mid16; }
  static __device__ __forceinline__ int sample(int v, int m) { return min(v, m); }
  static __device__ __forceinline__ int quant(float x) { return x > 0.f ? (x < 1.f ? (int)(x * 65535.f + 0.5f) : 65535) : 0; }
  typedef float Out;                                  // the value, divided where the level is made
  static __device__ __forceinline__ float out(int c) { return (float)c / 65535.f; }
  static __device__ __forceinline__ float value(float f, const float*) { return f; }
};

// subsampling, siting and whether every access is a whole vector: the five (SS, SIT) of yuv_launch, each FAST or not
template <int SS_, int SIT_, bool FAST_>
struct Layout {
  static constexpr int SS = SS_, SIT = SIT_;
  static constexpr bool FAST = FAST_;
};

template <class P>
__device__ __forceinline__ typename P::Acc mul(int a, int b) { return (typename P::Acc)a * (typename P::Acc)b; }

// clip(v >> S, 0, top), clamped BEFORE the shift.  An observation, not a diagnosed cause: written as shift-then-clamp, hipcc (HIP
// 7.2.26015, AMD clang 22.0.0git roc-7.2.0) turns two neighbouring ones into one v_ashr_pk_u8_i32 and ORs the other two bytes of
// the packed word on top of its result; run on the MI355X, bytes 2 and 3 of exactly those words were bitwise supersets of the
// right values while the emulator and the byte path agreed with the definition.  This form generates no such instruction and is
// bit-identical; whether the instruction's upper result bits or something else was at fault has not been established.
template <int S, class Acc>
__device__ __forceinline__ int clip_shr(Acc v, int top) {
  const Acc hi = (((Acc)top + 1) << S) - 1;
  // each width in the form hipcc compiles best: written with ?: the 8-bit decode grows by 108 instructions (no v_med3_i32), written
  // with min and max the deep decode takes up to 15 more VGPRs
  if constexpr (sizeof(Acc) == 4) v = min(max(v, (Acc)0), hi);
  else v = v < 0 ? 0 : (v > hi ? hi : v);
  return (int)(v >> S);
}

// N samples (a multiple of P::PER) at p, which is N * sizeof(T)-byte aligned: one load of N / PER little-endian words
template <class P, int N>
__device__ __forceinline__ void load_vec(const typename P::T* __restrict__ p, int m, int* o) {
  constexpr int BITS = 32 / P::PER;
  unsigned w[N / P::PER];
  __builtin_memcpy(w, __builtin_assume_aligned(p, sizeof(w)), sizeof(w));
#pragma unroll
  for (int j = 0; j < N; ++j) o[j] = P::sample((int)((w[j / P::PER] >> (BITS * (j % P::PER))) & ((1u << BITS) - 1u)), m);
}

// the same as one store; every v[j] is already clamped to the sample's width
template <class P, int N>
__device__ __forceinline__ void store_vec(typename P::T* __restrict__ p, const int* v) {
  constexpr int BITS = 32 / P::PER;
  unsigned w[N / P::PER] = {};
#pragma unroll
  for (int j = 0; j < N; ++j) w[j / P::PER] |= (unsigned)v[j] << (BITS * (j % P::PER));
  __builtin_memcpy(__builtin_assume_aligned(p, sizeof(w)), w, sizeof(w));
}

// 8 samples row[x0 .. x0 + 7] of a row of n; FAST: one load (in bounds and aligned), else single loads clamped to n - 1
template <class P, bool FAST>
__device__ __forceinline__ void load8(const typename P::T* __restrict__ row, int x0, int n, int m, int (&o)[8]) {
  if (FAST) {
    load_vec<P, 8>(row + x0, m, o);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = P::sample((int)row[min(x0 + j, n - 1)], m);
  }
}

// chroma columns c0 - 1 .. c0 + 4 of a row of n samples, clamped to the row, into o[0 .. 5]
template <class P, bool FAST>
__device__ __forceinline__ void load_c6(const typename P::T* __restrict__ row, int c0, int n, int m, int (&o)[6]) {
  if (FAST) {
    load_vec<P, 4>(row + c0, m, o + 1);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) o[1 + j] = P::sample((int)row[min(c0 + j, n - 1)], m);
  }
  o[0] = P::sample((int)row[max(c0 - 1, 0)], m);
  o[5] = P::sample((int)row[min(c0 + 4, n - 1)], m);
}

// n = 4 or 8 samples, each already clamped, of which the first `valid` exist
template <class P, bool FAST, int N>
__device__ __forceinline__ void store_n(typename P::T* __restrict__ d, const int* v, int valid) {
  if (FAST) {
    store_vec<P, N>(d, v);
  } else {
#pragma unroll
    for (int j = 0; j < N; ++j)
      if (j < valid) d[j] = (typename P::T)v[j];
  }
}

// one chroma plane, 16x (at most 2^20), for the 8 pixels x0 .. x0 + 7 of luma row y
template <class P, class L>
__device__ __forceinline__ void chroma16(const typename P::T* __restrict__ plane, int y, int x0, int Hc, int Wc, int m, int (&o)[8]) {
  if (L::SS == 444) {
    load8<P, L::FAST>(plane + (size_t)y * Wc, x0, Wc, m, o);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] *= 16;
    return;
  }
  int v[6];
  if (L::SS == 420) {
    const int cr = y >> 1, cn = (y & 1) ? min(cr + 1, Hc - 1) : max(cr - 1, 0);
    int a[6];
    load_c6<P, L::FAST>(plane + (size_t)cr * Wc, x0 >> 1, Wc, m, v);
    load_c6<P, L::FAST>(plane + (size_t)cn * Wc, x0 >> 1, Wc, m, a);
#pragma unroll
    for (int j = 0; j < 6; ++j) v[j] = 3 * v[j] + a[j];
  } else {
    load_c6<P, L::FAST>(plane + (size_t)y * Wc, x0 >> 1, Wc, m, v);
#pragma unroll
    for (int j = 0; j < 6; ++j) v[j] *= 4;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {                       // v[k + 1] is the pair's own column
    o[2 * k] = L::SIT == 0 ? 3 * v[k + 1] + v[k] : 4 * v[k + 1];
    o[2 * k + 1] = L::SIT == 0 ? 3 * v[k + 1] + v[k + 2] : 2 * v[k + 1] + 2 * v[k + 2];
  }
}

// a thread's 2 x 8 luma patch (x0, y0; `in` false past the last one) and the chroma planes' shape
template <int SS>
struct Patch {
  int x0, y0, Wc, Hc;
  size_t HW;
  bool in;
  __device__ __forceinline__ Patch(int H, int W) {
    const int PW = (W + 7) >> 3, PH = (H + 1) >> 1;
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    in = g < (long long)PW * PH;
    x0 = (int)(g % PW) * 8, y0 = (int)(g / PW) * 2;
    Wc = SS == 444 ? W : W >> 1, Hc = SS == 420 ? H >> 1 : H;
    HW = (size_t)H * W;
  }
};

// payload -> planar fp32 [3][H*W] (F32 true: P::value of each level) or, 8 bits only, uint8 [H][W][3] (F32 false)
template <class P, class L, bool F32>
__global__ void __launch_bounds__(256) yuv_decode_kernel(const typename P::T* __restrict__ src, void* __restrict__ dstv, int H, int W,
                                                         typename P::Dec k, const float* __restrict__ lut) {
  typedef typename P::Acc Acc;
  __shared__ float sl[256];                           // read by P::value of the 8-bit fp32 decode alone
  if (F32 && P::LUT) {
    sl[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
  }
  const Patch<L::SS> p(H, W);
  if (!p.in) return;
  const int x0 = p.x0, m = P::top(k), mid16 = P::mid16(k);
  const typename P::T* pu = src + p.HW;
  const typename P::T* pv = pu + (size_t)p.Hc * p.Wc;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int y = p.y0 + r;
    if (y >= H) break;
    int Y[8], U[8], V[8];
    typename P::Out c[24];
    load8<P, L::FAST>(src + (size_t)y * W, x0, W, m, Y);
    chroma16<P, L>(pu, y, x0, p.Hc, p.Wc, m, U);
    chroma16<P, L>(pv, y, x0, p.Hc, p.Wc, m, V);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const Acc ya = mul<P>(k.cy, 16 * (Y[j] - k.yo)) + ((Acc)1 << (P::S + 3));
      const int u = U[j] - mid16, v = V[j] - mid16;
      c[3 * j] = P::out(clip_shr<P::S + 4>(ya + mul<P>(k.crv, v), P::LMAX));
      c[3 * j + 1] = P::out(clip_shr<P::S + 4>(ya - mul<P>(k.cgu, u) - mul<P>(k.cgv, v), P::LMAX));
      c[3 * j + 2] = P::out(clip_shr<P::S + 4>(ya + mul<P>(k.cbu, u), P::LMAX));
    }
    const size_t at = (size_t)y * W + x0;
    if constexpr (F32) {
      float* d = static_cast<float*>(dstv) + at;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch, d += p.HW) {
        const auto f = [&](int j) { return P::value(c[3 * j + ch], sl); };
        if (L::FAST) {
          reinterpret_cast<float4*>(d)[0] = make_float4(f(0), f(1), f(2), f(3));
          reinterpret_cast<float4*>(d)[1] = make_float4(f(4), f(5), f(6), f(7));
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (x0 + j < W) d[j] = f(j);
        }
      }
    } else {
      unsigned char* d = static_cast<unsigned char*>(dstv) + at * 3;
      if (L::FAST) {                                  // 24 bytes at a multiple of 24: three 8-byte stores
#pragma unroll
        for (int q = 0; q < 3; ++q) store_vec<Px8, 8>(d + 8 * q, c + 8 * q);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (x0 + j < W) d[3 * j] = (unsigned char)c[3 * j], d[3 * j + 1] = (unsigned char)c[3 * j + 1], d[3 * j + 2] = (unsigned char)c[3 * j + 2];
      }
    }
  }
}

// 8 quantised levels of plane row `row` (W floats) at x0 .. x0 + 7, and the level left of them (column x0 - 1, clamped to 0)
template <class P, bool FAST, bool LEFT>
__device__ __forceinline__ void load_q8(const float* __restrict__ row, int x0, int W, int (&o)[8], int& left) {
  if (FAST) {
    const float4 a = reinterpret_cast<const float4*>(row + x0)[0], b = reinterpret_cast<const float4*>(row + x0)[1];
    o[0] = P::quant(a.x), o[1] = P::quant(a.y), o[2] = P::quant(a.z), o[3] = P::quant(a.w);
    o[4] = P::quant(b.x), o[5] = P::quant(b.y), o[6] = P::quant(b.z), o[7] = P::quant(b.w);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = P::quant(row[min(x0 + j, W - 1)]);
  }
  left = LEFT ? (x0 > 0 ? P::quant(row[x0 - 1]) : o[0]) : 0;
}

// planar fp32 [3][H*W] -> payload: the quantisation to levels and the conversion in one pass
template <class P, class L>
__global__ void __launch_bounds__(256) yuv_encode_kernel(const float* __restrict__ src, typename P::T* __restrict__ dst, int H, int W,
                                                         typename P::Enc k) {
  typedef typename P::Acc Acc;
  constexpr int SS = L::SS, S = P::S;
  const Patch<SS> p(H, W);
  if (!p.in) return;
  const int x0 = p.x0, m = P::top(k);
  typename P::T* du = dst + p.HW;
  typename P::T* dv = du + (size_t)p.Hc * p.Wc;
  constexpr bool LEFT = SS != 444 && L::SIT == 1;
  constexpr int NS = SS == 444 ? 8 : 4;               // chroma samples per patch row
  constexpr int SH = (SS == 444 ? 0 : (L::SIT == 0 ? 1 : 2)) + (SS == 420 ? 1 : 0);
  const Acc ybias = ((Acc)k.yo << S) + ((Acc)1 << (S - 1)), cbias = ((Acc)P::mid(k) << (S + SH)) + ((Acc)1 << (S - 1 + SH));
  int s[3][NS];                                       // footprint sums (at most 2^20), kept across the two rows for 4:2:0
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int y = p.y0 + r;
    if (y >= H) break;
    int q[3][8], left[3], Y[8];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) load_q8<P, L::FAST, LEFT>(src + ch * p.HW + (size_t)y * W, x0, W, q[ch], left[ch]);
#pragma unroll
    for (int j = 0; j < 8; ++j) Y[j] = clip_shr<S>(mul<P>(k.cyr, q[0][j]) + mul<P>(k.cyg, q[1][j]) + mul<P>(k.cyb, q[2][j]) + ybias, m);
    store_n<P, L::FAST, 8>(dst + (size_t)y * W + x0, Y, W - x0);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
#pragma unroll
      for (int n = 0; n < NS; ++n) {
        int v;
        if (SS == 444) v = q[ch][n];
        else if (!LEFT) v = q[ch][2 * n] + q[ch][2 * n + 1];
        else v = (n == 0 ? left[ch] : q[ch][2 * n - 1]) + 2 * q[ch][2 * n] + q[ch][2 * n + 1];
        s[ch][n] = (SS == 420 && r == 1) ? s[ch][n] + v : v;
      }
    }
    if (SS == 420 && r == 0) continue;                // H is even: the second row follows
    int U[NS], V[NS];
#pragma unroll
    for (int n = 0; n < NS; ++n) {
      U[n] = clip_shr<S + SH>(mul<P>(k.cur, s[0][n]) + mul<P>(k.cug, s[1][n]) + mul<P>(k.cub, s[2][n]) + cbias, m);
      V[n] = clip_shr<S + SH>(mul<P>(k.cvr, s[0][n]) + mul<P>(k.cvg, s[1][n]) + mul<P>(k.cvb, s[2][n]) + cbias, m);
    }
    const int cy = SS == 420 ? y >> 1 : y, cx = SS == 444 ? x0 : x0 >> 1;
    store_n<P, L::FAST, NS>(du + (size_t)cy * p.Wc + cx, U, p.Wc - cx);
    store_n<P, L::FAST, NS>(dv + (size_t)cy * p.Wc + cx, V, p.Wc - cx);
  }
}

bool yuv_args_ok(int H, int W, int ss, int siting) {
  if (H <= 0 || W <= 0 || (siting != 0 && siting != 1)) return false;
  if (ss == 444) return siting == 0;
  if (ss == 422) return W % 2 == 0;
  return ss == 420 && W % 2 == 0 && H % 2 == 0;
}

bool deep_ok(int depth) { return depth == 9 || depth == 10 || depth == 12 || depth == 14 || depth == 16; }

// the table's entries as the 32-bit factors the kernels multiply with; the offset (entry 0) must lie in 0..m
bool narrow(const long long* c, int n, int m, int* o) {
  for (int i = 0; i < n; ++i) {
    if (c[i] < -0x7fffffffLL || c[i] > 0x7fffffffLL) return false;
    o[i] = (int)c[i];
  }
  return o[0] >= 0 && o[0] <= m;
}

// one launch over the frame's patches: `launch(Layout, grid, block)` for the frame's (subsampling, siting), FAST with W % 8 == 0 and
// both pointers 16-byte aligned
template <class F>
int yuv_launch(const void* src, const void* dst, int H, int W, int ss, int siting, hipStream_t stream, F launch) {
  const bool fast = W % 8 == 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0;
  const dim3 grid((unsigned)zt_cdivl((long long)((W + 7) >> 3) * ((H + 1) >> 1), 256)), block(256);
#define ZT_LAYOUT(SS, SIT) (fast ? launch(Layout<SS, SIT, true>(), grid, block) : launch(Layout<SS, SIT, false>(), grid, block))
  if (ss == 444) ZT_LAYOUT(444, 0);
  else if (ss == 422 && siting == 0) ZT_LAYOUT(422, 0);
  else if (ss == 422) ZT_LAYOUT(422, 1);
  else if (siting == 0) ZT_LAYOUT(420, 0);
  else ZT_LAYOUT(420, 1);
#undef ZT_LAYOUT
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}

template <class P, bool F32>
int yuv_decode(const typename P::T* src, void* dst, int H, int W, int ss, int siting, typename P::Dec k, const float* lut, hipStream_t stream) {
  return yuv_launch(src, dst, H, W, ss, siting, stream, [=](auto l, dim3 grid, dim3 block) {
    hipLaunchKernelGGL((yuv_decode_kernel<P, decltype(l), F32>), grid, block, 0, stream, src, dst, H, W, k, lut);
  });
}

template <class P>
int yuv_encode(const float* src, typename P::T* dst, int H, int W, int ss, int siting, typename P::Enc k, hipStream_t stream) {
  return yuv_launch(src, dst, H, W, ss, siting, stream, [=](auto l, dim3 grid, dim3 block) {
    hipLaunchKernelGGL((yuv_encode_kernel<P, decltype(l)>), grid, block, 0, stream, src, dst, H, W, k);
  });
}

}  // namespace

extern "C" int zt_yuv_to_rgb_u8(const unsigned char* src, unsigned char* dst, int H, int W, int ss, int siting, const int* coef,
                                hipStream_t stream) {
  ZT_REQUIRE(src && dst && coef && yuv_args_ok(H, W, ss, siting));
  return yuv_decode<Px8, false>(src, dst, H, W, ss, siting, {coef[0], coef[1], coef[2], coef[3], coef[4], coef[5]}, nullptr, stream);
}

extern "C" int zt_yuv_to_planar_f32(const unsigned char* src, float* dst, int H, int W, int ss, int siting, const int* coef,
                                    const float* lut256, hipStream_t stream) {
  ZT_REQUIRE(src && dst && coef && lut256 && yuv_args_ok(H, W, ss, siting) && ((uintptr_t)dst & 3) == 0);
  return yuv_decode<Px8, true>(src, dst, H, W, ss, siting, {coef[0], coef[1], coef[2], coef[3], coef[4], coef[5]}, lut256, stream);
}

extern "C" int zt_rgb_f32_to_yuv(const float* src, unsigned char* dst, int H, int W, int ss, int siting, const int* coef,
                                 hipStream_t stream) {
  ZT_REQUIRE(src && dst && coef && yuv_args_ok(H, W, ss, siting) && ((uintptr_t)src & 3) == 0);
  return yuv_encode<Px8>(src, dst, H, W, ss, siting, {coef[0], coef[1], coef[2], coef[3], coef[4], coef[5], coef[6], coef[7], coef[8], coef[9]},
                         stream);
}

extern "C" int zt_yuv16_to_planar_f32(const uint16_t* src, float* dst, int H, int W, int ss, int siting, int depth, const long long* coef,
                                      hipStream_t stream) {
  ZT_REQUIRE(src && dst && coef && yuv_args_ok(H, W, ss, siting) && deep_ok(depth) && ((uintptr_t)src & 1) == 0 && ((uintptr_t)dst & 3) == 0);
  const int m = (1 << depth) - 1;
  int c[6];
  ZT_REQUIRE(narrow(coef, 6, m, c));
  return yuv_decode<PxDeep, true>(src, dst, H, W, ss, siting, {{c[0], c[1], c[2], c[3], c[4], c[5]}, m, 16 << (depth - 1)}, nullptr, stream);
}

extern "C" int zt_rgb_f32_to_yuv16(const float* src, uint16_t* dst, int H, int W, int ss, int siting, int depth, const long long* coef,
                                   hipStream_t stream) {
  ZT_REQUIRE(src && dst && coef && yuv_args_ok(H, W, ss, siting) && deep_ok(depth) && ((uintptr_t)src & 3) == 0 && ((uintptr_t)dst & 1) == 0);
  const int m = (1 << depth) - 1;
  int c[10];
  ZT_REQUIRE(narrow(coef, 10, m, c));
  return yuv_encode<PxDeep>(src, dst, H, W, ss, siting, {{c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], c[9]}, m, 1 << (depth - 1)},
                            stream);
}
