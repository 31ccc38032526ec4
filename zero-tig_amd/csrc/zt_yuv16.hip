// High-bit-depth raw video in and out of predict.py (--y4m_in with C420p10 ... C444p16, --y4m_out_depth): planar Y'CbCr of
// B = 9, 10, 12, 14 or 16 bits <-> RGB with chroma resampling, on the device.  A frame is the YUV4MPEG2 payload: plane Y [H][W],
// then U, then V (shapes as for 8 bits), contiguous little-endian uint16 with the value in the low B bits; a sample above
// m = 2^B - 1 is read as m.  Subsampling, siting, tap tables and footprints are those of zt_yuv.hip; the arithmetic
// is DESIGN 8f: integer and fixed, coefficients round(c 2^20), 16-bit RGB levels, int64 accumulators (peak about 2^41):
//   decode  y = 16 CY (min(Y, m) - yo), u = U16 - 16 mid, v = V16 - 16 mid (U16, V16: chroma at full resolution, 16x),
//           R16 = clip16((y + CRV v + 2^23) >> 24), G16 = clip16((y - CGU u - CGV v + 2^23) >> 24), B16 = clip16((y + CBU u + 2^23) >> 24),
//           value = float(L16) / 65535.f (an IEEE division)
//   encode  L16 = x > 0 ? (x < 1 ? (int)(x * 65535.f + 0.5f) : 65535) : 0 (NaN -> 0; a float32 multiply, then a float32 add),
//           Y = yo + ((CYR R + CYG G + CYB B + 2^19) >> 20), U = mid + ((CUR Rs + CUG Gs + CUB Bs + 2^(19 + sh)) >> (20 + sh)), V alike,
//           every plane clipped to 0..m; Rs, Gs, Bs are the footprint sums of the 16-bit levels.
// The coefficients (matrix, range and depth folded in) are computed by the host in double precision (zero-tig_amd/y4m.py) and
// travel as kernel arguments: no colour constant lives here.  They arrive as 64-bit values, every one of them fits 32 bits (the
// largest, CBU at 9 bits, is below 2^29), and every other factor is below 2^21, so each product is one 32 x 32 -> 64 bit multiply.
// Kernel shape as zt_yuv.hip: a thread owns a 2 x 8 luma patch, so every chroma sample is loaded (decode) or made (encode) once;
// with W % 8 == 0 and 16-byte aligned pointers luma is one 16-byte access per patch row and chroma 8 or 16 bytes, any other width
// takes 2-byte accesses with the same arithmetic.  No atomics, no LDS.
// Every result is clamped BEFORE its shift (the offset folded into the accumulator), and packed words are built as lo | (hi << 16)
// from values already clamped to 16 bits: the packing note at clip8_shr18 in zt_yuv.hip.
// zt_luma_grid_u16 is the grid pass of zt_scene.hip over min(Y, m) >> (B - 8).
#include "zt_common.h"

namespace {

typedef long long i64;

struct DecCoef16 { int yo, cy, crv, cgu, cgv, cbu, m, mid16; };
struct EncCoef16 { int yo, cyr, cyg, cyb, cur, cug, cub, cvr, cvg, cvb, m, mid; };

__device__ __forceinline__ i64 mul64(int a, int b) { return (i64)a * (i64)b; }

// clip(v >> S, 0, top), clamped before the shift
template <int S>
__device__ __forceinline__ int clip_shr(i64 v, int top) {
  const i64 hi = (((i64)top + 1) << S) - 1;
  v = v < 0 ? 0 : (v > hi ? hi : v);
  return (int)(v >> S);
}

__device__ __forceinline__ void unpack2(unsigned w, int m, int* o) { o[0] = min((int)(w & 0xffffu), m), o[1] = min((int)(w >> 16), m); }

// both arguments are in 0..65535
__device__ __forceinline__ unsigned pack2(int lo, int hi) { return (unsigned)lo | ((unsigned)hi << 16); }

// 8 samples row[x0 .. x0 + 7] of a row of n; FAST: one 16-byte load (in bounds and aligned), else 2-byte loads clamped to n - 1
template <bool FAST>
__device__ __forceinline__ void load8(const unsigned short* __restrict__ row, int x0, int n, int m, int (&o)[8]) {
  if (FAST) {
    const uint4 w = *reinterpret_cast<const uint4*>(row + x0);
    unpack2(w.x, m, o), unpack2(w.y, m, o + 2), unpack2(w.z, m, o + 4), unpack2(w.w, m, o + 6);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = min((int)row[min(x0 + j, n - 1)], m);
  }
}

// chroma columns c0 - 1 .. c0 + 4 of a row of n samples, clamped to the row, into o[0 .. 5]
template <bool FAST>
__device__ __forceinline__ void load_c6(const unsigned short* __restrict__ row, int c0, int n, int m, int (&o)[6]) {
  if (FAST) {
    const uint2 w = *reinterpret_cast<const uint2*>(row + c0);
    unpack2(w.x, m, o + 1), unpack2(w.y, m, o + 3);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) o[1 + j] = min((int)row[min(c0 + j, n - 1)], m);
  }
  o[0] = min((int)row[max(c0 - 1, 0)], m);
  o[5] = min((int)row[min(c0 + 4, n - 1)], m);
}

// one chroma plane, 16x (at most 2^20), for the 8 pixels x0 .. x0 + 7 of luma row y
template <int SS, int SIT, bool FAST>
__device__ __forceinline__ void chroma16(const unsigned short* __restrict__ plane, int y, int x0, int Hc, int Wc, int m, int (&o)[8]) {
  if (SS == 444) {
    load8<FAST>(plane + (size_t)y * Wc, x0, Wc, m, o);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] *= 16;
    return;
  }
  int v[6];
  if (SS == 420) {
    const int cr = y >> 1, cn = (y & 1) ? min(cr + 1, Hc - 1) : max(cr - 1, 0);
    int a[6];
    load_c6<FAST>(plane + (size_t)cr * Wc, x0 >> 1, Wc, m, v);
    load_c6<FAST>(plane + (size_t)cn * Wc, x0 >> 1, Wc, m, a);
#pragma unroll
    for (int j = 0; j < 6; ++j) v[j] = 3 * v[j] + a[j];
  } else {
    load_c6<FAST>(plane + (size_t)y * Wc, x0 >> 1, Wc, m, v);
#pragma unroll
    for (int j = 0; j < 6; ++j) v[j] *= 4;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {                       // v[k + 1] is the pair's own column
    o[2 * k] = SIT == 0 ? 3 * v[k + 1] + v[k] : 4 * v[k + 1];
    o[2 * k + 1] = SIT == 0 ? 3 * v[k + 1] + v[k + 2] : 2 * v[k + 1] + 2 * v[k + 2];
  }
}

// payload -> planar fp32 [3][H*W]
template <int SS, int SIT, bool FAST>
__global__ void __launch_bounds__(256) yuv16_decode_kernel(const unsigned short* __restrict__ src, float* __restrict__ dst, int H, int W,
                                                           DecCoef16 k) {
  const int PW = (W + 7) >> 3, PH = (H + 1) >> 1;
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= (long long)PW * PH) return;
  const int x0 = (int)(g % PW) * 8, y0 = (int)(g / PW) * 2;
  const int Wc = SS == 444 ? W : W >> 1, Hc = SS == 420 ? H >> 1 : H;
  const size_t HW = (size_t)H * W;
  const unsigned short* pu = src + HW;
  const unsigned short* pv = pu + (size_t)Hc * Wc;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int y = y0 + r;
    if (y >= H) break;
    int Y[8], U[8], V[8];
    float c[3][8];
    load8<FAST>(src + (size_t)y * W, x0, W, k.m, Y);
    chroma16<SS, SIT, FAST>(pu, y, x0, Hc, Wc, k.m, U);
    chroma16<SS, SIT, FAST>(pv, y, x0, Hc, Wc, k.m, V);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const i64 ya = mul64(k.cy, 16 * (Y[j] - k.yo)) + ((i64)1 << 23);
      const int u = U[j] - k.mid16, v = V[j] - k.mid16;
      c[0][j] = (float)clip_shr<24>(ya + mul64(k.crv, v), 65535) / 65535.f;
      c[1][j] = (float)clip_shr<24>(ya - mul64(k.cgu, u) - mul64(k.cgv, v), 65535) / 65535.f;
      c[2][j] = (float)clip_shr<24>(ya + mul64(k.cbu, u), 65535) / 65535.f;
    }
    float* d = dst + (size_t)y * W + x0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch, d += HW) {
      if (FAST) {
        reinterpret_cast<float4*>(d)[0] = make_float4(c[ch][0], c[ch][1], c[ch][2], c[ch][3]);
        reinterpret_cast<float4*>(d)[1] = make_float4(c[ch][4], c[ch][5], c[ch][6], c[ch][7]);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (x0 + j < W) d[j] = c[ch][j];
      }
    }
  }
}

__device__ __forceinline__ int quant16(float x) { return x > 0.f ? (x < 1.f ? (int)(x * 65535.f + 0.5f) : 65535) : 0; }

// 8 quantised 16-bit levels of plane row `row` (W floats) at x0 .. x0 + 7, and the level left of them (column x0 - 1, clamped to 0)
template <bool FAST, bool LEFT>
__device__ __forceinline__ void load_q8(const float* __restrict__ row, int x0, int W, int (&o)[8], int& left) {
  if (FAST) {
    const float4 a = reinterpret_cast<const float4*>(row + x0)[0], b = reinterpret_cast<const float4*>(row + x0)[1];
    o[0] = quant16(a.x), o[1] = quant16(a.y), o[2] = quant16(a.z), o[3] = quant16(a.w);
    o[4] = quant16(b.x), o[5] = quant16(b.y), o[6] = quant16(b.z), o[7] = quant16(b.w);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = quant16(row[min(x0 + j, W - 1)]);
  }
  left = LEFT ? (x0 > 0 ? quant16(row[x0 - 1]) : o[0]) : 0;
}

// n = 4 or 8 samples, each already clamped to 0..m
template <bool FAST>
__device__ __forceinline__ void store_u16(unsigned short* __restrict__ d, const int* v, int n, int valid) {
  if (FAST) {
    if (n == 8) {
      uint4 w;
      w.x = pack2(v[0], v[1]), w.y = pack2(v[2], v[3]), w.z = pack2(v[4], v[5]), w.w = pack2(v[6], v[7]);
      *reinterpret_cast<uint4*>(d) = w;
    } else {
      uint2 w;
      w.x = pack2(v[0], v[1]), w.y = pack2(v[2], v[3]);
      *reinterpret_cast<uint2*>(d) = w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j < n && j < valid) d[j] = (unsigned short)v[j];
  }
}

// planar fp32 [3][H*W] -> payload: the 16-bit quantisation and the conversion in one pass
template <int SS, int SIT, bool FAST>
__global__ void __launch_bounds__(256) yuv16_encode_kernel(const float* __restrict__ src, unsigned short* __restrict__ dst, int H, int W,
                                                           EncCoef16 k) {
  const int PW = (W + 7) >> 3, PH = (H + 1) >> 1;
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= (long long)PW * PH) return;
  const int x0 = (int)(g % PW) * 8, y0 = (int)(g / PW) * 2;
  const int Wc = SS == 444 ? W : W >> 1, Hc = SS == 420 ? H >> 1 : H;
  const size_t HW = (size_t)H * W;
  unsigned short* du = dst + HW;
  unsigned short* dv = du + (size_t)Hc * Wc;
  constexpr bool LEFT = SS != 444 && SIT == 1;
  constexpr int NS = SS == 444 ? 8 : 4;               // chroma samples per patch row
  constexpr int SH = (SS == 444 ? 0 : (SIT == 0 ? 1 : 2)) + (SS == 420 ? 1 : 0);
  const i64 ybias = ((i64)k.yo << 20) + ((i64)1 << 19), cbias = ((i64)k.mid << (20 + SH)) + ((i64)1 << (19 + SH));
  int s[3][NS];                                       // footprint sums (at most 2^20), kept across the two rows for 4:2:0
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int y = y0 + r;
    if (y >= H) break;
    int q[3][8], left[3], Y[8];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) load_q8<FAST, LEFT>(src + ch * HW + (size_t)y * W, x0, W, q[ch], left[ch]);
#pragma unroll
    for (int j = 0; j < 8; ++j) Y[j] = clip_shr<20>(mul64(k.cyr, q[0][j]) + mul64(k.cyg, q[1][j]) + mul64(k.cyb, q[2][j]) + ybias, k.m);
    store_u16<FAST>(dst + (size_t)y * W + x0, Y, 8, W - x0);
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
      U[n] = clip_shr<20 + SH>(mul64(k.cur, s[0][n]) + mul64(k.cug, s[1][n]) + mul64(k.cub, s[2][n]) + cbias, k.m);
      V[n] = clip_shr<20 + SH>(mul64(k.cvr, s[0][n]) + mul64(k.cvg, s[1][n]) + mul64(k.cvb, s[2][n]) + cbias, k.m);
    }
    const int cy = SS == 420 ? y >> 1 : y, cx = SS == 444 ? x0 : x0 >> 1;
    store_u16<FAST>(du + (size_t)cy * Wc + cx, U, NS, Wc - cx);
    store_u16<FAST>(dv + (size_t)cy * Wc + cx, V, NS, Wc - cx);
  }
}

constexpr int CELL = 16;

// the two 8-bit levels of a packed pair, each less yo8 and floored at 0, summed
__device__ __forceinline__ unsigned relu_sum2(unsigned w, int m, int sh, int yo) {
  return (unsigned)(max((min((int)(w & 0xffffu), m) >> sh) - yo, 0) + max((min((int)(w >> 16), m) >> sh) - yo, 0));
}

__device__ __forceinline__ unsigned relu_sum8(uint4 v, int m, int sh, int yo) {
  return relu_sum2(v.x, m, sh, yo) + relu_sum2(v.y, m, sh, yo) + relu_sum2(v.z, m, sh, yo) + relu_sum2(v.w, m, sh, yo);
}

// a lane per cell as luma_grid_kernel of zt_scene.hip; a whole cell is 32 loads of 16 bytes, issued as two batches of 8 rows
template <bool VEC>
__global__ void __launch_bounds__(64) luma_grid16_kernel(const unsigned short* __restrict__ y, int H, int W, int m, int sh, int yo, int gh,
                                                         int gw, unsigned* __restrict__ grid) {
  const int g = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (g >= gh * gw) return;
  const int r0 = (g / gw) * CELL, c0 = (g % gw) * CELL;
  const unsigned short* p = y + (size_t)r0 * W + c0;
  unsigned s = 0;
  if (VEC && r0 + CELL <= H) {                       // W % 16 == 0: the cell is whole
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      uint4 v[CELL];
#pragma unroll
      for (int i = 0; i < CELL; ++i) v[i] = *reinterpret_cast<const uint4*>(p + (size_t)(8 * half + (i >> 1)) * W + 8 * (i & 1));
      __builtin_amdgcn_sched_barrier(0);             // the batch's 16 loads in flight before the first add
#pragma unroll
      for (int i = 0; i < CELL; ++i) s += relu_sum8(v[i], m, sh, yo);
    }
  } else {
    const int nr = min(CELL, H - r0), nc = min(CELL, W - c0);
    for (int r = 0; r < nr; ++r)
      for (int c = 0; c < nc; ++c) s += (unsigned)max((min((int)p[(size_t)r * W + c], m) >> sh) - yo, 0);
  }
  grid[g] = s;
}

bool yuv16_args_ok(int H, int W, int ss, int siting, int depth) {
  if (depth != 9 && depth != 10 && depth != 12 && depth != 14 && depth != 16) return false;
  if (H <= 0 || W <= 0 || (siting != 0 && siting != 1)) return false;
  if (ss == 444) return siting == 0;
  if (ss == 422) return W % 2 == 0;
  return ss == 420 && W % 2 == 0 && H % 2 == 0;
}

// the table's entries as the 32-bit factors the kernels multiply with; the offset (entry 0) must lie in 0..m
bool narrow(const long long* c, int n, int m, int* o) {
  for (int i = 0; i < n; ++i) {
    if (c[i] < -0x7fffffffLL || c[i] > 0x7fffffffLL) return false;
    o[i] = (int)c[i];
  }
  return o[0] >= 0 && o[0] <= m;
}

unsigned yuv16_blocks(int H, int W) { return (unsigned)zt_cdivl((long long)((W + 7) >> 3) * ((H + 1) >> 1), 256); }

}  // namespace

extern "C" int zt_yuv16_to_planar_f32(const uint16_t* src, float* dst, int H, int W, int ss, int siting, int depth, const long long* coef,
                                      hipStream_t stream) {
  ZT_REQUIRE(src && dst && coef && yuv16_args_ok(H, W, ss, siting, depth) && ((uintptr_t)src & 1) == 0 && ((uintptr_t)dst & 3) == 0);
  const int m = (1 << depth) - 1;
  int c[6];
  ZT_REQUIRE(narrow(coef, 6, m, c));
  const DecCoef16 k = {c[0], c[1], c[2], c[3], c[4], c[5], m, 16 << (depth - 1)};
  const bool fast = W % 8 == 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0;
  const dim3 grid(yuv16_blocks(H, W)), block(256);
#define ZT_DEC16(SS, SIT)                                                                                              \
  do {                                                                                                                 \
    if (fast) hipLaunchKernelGGL((yuv16_decode_kernel<SS, SIT, true>), grid, block, 0, stream, src, dst, H, W, k);      \
    else hipLaunchKernelGGL((yuv16_decode_kernel<SS, SIT, false>), grid, block, 0, stream, src, dst, H, W, k);          \
  } while (0)
  if (ss == 444) ZT_DEC16(444, 0);
  else if (ss == 422 && siting == 0) ZT_DEC16(422, 0);
  else if (ss == 422) ZT_DEC16(422, 1);
  else if (siting == 0) ZT_DEC16(420, 0);
  else ZT_DEC16(420, 1);
#undef ZT_DEC16
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}

extern "C" int zt_rgb_f32_to_yuv16(const float* src, uint16_t* dst, int H, int W, int ss, int siting, int depth, const long long* coef,
                                   hipStream_t stream) {
  ZT_REQUIRE(src && dst && coef && yuv16_args_ok(H, W, ss, siting, depth) && ((uintptr_t)src & 3) == 0 && ((uintptr_t)dst & 1) == 0);
  const int m = (1 << depth) - 1;
  int c[10];
  ZT_REQUIRE(narrow(coef, 10, m, c));
  const EncCoef16 k = {c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], c[9], m, 1 << (depth - 1)};
  const bool fast = W % 8 == 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0;
  const dim3 grid(yuv16_blocks(H, W)), block(256);
#define ZT_ENC16(SS, SIT)                                                                                              \
  do {                                                                                                                 \
    if (fast) hipLaunchKernelGGL((yuv16_encode_kernel<SS, SIT, true>), grid, block, 0, stream, src, dst, H, W, k);      \
    else hipLaunchKernelGGL((yuv16_encode_kernel<SS, SIT, false>), grid, block, 0, stream, src, dst, H, W, k);          \
  } while (0)
  if (ss == 444) ZT_ENC16(444, 0);
  else if (ss == 422 && siting == 0) ZT_ENC16(422, 0);
  else if (ss == 422) ZT_ENC16(422, 1);
  else if (siting == 0) ZT_ENC16(420, 0);
  else ZT_ENC16(420, 1);
#undef ZT_ENC16
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}

extern "C" int zt_luma_grid_u16(const uint16_t* y, int H, int W, int depth, int yo8, unsigned int* grid, hipStream_t stream) {
  ZT_REQUIRE(y && grid && H > 0 && W > 0 && yo8 >= 0 && yo8 <= 255 && ((uintptr_t)y & 1) == 0 && ((uintptr_t)grid & 3) == 0);
  ZT_REQUIRE(depth == 9 || depth == 10 || depth == 12 || depth == 14 || depth == 16);
  const int gh = zt_cdiv(H, CELL), gw = zt_cdiv(W, CELL), m = (1 << depth) - 1, sh = depth - 8;
  ZT_REQUIRE((long long)gh * gw <= 0x7fffffffLL - 64);
  const dim3 blocks((unsigned)zt_cdiv(gh * gw, 64)), block(64);
  if (W % 16 == 0 && ((uintptr_t)y & 15) == 0) hipLaunchKernelGGL(luma_grid16_kernel<true>, blocks, block, 0, stream, y, H, W, m, sh, yo8, gh, gw, grid);
  else hipLaunchKernelGGL(luma_grid16_kernel<false>, blocks, block, 0, stream, y, H, W, m, sh, yo8, gh, gw, grid);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}
