// Raw video in and out of predict.py (--y4m_in / --y4m_out): 8-bit planar Y'CbCr <-> RGB with chroma resampling, on the device.
// A frame is the YUV4MPEG2 payload: plane Y [H][W], then U, then V ([H/2][W/2] for 4:2:0, [H][W/2] for 4:2:2, [H][W] for 4:4:4),
// contiguous uint8.  The arithmetic is integer and fixed, so the result is the same on every machine:
//   decode  chroma upsampled to full resolution as an integer carrying a factor of 16 (horizontal weights sum to 4: centre siting
//           (3, 1) towards the nearer neighbour, left siting 4 / (2, 2); vertical weights (3, 1) for 4:2:0, 4 otherwise; clamped
//           at the plane's edges), y = 16 CY (Y - yo), u = U16 - 2048, v = V16 - 2048,
//           R = clip8((y + CRV v + 2^17) >> 18), G = clip8((y - CGU u - CGV v + 2^17) >> 18), B = clip8((y + CBU u + 2^17) >> 18)
//   encode  Y = yo + ((CYR R + CYG G + CYB B + 2^13) >> 14); chroma from the integer RGB sums over the sample's footprint (box for
//           centre siting, [1, 2, 1] for left siting, both rows for 4:2:0; weight total 2^sh):
//           U = 128 + ((CUR Rs + CUG Gs + CUB Bs + 2^(13 + sh)) >> (14 + sh)), V alike; everything clipped to 0..255.
// The coefficients (round(c 2^14), matrix and range folded in) are computed by the host in double precision (zero-tig_amd/y4m.py)
// and travel as kernel arguments: no colour constant lives here.
// Byte kernels of a few MB, HBM-bound: a thread owns a 2 x 8 luma patch, so every chroma sample is loaded (decode) or made
// (encode) once; with W % 8 == 0 every access is 4, 8 or 16 bytes wide along the row, any other width takes byte accesses with
// the same arithmetic.  No atomics, no scratch; the only LDS is the 256-entry ToTensor table of the fused decode.
#include "zt_common.h"

namespace {

struct DecCoef { int yo, cy, crv, cgu, cgv, cbu; };
struct EncCoef { int yo, cyr, cyg, cyb, cur, cug, cub, cvr, cvg, cvb; };

__device__ __forceinline__ int clip255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// clip8(v >> 18), clamped BEFORE the shift.  An observation, not a diagnosed cause: written as shift-then-clamp, hipcc (HIP
// 7.2.26015, AMD clang 22.0.0git roc-7.2.0) turns two neighbouring ones into one v_ashr_pk_u8_i32 and ORs the other two bytes of
// the packed word on top of its result; run on the MI355X, bytes 2 and 3 of exactly those words were bitwise supersets of the
// right values while the emulator and the byte path agreed with the definition.  This form generates no such instruction and is
// bit-identical; whether the instruction's upper result bits or something else was at fault has not been established.
__device__ __forceinline__ int clip8_shr18(int v) { return (int)((unsigned)min(max(v, 0), (256 << 18) - 1) >> 18); }

__device__ __forceinline__ void unpack4(unsigned w, int* o) {
  o[0] = (int)(w & 255u), o[1] = (int)((w >> 8) & 255u), o[2] = (int)((w >> 16) & 255u), o[3] = (int)(w >> 24);
}

__device__ __forceinline__ unsigned pack4(int a, int b, int c, int d) {
  return (unsigned)a | ((unsigned)b << 8) | ((unsigned)c << 16) | ((unsigned)d << 24);
}

// 8 bytes row[x0 .. x0 + 7] of a row of n bytes; FAST: one 8-byte load (in bounds and aligned), else byte loads clamped to n - 1
template <bool FAST>
__device__ __forceinline__ void load8(const unsigned char* __restrict__ row, int x0, int n, int (&o)[8]) {
  if (FAST) {
    const uint2 w = *reinterpret_cast<const uint2*>(row + x0);
    unpack4(w.x, o), unpack4(w.y, o + 4);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (int)row[min(x0 + j, n - 1)];
  }
}

// chroma columns c0 - 1 .. c0 + 4 of a row of n samples, clamped to the row, into o[0 .. 5]
template <bool FAST>
__device__ __forceinline__ void load_c6(const unsigned char* __restrict__ row, int c0, int n, int (&o)[6]) {
  if (FAST) {
    unpack4(*reinterpret_cast<const unsigned*>(row + c0), o + 1);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) o[1 + j] = (int)row[min(c0 + j, n - 1)];
  }
  o[0] = (int)row[max(c0 - 1, 0)];
  o[5] = (int)row[min(c0 + 4, n - 1)];
}

// one chroma plane, 16x, for the 8 pixels x0 .. x0 + 7 of luma row y
template <int SS, int SIT, bool FAST>
__device__ __forceinline__ void chroma16(const unsigned char* __restrict__ plane, int y, int x0, int Hc, int Wc, int (&o)[8]) {
  if (SS == 444) {
    load8<FAST>(plane + (size_t)y * Wc, x0, Wc, o);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] *= 16;
    return;
  }
  int v[6];
  if (SS == 420) {
    const int cr = y >> 1, cn = (y & 1) ? min(cr + 1, Hc - 1) : max(cr - 1, 0);
    int a[6];
    load_c6<FAST>(plane + (size_t)cr * Wc, x0 >> 1, Wc, v);
    load_c6<FAST>(plane + (size_t)cn * Wc, x0 >> 1, Wc, a);
#pragma unroll
    for (int j = 0; j < 6; ++j) v[j] = 3 * v[j] + a[j];
  } else {
    load_c6<FAST>(plane + (size_t)y * Wc, x0 >> 1, Wc, v);
#pragma unroll
    for (int j = 0; j < 6; ++j) v[j] *= 4;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {                       // v[k + 1] is the pair's own column
    o[2 * k] = SIT == 0 ? 3 * v[k + 1] + v[k] : 4 * v[k + 1];
    o[2 * k + 1] = SIT == 0 ? 3 * v[k + 1] + v[k + 2] : 2 * v[k + 1] + 2 * v[k + 2];
  }
}

// payload -> uint8 [H][W][3] (F32 false) or planar fp32 [3][H*W] through the ToTensor table (F32 true)
template <int SS, int SIT, bool F32, bool FAST>
__global__ void __launch_bounds__(256) yuv_decode_kernel(const unsigned char* __restrict__ src, void* __restrict__ dstv, int H, int W,
                                                         DecCoef k, const float* __restrict__ lut) {
  __shared__ float sl[256];
  if (F32) {
    sl[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
  }
  const int PW = (W + 7) >> 3, PH = (H + 1) >> 1;
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= (long long)PW * PH) return;
  const int x0 = (int)(g % PW) * 8, y0 = (int)(g / PW) * 2;
  const int Wc = SS == 444 ? W : W >> 1, Hc = SS == 420 ? H >> 1 : H;
  const size_t HW = (size_t)H * W;
  const unsigned char* pu = src + HW;
  const unsigned char* pv = pu + (size_t)Hc * Wc;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int y = y0 + r;
    if (y >= H) break;
    int Y[8], U[8], V[8], c[24];
    load8<FAST>(src + (size_t)y * W, x0, W, Y);
    chroma16<SS, SIT, FAST>(pu, y, x0, Hc, Wc, U);
    chroma16<SS, SIT, FAST>(pv, y, x0, Hc, Wc, V);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int ya = 16 * k.cy * (Y[j] - k.yo) + (1 << 17), u = U[j] - 2048, v = V[j] - 2048;
      c[3 * j] = clip8_shr18(ya + k.crv * v);
      c[3 * j + 1] = clip8_shr18(ya - k.cgu * u - k.cgv * v);
      c[3 * j + 2] = clip8_shr18(ya + k.cbu * u);
    }
    const size_t p = (size_t)y * W + x0;
    if (F32) {
      float* d = static_cast<float*>(dstv) + p;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch, d += HW) {
        if (FAST) {
          reinterpret_cast<float4*>(d)[0] = make_float4(sl[c[ch]], sl[c[3 + ch]], sl[c[6 + ch]], sl[c[9 + ch]]);
          reinterpret_cast<float4*>(d)[1] = make_float4(sl[c[12 + ch]], sl[c[15 + ch]], sl[c[18 + ch]], sl[c[21 + ch]]);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (x0 + j < W) d[j] = sl[c[3 * j + ch]];
        }
      }
    } else {
      unsigned char* d = static_cast<unsigned char*>(dstv) + p * 3;
      if (FAST) {                                     // 24 bytes at a multiple of 24: three 8-byte stores
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          uint2 w;
          w.x = pack4(c[8 * q], c[8 * q + 1], c[8 * q + 2], c[8 * q + 3]);
          w.y = pack4(c[8 * q + 4], c[8 * q + 5], c[8 * q + 6], c[8 * q + 7]);
          reinterpret_cast<uint2*>(d)[q] = w;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (x0 + j < W) d[3 * j] = (unsigned char)c[3 * j], d[3 * j + 1] = (unsigned char)c[3 * j + 1], d[3 * j + 2] = (unsigned char)c[3 * j + 2];
      }
    }
  }
}

// 8 quantised levels of plane row `row` (W floats) at x0 .. x0 + 7, and the level left of them (column x0 - 1, clamped to 0)
template <bool FAST, bool LEFT>
__device__ __forceinline__ void load_q8(const float* __restrict__ row, int x0, int W, int (&o)[8], int& left) {
  if (FAST) {
    const float4 a = reinterpret_cast<const float4*>(row + x0)[0], b = reinterpret_cast<const float4*>(row + x0)[1];
    o[0] = zt_quant_u8(a.x, 0), o[1] = zt_quant_u8(a.y, 0), o[2] = zt_quant_u8(a.z, 0), o[3] = zt_quant_u8(a.w, 0);
    o[4] = zt_quant_u8(b.x, 0), o[5] = zt_quant_u8(b.y, 0), o[6] = zt_quant_u8(b.z, 0), o[7] = zt_quant_u8(b.w, 0);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = zt_quant_u8(row[min(x0 + j, W - 1)], 0);
  }
  left = LEFT ? (x0 > 0 ? zt_quant_u8(row[x0 - 1], 0) : o[0]) : 0;
}

template <bool FAST>
__device__ __forceinline__ void store_bytes(unsigned char* __restrict__ d, const int* v, int n, int valid) {   // n = 4 or 8
  if (FAST) {
    reinterpret_cast<unsigned*>(d)[0] = pack4(v[0], v[1], v[2], v[3]);
    if (n == 8) reinterpret_cast<unsigned*>(d)[1] = pack4(v[4], v[5], v[6], v[7]);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j < n && j < valid) d[j] = (unsigned char)v[j];
  }
}

// planar fp32 [3][H*W] -> payload: truncating quantisation (zt_quantize_u8_hwc mode 0) and the conversion in one pass
template <int SS, int SIT, bool FAST>
__global__ void __launch_bounds__(256) yuv_encode_kernel(const float* __restrict__ src, unsigned char* __restrict__ dst, int H, int W,
                                                         EncCoef k) {
  const int PW = (W + 7) >> 3, PH = (H + 1) >> 1;
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= (long long)PW * PH) return;
  const int x0 = (int)(g % PW) * 8, y0 = (int)(g / PW) * 2;
  const int Wc = SS == 444 ? W : W >> 1, Hc = SS == 420 ? H >> 1 : H;
  const size_t HW = (size_t)H * W;
  unsigned char* du = dst + HW;
  unsigned char* dv = du + (size_t)Hc * Wc;
  constexpr bool LEFT = SS != 444 && SIT == 1;
  constexpr int NS = SS == 444 ? 8 : 4;               // chroma samples per patch row
  constexpr int SH = (SS == 444 ? 0 : (SIT == 0 ? 1 : 2)) + (SS == 420 ? 1 : 0);
  int s[3][NS];                                       // footprint sums, kept across the two rows for 4:2:0
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int y = y0 + r;
    if (y >= H) break;
    int q[3][8], left[3], Y[8];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) load_q8<FAST, LEFT>(src + ch * HW + (size_t)y * W, x0, W, q[ch], left[ch]);
#pragma unroll
    for (int j = 0; j < 8; ++j) Y[j] = clip255(k.yo + ((k.cyr * q[0][j] + k.cyg * q[1][j] + k.cyb * q[2][j] + (1 << 13)) >> 14));
    store_bytes<FAST>(dst + (size_t)y * W + x0, Y, 8, W - x0);
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
      U[n] = clip255(128 + ((k.cur * s[0][n] + k.cug * s[1][n] + k.cub * s[2][n] + (1 << (13 + SH))) >> (14 + SH)));
      V[n] = clip255(128 + ((k.cvr * s[0][n] + k.cvg * s[1][n] + k.cvb * s[2][n] + (1 << (13 + SH))) >> (14 + SH)));
    }
    const int cy = SS == 420 ? y >> 1 : y, cx = SS == 444 ? x0 : x0 >> 1;
    store_bytes<FAST>(du + (size_t)cy * Wc + cx, U, NS, Wc - cx);
    store_bytes<FAST>(dv + (size_t)cy * Wc + cx, V, NS, Wc - cx);
  }
}

bool yuv_args_ok(int H, int W, int ss, int siting) {
  if (H <= 0 || W <= 0 || (siting != 0 && siting != 1)) return false;
  if (ss == 444) return siting == 0;
  if (ss == 422) return W % 2 == 0;
  return ss == 420 && W % 2 == 0 && H % 2 == 0;
}

unsigned yuv_blocks(int H, int W) { return (unsigned)zt_cdivl((long long)((W + 7) >> 3) * ((H + 1) >> 1), 256); }

template <bool F32>
int yuv_decode(const unsigned char* src, void* dst, int H, int W, int ss, int siting, const int* c, const float* lut, hipStream_t stream) {
  const DecCoef k = {c[0], c[1], c[2], c[3], c[4], c[5]};
  const bool fast = W % 8 == 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0;
  const dim3 grid(yuv_blocks(H, W)), block(256);
#define ZT_DEC(SS, SIT)                                                                                                          \
  do {                                                                                                                           \
    if (fast) hipLaunchKernelGGL((yuv_decode_kernel<SS, SIT, F32, true>), grid, block, 0, stream, src, dst, H, W, k, lut);        \
    else hipLaunchKernelGGL((yuv_decode_kernel<SS, SIT, F32, false>), grid, block, 0, stream, src, dst, H, W, k, lut);            \
  } while (0)
  if (ss == 444) ZT_DEC(444, 0);
  else if (ss == 422 && siting == 0) ZT_DEC(422, 0);
  else if (ss == 422) ZT_DEC(422, 1);
  else if (siting == 0) ZT_DEC(420, 0);
  else ZT_DEC(420, 1);
#undef ZT_DEC
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}

}  // namespace

extern "C" int zt_yuv_to_rgb_u8(const unsigned char* src, unsigned char* dst, int H, int W, int ss, int siting, const int* coef,
                                hipStream_t stream) {
  ZT_REQUIRE(src && dst && coef && yuv_args_ok(H, W, ss, siting));
  return yuv_decode<false>(src, dst, H, W, ss, siting, coef, nullptr, stream);
}

extern "C" int zt_yuv_to_planar_f32(const unsigned char* src, float* dst, int H, int W, int ss, int siting, const int* coef,
                                    const float* lut256, hipStream_t stream) {
  ZT_REQUIRE(src && dst && coef && lut256 && yuv_args_ok(H, W, ss, siting) && ((uintptr_t)dst & 3) == 0);
  return yuv_decode<true>(src, dst, H, W, ss, siting, coef, lut256, stream);
}

extern "C" int zt_rgb_f32_to_yuv(const float* src, unsigned char* dst, int H, int W, int ss, int siting, const int* coef,
                                 hipStream_t stream) {
  ZT_REQUIRE(src && dst && coef && yuv_args_ok(H, W, ss, siting) && ((uintptr_t)src & 3) == 0);
  const EncCoef k = {coef[0], coef[1], coef[2], coef[3], coef[4], coef[5], coef[6], coef[7], coef[8], coef[9]};
  const bool fast = W % 8 == 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0;
  const dim3 grid(yuv_blocks(H, W)), block(256);
#define ZT_ENC(SS, SIT)                                                                                                \
  do {                                                                                                                 \
    if (fast) hipLaunchKernelGGL((yuv_encode_kernel<SS, SIT, true>), grid, block, 0, stream, src, dst, H, W, k);        \
    else hipLaunchKernelGGL((yuv_encode_kernel<SS, SIT, false>), grid, block, 0, stream, src, dst, H, W, k);            \
  } while (0)
  if (ss == 444) ZT_ENC(444, 0);
  else if (ss == 422 && siting == 0) ZT_ENC(422, 0);
  else if (ss == 422) ZT_ENC(422, 1);
  else if (siting == 0) ZT_ENC(420, 0);
  else ZT_ENC(420, 1);
#undef ZT_ENC
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}
