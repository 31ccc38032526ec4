// Looking at what evals.py --tc 1 measures (evals.py --tc_viz / --tc_flo_dir, zero-tig_amd/temporal.py): the colour wheel
// of Baker et al. 2007 for a flow field, the four-panel diagnostic picture of a frame pair, and the payload of a Middlebury .flo
// file.  The flows are planar [2][Hf][Wf] fp32 in pixels, the flow of pixel (y, x) at [(y + oy) * Wf + (x + ox)], as in zt_temporal.hip.
// IEEE fp32 throughout, one rounding per operation (built with -ffp-contract=off, no fmaf here), no library transcendental: sqrtf and
// / are correctly rounded, the angle is a polynomial.  A numpy float32 restatement therefore reproduces every output bit for bit.
//
// Colour of a flow (u, v) at the scale R (a float on the device):
//   den = R + 1e-5f; un = u / den, vn = v / den; r2 = un * un + vn * vn; rad = sqrtf(r2)
//   r2 not finite (NaN or inf: a NaN or inf component, a component so large that its square overflows, a NaN scale): black
//   a = angle(y = -vn, x = -un), the value of atan2 with its sign conventions, the sign of a zero included:
//     ax = |x|, ay = |y|, t = min(ax, ay) / max(ax, ay) (0 when the maximum is 0)
//     t > 0.41421357f: base = pi/4, t = (t - 1) / (t + 1); otherwise base = 0
//     z = t * t; p = ((((C4 * z - C3) * z + C2) * z - C1) * z) * t + t; a = base + p
//     ay > ax: a = pi/2 - a;  x has its sign bit set: a = pi - a;  a takes the sign bit of y
//   fk = (a / pi + 1) * 27; k0 = min(max((int)floorf(fk), 0), 54); f = fk - floorf(fk); k1 = k0 + 1, 55 -> 0
//   per channel c: col = (1 - f) * (wheel[k0][c] / 255) + f * (wheel[k1][c] / 255)
//                  rad <= 1: col = 1 - rad * (1 - col); otherwise col = col * 0.75f
//                  level = (int)floorf(255 * col) clamped to 0..255
// The wheel is built from the paper's six segment lengths (15, 6, 4, 11, 13, 6).
// A maximum does not depend on the order it is taken in and nothing else is reduced: no atomics, same input, same bits.
// Mapping as in zt_temporal.hip: a thread owns four neighbouring x, a workgroup 256 columns x 4 rows; 16-byte loads and stores where
// pitch, offset and pointers allow (decided separately for images, flows and each output), value by value otherwise.
#include <math.h>

#include "zt_common.h"

namespace {

constexpr int FV_PX = 4;
constexpr int FV_TW = 64 * FV_PX;
constexpr int FV_NCOL = 55;

struct Wheel {
  unsigned char level[FV_NCOL][3];
  float frac[FV_NCOL][3];                 // level / 255, the division rounded once
};

constexpr Wheel make_wheel() {
  Wheel w = {};
  const int seg[6] = {15, 6, 4, 11, 13, 6};               // red-yellow, yellow-green, green-cyan, cyan-blue, blue-magenta, magenta-red
  const int full[6] = {0, 1, 1, 2, 2, 0};                 // the channel that stays at 255 through the segment
  const int ramp[6] = {1, 0, 2, 1, 0, 2};                 // the channel that moves: up in the even segments, down in the odd ones
  int k = 0;
  for (int s = 0; s < 6; ++s)
    for (int i = 0; i < seg[s]; ++i, ++k) {
      const int r = 255 * i / seg[s];
      w.level[k][full[s]] = 255;
      w.level[k][ramp[s]] = (unsigned char)(s % 2 == 0 ? r : 255 - r);
    }
  for (int i = 0; i < FV_NCOL; ++i)
    for (int c = 0; c < 3; ++c) w.frac[i][c] = (float)w.level[i][c] / 255.f;
  return w;
}

constexpr Wheel WHEEL_HOST = make_wheel();
__device__ const Wheel WHEEL = make_wheel();

constexpr float FV_PI = 3.14159274f, FV_PI_2 = 1.57079637f, FV_PI_4 = 0.785398185f;
constexpr float FV_INF = __builtin_huge_valf();

template <bool VEC>
__device__ __forceinline__ void load4(const float* __restrict__ row, int x, int n, float (&v)[FV_PX]) {
  if (VEC) {
    const float4 q = *reinterpret_cast<const float4*>(row + x);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < FV_PX; ++k) v[k] = x + k < n ? row[x + k] : 0.f;
  }
}

template <bool VEC>
__device__ __forceinline__ void store4(float* __restrict__ row, int x, int n, const float (&v)[FV_PX]) {
  if (VEC) {
    *reinterpret_cast<float4*>(row + x) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < FV_PX; ++k)
      if (x + k < n) row[x + k] = v[k];
  }
}

// atan2(y, x) from plain fp32 operations
__device__ __forceinline__ float angle(float y, float x) {
  const float ax = fabsf(x), ay = fabsf(y);
  const float mx = ax > ay ? ax : ay, mn = ax > ay ? ay : ax;
  float t = mx == 0.f ? 0.f : mn / mx;
  float base = 0.f;
  if (t > 0.41421357f) {
    base = FV_PI_4;
    t = (t - 1.f) / (t + 1.f);
  }
  const float z = t * t;
  float p = 8.05374449538e-2f * z - 1.38776856032e-1f;
  p = p * z + 1.99777106478e-1f;
  p = p * z - 3.33329491539e-1f;
  p = p * z;
  p = p * t + t;
  float a = base + p;
  if (ay > ax) a = FV_PI_2 - a;
  if (__builtin_signbitf(x)) a = FV_PI - a;
  return __builtin_copysignf(a, y);
}

// the three levels (0..255) of the flow (u, v) at the scale 1 / den; bgr swaps the first and the last
__device__ __forceinline__ void flow_levels(float u, float v, float den, bool bgr, int (&lv)[3]) {
  const float un = u / den, vn = v / den;
  const float r2 = un * un + vn * vn;
  if (!(r2 < FV_INF)) {                                   // NaN compares false
    lv[0] = lv[1] = lv[2] = 0;
    return;
  }
  const float rad = sqrtf(r2);
  const float a = angle(-vn, -un);
  const float fk = (a / FV_PI + 1.f) * 27.f;
  const float fl = floorf(fk);
  const int k0 = min(max((int)fl, 0), FV_NCOL - 1);
  const int k1 = k0 + 1 == FV_NCOL ? 0 : k0 + 1;
  const float f = fk - fl;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float col = (1.f - f) * WHEEL.frac[k0][c] + f * WHEEL.frac[k1][c];
    col = rad <= 1.f ? 1.f - rad * (1.f - col) : col * 0.75f;
    const int level = (int)floorf(255.f * col);
    lv[bgr ? 2 - c : c] = min(max(level, 0), 255);
  }
}

// ---- largest finite radius of one or two flows ------------------------------------------------------------------------------------
template <bool VF>
__global__ void __launch_bounds__(256) radmax_kernel(const float* __restrict__ fa, const float* __restrict__ fb, int H, int W, int Hf,
                                                     int Wf, int oy, int ox, int ntx, int ntiles, float* __restrict__ part) {
  __shared__ float red[4];
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  const size_t fplane = (size_t)Hf * Wf;
  float m = 0.f;
  for (int tile = (int)blockIdx.x; tile < ntiles; tile += (int)gridDim.x) {
    const int ty = tile / ntx, tx = tile - ty * ntx;
    const int y = ty * 4 + wave, x = tx * FV_TW + lane * FV_PX;
    if (y >= H || x >= W) continue;
    const size_t fo = (size_t)(y + oy) * Wf + ox;
    for (int q = 0; q < 2; ++q) {
      const float* __restrict__ fl = q ? fb : fa;
      if (!fl) continue;
      float u[FV_PX], v[FV_PX];
      load4<VF>(fl + fo, x, W, u);
      load4<VF>(fl + fplane + fo, x, W, v);
#pragma unroll
      for (int k = 0; k < FV_PX; ++k) {
        const float r2 = u[k] * u[k] + v[k] * v[k];
        if (x + k < W && r2 < FV_INF) m = fmaxf(m, sqrtf(r2));
      }
    }
  }
#pragma unroll
  for (int k = 32; k >= 1; k >>= 1) m = fmaxf(m, __shfl_xor(m, k));
  if (lane == 0) red[wave] = m;
  __syncthreads();
  if (t == 0) part[blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__global__ void __launch_bounds__(256) radmax_final_kernel(const float* __restrict__ part, int nblk, float* __restrict__ out1) {
  __shared__ float red[256];
  const int t = (int)threadIdx.x;
  float m = 0.f;
  for (int i = t; i < nblk; i += 256) m = fmaxf(m, part[i]);
  red[t] = m;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (t < k) red[t] = fmaxf(red[t], red[t + k]);
    __syncthreads();
  }
  if (t == 0) out1[0] = red[0];
}

// ---- the colour wheel ---------------------------------------------------------------------------------------------------------------
// VU: the twelve bytes of a thread's four pixels as three 32-bit stores; VO: the planar output 16 bytes wide
template <bool VF, bool VU, bool VO>
__global__ void __launch_bounds__(256) flow_to_rgb_kernel(const float* __restrict__ flow, int H, int W, int Hf, int Wf, int oy, int ox,
                                                          const float* __restrict__ rad_dev, unsigned char* __restrict__ out_u8,
                                                          float* __restrict__ out_f32, int bgr) {
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  const int y = (int)blockIdx.y * 4 + wave, x = (int)blockIdx.x * FV_TW + lane * FV_PX;
  if (y >= H || x >= W) return;
  const size_t plane = (size_t)H * W, fplane = (size_t)Hf * Wf;
  const float den = rad_dev[0] + 1e-5f;
  float u[FV_PX], v[FV_PX];
  const size_t fo = (size_t)(y + oy) * Wf + ox;
  load4<VF>(flow + fo, x, W, u);
  load4<VF>(flow + fplane + fo, x, W, v);
  int lv[FV_PX][3];
#pragma unroll
  for (int k = 0; k < FV_PX; ++k) flow_levels(u[k], v[k], den, bgr != 0, lv[k]);
  if (out_u8) {
    unsigned char* __restrict__ o = out_u8 + ((size_t)y * W + x) * 3;
    if (VU) {
      unsigned w[3] = {0, 0, 0};
#pragma unroll
      for (int b = 0; b < 12; ++b) w[b >> 2] |= (unsigned)lv[b / 3][b % 3] << (8 * (b & 3));
      unsigned* __restrict__ o32 = reinterpret_cast<unsigned*>(o);
      o32[0] = w[0], o32[1] = w[1], o32[2] = w[2];
    } else {
#pragma unroll
      for (int k = 0; k < FV_PX; ++k)
        if (x + k < W) o[3 * k] = (unsigned char)lv[k][0], o[3 * k + 1] = (unsigned char)lv[k][1], o[3 * k + 2] = (unsigned char)lv[k][2];
    }
  }
  if (out_f32) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float r[FV_PX];
#pragma unroll
      for (int k = 0; k < FV_PX; ++k) r[k] = (float)lv[k][c] / 255.f;
      store4<VO>(out_f32 + c * plane + (size_t)y * W, x, W, r);
    }
  }
}

// ---- planar padded flow -> interleaved [H][W][2] ------------------------------------------------------------------------------------
template <bool VF, bool VO>
__global__ void __launch_bounds__(256) flow_pack_kernel(const float* __restrict__ flow, int H, int W, int Hf, int Wf, int oy, int ox,
                                                        float* __restrict__ out) {
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  const int y = (int)blockIdx.y * 4 + wave, x = (int)blockIdx.x * FV_TW + lane * FV_PX;
  if (y >= H || x >= W) return;
  float u[FV_PX], v[FV_PX];
  const size_t fo = (size_t)(y + oy) * Wf + ox;
  load4<VF>(flow + fo, x, W, u);
  load4<VF>(flow + (size_t)Hf * Wf + fo, x, W, v);
  float* __restrict__ o = out + ((size_t)y * W + x) * 2;
  if (VO) {
    reinterpret_cast<float4*>(o)[0] = make_float4(u[0], v[0], u[1], v[1]);
    reinterpret_cast<float4*>(o)[1] = make_float4(u[2], v[2], u[3], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < FV_PX; ++k)
      if (x + k < W) o[2 * k] = u[k], o[2 * k + 1] = v[k];
  }
}

// ---- the four-panel picture -------------------------------------------------------------------------------------------------------
struct Taps {
  int o00, o01, o10, o11;
};

__device__ __forceinline__ float bil(const float* __restrict__ p, const Taps& t, float ax, float ay) {
  const float bx = 1.f - ax, by = 1.f - ay;
  const float top = bx * p[t.o00] + ax * p[t.o01];
  const float bot = bx * p[t.o10] + ax * p[t.o11];
  return by * top + ay * bot;
}

// out: planar [3][2H][2W]; top left / top right: the wheel colour of fb / ff at the pixel; bottom left: cur where the pixel is valid,
// magenta where it lands outside the frame, cyan where it fails the forward-backward test; bottom right: min(1, sqrtf(e / 3) * gain)
// where valid, 0 elsewhere.  u, v, inside, ax, ay, fu, fv, valid, e: the arithmetic of warp_error_kernel (zt_temporal.hip), operation
// for operation.  PAIR = false (no previous frame): white, cur, black; neither the flows nor the scale are read.
template <bool PAIR, bool VI, bool VF, bool VO>
__global__ void __launch_bounds__(256) tc_viz_kernel(const float* __restrict__ cur, const float* __restrict__ prev,
                                                     const float* __restrict__ fb, const float* __restrict__ ff, int H, int W, int Hf,
                                                     int Wf, int oy, int ox, const float* __restrict__ rad_dev, float gain,
                                                     float* __restrict__ out) {
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  const int y = (int)blockIdx.y * 4 + wave, x = (int)blockIdx.x * FV_TW + lane * FV_PX;
  if (y >= H || x >= W) return;
  const size_t plane = (size_t)H * W, fplane = (size_t)Hf * Wf;
  const int W2 = 2 * W;
  const size_t oplane = (size_t)2 * H * W2;
  float c[3][FV_PX];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) load4<VI>(cur + ch * plane + (size_t)y * W, x, W, c[ch]);
  float tl[3][FV_PX], tr[3][FV_PX], bl[3][FV_PX], br[FV_PX];
  if (!PAIR) {
#pragma unroll
    for (int k = 0; k < FV_PX; ++k) {
      br[k] = 0.f;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) tl[ch][k] = 1.f, tr[ch][k] = 1.f, bl[ch][k] = c[ch][k];
    }
  } else {
    const float xmax = (float)(W - 1), ymax = (float)(H - 1);
    const float den = rad_dev[0] + 1e-5f;
    float u[FV_PX], v[FV_PX], gu[FV_PX], gv[FV_PX];
    const size_t fo = (size_t)(y + oy) * Wf + ox;
    load4<VF>(fb + fo, x, W, u);
    load4<VF>(fb + fplane + fo, x, W, v);
    load4<VF>(ff + fo, x, W, gu);
    load4<VF>(ff + fplane + fo, x, W, gv);
#pragma unroll
    for (int k = 0; k < FV_PX; ++k) {
      br[k] = 0.f;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) tl[ch][k] = 0.f, tr[ch][k] = 0.f, bl[ch][k] = 0.f;
      if (x + k < W) {
        int lv[3];
        flow_levels(u[k], v[k], den, false, lv);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) tl[ch][k] = (float)lv[ch] / 255.f;
        flow_levels(gu[k], gv[k], den, false, lv);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) tr[ch][k] = (float)lv[ch] / 255.f;
        float px = (float)(x + k) + u[k], py = (float)y + v[k];
        const bool inside = px >= 0.f && px <= xmax && py >= 0.f && py <= ymax;      // false for NaN
        px = inside ? px : 0.f;
        py = inside ? py : 0.f;
        const float fx0 = floorf(px), fy0 = floorf(py);
        const float ax = px - fx0, ay = py - fy0;
        const int x0 = (int)fx0, y0 = (int)fy0;                                       // in [0, W - 1] x [0, H - 1]
        const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
        const Taps ti = {y0 * W + x0, y0 * W + x1, y1 * W + x0, y1 * W + x1};
        const int r0 = (y0 + oy) * Wf + ox, r1 = (y1 + oy) * Wf + ox;
        const Taps tf = {r0 + x0, r0 + x1, r1 + x0, r1 + x1};
        const float fu = bil(ff, tf, ax, ay), fv = bil(ff + fplane, tf, ax, ay);
        const float su = u[k] + fu, sv = v[k] + fv;
        const float lhs = su * su + sv * sv;
        const float rhs = 0.01f * ((u[k] * u[k] + v[k] * v[k]) + (fu * fu + fv * fv)) + 0.5f;
        const bool valid = inside && lhs <= rhs;
        const float d0 = c[0][k] - bil(prev, ti, ax, ay);
        const float d1 = c[1][k] - bil(prev + plane, ti, ax, ay);
        const float d2 = c[2][k] - bil(prev + 2 * plane, ti, ax, ay);
        const float e = (d0 * d0 + d1 * d1) + d2 * d2;
        bl[0][k] = valid ? c[0][k] : (inside ? 0.f : 1.f);
        bl[1][k] = valid ? c[1][k] : (inside ? 1.f : 0.f);
        bl[2][k] = valid ? c[2][k] : 1.f;
        br[k] = valid ? fminf(1.f, sqrtf(e / 3.f) * gain) : 0.f;
      }
    }
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    float* __restrict__ top = out + ch * oplane + (size_t)y * W2;
    float* __restrict__ bot = out + ch * oplane + (size_t)(y + H) * W2;
    store4<VO>(top, x, W, tl[ch]);
    store4<VO>(top + W, x, W, tr[ch]);
    store4<VO>(bot, x, W, bl[ch]);
    store4<VO>(bot + W, x, W, br);
  }
}

// the checks the four entry points share: the window inside the padded flow, offsets that fit 32 bits
inline bool window_ok(int H, int W, int Hf, int Wf, int oy, int ox) {
  return H >= 1 && W >= 1 && oy >= 0 && ox >= 0 && (long long)Hf >= (long long)H + oy && (long long)Wf >= (long long)W + ox &&
         (long long)Hf * Wf < (1LL << 31) && zt_cdiv(H, 4) <= 65535;
}

inline bool flow_vec(const float* f, int W, int Wf, int ox) {
  return W % 4 == 0 && Wf % 4 == 0 && ox % 4 == 0 && ((uintptr_t)f & 15) == 0;
}

}  // namespace

extern "C" int zt_flow_wheel(unsigned char* out165) {
  ZT_REQUIRE(out165);
  for (int k = 0; k < FV_NCOL; ++k)
    for (int c = 0; c < 3; ++c) out165[3 * k + c] = WHEEL_HOST.level[k][c];
  return ZT_OK;
}

extern "C" int zt_flow_radmax_f32(const float* fa, const float* fb, int H, int W, int Hf, int Wf, int oy, int ox, float* ws, int nblk,
                                  float* out1, hipStream_t stream) {
  ZT_REQUIRE(fa && ws && out1);
  ZT_REQUIRE(window_ok(H, W, Hf, Wf, oy, ox) && nblk >= 1 && nblk <= 4096);
  ZT_REQUIRE((((uintptr_t)fa | (uintptr_t)fb | (uintptr_t)ws | (uintptr_t)out1) & 3) == 0);
  const int ntx = zt_cdiv(W, FV_TW), ntiles = ntx * zt_cdiv(H, 4);
  const int grid = ntiles < nblk ? ntiles : nblk;                   // the final pass reads exactly the partials written
  if (flow_vec(fa, W, Wf, ox) && ((uintptr_t)fb & 15) == 0)
    hipLaunchKernelGGL((radmax_kernel<true>), dim3(grid), dim3(256), 0, stream, fa, fb, H, W, Hf, Wf, oy, ox, ntx, ntiles, ws);
  else
    hipLaunchKernelGGL((radmax_kernel<false>), dim3(grid), dim3(256), 0, stream, fa, fb, H, W, Hf, Wf, oy, ox, ntx, ntiles, ws);
  ZT_LAUNCH_CHECK();
  hipLaunchKernelGGL(radmax_final_kernel, dim3(1), dim3(256), 0, stream, (const float*)ws, grid, out1);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}

extern "C" int zt_flow_to_rgb(const float* flow, int H, int W, int Hf, int Wf, int oy, int ox, const float* rad_dev,
                              unsigned char* out_u8, float* out_f32, int bgr, hipStream_t stream) {
  ZT_REQUIRE(flow && rad_dev && (out_u8 || out_f32));
  ZT_REQUIRE(window_ok(H, W, Hf, Wf, oy, ox) && (bgr == 0 || bgr == 1));
  ZT_REQUIRE((long long)H * W * 3 < (1LL << 31));
  ZT_REQUIRE((((uintptr_t)flow | (uintptr_t)rad_dev | (uintptr_t)out_f32) & 3) == 0);
  const bool vf = flow_vec(flow, W, Wf, ox);
  const bool vu = W % 4 == 0 && ((uintptr_t)out_u8 & 3) == 0;
  const bool vo = W % 4 == 0 && ((uintptr_t)out_f32 & 15) == 0;
  const dim3 grid(zt_cdiv(W, FV_TW), zt_cdiv(H, 4));
#define ZT_FV_LAUNCH(VF, VU, VO)                                                                                                   \
  hipLaunchKernelGGL((flow_to_rgb_kernel<VF, VU, VO>), grid, dim3(256), 0, stream, flow, H, W, Hf, Wf, oy, ox, rad_dev, out_u8, out_f32, \
                     bgr)
#define ZT_FV_OUT(VF)                              \
  do {                                             \
    if (vu && vo) ZT_FV_LAUNCH(VF, true, true);    \
    else if (vu) ZT_FV_LAUNCH(VF, true, false);    \
    else if (vo) ZT_FV_LAUNCH(VF, false, true);    \
    else ZT_FV_LAUNCH(VF, false, false);           \
  } while (0)
  if (vf) ZT_FV_OUT(true);
  else ZT_FV_OUT(false);
#undef ZT_FV_OUT
#undef ZT_FV_LAUNCH
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}

extern "C" int zt_flow_pack_hwc_f32(const float* flow, int H, int W, int Hf, int Wf, int oy, int ox, float* out, hipStream_t stream) {
  ZT_REQUIRE(flow && out);
  ZT_REQUIRE(window_ok(H, W, Hf, Wf, oy, ox));
  ZT_REQUIRE((((uintptr_t)flow | (uintptr_t)out) & 3) == 0);
  const bool vf = flow_vec(flow, W, Wf, ox);
  const bool vo = W % 4 == 0 && ((uintptr_t)out & 15) == 0;
  const dim3 grid(zt_cdiv(W, FV_TW), zt_cdiv(H, 4));
#define ZT_FV_LAUNCH(VF, VO) \
  hipLaunchKernelGGL((flow_pack_kernel<VF, VO>), grid, dim3(256), 0, stream, flow, H, W, Hf, Wf, oy, ox, out)
  if (vf && vo) ZT_FV_LAUNCH(true, true);
  else if (vf) ZT_FV_LAUNCH(true, false);
  else if (vo) ZT_FV_LAUNCH(false, true);
  else ZT_FV_LAUNCH(false, false);
#undef ZT_FV_LAUNCH
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}

extern "C" int zt_tc_viz_f32(const float* cur, const float* prev, const float* fb, const float* ff, int H, int W, int Hf, int Wf,
                             int oy, int ox, const float* rad_dev, float gain, float* out, hipStream_t stream) {
  ZT_REQUIRE(cur && out && H >= 1 && W >= 1 && zt_cdiv(H, 4) <= 65535);
  ZT_REQUIRE((long long)H * W * 4 < (1LL << 31));                    // the picture's plane: offsets of a row start fit 32 bits
  ZT_REQUIRE(gain >= 0.f && gain < FV_INF);                          // false for NaN
  ZT_REQUIRE((((uintptr_t)cur | (uintptr_t)prev | (uintptr_t)fb | (uintptr_t)ff | (uintptr_t)rad_dev | (uintptr_t)out) & 3) == 0);
  const bool vi = W % 4 == 0 && ((uintptr_t)cur & 15) == 0;
  const bool vo = W % 4 == 0 && ((uintptr_t)out & 15) == 0;
  const dim3 grid(zt_cdiv(W, FV_TW), zt_cdiv(H, 4));
#define ZT_FV_LAUNCH(PAIR, VI, VF, VO)                                                                                                \
  hipLaunchKernelGGL((tc_viz_kernel<PAIR, VI, VF, VO>), grid, dim3(256), 0, stream, cur, prev, fb, ff, H, W, Hf, Wf, oy, ox, rad_dev, \
                     gain, out)
  if (!prev) {
    if (vi && vo) ZT_FV_LAUNCH(false, true, false, true);
    else if (vi) ZT_FV_LAUNCH(false, true, false, false);
    else if (vo) ZT_FV_LAUNCH(false, false, false, true);
    else ZT_FV_LAUNCH(false, false, false, false);
    ZT_LAUNCH_CHECK();
    return ZT_OK;
  }
  ZT_REQUIRE(fb && ff && rad_dev && window_ok(H, W, Hf, Wf, oy, ox));
  const bool vf = flow_vec(fb, W, Wf, ox) && ((uintptr_t)ff & 15) == 0;
  if (vi && vf && vo) ZT_FV_LAUNCH(true, true, true, true);
  else if (vi && vo) ZT_FV_LAUNCH(true, true, false, true);
  else if (vi && vf) ZT_FV_LAUNCH(true, true, true, false);
  else if (vf && vo) ZT_FV_LAUNCH(true, false, true, true);
  else if (vi) ZT_FV_LAUNCH(true, true, false, false);
  else if (vf) ZT_FV_LAUNCH(true, false, true, false);
  else if (vo) ZT_FV_LAUNCH(true, false, false, true);
  else ZT_FV_LAUNCH(true, false, false, false);
#undef ZT_FV_LAUNCH
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}
