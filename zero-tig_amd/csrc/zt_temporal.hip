// Temporal consistency of a video against its own previous frame (evals.py --tc 1, zero-tig_amd/temporal.py): the
// warping error of Lai et al. 2018 with the forward-backward occlusion test of Ruder et al. 2016, the frame difference without
// motion compensation and the brightness difference behind MABD (Jiang and Zheng 2019), all from ONE pass over a frame pair.
//   cur, prev  planar [3][H][W] fp32
//   fb, ff     planar [2][Hf][Wf] fp32, in pixels: the backward flow (cur -> prev) and the forward flow (prev -> cur); the flow of
//              pixel (y, x) sits at [(y + oy) * Wf + (x + ox)] (RAFT's centred padding)
// Per pixel, IEEE fp32, one rounding per operation (the library is built with -ffp-contract=off and this file holds no fmaf), so
// that a numpy float32 restatement reproduces every per-pixel value bit for bit:
//   px = (float)x + u, py = (float)y + v                    (u, v) = fb at the pixel
//   inside = 0 <= px <= W - 1 && 0 <= py <= H - 1           NaN compares false; outside: px = py = 0, so that no address is
//                                                           ever formed from an unchecked coordinate
//   x0 = floor(px), ax = px - x0, x1 = min(x0 + 1, W - 1)   and the same in y
//   bil(p) = (1 - ay) * ((1 - ax) * p[y0][x0] + ax * p[y0][x1]) + ay * ((1 - ax) * p[y1][x0] + ax * p[y1][x1])
//   fu, fv = bil(ff); su = u + fu, sv = v + fv
//   valid = inside && su^2 + sv^2 <= 0.01 * ((u^2 + v^2) + (fu^2 + fv^2)) + 0.5
//   e  = sum_c (cur_c - bil(prev_c))^2,  e0 = sum_c (cur_c - prev_c)^2,  b = |sum_c cur_c - sum_c prev_c|     ((c0 + c1) + c2)
// out_n = number of valid pixels (exact); out3 = { sum over valid of e, sum over all of e0, sum over all of b } in fp64.
// No atomics: a thread adds its pixels in a fixed order, a wave by a butterfly, a workgroup over its four waves in index order,
// and one workgroup adds the per-block partials in index order -- same input (and same nblk), same bits.
// A gather kernel like zt_warp.hip: per pixel 2 + 3 + 3 coalesced values and 4 taps x 5 planes gathered.  A thread owns four
// neighbouring x; the coalesced part is read 16 bytes wide where the row pitch, the offset and the pointers allow it (images and
// flows decided separately), sample by sample with the same arithmetic otherwise.
#include "zt_common.h"

namespace {

typedef unsigned long long u64;

constexpr int TC_PX = 4;                  // neighbouring x of one thread
constexpr int TC_TW = 64 * TC_PX;         // tile: 256 columns x 4 rows, one row per wave

// four neighbouring values of a row: one 16-byte load (VEC: the caller has checked pitch and alignment, so the group is whole),
// or the values that exist, one by one
template <bool VEC>
__device__ __forceinline__ void load4(const float* __restrict__ row, int x, int n, float (&v)[TC_PX]) {
  if (VEC) {
    const float4 q = *reinterpret_cast<const float4*>(row + x);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < TC_PX; ++k) v[k] = x + k < n ? row[x + k] : 0.f;
  }
}

__device__ __forceinline__ double shfl_xor_f64(double v, int m) {
  u64 b;
  __builtin_memcpy(&b, &v, 8);
  const unsigned lo = __shfl_xor((unsigned)b, m), hi = __shfl_xor((unsigned)(b >> 32), m);
  b = ((u64)hi << 32) | lo;
  __builtin_memcpy(&v, &b, 8);
  return v;
}

struct Taps {
  int o00, o01, o10, o11;                 // y0 * pitch + x0, ... for one pitch
};

__device__ __forceinline__ float bil(const float* __restrict__ p, const Taps& t, float ax, float ay) {
  const float bx = 1.f - ax, by = 1.f - ay;
  const float top = bx * p[t.o00] + ax * p[t.o01];
  const float bot = bx * p[t.o10] + ax * p[t.o11];
  return by * top + ay * bot;
}

// partial layout in ws: u64 n[nblk], then double s[3][nblk]
template <bool VI, bool VF>
__global__ void __launch_bounds__(256) warp_error_kernel(const float* __restrict__ cur, const float* __restrict__ prev,
                                                         const float* __restrict__ fb, const float* __restrict__ ff, int H, int W,
                                                         int Hf, int Wf, int oy, int ox, int ntx, int ntiles,
                                                         u64* __restrict__ part_n, double* __restrict__ part_s) {
  __shared__ u64 red_n[4];
  __shared__ double red_s[3][4];
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  const size_t plane = (size_t)H * W, fplane = (size_t)Hf * Wf;
  const float xmax = (float)(W - 1), ymax = (float)(H - 1);
  unsigned cnt = 0;
  double s_e = 0.0, s_e0 = 0.0, s_b = 0.0;
  for (int tile = (int)blockIdx.x; tile < ntiles; tile += (int)gridDim.x) {
    const int ty = tile / ntx, tx = tile - ty * ntx;
    const int y = ty * 4 + wave, x = tx * TC_TW + lane * TC_PX;
    if (y >= H || x >= W) continue;
    float u[TC_PX], v[TC_PX], c[3][TC_PX], p[3][TC_PX];
    const size_t fo = (size_t)(y + oy) * Wf + ox;
    load4<VF>(fb + fo, x, W, u);
    load4<VF>(fb + fplane + fo, x, W, v);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      load4<VI>(cur + ch * plane + (size_t)y * W, x, W, c[ch]);
      load4<VI>(prev + ch * plane + (size_t)y * W, x, W, p[ch]);
    }
#pragma unroll
    for (int k = 0; k < TC_PX; ++k) {
      if (x + k < W) {
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
        const float s0 = c[0][k] - p[0][k], s1 = c[1][k] - p[1][k], s2 = c[2][k] - p[2][k];
        const float e0 = (s0 * s0 + s1 * s1) + s2 * s2;
        const float b = fabsf(((c[0][k] + c[1][k]) + c[2][k]) - ((p[0][k] + p[1][k]) + p[2][k]));
        cnt += valid ? 1u : 0u;
        s_e += valid ? (double)e : 0.0;
        s_e0 += (double)e0;
        s_b += (double)b;
      }
    }
  }
#pragma unroll
  for (int k = 32; k >= 1; k >>= 1) {
    cnt += __shfl_xor(cnt, k);
    s_e += shfl_xor_f64(s_e, k);
    s_e0 += shfl_xor_f64(s_e0, k);
    s_b += shfl_xor_f64(s_b, k);
  }
  if (lane == 0) red_n[wave] = cnt, red_s[0][wave] = s_e, red_s[1][wave] = s_e0, red_s[2][wave] = s_b;
  __syncthreads();
  if (t == 0) part_n[blockIdx.x] = ((red_n[0] + red_n[1]) + red_n[2]) + red_n[3];
  if (t >= 1 && t < 4)
    part_s[(size_t)(t - 1) * gridDim.x + blockIdx.x] = ((red_s[t - 1][0] + red_s[t - 1][1]) + red_s[t - 1][2]) + red_s[t - 1][3];
}

// one workgroup: thread t adds partials t, t + 256, ... in index order, then a tree
__global__ void __launch_bounds__(256) warp_error_final_kernel(const u64* __restrict__ part_n, const double* __restrict__ part_s,
                                                               int nblk, long long* __restrict__ out_n, double* __restrict__ out3) {
  __shared__ u64 rn[256];
  __shared__ double rs[256];
  const int t = (int)threadIdx.x;
  u64 n = 0;
  for (int i = t; i < nblk; i += 256) n += part_n[i];
  rn[t] = n;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (t < k) rn[t] += rn[t + k];
    __syncthreads();
  }
  if (t == 0) out_n[0] = (long long)rn[0];
  for (int q = 0; q < 3; ++q) {
    double s = 0.0;
    for (int i = t; i < nblk; i += 256) s += part_s[(size_t)q * nblk + i];
    rs[t] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
      if (t < k) rs[t] += rs[t + k];
      __syncthreads();
    }
    if (t == 0) out3[q] = rs[0];
    __syncthreads();
  }
}

}  // namespace

extern "C" int zt_warp_error_f32(const float* cur, const float* prev, const float* fb, const float* ff, int H, int W, int Hf,
                                 int Wf, int oy, int ox, void* ws, int nblk, long long* out_n, double* out3, hipStream_t stream) {
  ZT_REQUIRE(cur && prev && fb && ff && ws && out_n && out3);
  ZT_REQUIRE(H >= 1 && W >= 1 && oy >= 0 && ox >= 0 && nblk >= 1 && nblk <= 4096);
  ZT_REQUIRE((long long)Hf >= (long long)H + oy && (long long)Wf >= (long long)W + ox);
  ZT_REQUIRE((long long)Hf * Wf < (1LL << 31));                    // tap offsets are 32-bit; H * W <= Hf * Wf
  ZT_REQUIRE((((uintptr_t)ws | (uintptr_t)out_n | (uintptr_t)out3) & 7) == 0);
  ZT_REQUIRE((((uintptr_t)cur | (uintptr_t)prev | (uintptr_t)fb | (uintptr_t)ff) & 3) == 0);
  const int ntx = zt_cdiv(W, TC_TW), ntiles = ntx * zt_cdiv(H, 4);
  const int grid = ntiles < nblk ? ntiles : nblk;                   // the final pass reads exactly the partials written
  u64* part_n = (u64*)ws;
  double* part_s = (double*)(part_n + grid);
  const bool vi = W % 4 == 0 && (((uintptr_t)cur | (uintptr_t)prev) & 15) == 0;
  const bool vf = W % 4 == 0 && Wf % 4 == 0 && ox % 4 == 0 && ((uintptr_t)fb & 15) == 0;
#define ZT_TC_LAUNCH(VI, VF)                                                                                                      \
  hipLaunchKernelGGL((warp_error_kernel<VI, VF>), dim3(grid), dim3(256), 0, stream, cur, prev, fb, ff, H, W, Hf, Wf, oy, ox, ntx, \
                     ntiles, part_n, part_s)
  if (vi && vf) ZT_TC_LAUNCH(true, true);
  else if (vi) ZT_TC_LAUNCH(true, false);
  else if (vf) ZT_TC_LAUNCH(false, true);
  else ZT_TC_LAUNCH(false, false);
#undef ZT_TC_LAUNCH
  ZT_LAUNCH_CHECK();
  hipLaunchKernelGGL(warp_error_final_kernel, dim3(1), dim3(256), 0, stream, (const u64*)part_n, (const double*)part_s, grid, out_n,
                     out3);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}
