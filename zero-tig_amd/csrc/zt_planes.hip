// Plane metrics of a raw video stream (evals.py --y4m_in / --y4m_gt): what people quote for a video, at the stream's
// own bit depth, computed on the two Y4M payloads themselves.
//   samples  depth 8: uint8; depth B in {9, 10, 12, 14, 16}: little-endian uint16, a sample above m = 2^B - 1 is read as m (the
//            convention of zt_yuv.hip).
//   sse      out3[p] = sum over plane p (Y, U, V of the payload) of (a - b)^2, exact unsigned 64-bit; ONE pass over both payloads:
//            the payload is walked as one run of N samples and a sample's plane follows from its index.  A difference is below
//            2^16 and its square below 2^32, so a plane of fewer than 2^31 samples sums below 2^63.
//   ssim     skimage structural_similarity(a, b, data_range=m) of one plane [H][W]: 7x7 uniform window, sample covariance (49/48),
//            C1 = (0.01 m)^2, C2 = (0.03 m)^2, 3-sample border cropped, mean over the windows inside the plane -- the definition
//            of zt_ssim_u8_f32 for one channel, with the same three phases (stage, horizontal running sums, vertical running
//            sums + S in fp64 + block partial).  The five window sums are exact integers:
//              depth <= 12   49 * 4095^2 < 2^30: 32-bit sums, the 38 x 64 table of horizontal sums is 16 bytes an entry (38 KB)
//              depth 14, 16  49 * 65535^2 = 2^37.6: sxx / syy / sxy are 64-bit, an entry is 32 bytes; the tile shrinks to 16 rows
//                            (22 x 64 entries, 44 KB) so that three workgroups still share a CU's LDS
// No atomics; every partial has one owner and the final reduce adds them in index order: same input, same bits.
// Byte kernels of a few MB a call: 16-byte loads where the plane allows them (W a multiple of 16 bytes of samples, 16-byte aligned
// pointers), sample-wide loads with the same arithmetic otherwise (a chroma plane of an odd-sized stream, a pointer into a buffer).
#include "zt_common.h"

namespace {

typedef unsigned long long u64;

template <class T>
__device__ __forceinline__ int sample(unsigned v, int m) {
  return sizeof(T) == 1 ? (int)v : min((int)v, m);
}

// ================================================================ SSE =====================================================
// plane of sample i: n0 = samples of Y, n1 = n0 + samples of U
__device__ __forceinline__ int plane_of(long long i, long long n0, long long n1) { return i >= n1 ? 2 : (i >= n0 ? 1 : 0); }

// s[p] += v without a runtime-indexed array (which would live in scratch)
__device__ __forceinline__ void add_plane(int p, u64 v, u64& s0, u64& s1, u64& s2) {
  s0 += p == 0 ? v : 0ull;
  s1 += p == 1 ? v : 0ull;
  s2 += p == 2 ? v : 0ull;
}

template <class T>
__device__ __forceinline__ u64 sq1(unsigned a, unsigned b, int m) {
  const int x = sample<T>(a, m), y = sample<T>(b, m);
  const unsigned d = (unsigned)(x > y ? x - y : y - x);
  return (u64)(d * d);                                 // d < 2^16: the product fits 32 bits unsigned
}

// the squared differences of sample j of two 16-byte loads
template <class T>
__device__ __forceinline__ u64 sq_at(const unsigned (&wa)[4], const unsigned (&wb)[4], int j, int m) {
  constexpr int BITS = 8 * sizeof(T), PER = 32 / BITS;
  const unsigned mask = (1u << BITS) - 1u;
  return sq1<T>((wa[j / PER] >> (BITS * (j % PER))) & mask, (wb[j / PER] >> (BITS * (j % PER))) & mask, m);
}

__device__ __forceinline__ u64 shfl_xor_u64(u64 v, int m) {
  const unsigned lo = __shfl_xor((unsigned)v, m), hi = __shfl_xor((unsigned)(v >> 32), m);
  return ((u64)hi << 32) | lo;
}

// VEC: a and b are 16-byte aligned; vectors of K = 16 / sizeof(T) samples, the N % K samples behind them by block 0.
// partial[p * gridDim.x + block] = the block's share of plane p.
template <class T, bool VEC>
__global__ void __launch_bounds__(256) yuv_sse_kernel(const T* __restrict__ a, const T* __restrict__ b, long long N, long long n0,
                                                      long long n1, int m, u64* __restrict__ partial) {
  __shared__ u64 part[3][4];
  constexpr int K = 16 / sizeof(T);
  const int t = (int)threadIdx.x;
  const long long gid = (long long)blockIdx.x * 256 + t, stride = (long long)gridDim.x * 256;
  u64 s0 = 0, s1 = 0, s2 = 0;
  if (VEC) {
    const long long nvec = N / K;
    for (long long v = gid; v < nvec; v += stride) {
      const uint4 va = reinterpret_cast<const uint4*>(a)[v], vb = reinterpret_cast<const uint4*>(b)[v];
      const unsigned wa[4] = {va.x, va.y, va.z, va.w}, wb[4] = {vb.x, vb.y, vb.z, vb.w};
      const long long i = v * K;
      const int p = plane_of(i, n0, n1);
      const long long end = p == 0 ? n0 : (p == 1 ? n1 : N);
      if (i + K <= end) {                              // the whole vector lies in one plane
        u64 s = 0;
#pragma unroll
        for (int j = 0; j < K; ++j) s += sq_at<T>(wa, wb, j, m);
        add_plane(p, s, s0, s1, s2);
      } else {
#pragma unroll
        for (int j = 0; j < K; ++j) add_plane(plane_of(i + j, n0, n1), sq_at<T>(wa, wb, j, m), s0, s1, s2);
      }
    }
    const long long i = nvec * K + t;
    if (blockIdx.x == 0 && t < K && i < N) add_plane(plane_of(i, n0, n1), sq1<T>(a[i], b[i], m), s0, s1, s2);
  } else {
    for (long long i = gid; i < N; i += stride) add_plane(plane_of(i, n0, n1), sq1<T>(a[i], b[i], m), s0, s1, s2);
  }
#pragma unroll
  for (int k = 32; k >= 1; k >>= 1) s0 += shfl_xor_u64(s0, k), s1 += shfl_xor_u64(s1, k), s2 += shfl_xor_u64(s2, k);
  if ((t & 63) == 0) part[0][t >> 6] = s0, part[1][t >> 6] = s1, part[2][t >> 6] = s2;
  __syncthreads();
  if (t < 3) partial[(size_t)t * gridDim.x + blockIdx.x] = part[t][0] + part[t][1] + part[t][2] + part[t][3];
}

// one workgroup: per plane, thread t adds partials t, t + 256, ... in index order, then a tree
__global__ void __launch_bounds__(256) yuv_sse_final_kernel(const u64* __restrict__ partial, int nblk, u64* __restrict__ out3) {
  __shared__ u64 red[256];
  const int t = (int)threadIdx.x;
  for (int p = 0; p < 3; ++p) {
    u64 s = 0;
    for (int i = t; i < nblk; i += 256) s += partial[(size_t)p * nblk + i];
    red[t] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
      if (t < k) red[t] += red[t + k];
      __syncthreads();
    }
    if (t == 0) out3[p] = red[0];
    __syncthreads();
  }
}

template <class T>
int yuv_sse(const T* a, const T* b, int W, long long N, long long n0, long long n1, int m, u64* partial, int nblk, u64* out3,
            hipStream_t stream) {
  const bool vec = W % (16 / (int)sizeof(T)) == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0;
  if (vec) hipLaunchKernelGGL((yuv_sse_kernel<T, true>), dim3(nblk), dim3(256), 0, stream, a, b, N, n0, n1, m, partial);
  else hipLaunchKernelGGL((yuv_sse_kernel<T, false>), dim3(nblk), dim3(256), 0, stream, a, b, N, n0, n1, m, partial);
  ZT_LAUNCH_CHECK();
  hipLaunchKernelGGL(yuv_sse_final_kernel, dim3(1), dim3(256), 0, stream, (const u64*)partial, nblk, out3);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}

// ================================================================ SSIM ====================================================
constexpr int SP_TW = 64;                 // output columns per workgroup

// one entry of the table of horizontal 7-tap sums.  Acc = int: sx and sy share a word (7 * 4095 < 2^16), 7 * 4095^2 < 2^27;
// Acc = long long: 7 * 65535 < 2^19 and 7 * 65535^2 < 2^35
template <class Acc> struct HSum;
template <> struct alignas(16) HSum<int> {
  unsigned xy16, xx, yy, xy;
  __device__ __forceinline__ void set(int sx, int sy, int sxx, int syy, int sxy) {
    xy16 = (unsigned)sx | ((unsigned)sy << 16), xx = (unsigned)sxx, yy = (unsigned)syy, xy = (unsigned)sxy;
  }
  __device__ __forceinline__ int sx() const { return (int)(xy16 & 0xFFFFu); }
  __device__ __forceinline__ int sy() const { return (int)(xy16 >> 16); }
  __device__ __forceinline__ int sxx() const { return (int)xx; }
  __device__ __forceinline__ int syy() const { return (int)yy; }
  __device__ __forceinline__ int sxy() const { return (int)xy; }
};
template <> struct alignas(16) HSum<long long> {
  unsigned x, y;
  long long xx, yy, xy;
  __device__ __forceinline__ void set(int sx, int sy, long long sxx, long long syy, long long sxy) {
    x = (unsigned)sx, y = (unsigned)sy, xx = sxx, yy = syy, xy = sxy;
  }
  __device__ __forceinline__ int sx() const { return (int)x; }
  __device__ __forceinline__ int sy() const { return (int)y; }
  __device__ __forceinline__ long long sxx() const { return xx; }
  __device__ __forceinline__ long long syy() const { return yy; }
  __device__ __forceinline__ long long sxy() const { return xy; }
};

// grid (tiles x, tiles y); workgroup = TH x 64 outputs.  Phase 1 stages the clamped samples of both planes ((TH + 6) rows of
// NG groups of G = 16 / sizeof(T) samples, zeros outside the plane: such samples only reach outputs that are masked), phase 2
// forms the horizontal 7-tap sums of x, y, xx, yy, xy with a running sum over 8 outputs per thread, phase 3 the vertical 7-tap
// sums over TH / 4 outputs per thread, S in fp64 and the block's partial sum.
template <class T, class Acc, int TH, bool VEC>
__global__ void __launch_bounds__(256) ssim_plane_kernel(const T* __restrict__ a, const T* __restrict__ b, int H, int W, int m,
                                                         double* __restrict__ partial) {
  constexpr int IH = TH + 6, G = 16 / (int)sizeof(T), NG = (SP_TW + 6 + G - 1) / G, RO = TH / 4;
  __shared__ uint4 xa[IH * NG], ya[IH * NG];
  __shared__ HSum<Acc> hs[IH * SP_TW];
  __shared__ double red[256];
  const int t = (int)threadIdx.x;
  const int tx0 = (int)blockIdx.x * SP_TW, ty0 = (int)blockIdx.y * TH;

  for (int it = t; it < IH * NG; it += 256) {
    const int r = it / NG, g = it - r * NG;
    const int gy = ty0 + r, gx = tx0 + G * g;
    alignas(16) T va[G], vb[G];
    if (gy >= H || gx >= W) {
#pragma unroll
      for (int k = 0; k < G; ++k) va[k] = 0, vb[k] = 0;
    } else {
      const T* pa = a + (size_t)gy * W + gx;
      const T* pb = b + (size_t)gy * W + gx;
      if (VEC) {                                       // W % G == 0: the group is whole and 16-byte aligned
        __builtin_memcpy(va, __builtin_assume_aligned(pa, 16), 16);
        __builtin_memcpy(vb, __builtin_assume_aligned(pb, 16), 16);
      } else {
#pragma unroll
        for (int k = 0; k < G; ++k) {
          va[k] = gx + k < W ? pa[k] : (T)0;
          vb[k] = gx + k < W ? pb[k] : (T)0;
        }
      }
      if (sizeof(T) == 2) {
#pragma unroll
        for (int k = 0; k < G; ++k) va[k] = (T)min((int)va[k], m), vb[k] = (T)min((int)vb[k], m);
      }
    }
    uint4 qa, qb;
    __builtin_memcpy(&qa, va, 16);
    __builtin_memcpy(&qb, vb, 16);
    xa[it] = qa;
    ya[it] = qb;
  }
  __syncthreads();

  const T* sa = reinterpret_cast<const T*>(xa);
  const T* sb = reinterpret_cast<const T*>(ya);
  for (int it = t; it < IH * (SP_TW / 8); it += 256) {
    const int r = it >> 3, c0 = (it & 7) * 8;
    alignas(16) T ra[16], rb[16];                      // columns c0 .. c0 + 15 of the staged row (c0 + 15 < NG * G)
    __builtin_memcpy(ra, __builtin_assume_aligned(sa + r * (NG * G) + c0, 8 * sizeof(T)), sizeof(ra));
    __builtin_memcpy(rb, __builtin_assume_aligned(sb + r * (NG * G) + c0, 8 * sizeof(T)), sizeof(rb));
    int px[14], py[14];
#pragma unroll
    for (int k = 0; k < 14; ++k) {
      // every sample as a plain 32-bit integer in a register of its own before any arithmetic: left to itself hipcc (HIP 7.2,
      // AMD clang 22.0.0git) folds the byte extraction into sub-dword-addressed adds and 4-way byte dot products, and the
      // sliding sums of the 8-bit kernel then came out wrong on the MI355X (SSIM 2.97 for 0.057 at 30 x 44) while the host
      // emulator and the 7 x 7 case, which has no sliding step, agreed with the reference.  With the samples pinned like this
      // every case of tests/test_planes.py passes on the device.  Observed, not diagnosed down to the instruction.
      px[k] = (int)ra[k], py[k] = (int)rb[k];
      ZT_OPAQUE(px[k]);
      ZT_OPAQUE(py[k]);
    }
    int sx = 0, sy = 0;
    Acc sxx = 0, syy = 0, sxy = 0;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      sx += px[k]; sy += py[k];
      sxx += (Acc)px[k] * px[k]; syy += (Acc)py[k] * py[k]; sxy += (Acc)px[k] * py[k];
    }
#pragma unroll
    for (int o = 0; o < 8; ++o) {
      hs[r * SP_TW + c0 + o].set(sx, sy, sxx, syy, sxy);
      if (o < 7) {
        sx += px[o + 7] - px[o]; sy += py[o + 7] - py[o];
        sxx += (Acc)px[o + 7] * px[o + 7] - (Acc)px[o] * px[o];
        syy += (Acc)py[o + 7] * py[o + 7] - (Acc)py[o] * py[o];
        sxy += (Acc)px[o + 7] * py[o + 7] - (Acc)px[o] * py[o];
      }
    }
  }
  __syncthreads();

  const int col = t & 63, r0 = (t >> 6) * RO;
  const int gx = tx0 + col;
  int sx = 0, sy = 0;
  Acc sxx = 0, syy = 0, sxy = 0;
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    const HSum<Acc> v = hs[(r0 + k) * SP_TW + col];
    sx += v.sx(); sy += v.sy(); sxx += v.sxx(); syy += v.syy(); sxy += v.sxy();
  }
  const double C1 = (0.01 * (double)m) * (0.01 * (double)m), C2 = (0.03 * (double)m) * (0.03 * (double)m), cov_norm = 49.0 / 48.0;
  double acc = 0.0;
#pragma unroll
  for (int o = 0; o < RO; ++o) {
    if (gx < W - 6 && ty0 + r0 + o < H - 6) {
      const double ux = (double)sx / 49.0, uy = (double)sy / 49.0;
      const double vx = cov_norm * ((double)sxx / 49.0 - ux * ux);
      const double vy = cov_norm * ((double)syy / 49.0 - uy * uy);
      const double vxy = cov_norm * ((double)sxy / 49.0 - ux * uy);
      acc += ((2.0 * ux * uy + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2));
    }
    if (o < RO - 1) {
      const HSum<Acc> p = hs[(r0 + o + 7) * SP_TW + col], q = hs[(r0 + o) * SP_TW + col];
      sx += p.sx() - q.sx(); sy += p.sy() - q.sy();
      sxx += p.sxx() - q.sxx(); syy += p.syy() - q.syy(); sxy += p.sxy() - q.sxy();
    }
  }
  red[t] = acc;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (t < k) red[t] += red[t + k];
    __syncthreads();
  }
  if (t == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = red[0];
}

// one workgroup: thread t adds partials t, t + 256, ... in index order, then the same tree as above
__global__ void __launch_bounds__(256) ssim_plane_final_kernel(const double* __restrict__ partial, int n, double nwin, double* __restrict__ out) {
  __shared__ double red[256];
  const int t = (int)threadIdx.x;
  double s = 0.0;
  for (int i = t; i < n; i += 256) s += partial[i];
  red[t] = s;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (t < k) red[t] += red[t + k];
    __syncthreads();
  }
  if (t == 0) out[0] = red[0] / nwin;
}

template <class T, class Acc, int TH>
int ssim_plane(const T* a, const T* b, int H, int W, int m, double* partial, int npartial, double* out, hipStream_t stream) {
  const int ntx = zt_cdiv(W - 6, SP_TW), nty = zt_cdiv(H - 6, TH);
  ZT_REQUIRE((long long)ntx * nty <= (long long)npartial);
  const bool vec = W % (16 / (int)sizeof(T)) == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0;
  if (vec) hipLaunchKernelGGL((ssim_plane_kernel<T, Acc, TH, true>), dim3(ntx, nty), dim3(256), 0, stream, a, b, H, W, m, partial);
  else hipLaunchKernelGGL((ssim_plane_kernel<T, Acc, TH, false>), dim3(ntx, nty), dim3(256), 0, stream, a, b, H, W, m, partial);
  ZT_LAUNCH_CHECK();
  hipLaunchKernelGGL(ssim_plane_final_kernel, dim3(1), dim3(256), 0, stream, (const double*)partial, ntx * nty,
                     (double)(H - 6) * (double)(W - 6), out);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}

bool depth_ok(int depth) { return depth == 8 || depth == 9 || depth == 10 || depth == 12 || depth == 14 || depth == 16; }

}  // namespace

extern "C" int zt_yuv_sse(const void* a, const void* b, int H, int W, int ss, int depth, unsigned long long* partial, int nblk,
                          unsigned long long* out3, hipStream_t stream) {
  ZT_REQUIRE(a && b && partial && out3 && H > 0 && W > 0 && depth_ok(depth) && nblk > 0 && nblk <= 4096);
  ZT_REQUIRE((((uintptr_t)partial | (uintptr_t)out3) & 7) == 0);
  ZT_REQUIRE(ss == 444 || (ss == 422 && W % 2 == 0) || (ss == 420 && W % 2 == 0 && H % 2 == 0));
  const long long n0 = (long long)H * W;
  ZT_REQUIRE(n0 < (1LL << 31));                        // 65535^2 * 2^31 < 2^63: no plane's sum can wrap
  const long long nc = (long long)(ss == 420 ? H / 2 : H) * (ss == 444 ? W : W / 2);
  const int m = (1 << depth) - 1;
  if (depth == 8)
    return yuv_sse((const unsigned char*)a, (const unsigned char*)b, W, n0 + 2 * nc, n0, n0 + nc, m, partial, nblk, out3, stream);
  ZT_REQUIRE((((uintptr_t)a | (uintptr_t)b) & 1) == 0);
  return yuv_sse((const uint16_t*)a, (const uint16_t*)b, W, n0 + 2 * nc, n0, n0 + nc, m, partial, nblk, out3, stream);
}

extern "C" int zt_ssim_plane(const void* a, const void* b, int H, int W, int depth, double* partial, int npartial, double* out,
                             hipStream_t stream) {
  ZT_REQUIRE(a && b && partial && out && depth_ok(depth) && H >= 7 && W >= 7 && H <= (1 << 20) && W <= (1 << 20));
  ZT_REQUIRE((((uintptr_t)partial | (uintptr_t)out) & 7) == 0);
  const int m = (1 << depth) - 1;
  if (depth == 8) return ssim_plane<unsigned char, int, 32>((const unsigned char*)a, (const unsigned char*)b, H, W, m, partial, npartial, out, stream);
  ZT_REQUIRE((((uintptr_t)a | (uintptr_t)b) & 1) == 0);
  if (depth <= 12) return ssim_plane<uint16_t, int, 32>((const uint16_t*)a, (const uint16_t*)b, H, W, m, partial, npartial, out, stream);
  return ssim_plane<uint16_t, long long, 16>((const uint16_t*)a, (const uint16_t*)b, H, W, m, partial, npartial, out, stream);
}
