// Scene cuts in a raw video stream (predict.py --y4m_scene_cut, zero-tig_amd/scenecut.py): the two integer passes of DESIGN 8e.
//   grid  the luma plane Y [H][W] (uint8) is cut into 16 x 16 cells, gh = ceil(H / 16) rows of gw = ceil(W / 16); edge cells hold
//         the pixels that exist.  G[i][j] = sum over the cell of max(Y - yo, 0), uint32 (at most 256 * 255).  A plane of B = 9 .. 16
//         bits (uint16) is read at 8 bits: min(Y, 2^B - 1) >> (B - 8) in place of Y.
//   pair  sad = sum |a[k] - b[k]|, tot = sum (a[k] + b[k]) over two grids, both uint64 (a 4K grid of saturated cells passes 2^32).
// The host divides (scenecut.py).  Integer, no atomics, every output word has one owner: deterministic.
// A frame is 2 MB and a grid 32 KB: the launches are what costs, so each pass is ONE kernel with one dependent phase of loads.
//   grid  a lane per cell, cells numbered along the grid's rows, 64 per workgroup: with W % 16 == 0 and a 16-byte aligned plane a
//         lane issues the 16 row loads of its cell (16 bytes each, a wave reads 1 KB runs along a row) before the first add (uint16:
//         32 loads, as two batches of 8 rows); cells cut by the bottom edge, and every cell of any other width or alignment, take
//         single-sample loads with the same arithmetic.
//   pair  one workgroup of 1024 lanes, 16-byte loads when both grids are aligned; wave sums by shuffles, 16 partial pairs in LDS.
#include "zt_common.h"

namespace {

constexpr int CELL = 16;

// one sample's term: bytes as they are; shorts of depth B hold a value up to m = 2^B - 1 (above it: m), taken at 8 bits (sh = B - 8)
template <class T>
__device__ __forceinline__ unsigned term(int Y, int m, int sh, int yo) {
  return (unsigned)max((sizeof(T) == 1 ? Y : min(Y, m) >> sh) - yo, 0);
}

// the terms of the 16 / sizeof(T) samples of a 16-byte load
template <class T>
__device__ __forceinline__ unsigned term_sum(uint4 v, int m, int sh, int yo) {
  constexpr int BITS = 8 * sizeof(T);
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
  unsigned s = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 32 / BITS; ++j) s += term<T>((int)((w[i] >> (BITS * j)) & ((1u << BITS) - 1u)), m, sh, yo);
  return s;
}

template <class T, bool VEC>
__global__ void __launch_bounds__(64) luma_grid_kernel(const T* __restrict__ y, int H, int W, int m, int sh, int yo, int gh, int gw,
                                                       unsigned* __restrict__ grid) {
  const int g = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (g >= gh * gw) return;
  const int r0 = (g / gw) * CELL, c0 = (g % gw) * CELL;
  const T* p = y + (size_t)r0 * W + c0;
  unsigned s = 0;
  if (VEC && r0 + CELL <= H) {                       // W % 16 == 0: the cell is whole, sizeof(T) loads of 16 bytes a row
    constexpr int NB = sizeof(T);
#pragma unroll
    for (int b = 0; b < NB; ++b) {                   // a batch is 16 loads: CELL / NB rows
      uint4 v[CELL];
#pragma unroll
      for (int i = 0; i < CELL; ++i) v[i] = *reinterpret_cast<const uint4*>(p + (size_t)(CELL / NB * b + i / NB) * W + 16 / NB * (i % NB));
      __builtin_amdgcn_sched_barrier(0);             // all 16 loads in flight before the first add (hipcc interleaves them otherwise)
#pragma unroll
      for (int i = 0; i < CELL; ++i) s += term_sum<T>(v[i], m, sh, yo);
    }
  } else {
    const int nr = min(CELL, H - r0), nc = min(CELL, W - c0);
    for (int r = 0; r < nr; ++r)
      for (int c = 0; c < nc; ++c) s += term<T>((int)p[(size_t)r * W + c], m, sh, yo);
  }
  grid[g] = s;
}

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int m) {
  const unsigned lo = __shfl_xor((unsigned)v, m), hi = __shfl_xor((unsigned)(v >> 32), m);
  return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ void sad_add(unsigned a, unsigned b, unsigned long long& sad, unsigned long long& tot) {
  sad += a > b ? a - b : b - a;
  tot += (unsigned long long)a + b;
}

constexpr int SAD_T = 1024;

template <bool VEC>
__global__ void __launch_bounds__(SAD_T) grid_sad_kernel(const unsigned* __restrict__ a, const unsigned* __restrict__ b, int n,
                                                         unsigned long long* __restrict__ out2) {
  __shared__ unsigned long long part[2][SAD_T / 64];
  const int t = (int)threadIdx.x;
  unsigned long long sad = 0, tot = 0;
  const int nv = VEC ? n >> 2 : 0;
  for (int i = t; i < nv; i += SAD_T) {
    const uint4 va = reinterpret_cast<const uint4*>(a)[i], vb = reinterpret_cast<const uint4*>(b)[i];
    sad_add(va.x, vb.x, sad, tot), sad_add(va.y, vb.y, sad, tot), sad_add(va.z, vb.z, sad, tot), sad_add(va.w, vb.w, sad, tot);
  }
  for (int i = 4 * nv + t; i < n; i += SAD_T) sad_add(a[i], b[i], sad, tot);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) sad += shfl_xor_u64(sad, m), tot += shfl_xor_u64(tot, m);
  if ((t & 63) == 0) part[0][t >> 6] = sad, part[1][t >> 6] = tot;
  __syncthreads();
  if (t < 2) {                                        // lane 0 owns sad, lane 1 owns tot
    unsigned long long s = 0;
    for (int w = 0; w < SAD_T / 64; ++w) s += part[t][w];
    out2[t] = s;
  }
}

template <class T>
int luma_grid(const T* y, int H, int W, int m, int sh, int yo, unsigned int* grid, hipStream_t stream) {
  const int gh = zt_cdiv(H, CELL), gw = zt_cdiv(W, CELL);
  ZT_REQUIRE((long long)gh * gw <= 0x7fffffffLL - 64);
  const dim3 blocks((unsigned)zt_cdiv(gh * gw, 64)), block(64);
  if (W % 16 == 0 && ((uintptr_t)y & 15) == 0) hipLaunchKernelGGL((luma_grid_kernel<T, true>), blocks, block, 0, stream, y, H, W, m, sh, yo, gh, gw, grid);
  else hipLaunchKernelGGL((luma_grid_kernel<T, false>), blocks, block, 0, stream, y, H, W, m, sh, yo, gh, gw, grid);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}

}  // namespace

extern "C" int zt_luma_grid_u8(const unsigned char* y, int H, int W, int yo, unsigned int* grid, hipStream_t stream) {
  ZT_REQUIRE(y && grid && H > 0 && W > 0 && yo >= 0 && yo <= 255 && ((uintptr_t)grid & 3) == 0);
  return luma_grid(y, H, W, 255, 0, yo, grid, stream);
}

extern "C" int zt_luma_grid_u16(const uint16_t* y, int H, int W, int depth, int yo8, unsigned int* grid, hipStream_t stream) {
  ZT_REQUIRE(y && grid && H > 0 && W > 0 && yo8 >= 0 && yo8 <= 255 && ((uintptr_t)y & 1) == 0 && ((uintptr_t)grid & 3) == 0);
  ZT_REQUIRE(depth == 9 || depth == 10 || depth == 12 || depth == 14 || depth == 16);
  return luma_grid(y, H, W, (1 << depth) - 1, depth - 8, yo8, grid, stream);
}

extern "C" int zt_grid_sad_u32(const unsigned int* a, const unsigned int* b, int n, unsigned long long* out2, hipStream_t stream) {
  ZT_REQUIRE(a && b && out2 && n > 0 && (((uintptr_t)a | (uintptr_t)b) & 3) == 0 && ((uintptr_t)out2 & 7) == 0);
  const dim3 blocks(1), block(SAD_T);
  if ((((uintptr_t)a | (uintptr_t)b) & 15) == 0) hipLaunchKernelGGL(grid_sad_kernel<true>, blocks, block, 0, stream, a, b, n, out2);
  else hipLaunchKernelGGL(grid_sad_kernel<false>, blocks, block, 0, stream, a, b, n, out2);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}
