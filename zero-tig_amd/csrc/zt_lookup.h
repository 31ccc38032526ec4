// What the RAFT lookups share: the 9 x 9 bilinear window of corr.py:29-50 from the window coordinate onwards, the flow bookkeeping
// of raft.py:112-120 and the 2 x 2 pooling order of the pyramids.  corr_lookup_kernel / flow_step_kernel / corr_pool_kernel
// (zt_raft.hip) and corr_alt_lookup_kernel / fmap_pyramid_kernel (zt_corr_alt.hip) are bit-identical where they compute the same
// thing because they call the one definition here (tests/test_corr_alt.py, tests/test_raft_loop.py).
#pragma once
#include "zt_common.h"

// Flow bookkeeping of the PREVIOUS refinement iteration (raft.py:112-120), fused into a lookup (zt_corr_lookup_step,
// zt_corr_alt_lookup_step) or on its own (zt_raft_flow_step): the coordinates looked up are coords + delta, written to coords_out (in
// a lookup a different buffer: other threads of the pixel still read coords) together with flow = coords_out - grid for the
// up-sampler (f4, fp32) and the two nhwc consumers of the same iteration (fhx, fin; the kernel's storage type T)
struct ZtFlowBook {
  const float* delta;       // [npx][ldd] (x, y), NULL: nothing to add
  float* coords_out;        // [npx][2]
  float* f4;
  void* fhx;
  void* fin;
  int ldd, ldf4, ldfhx, ldfin, w0;
};

// what a lookup launcher requires of its book; coords = the coordinates the lookup reads
static inline bool zt_flow_book_ok(const ZtFlowBook& b, const float* coords) {
  if (b.coords_out && b.coords_out == coords) return false;
  return !b.delta || b.coords_out;                  // a delta that is looked up but not recorded would be lost
}

// Sizes of the four pyramid levels over an h x w map (floor halving, corr.py:25-27).  false: a level has a single row or column,
// which divides by zero in the reference (SURVEY A-13)
static inline bool zt_lookup_levels(int h, int w, int (&hl)[4], int (&wl)[4]) {
  for (int l = 0; l < 4; ++l) {
    hl[l] = h; wl[l] = w;
    if (h < 2 || w < 2) return false;
    h /= 2; w /= 2;
  }
  return true;
}

// avg_pool2d(2, stride 2) of one cell, in the order every pyramid here sums its four sources (zt_corr.hip pools its own way)
__device__ __forceinline__ float zt_pool4(float a, float b, float c, float d) { return (((a + b) + c) + d) * 0.25f; }

// the coordinate pixel n looks up: coords + the pending delta, one fp32 add, so every kernel that forms it gets the same bits
__device__ __forceinline__ void zt_lookup_coords(const float* coords, const ZtFlowBook& b, int n, float* px, float* py) {
  *px = coords[(size_t)n * 2 + 0];
  *py = coords[(size_t)n * 2 + 1];
  if (b.delta) {
    *px += b.delta[(size_t)n * b.ldd + 0];
    *py += b.delta[(size_t)n * b.ldd + 1];
  }
}

template <typename T>
__device__ __forceinline__ void zt_flow_store(void* dst, size_t o, float fx, float fy) {
  if (!dst) return;
  ZtIO<T>::st((T*)dst + o + 0, fx);
  ZtIO<T>::st((T*)dst + o + 1, fy);
}

// records pixel n's coordinate (px, py) and its flow in every destination of the book that is not NULL (one thread per pixel)
template <typename T>
__device__ __forceinline__ void zt_flow_record(const ZtFlowBook& b, int n, float px, float py) {
  zt_flow_store<float>(b.coords_out, (size_t)n * 2, px, py);
  const float fx = px - (float)(n % b.w0), fy = py - (float)(n / b.w0);
  zt_flow_store<float>(b.f4, (size_t)n * b.ldf4, fx, fy);
  zt_flow_store<T>(b.fhx, (size_t)n * b.ldfhx, fx, fy);
  zt_flow_store<T>(b.fin, (size_t)n * b.ldfin, fx, fy);
}

// the tap coordinate of window position i along one axis of level l (corr.py:37-43 + utils.py:285-299, align_corners=True):
// returns the lower tap and the weight of the upper one.  The clamp keeps every later index inside [-2, size + 1] for huge,
// infinite and NaN coordinates
__device__ __forceinline__ int zt_lookup_tap(float p, int l, int i, int size, float* w1) {
  float c = p / (float)(1 << l) + (float)(i - 4);
  float g = 2.f * c / (float)(size - 1) - 1.f;
  float ic = (g + 1.f) * ((float)(size - 1) / 2.f);
  float f0 = floorf(ic);
  *w1 = ic - f0;
  return (int)fminf(fmaxf(f0, -2.f), (float)size + 1.f);
}

// bilinear sample of a W x H map at lower taps (x0, y0) with upper weights (wx1, wy1), zeros padding; tap(xx, yy) -> float reads a
// point inside the map
template <typename F>
__device__ __forceinline__ float zt_lookup_sample(int x0, int y0, float wx1, float wy1, int W, int H, F&& tap) {
  const float wx0 = 1.f - wx1, wy0 = 1.f - wy1;
  auto at = [&](int xx, int yy) { return (xx >= 0 && xx < W && yy >= 0 && yy < H) ? tap(xx, yy) : 0.f; };
  float v = at(x0, y0) * (wx0 * wy0);
  v = fmaf(at(x0 + 1, y0), wx1 * wy0, v);
  v = fmaf(at(x0, y0 + 1), wx0 * wy1, v);
  return fmaf(at(x0 + 1, y0 + 1), wx1 * wy1, v);
}
