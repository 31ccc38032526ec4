// Stencil primitives of the Zero-TIG hot path on planar fp32 [C][H][W] tensors, with the adjoints the
// hand-written backward pass needs.  All are HBM-bound (a few reads + one write per element).
//   pair_downsampler      utils/utils.py:15-24
//   blur (21x21 Gaussian) utils/utils.py:26-39, 52-58      (rank-1 kernel -> two 21-tap passes)
//   LocalMean             utils/utils.py:41-50
//   calculate_local_variance utils/utils.py:60-79
//   TextureDifference     loss.py:99-136
//   SmoothLoss.rgb2yCbCr  loss.py:178-190
#include "zt_common.h"

namespace {

// ------------------------------------------------------------------------------------------------ pair downsample
__global__ void __launch_bounds__(256) pair_down_kernel(const float* __restrict__ src, float* __restrict__ o1,
                                                        float* __restrict__ o2, int C, int H, int W, int h, int w) {
  int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x >= w || y >= h) return;
  for (int c = 0; c < C; ++c) {
    const float* p = src + (size_t)c * H * W + (size_t)(2 * y) * W + 2 * x;
    float a = p[0], b = p[1], cc = p[W], d = p[W + 1];
    o1[(size_t)c * h * w + (size_t)y * w + x] = 0.5f * b + 0.5f * cc;
    o2[(size_t)c * h * w + (size_t)y * w + x] = 0.5f * a + 0.5f * d;
  }
}

// dst (+)= adjoint(pair_down)(g1, g2); rows/cols beyond 2h/2w receive zero
__global__ void __launch_bounds__(256) pair_down_adj_kernel(const float* __restrict__ g1, const float* __restrict__ g2,
                                                            float* __restrict__ dst, int C, int H, int W, int h, int w,
                                                            int accumulate) {
  int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x >= W || y >= H) return;
  int hy = y >> 1, hx = x >> 1;
  bool inside = hy < h && hx < w;
  bool diag = ((y ^ x) & 1) == 0;       // (even,even) and (odd,odd) feed output 2; the anti-diagonal feeds output 1
  for (int c = 0; c < C; ++c) {
    float v = 0.f;
    if (inside) v = 0.5f * (diag ? g2 : g1)[(size_t)c * h * w + (size_t)hy * w + hx];
    size_t o = (size_t)c * H * W + (size_t)y * W + x;
    dst[o] = accumulate ? dst[o] + v : v;
  }
}

// ------------------------------------------------------------------------------------------------ 21-tap separable blur
struct Taps21 {
  float t[21];
};

// adjoint of one reflect-padded pass: g_ext(u) = sum_j t_j * gy(u - j) on the extended domain, folded back
template <bool VERT>
__device__ __forceinline__ float blur_ext(const float* __restrict__ p, int fixed, int u, int n, int W, const Taps21& k) {
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < 21; ++j) {
    int i = u - (j - 10);
    if (i >= 0 && i < n) acc = fmaf(k.t[j], VERT ? p[(size_t)i * W + fixed] : p[(size_t)fixed * W + i], acc);
  }
  return acc;
}

// Vertical passes as a register sliding window: a thread owns one column and BRY consecutive output rows, loads the BRY + 20
// inputs it needs once (coalesced across the wave) and keeps them in registers -- 2.25 loads per output instead of 21 that
// miss L1 (rows are 7.7 KB apart).  Same fmaf order as the plain kernels: bit-identical results.
constexpr int BRY = 16;

template <bool ADJ>
__global__ void __launch_bounds__(256) blur_vert_kernel(const float* __restrict__ src, float* __restrict__ dst, int C, int H, int W,
                                                        Taps21 k, int accumulate) {
  const int x = blockIdx.x * 64 + threadIdx.x;
  const int r0 = (blockIdx.y * 4 + threadIdx.y) * BRY;
  if (x >= W || r0 >= H) return;
  for (int c = 0; c < C; ++c) {
    const float* p = src + (size_t)c * H * W;
    float win[BRY + 20];
#pragma unroll
    for (int m = 0; m < BRY + 20; ++m) {
      const int i = r0 - 10 + m;
      if (ADJ) win[m] = (i >= 0 && i < H) ? p[(size_t)i * W + x] : 0.f;                // extended-domain correlation: zero outside
      else win[m] = p[(size_t)zt_reflect(i < H + 10 ? i : H + 9, H) * W + x];           // reflect padding (rows past the last segment unused)
    }
#pragma unroll
    for (int r = 0; r < BRY; ++r) {
      const int y = r0 + r;
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < 21; ++j) acc = fmaf(k.t[j], ADJ ? win[r + 20 - j] : win[r + j], acc);
      if (y < H) {
        const size_t o = (size_t)c * H * W + (size_t)y * W + x;
        dst[o] = (ADJ && accumulate) ? dst[o] + acc : acc;
      }
    }
  }
}

// Horizontal passes through an LDS row segment (256 outputs + 20 halo): one coalesced global load per input, 21 conflict-free
// LDS reads per output; same fmaf order as the plain kernels.
template <bool ADJ>
__global__ void __launch_bounds__(256) blur_horz_kernel(const float* __restrict__ src, float* __restrict__ dst, int C, int H, int W,
                                                        Taps21 k, int accumulate) {
  __shared__ float buf[256 + 20];
  const int x0 = blockIdx.x * 256, y = blockIdx.y, x = x0 + threadIdx.x;
  for (int c = 0; c < C; ++c) {
    const float* p = src + ((size_t)c * H + y) * W;
    for (int i = threadIdx.x; i < 256 + 20; i += 256) {
      const int gx = x0 - 10 + i;
      if (ADJ) buf[i] = (gx >= 0 && gx < W) ? p[gx] : 0.f;
      else buf[i] = p[zt_reflect(gx < W + 10 ? gx : W + 9, W)];
    }
    __syncthreads();
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 21; ++j) acc = fmaf(k.t[j], ADJ ? buf[threadIdx.x + 20 - j] : buf[threadIdx.x + j], acc);
    if (x < W) {
      const size_t o = ((size_t)c * H + y) * W + x;
      dst[o] = (ADJ && accumulate) ? dst[o] + acc : acc;
    }
    __syncthreads();
  }
}

// second half of the horizontal adjoint: fold columns 1..10 and W-11..W-2, then (optionally) accumulate into the destination
__global__ void __launch_bounds__(256) blur_horz_fold_kernel(const float* __restrict__ src, float* __restrict__ dst, int C, int H, int W,
                                                             Taps21 k) {
  const int y = blockIdx.x * 256 + threadIdx.x;
  const bool left = blockIdx.y < 10;                            // W > 21: the two column groups are disjoint
  const int x = left ? 1 + blockIdx.y : W - 11 + (blockIdx.y - 10);
  if (y >= H) return;
  for (int c = 0; c < C; ++c) {
    const float* p = src + (size_t)c * H * W;
    dst[(size_t)c * H * W + (size_t)y * W + x] += blur_ext<false>(p, y, left ? -x : 2 * (W - 1) - x, W, W, k);
  }
}

// second half of the vertical adjoint: fold the reflected borders back into rows 1..10 and H-11..H-2 (20 rows only)
__global__ void __launch_bounds__(256) blur_vert_fold_kernel(const float* __restrict__ src, float* __restrict__ dst, int C, int H, int W,
                                                             Taps21 k) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  const bool top = blockIdx.y < 10;                             // H > 21 (checked by the launcher): the two row groups are disjoint
  const int y = top ? 1 + blockIdx.y : H - 11 + (blockIdx.y - 10);
  if (x >= W) return;
  for (int c = 0; c < C; ++c) {
    const float* p = src + (size_t)c * H * W;
    const size_t o = (size_t)c * H * W + (size_t)y * W + x;
    dst[o] += blur_ext<true>(p, x, top ? -y : 2 * (H - 1) - y, H, W, k);
  }
}

// ------------------------------------------------------------------------------------------------ 5x5 tiles
// Every 5x5 kernel below works on a 64 x 16 output tile with a 64 x 4 block: the inputs are staged once in LDS with their
// halo (coalesced loads) and the taps come from LDS, in the order of the per-pixel global gathers they replace.
constexpr int TX = 64, TY = 16;
constexpr int PW = TX + 4, PH = TY + 4;      // tile with the +-2 halo of one 5x5 window
constexpr int XW = TX + 8, XH = TY + 8;      // tile with the +-4 halo of two stacked windows

inline dim3 tile_grid(int W, int H, int C) { return dim3(zt_cdiv(W, TX), zt_cdiv(H, TY), C); }

__device__ __forceinline__ bool in_image(int gy, int gx, int H, int W) { return gy >= 0 && gy < H && gx >= 0 && gx < W; }

// in-image offset of the reflect-padded pixel (slots past the reflected border are never used)
__device__ __forceinline__ size_t reflect_at(int gy, int gx, int H, int W) {
  return (size_t)zt_reflect(gy < H + 2 ? gy : H + 1, H) * W + zt_reflect(gx < W + 2 ? gx : W + 1, W);
}

// in-image offset of the nearest pixel: the reflect adjoints read the tile only for pixels at least three away from every
// border, whose 25 sources are all inside the image
__device__ __forceinline__ size_t clamp_at(int gy, int gx, int H, int W) {
  gy = gy < 0 ? 0 : (gy >= H ? H - 1 : gy);
  gx = gx < 0 ? 0 : (gx >= W ? W - 1 : gx);
  return (size_t)gy * W + gx;
}

// t[k][ly][lx] = v[k] of load(gy, gx, v) over the tile at (x0, y0) with its +-HALO halo: (gy, gx) = (y0 + ly - HALO,
// x0 + lx - HALO) may lie outside the image, the loader decides what such a slot holds
template <int HALO, int K, typename F>
__device__ __forceinline__ void tile_fill(float (*t)[TY + 2 * HALO][TX + 2 * HALO], int x0, int y0, F load) {
  constexpr int TW = TX + 2 * HALO, TH = TY + 2 * HALO;
  for (int i = threadIdx.y * 64 + threadIdx.x; i < TH * TW; i += 256) {
    const int ly = i / TW, lx = i - ly * TW;
    float v[K];
    load(y0 + ly - HALO, x0 + lx - HALO, v);
#pragma unroll
    for (int k = 0; k < K; ++k) t[k][ly][lx] = v[k];
  }
}

// f(ly, lx, y, x) for the thread's pixels of the tile that lie inside the H x W image: column threadIdx.x, rows threadIdx.y + 4 j
template <typename F>
__device__ __forceinline__ void for_owned(int x0, int y0, int H, int W, F f) {
  const int lx = threadIdx.x, x = x0 + lx;
#pragma unroll
  for (int j = 0; j < TY / 4; ++j) {
    const int ly = threadIdx.y + 4 * j, y = y0 + ly;
    if (x < W && y < H) f(ly, lx, y, x);
  }
}

// The 5-tap sums of the separable boxes, left to right and top to bottom (the bit-exact tests replay this order).
// dst[r][c] = sum_{dx < 5} src[r][c + dx], or of its square: ROWS x DW sums from rows of SW floats
template <int ROWS, int SW, int DW, bool SQUARE>
__device__ __forceinline__ void row_sums5(const float* src, float* dst) {
  for (int i = threadIdx.y * 64 + threadIdx.x; i < ROWS * DW; i += 256) {
    const int r = i / DW, c = i - r * DW;
    float v[5];
#pragma unroll
    for (int dx = 0; dx < 5; ++dx) {
      const float s = src[r * SW + c + dx];
      v[dx] = SQUARE ? s * s : s;
    }
    dst[r * DW + c] = (((v[0] + v[1]) + v[2]) + v[3]) + v[4];
  }
}

template <int LD>
__device__ __forceinline__ float col_sum5(const float* p) {
  return (((p[0] + p[LD]) + p[2 * LD]) + p[3 * LD]) + p[4 * LD];
}

// ------------------------------------------------------------------------------------------------ 5x5 reflect mean
__global__ void __launch_bounds__(256) box5_reflect_kernel(const float* __restrict__ src, float* __restrict__ dst, int C,
                                                           int H, int W) {
  __shared__ float t[PH][PW];
  const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
  const size_t plane = (size_t)blockIdx.z * H * W;
  const float* p = src + plane;
  tile_fill<2, 1>(&t, x0, y0, [&](int gy, int gx, float (&v)[1]) { v[0] = p[reflect_at(gy, gx, H, W)]; });
  __syncthreads();
  for_owned(x0, y0, H, W, [&](int ly, int lx, int y, int x) {
    float acc = 0.f;
#pragma unroll
    for (int dy = 0; dy < 5; ++dy)
#pragma unroll
      for (int dx = 0; dx < 5; ++dx) acc += t[ly + dy][lx + dx];
    dst[plane + (size_t)y * W + x] = acc / 25.f;
  });
}

__device__ __forceinline__ int fold_sources(int k, int n, int* u) {
  int m = 0;
  u[m++] = k;
  if (k >= 1 && k <= 2) u[m++] = -k;
  if (k <= n - 2 && k >= n - 3) u[m++] = 2 * (n - 1) - k;
  return m;
}

// adjoint(box5_reflect)(src) at (y, x), before the /25: pixels at least three away from every border have one fold source per
// axis and all 25 taps inside the image -- they read the staged tile t (t[ly + 2][lx + 2] is the pixel itself); the others
// gather from global memory with the folds.  Same dy, dx order on both paths.
__device__ __forceinline__ float b5_adj_sum(const float* __restrict__ p, const float (*t)[PW], int ly, int lx, int y, int x,
                                            int H, int W) {
  float acc = 0.f;
  if (y >= 3 && y < H - 3 && x >= 3 && x < W - 3) {
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
      for (int dx = -2; dx <= 2; ++dx) acc += t[ly + 2 - dy][lx + 2 - dx];
    return acc;
  }
  int uy[3], ux[3];
  const int ny = fold_sources(y, H, uy), nx = fold_sources(x, W, ux);
  for (int a = 0; a < ny; ++a)
    for (int b = 0; b < nx; ++b)
      for (int dy = -2; dy <= 2; ++dy) {
        int yy = uy[a] - dy;
        if (yy < 0 || yy >= H) continue;
        for (int dx = -2; dx <= 2; ++dx) {
          int xx = ux[b] - dx;
          if (xx >= 0 && xx < W) acc += p[(size_t)yy * W + xx];
        }
      }
  return acc;
}

// dst = scale_out * adjoint(box5_reflect)(src)   (accumulate: dst += ...)
__global__ void __launch_bounds__(256) box5_reflect_adj_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                               int C, int H, int W, float scale, int accumulate) {
  __shared__ float t[PH][PW];
  const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
  const size_t plane = (size_t)blockIdx.z * H * W;
  const float* p = src + plane;
  tile_fill<2, 1>(&t, x0, y0, [&](int gy, int gx, float (&v)[1]) { v[0] = p[clamp_at(gy, gx, H, W)]; });
  __syncthreads();
  for_owned(x0, y0, H, W, [&](int ly, int lx, int y, int x) {
    const float acc = b5_adj_sum(p, t, ly, lx, y, x, H, W) / 25.f * scale;
    const size_t o = plane + (size_t)y * W + x;
    dst[o] = accumulate ? dst[o] + acc : acc;
  });
}

// dst[C][H][W] = adjoint(pair_down)(g1 - adjoint(box5_reflect)(u1), g2 - adjoint(box5_reflect)(u2)) in one pass over the
// half-resolution tiles: what box5_reflect_adj (scale -1, accumulate) twice and pair_down_adj did through two read-modify-
// write passes of g1 / g2.  A thread owns one half-resolution pixel and writes its 2 x 2 full-resolution block (0.5 g2 on the
// diagonal, 0.5 g1 off it); rows / columns at or beyond 2h / 2w are zeroed by the last half-resolution row / column.
__global__ void __launch_bounds__(256) half_bwd_kernel(const float* __restrict__ u1, const float* __restrict__ u2,
                                                       const float* __restrict__ g1, const float* __restrict__ g2,
                                                       float* __restrict__ dst, int C, int H, int W, int h, int w) {
  __shared__ float t[2][PH][PW];
  const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
  const size_t hplane = (size_t)blockIdx.z * h * w;
  const float* p1 = u1 + hplane;
  const float* p2 = u2 + hplane;
  tile_fill<2, 2>(t, x0, y0, [&](int gy, int gx, float (&v)[2]) {
    const size_t o = clamp_at(gy, gx, h, w);
    v[0] = p1[o];
    v[1] = p2[o];
  });
  __syncthreads();
  float* d = dst + (size_t)blockIdx.z * H * W;
  const bool pair = (W & 1) == 0 && ((uintptr_t)dst & 7) == 0;   // even rows on an aligned base: the two pixels of a row are one 8-byte store
  for_owned(x0, y0, h, w, [&](int ly, int lx, int y, int x) {
    const size_t ho = hplane + (size_t)y * w + x;
    const float a1 = b5_adj_sum(p1, t[0], ly, lx, y, x, h, w) / 25.f * -1.f;
    const float a2 = b5_adj_sum(p2, t[1], ly, lx, y, x, h, w) / 25.f * -1.f;
    const float v1 = 0.5f * (g1[ho] + a1), v2 = 0.5f * (g2[ho] + a2);
    float* r0 = d + (size_t)(2 * y) * W + 2 * x;
    float* r1 = r0 + W;
    if (pair) {
      *reinterpret_cast<float2*>(r0) = make_float2(v2, v1);
      *reinterpret_cast<float2*>(r1) = make_float2(v1, v2);
    } else {
      r0[0] = v2; r0[1] = v1;
      r1[0] = v1; r1[1] = v2;
    }
    const bool lastx = x == w - 1 && 2 * w < W, lasty = y == h - 1 && 2 * h < H;
    if (lastx) r0[2] = r1[2] = 0.f;
    if (lasty) {
      r1[W] = r1[W + 1] = 0.f;
      if (lastx) r1[W + 2] = 0.f;
    }
  });
}

// ------------------------------------------------------------------------------------------------ local variance (zero pad)
// Both 5x5 boxes are separable in LDS (5 + 5 reads per output instead of 25, halo ratio 1.7 instead of 2.5): the 32 x 8 /
// 25-tap form ran at ~0.9 TB/s of its 50-100 MB.  One pipeline for K maps per tile: stage the +-4 tile (zero outside the
// image), row sums, column sums + the pointwise step into the +-2 tile, row sums, column sums + the epilogue.  Per element:
// row sums left to right, column sums top to bottom, then / 25.
//
// forward: D = x - box0(x)/25 ; V = box0(D^2)/25 for every map.
//   K = 1: x = a, or a - b when b != nullptr; D0 may be null.
//   K = 2: x0 = a, x1 = b - a -- localvar(a) and localvar(b - a) in one launch with a and b loaded once.
template <int K>
__global__ void __launch_bounds__(256) localvar_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                           float* __restrict__ D0, float* __restrict__ V0,
                                                           float* __restrict__ D1, float* __restrict__ V1, int C, int H,
                                                           int W) {
  __shared__ float xs[K][XH][XW];
  __shared__ float hs[K][XH][PW];
  __shared__ float ds[K][PH][PW];
  const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
  const size_t plane = (size_t)blockIdx.z * H * W;
  const float* pa = a + plane;
  const float* pb = b ? b + plane : nullptr;
  float* const Dd[2] = {D0, D1};
  float* const Vd[2] = {V0, V1};
  tile_fill<4, K>(xs, x0, y0, [&](int gy, int gx, float (&x)[K]) {
    const bool in = in_image(gy, gx, H, W);
    const size_t o = (size_t)(in ? gy : 0) * W + (in ? gx : 0);   // outside: load pixel (0, 0), then select 0
    const float va = pa[o];
    if constexpr (K == 1) {
      float v = va;
      if (pb) v -= pb[o];
      x[0] = in ? v : 0.f;
    } else {
      float v = pb[o];
      v -= va;
      x[0] = in ? va : 0.f;
      x[1] = in ? v : 0.f;
    }
  });
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) row_sums5<XH, XW, PW, false>(&xs[k][0][0], &hs[k][0][0]);
  __syncthreads();
  tile_fill<2, K>(ds, x0, y0, [&](int gy, int gx, float (&d)[K]) {
    const int r = gy - y0 + 2, cc = gx - x0 + 2;
    const bool in = in_image(gy, gx, H, W);
    const bool owned = r >= 2 && r < TY + 2 && cc >= 2 && cc < TX + 2;   // D is written by the tile that owns the pixel
#pragma unroll
    for (int k = 0; k < K; ++k) {
      d[k] = 0.f;
      if (in) {
        d[k] = xs[k][r + 2][cc + 2] - col_sum5<PW>(&hs[k][r][cc]) / 25.f;
        if (Dd[k] && owned) Dd[k][plane + (size_t)gy * W + gx] = d[k];
      }
    }
  });
  __syncthreads();
  float* const h2[2] = {&hs[0][0][0], &hs[K - 1][0][0]};             // hs is dead: 20 x 64 row sums per map fit its 24 x 68
#pragma unroll
  for (int k = 0; k < K; ++k) row_sums5<PH, PW, TX, true>(&ds[k][0][0], h2[k]);
  __syncthreads();
  for_owned(x0, y0, H, W, [&](int ly, int lx, int y, int x) {
#pragma unroll
    for (int k = 0; k < K; ++k) Vd[k][plane + (size_t)y * W + x] = col_sum5<TX>(h2[k] + ly * TX + lx) / 25.f;
  });
}

// backward: with S = box0(gV)/25 (gV staged and S formed once per tile slot) and E_k = 2 D_k S, v_k = E_k - box0(E_k)/25.
//   K = 1: out0 (+)= sign * v_0.
//   K = 2 (D0 = DN, D1 = DH2, out0 = dH3, out1 = dH2x): dH3 += -v_N and dH2x = v_H + v_N -- localvar_bwd(DN, gV, -1,
//   accumulate), localvar_bwd(DH2, gV, +1) and localvar_bwd(DN, gV, +1, accumulate) with the DN stencil evaluated once and
//   dH2x written once.
template <int K>
__global__ void __launch_bounds__(256) localvar_bwd_kernel(const float* __restrict__ D0, const float* __restrict__ D1,
                                                           const float* __restrict__ gV, float* __restrict__ out0,
                                                           float* __restrict__ out1, int C, int H, int W, float sign,
                                                           int accumulate) {
  static_assert(K == 1 || K == 2, "one dead buffer per map for the second row sums");
  __shared__ float gs[1][XH][XW];
  __shared__ float hs[XH][PW];
  __shared__ float es[K][PH][PW];
  const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
  const size_t plane = (size_t)blockIdx.z * H * W;
  const float* pg = gV + plane;
  const float* const Dd[2] = {D0, D1};
  tile_fill<4, 1>(gs, x0, y0, [&](int gy, int gx, float (&g)[1]) {
    const bool in = in_image(gy, gx, H, W);
    const float v = pg[(size_t)(in ? gy : 0) * W + (in ? gx : 0)];  // outside: load pixel (0, 0), then select 0
    g[0] = in ? v : 0.f;
  });
  __syncthreads();
  row_sums5<XH, XW, PW, false>(&gs[0][0][0], &hs[0][0]);
  __syncthreads();
  tile_fill<2, K>(es, x0, y0, [&](int gy, int gx, float (&e)[K]) {
    const bool in = in_image(gy, gx, H, W);
    const float S = in ? col_sum5<PW>(&hs[gy - y0 + 2][gx - x0 + 2]) / 25.f : 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) e[k] = in ? 2.f * Dd[k][plane + (size_t)gy * W + gx] * S : 0.f;
  });
  __syncthreads();
  float* const h2[2] = {&gs[0][0][0], &hs[0][0]};                    // gs and hs are dead: 20 x 64 row sums fit either
#pragma unroll
  for (int k = 0; k < K; ++k) row_sums5<PH, PW, TX, false>(&es[k][0][0], h2[k]);
  __syncthreads();
  for_owned(x0, y0, H, W, [&](int ly, int lx, int y, int x) {
    float v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = es[k][ly + 2][lx + 2] - col_sum5<TX>(h2[k] + ly * TX + lx) / 25.f;
    const size_t o = plane + (size_t)y * W + x;
    if constexpr (K == 1) {
      const float r = sign * v[0];
      out0[o] = accumulate ? out0[o] + r : r;
    } else {
      out0[o] = out0[o] + -1.f * v[0];
      out1[o] = v[1] + v[0];
    }
  });
}

// ------------------------------------------------------------------------------------------------ texture mask
__device__ __forceinline__ float gray144(const float* __restrict__ p, size_t plane, size_t o) {
  return 0.144f * p[o] + 0.587f * p[plane + o] + 0.299f * p[2 * plane + o];
}

// std over the 5x5 reflect window of a staged gray tile (t[ly + 2][lx + 2] is the pixel): sum first, then the squared
// deviations in the same index order
__device__ __forceinline__ float local_std5(const float (*t)[PW], int ly, int lx) {
  float v[25];
  float s = 0.f;
  int n = 0;
#pragma unroll
  for (int dy = 0; dy < 5; ++dy) {
#pragma unroll
    for (int dx = 0; dx < 5; ++dx) {
      float g = t[ly + dy][lx + dx];
      v[n++] = g;
      s += g;
    }
  }
  float mu = s / 25.f, q = 0.f;
#pragma unroll
  for (int i = 0; i < 25; ++i) {
    float d = v[i] - mu;
    q += d * d;
  }
  return sqrtf(q / 25.f + 1e-9f);
}

// The gray planes of both inputs are formed once per tile slot (reflection resolved while staging) instead of 25 times per pixel.
__global__ void __launch_bounds__(256) texture_mask_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                           float* __restrict__ mask, float* __restrict__ ratio, int H,
                                                           int W) {
  __shared__ float t[2][PH][PW];
  const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
  const size_t plane = (size_t)H * W;
  tile_fill<2, 2>(t, x0, y0, [&](int gy, int gx, float (&v)[2]) {
    const size_t o = reflect_at(gy, gx, H, W);
    v[0] = gray144(a, plane, o);
    v[1] = gray144(b, plane, o);
  });
  __syncthreads();
  for_owned(x0, y0, H, W, [&](int ly, int lx, int y, int x) {
    float s1 = local_std5(t[0], ly, lx), s2 = local_std5(t[1], ly, lx);
    float r = (2.f * s1 * s2) / (s1 * s1 + s2 * s2 + 1e-5f);
    size_t o = (size_t)y * W + x;
    mask[o] = r > 0.975f ? 1.f : 0.f;
    if (ratio) ratio[o] = r;
  });
}

// ------------------------------------------------------------------------------------------------ "YCbCr" over flat memory
__global__ void __launch_bounds__(256) ycc_flat_kernel(const float* __restrict__ src, float* __restrict__ dst, long long ntriples) {
  long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= ntriples) return;
  float r = src[3 * t], g = src[3 * t + 1], b = src[3 * t + 2];
  // im_flat.mm(mat) + bias, mat rows = input element, cols = output element (loss.py:182-186)
  dst[3 * t + 0] = (r * 0.257f + g * 0.564f + b * 0.098f) + (float)(16.0 / 255.0);
  dst[3 * t + 1] = (r * -0.148f + g * -0.291f + b * 0.439f) + (float)(128.0 / 255.0);
  dst[3 * t + 2] = (r * 0.439f + g * -0.368f + b * -0.071f) + (float)(128.0 / 255.0);
}

inline dim3 grid2d(int W, int H) { return dim3(zt_cdiv(W, 64), zt_cdiv(H, 4)); }

}  // namespace

extern "C" int zt_pair_down_f32(const float* src, float* o1, float* o2, int C, int H, int W, hipStream_t stream) {
  ZT_REQUIRE(src && o1 && o2 && C > 0 && H >= 2 && W >= 2);
  int h = H / 2, w = W / 2;
  hipLaunchKernelGGL(pair_down_kernel, grid2d(w, h), dim3(64, 4), 0, stream, src, o1, o2, C, H, W, h, w);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}

extern "C" int zt_pair_down_adj_f32(const float* g1, const float* g2, float* dst, int C, int H, int W, int accumulate,
                                    hipStream_t stream) {
  ZT_REQUIRE(g1 && g2 && dst && C > 0 && H >= 2 && W >= 2);
  hipLaunchKernelGGL(pair_down_adj_kernel, grid2d(W, H), dim3(64, 4), 0, stream, g1, g2, dst, C, H, W, H / 2, W / 2, accumulate);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}

extern "C" int zt_blur21_f32(const float* src, float* tmp, float* dst, const float* taps21_host, int C, int H, int W,
                             hipStream_t stream) {
  ZT_REQUIRE(src && tmp && dst && taps21_host && H > 10 && W > 10);
  Taps21 k;
  for (int i = 0; i < 21; ++i) k.t[i] = taps21_host[i];
  hipLaunchKernelGGL(blur_horz_kernel<false>, dim3(zt_cdiv(W, 256), H), dim3(256), 0, stream, src, tmp, C, H, W, k, 0);
  hipLaunchKernelGGL(blur_vert_kernel<false>, dim3(zt_cdiv(W, 64), zt_cdiv(H, 4 * BRY)), dim3(64, 4), 0, stream, (const float*)tmp, dst, C, H, W, k, 0);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}

extern "C" int zt_blur21_adj_f32(const float* g, float* tmp, float* dst, const float* taps21_host, int C, int H, int W,
                                 int accumulate, hipStream_t stream) {
  ZT_REQUIRE(g && tmp && dst && taps21_host && H > 21 && W > 21);
  Taps21 k;
  for (int i = 0; i < 21; ++i) k.t[i] = taps21_host[i];
  hipLaunchKernelGGL(blur_vert_kernel<true>, dim3(zt_cdiv(W, 64), zt_cdiv(H, 4 * BRY)), dim3(64, 4), 0, stream, g, tmp, C, H, W, k, 0);
  hipLaunchKernelGGL(blur_vert_fold_kernel, dim3(zt_cdiv(W, 256), 20), dim3(256), 0, stream, g, tmp, C, H, W, k);
  hipLaunchKernelGGL(blur_horz_kernel<true>, dim3(zt_cdiv(W, 256), H), dim3(256), 0, stream, (const float*)tmp, dst, C, H, W, k, accumulate);
  hipLaunchKernelGGL(blur_horz_fold_kernel, dim3(zt_cdiv(H, 256), 20), dim3(256), 0, stream, (const float*)tmp, dst, C, H, W, k);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}

extern "C" int zt_box5_reflect_f32(const float* src, float* dst, int C, int H, int W, hipStream_t stream) {
  ZT_REQUIRE(src && dst && H > 2 && W > 2);
  hipLaunchKernelGGL(box5_reflect_kernel, tile_grid(W, H, C), dim3(64, 4), 0, stream, src, dst, C, H, W);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}

extern "C" int zt_box5_reflect_adj_f32(const float* src, float* dst, int C, int H, int W, float scale, int accumulate,
                                       hipStream_t stream) {
  ZT_REQUIRE(src && dst && H > 5 && W > 5);
  hipLaunchKernelGGL(box5_reflect_adj_kernel, tile_grid(W, H, C), dim3(64, 4), 0, stream, src, dst, C, H, W, scale, accumulate);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}

extern "C" int zt_localvar_fwd_f32(const float* a, const float* b, float* D, float* V, int C, int H, int W,
                                   hipStream_t stream) {
  ZT_REQUIRE(a && V && C > 0);
  hipLaunchKernelGGL(localvar_fwd_kernel<1>, tile_grid(W, H, C), dim3(64, 4), 0, stream, a, b, D, V, (float*)nullptr, (float*)nullptr, C, H, W);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}

extern "C" int zt_localvar_bwd_f32(const float* D, const float* gV, float* xbar, int C, int H, int W, float sign,
                                   int accumulate, hipStream_t stream) {
  ZT_REQUIRE(D && gV && xbar && C > 0);
  hipLaunchKernelGGL(localvar_bwd_kernel<1>, tile_grid(W, H, C), dim3(64, 4), 0, stream, D, (const float*)nullptr, gV, xbar, (float*)nullptr, C, H, W, sign, accumulate);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}

extern "C" int zt_half_bwd_f32(const float* u1, const float* u2, const float* g1, const float* g2, float* dst, int C, int H,
                               int W, hipStream_t stream) {
  ZT_REQUIRE(u1 && u2 && g1 && g2 && dst && C > 0 && H / 2 > 5 && W / 2 > 5);
  hipLaunchKernelGGL(half_bwd_kernel, tile_grid(W / 2, H / 2, C), dim3(64, 4), 0, stream, u1, u2, g1, g2, dst, C, H, W, H / 2, W / 2);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}

extern "C" int zt_localvar_fwd_pair_f32(const float* a, const float* b, float* DA, float* VA, float* DX, float* VX, int C, int H,
                                        int W, hipStream_t stream) {
  ZT_REQUIRE(a && b && DA && VA && DX && VX && C > 0);
  hipLaunchKernelGGL(localvar_fwd_kernel<2>, tile_grid(W, H, C), dim3(64, 4), 0, stream, a, b, DA, VA, DX, VX, C, H, W);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}

extern "C" int zt_localvar_bwd_pair_f32(const float* DN, const float* DH2, const float* gV, float* dH3, float* dH2x, int C, int H,
                                        int W, hipStream_t stream) {
  ZT_REQUIRE(DN && DH2 && gV && dH3 && dH2x && C > 0);
  hipLaunchKernelGGL(localvar_bwd_kernel<2>, tile_grid(W, H, C), dim3(64, 4), 0, stream, DN, DH2, gV, dH3, dH2x, C, H, W, 0.f, 0);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}

extern "C" int zt_texture_mask_f32(const float* a, const float* b, float* mask, float* ratio, int H, int W,
                                   hipStream_t stream) {
  ZT_REQUIRE(a && b && mask && H > 2 && W > 2);
  hipLaunchKernelGGL(texture_mask_kernel, tile_grid(W, H, 1), dim3(64, 4), 0, stream, a, b, mask, ratio, H, W);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}

extern "C" int zt_ycc_flat_f32(const float* src, float* dst, long long nelem, hipStream_t stream) {
  ZT_REQUIRE(src && dst && nelem % 3 == 0);
  long long nt = nelem / 3;
  hipLaunchKernelGGL(ycc_flat_kernel, dim3((unsigned)zt_cdivl(nt, 256)), dim3(256), 0, stream, src, dst, nt);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}
