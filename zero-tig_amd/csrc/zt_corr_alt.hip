// On-the-fly correlation lookup (reference model/RAFT/corr.py:63-91, AlternateCorrBlock): the 4 x 81 window of corr.py:29-50
// computed straight from the two feature maps, without the all-pairs volume.  avg_pool2d over the last two axes of the volume
// equals the correlation with the equally pooled fmap2 (same floor at odd sizes), so level l of query pixel n is
//   D_l[y][x] = alpha * < f1[n][0..255], P_l[y][x][0..255] >,   P_0 = fmap2,   P_{l+1} = avg_pool2d(P_l) (fp32, each level from
//   the rounded level below, zt_fmap_pyramid).
// Everything from the window coordinate to the output is corr_lookup_kernel's (zt_raft.hip): both call zt_lookup.h, here with
// taps D_l instead of volume reads, so with integer operands the two paths agree bit for bit (tests/test_corr_alt.py).
#include "zt_lookup.h"

namespace {

constexpr int CA_C = 256;        // channels of the feature maps (fnet.conv2)
constexpr int CA_G = 12;         // side of the integer grid kept per level: 9 window positions + 1 bilinear neighbour + 2 of slack

// P_{l+1}[y][x] = zt_pool4(P_l[2y][2x], P_l[2y][2x+1], P_l[2y+1][2x], P_l[2y+1][2x+1]): corr_pool_kernel's order.
// One workgroup per 8 x 8 block of level 0 (= 4 x 4 of level 1, 2 x 2 of level 2, one pixel of level 3), one thread per channel,
// the three levels in registers.  A cell of level l + 1 exists iff its index is below floor(size_l / 2), and then its four sources
// exist too, so every read is of a checked cell.
template <typename T>
__global__ void __launch_bounds__(256) fmap_pyramid_kernel(const T* __restrict__ f2, int ld2, int h, int w, float* __restrict__ p1,
                                                           float* __restrict__ p2, float* __restrict__ p3) {
  const int c = threadIdx.x;
  const int bx = blockIdx.x, by = blockIdx.y;
  const int h1 = h / 2, w1 = w / 2, h2 = h1 / 2, w2 = w1 / 2, h3 = h2 / 2, w3 = w2 / 2;
  float l1[4][4], l2[2][2];
#pragma unroll
  for (int y = 0; y < 4; ++y)
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      const int y1 = by * 4 + y, x1 = bx * 4 + x;
      float v = 0.f;
      if (y1 < h1 && x1 < w1) {
        const T* p = f2 + ((size_t)(2 * y1) * w + 2 * x1) * ld2 + c;
        const size_t row = (size_t)w * ld2;
        v = zt_pool4(ZtIO<T>::ld(p), ZtIO<T>::ld(p + ld2), ZtIO<T>::ld(p + row), ZtIO<T>::ld(p + row + ld2));
        p1[((size_t)y1 * w1 + x1) * CA_C + c] = v;
      }
      l1[y][x] = v;
    }
#pragma unroll
  for (int y = 0; y < 2; ++y)
#pragma unroll
    for (int x = 0; x < 2; ++x) {
      const int y2 = by * 2 + y, x2 = bx * 2 + x;
      float v = 0.f;
      if (y2 < h2 && x2 < w2) {
        v = zt_pool4(l1[2 * y][2 * x], l1[2 * y][2 * x + 1], l1[2 * y + 1][2 * x], l1[2 * y + 1][2 * x + 1]);
        p2[((size_t)y2 * w2 + x2) * CA_C + c] = v;
      }
      l2[y][x] = v;
    }
  if (by < h3 && bx < w3) p3[((size_t)by * w3 + bx) * CA_C + c] = zt_pool4(l2[0][0], l2[0][1], l2[1][0], l2[1][1]);
}

struct AltArgs {
  const void* f1;           // [npx][ld1], storage type TF
  const void* p0;           // level 0 = fmap2 [h*w][ld0], storage type TF
  const float* p[3];        // levels 1..3, fp32 [hl*wl][256]
  int h[4], w[4];
  int ld1, ld0;
  float alpha;
  const float* coords;      // [npx][2] (x, y)
  void* out;                // [npx][ldo], storage type TO
  int npx, ldo;
  ZtFlowBook book;          // zt_corr_alt_lookup_step: the previous iteration's flow bookkeeping rides in this lookup
};

// Sums of PV values per lane over groups of lanes in PV + log2 shuffles instead of PV * 6: each step sends the half of the values
// the partner keeps and adds the half it receives.  MASK is the top lane bit of the group; lanes of a group end up with the total
// of value (lane >> 2) & (PV - 1) (groups of 4 * PV lanes; the last two steps are plain butterflies).
template <int CNT, int MASK>
__device__ __forceinline__ void ca_reduce_step(float* v, int lane) {
  if constexpr (CNT >= 1) {
    const bool up = (lane & MASK) != 0;
#pragma unroll
    for (int k = 0; k < CNT; ++k) {
      const float send = up ? v[k] : v[k + CNT], keep = up ? v[k + CNT] : v[k];
      v[k] = keep + __shfl_xor(send, MASK);
    }
    ca_reduce_step<CNT / 2, MASK / 2>(v, lane);
  } else if constexpr (MASK >= 1) {
    v[0] += __shfl_xor(v[0], MASK);
    ca_reduce_step<0, MASK / 2>(v, lane);
  }
}

// One workgroup per query pixel, wave l = pyramid level l.  The wave keeps the query's 256 channels in registers, walks the rows of
// the integer grid under its 9 x 9 window (at most CA_G x CA_G points, clipped to the map), reads each row as one run of
// contiguous channels with 16-byte loads per lane (fp32: 64 lanes x 4 channels per point; bf16: 32 lanes x 8 channels, two points
// per load), reduces the row's dots across lanes, keeps alpha * dot in LDS and then forms its 81 bilinear samples from there.
template <typename TF, typename TO>
__global__ void __launch_bounds__(256) corr_alt_lookup_kernel(AltArgs a) {
  __shared__ float D[4][CA_G * CA_G];
  const int n = blockIdx.x;
  const int lane = threadIdx.x & 63, l = threadIdx.x >> 6;
  const int H = a.h[l], W = a.w[l];
  float px, py;
  zt_lookup_coords(a.coords, a.book, n, &px, &py);
  if (threadIdx.x == 0 && a.book.coords_out) zt_flow_record<TO>(a.book, n, px, py);
  // The grid this level needs: the tap coordinate is non-decreasing in the window position (every operation of zt_lookup_tap is
  // monotonic under rounding), so all taps lie in [tap(0), tap(8) + 1].  That span is 10 points, 11 or 12 where the
  // normalise / de-normalise round trip moves a floor at one end (its error is far below 1 for maps up to 4096, which the launcher
  // requires), and 2 where the clamp has collapsed a far-away window.
  float dummy;
  const int xmin = zt_lookup_tap(px, l, 0, W, &dummy), ymin = zt_lookup_tap(py, l, 0, H, &dummy);
  const int xmax = min(zt_lookup_tap(px, l, 8, W, &dummy) + 1, xmin + CA_G - 1);
  const int ymax = min(zt_lookup_tap(py, l, 8, H, &dummy) + 1, ymin + CA_G - 1);
  const int xa = max(xmin, 0), xb = min(xmax, W - 1), ya = max(ymin, 0), yb = min(ymax, H - 1);     // the part inside the map
  const int nx = xb - xa + 1;                                     // <= CA_G; <= 0: nothing of this level is inside
  float* Dl = D[l];
  for (int k = lane; k < CA_G * CA_G; k += 64) Dl[k] = 0.f;       // points outside the map stay 0 (zeros padding)
  __syncthreads();
  if (l == 0 && sizeof(TF) == 2) {
    // bf16 level 0: lanes 0..31 take the even points of a row, lanes 32..63 the odd ones, 8 channels per lane
    const zt_bf16* P = (const zt_bf16*)a.p0;
    const int g = lane >> 5, c0 = (lane & 31) * 8;
    float q[8];
    zt_ld8((const zt_bf16*)a.f1 + (size_t)n * a.ld1 + c0, q);
    for (int y = ya; y <= yb && nx > 0; ++y) {
      float v[8];
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        v[m] = 0.f;
        const int k = 2 * m + g;
        if (m < CA_G / 2 && k < nx) {
          float f[8];
          zt_ld8(P + ((size_t)y * W + (xa + k)) * a.ld0 + c0, f);
#pragma unroll
          for (int j = 0; j < 8; ++j) v[m] = fmaf(q[j], f[j], v[m]);
        }
      }
      ca_reduce_step<4, 16>(v, lane);
      const int k = 2 * ((lane >> 2) & 7) + g;
      if ((lane & 3) == 0 && k < nx) Dl[(y - ymin) * CA_G + (xa - xmin) + k] = a.alpha * v[0];
    }
  } else {
    // fp32 rows (levels 1..3 always; level 0 of the fp32 plan): 4 channels per lane, one point per load
    const float* P = l == 0 ? (const float*)a.p0 : a.p[l == 0 ? 0 : l - 1];
    const int ldp = l == 0 ? a.ld0 : CA_C;
    const float4 q = ZtIO<TF>::ld4((const TF*)a.f1 + (size_t)n * a.ld1 + lane * 4);
    for (int y = ya; y <= yb && nx > 0; ++y) {
      float v[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        v[k] = 0.f;
        if (k < CA_G && k < nx) {
          const float4 f = *reinterpret_cast<const float4*>(P + ((size_t)y * W + (xa + k)) * ldp + lane * 4);
          v[k] = fmaf(q.w, f.w, fmaf(q.z, f.z, fmaf(q.y, f.y, q.x * f.x)));
        }
      }
      ca_reduce_step<8, 32>(v, lane);
      const int k = (lane >> 2) & 15;
      if ((lane & 3) == 0 && k < nx) Dl[(y - ymin) * CA_G + (xa - xmin) + k] = a.alpha * v[0];
    }
  }
  __syncthreads();
  // corr.py:29-50 + utils.py:285-299: channel = level*81 + i*9 + j with the FIRST window axis (i) moving x
  for (int r = lane; r < 81; r += 64) {
    const int i = r / 9, j = r - i * 9;
    float wx1, wy1;
    const int x0 = zt_lookup_tap(px, l, i, W, &wx1), y0 = zt_lookup_tap(py, l, j, H, &wy1);
    // a tap inside the map is inside the grid by the argument above; should that ever fail, the result is a NaN, not a wrong number
    const float v = zt_lookup_sample(x0, y0, wx1, wy1, W, H, [&](int xx, int yy) {
      const int gx = xx - xmin, gy = yy - ymin;
      return (gx >= 0 && gx < CA_G && gy >= 0 && gy < CA_G) ? Dl[gy * CA_G + gx] : __builtin_nanf("");
    });
    ZtIO<TO>::st((TO*)a.out + (size_t)n * a.ldo + l * 81 + r, v);
  }
}

}  // namespace

extern "C" int zt_fmap_pyramid(const void* f2, int dt, int ld2, int h, int w, float* p1, float* p2, float* p3, hipStream_t stream) {
  ZT_REQUIRE(f2 && p1 && p2 && p3 && ld2 >= CA_C);
  ZT_REQUIRE(h / 8 >= 2 && w / 8 >= 2);      // a 1-pixel level divides by zero in the reference (SURVEY A-13)
  dim3 grid(zt_cdiv(w, 8), zt_cdiv(h, 8));
  if (dt == 0) hipLaunchKernelGGL(fmap_pyramid_kernel<float>, grid, dim3(256), 0, stream, (const float*)f2, ld2, h, w, p1, p2, p3);
  else hipLaunchKernelGGL(fmap_pyramid_kernel<zt_bf16>, grid, dim3(256), 0, stream, (const zt_bf16*)f2, ld2, h, w, p1, p2, p3);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}

extern "C" int zt_corr_alt_lookup_step(const void* f1, int ld1, const void* p0, int ld0, int dt_f, const float* p1, const float* p2,
                                       const float* p3, int h, int w, float alpha, const float* coords, void* out, int dt, int ldo,
                                       int npx, const float* delta, int ldd, float* coords_out, float* f4, int ldf4, void* fhx,
                                       int ldfhx, void* fin, int ldfin, hipStream_t stream) {
  ZT_REQUIRE(f1 && p0 && p1 && p2 && p3 && coords && out && ldo >= 324 && ld1 >= CA_C && ld0 >= CA_C);
  ZT_REQUIRE(ld1 % 8 == 0 && ld0 % 8 == 0);         // 16-byte loads of bf16 rows (fp32 rows need % 4 only)
  ZT_REQUIRE(npx == h * w && h <= 4096 && w <= 4096);
  AltArgs a;
  a.book = {delta, coords_out, f4, fhx, fin, ldd, ldf4, ldfhx, ldfin, w};
  ZT_REQUIRE(zt_flow_book_ok(a.book, coords) && zt_lookup_levels(h, w, a.h, a.w));
  a.f1 = f1; a.ld1 = ld1; a.p0 = p0; a.ld0 = ld0; a.p[0] = p1; a.p[1] = p2; a.p[2] = p3; a.alpha = alpha;
  a.coords = coords; a.out = out; a.npx = npx; a.ldo = ldo;
  const dim3 grid((unsigned)npx), block(256);
  if (dt_f == 0 && dt == 0) hipLaunchKernelGGL((corr_alt_lookup_kernel<float, float>), grid, block, 0, stream, a);
  else if (dt_f == 0) hipLaunchKernelGGL((corr_alt_lookup_kernel<float, zt_bf16>), grid, block, 0, stream, a);
  else if (dt == 0) hipLaunchKernelGGL((corr_alt_lookup_kernel<zt_bf16, float>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((corr_alt_lookup_kernel<zt_bf16, zt_bf16>), grid, block, 0, stream, a);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}

extern "C" int zt_corr_alt_lookup(const void* f1, int ld1, const void* p0, int ld0, int dt_f, const float* p1, const float* p2,
                                  const float* p3, int h, int w, float alpha, const float* coords, void* out, int dt, int ldo, int npx,
                                  hipStream_t stream) {
  return zt_corr_alt_lookup_step(f1, ld1, p0, ld0, dt_f, p1, p2, p3, h, w, alpha, coords, out, dt, ldo, npx, nullptr, 0, nullptr, nullptr,
                                 0, nullptr, 0, nullptr, 0, stream);
}
