// NIQE of evals.py --niqe: the block sums of both scales from ONE read of the frame, and the frame's features.
//   nq_grey_kernel: the frame's 8-bit grey levels of the cropped image, as bytes, into the workspace (Hc x Wc, 2 MB at 1080p: it
//         stays in the L2 / MALL for the tiles that follow).  The only pass over the fp32 frame.
//   nq_block_kernel: a workgroup takes tiles in a loop; a tile is one 96 x 96 block of one scale, whole.  The grey levels of the
//         block and its halo are staged in LDS as bytes (102 x 102 clamped at scale 1, 114 x 114 reflected at scale 2), at scale 2
//         the 54 x 54 samples of the half-size image are made from them in integers.  Thread (column, strip of P / 8 rows) walks down
//         its column: the row-filtered pair of the next row into a ring of seven registers, the column filter off the ring, the
//         MSCN sample into the P x P tile in LDS.  No row-filtered field is ever stored: 61 KB of LDS a workgroup, two workgroups a
//         CU.  Then all threads take the tile's samples and their four circular neighbours for the 25 sums, which are added over the
//         lanes by a fixed butterfly and over the waves in order.  A tile's sums do not depend on the grid.
//   nq_frame_kernel: one workgroup, rows in chunks of 64: the ten fits of a row into LDS, then the column sums; again for the scatter.
#include "zt_common.h"

namespace {

constexpr int NQ_THREADS = 768;                   // 96 columns x 8 strips
constexpr int NQ_WAVES = NQ_THREADS / 64;
constexpr int NQ_B = 96;                          // block side in source pixels
constexpr int NQ_G1 = 102, NQ_G2 = 114, NQ_X2 = 54;
constexpr int NQ_DEFAULT_WG = 4096;
constexpr int NQ_GRID = 9801;                     // alpha = 0.2 + 0.001 i
constexpr int NQ_F_THREADS = 1024;
constexpr int NQ_CHUNK = 64;                      // rows of features in LDS
constexpr int NQ_NF = 36, NQ_NP = 666;

__device__ __forceinline__ double nq_lanes_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    unsigned long long u;
    __builtin_memcpy(&u, &v, 8);
    const unsigned lo = __shfl_xor((unsigned)u, m), hi = __shfl_xor((unsigned)(u >> 32), m);
    u = ((unsigned long long)hi << 32) | lo;
    double o;
    __builtin_memcpy(&o, &u, 8);
    v += o;
  }
  return v;
}

__device__ __forceinline__ int nq_grey(float r, float g, float b) {
  return (int)((19591u * (unsigned)zt_quant_u8(r, 1) + 38472u * (unsigned)zt_quant_u8(g, 1) + 7473u * (unsigned)zt_quant_u8(b, 1) +
                32768u) >> 16);
}

// four pixels a thread: one 32-bit store of four grey bytes (Wc is a multiple of 96)
__global__ void __launch_bounds__(256) nq_grey_kernel(const float* __restrict__ x, int H, int W, int Hc, int Wc, int vec,
                                                      unsigned* __restrict__ grey) {
  const int q = Wc >> 2;
  const long long n = (long long)Hc * q;
  const size_t plane = (size_t)H * W;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int row = (int)(i / q), c4 = (int)(i - (long long)row * q) << 2;
    const size_t p = (size_t)row * W + c4;
    float r[4], g[4], b[4];
    if (vec) {
      const float4 vr = *reinterpret_cast<const float4*>(x + p), vg = *reinterpret_cast<const float4*>(x + plane + p),
                   vb = *reinterpret_cast<const float4*>(x + 2 * plane + p);
      r[0] = vr.x, r[1] = vr.y, r[2] = vr.z, r[3] = vr.w;
      g[0] = vg.x, g[1] = vg.y, g[2] = vg.z, g[3] = vg.w;
      b[0] = vb.x, b[1] = vb.y, b[2] = vb.z, b[3] = vb.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) r[k] = x[p + k], g[k] = x[plane + p + k], b[k] = x[2 * plane + p + k];
    }
    unsigned o = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) o |= (unsigned)nq_grey(r[k], g[k], b[k]) << (8 * k);
    grey[i] = o;
  }
}

// reflection with the edge repeated: -1 -> 0, -2 -> 1, n -> n - 1
__device__ __forceinline__ int nq_reflect(int i, int n) { return i < 0 ? -i - 1 : i >= n ? 2 * n - 1 - i : i; }

// the MSCN samples of one tile: P = 96 off the bytes `gb` (rows of 102), P = 48 off the fp32 samples `x2` (rows of 54)
template <int P>
__device__ __forceinline__ void nq_mscn(const unsigned char* gb, const float* x2, float* ms, const float (&w)[7], int t, double& ssig) {
  constexpr int R = P / 8;
  if (t >= 8 * P) return;
  const int c = t % P, y0 = (t / P) * R;
  float hm[7], hq[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) hm[k] = 0.f, hq[k] = 0.f;
#pragma unroll
  for (int r = 0; r < R + 6; ++r) {
    float p[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) p[k] = P == 96 ? (float)gb[(y0 + r) * NQ_G1 + c + k] : x2[(y0 + r) * NQ_X2 + c + k];
    float a = w[0] * p[0], q = w[0] * (p[0] * p[0]);
#pragma unroll
    for (int k = 1; k < 7; ++k) {
      a = a + w[k] * p[k];
      q = q + w[k] * (p[k] * p[k]);
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) hm[k] = hm[k + 1], hq[k] = hq[k + 1];
    hm[6] = a, hq[6] = q;
    if (r >= 6) {
      float mu = w[0] * hm[0], m2 = w[0] * hq[0];
#pragma unroll
      for (int k = 1; k < 7; ++k) {
        mu = mu + w[k] * hm[k];
        m2 = m2 + w[k] * hq[k];
      }
      const int y = y0 + r - 6;
      const float xc = P == 96 ? (float)gb[(y + 3) * NQ_G1 + c + 3] : x2[(y + 3) * NQ_X2 + c + 3];
      const float sigma = sqrtf(fabsf(m2 - mu * mu));
      ms[y * P + c] = (xc - mu) / (sigma + 1.0f);
      if (P == 96) ssig += (double)sigma;       // the sharpness of the block is taken at scale 1
    }
  }
}

__global__ void __launch_bounds__(NQ_THREADS) nq_block_kernel(const unsigned char* __restrict__ grey, int Hc, int Wc,
                                                             const float* __restrict__ win, long long* __restrict__ out_i,
                                                             double* __restrict__ out_f) {
  __shared__ unsigned gb4[(NQ_G2 * NQ_G2 + 3) / 4];
  __shared__ float x2[NQ_X2 * NQ_X2];
  __shared__ float ms[NQ_B * NQ_B];
  __shared__ double wsum[16][NQ_WAVES];
  __shared__ unsigned wcnt[10][NQ_WAVES];
  unsigned char* gb = reinterpret_cast<unsigned char*>(gb4);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int k1 = Wc / NQ_B, k2 = Hc / NQ_B, nblk = k1 * k2;
  float w[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) w[k] = win[k];

  for (int u = blockIdx.x; u < 2 * nblk; u += gridDim.x) {
    const int scale = u / nblk, blk = u - scale * nblk;
    const int by = blk / k1, bx = blk - by * k1;
    const int P = scale ? NQ_B / 2 : NQ_B;
    double ssig = 0.0;
    if (!scale) {
      for (int idx = t; idx < NQ_G1 * NQ_G1; idx += NQ_THREADS) {
        const int rr = idx / NQ_G1, cc = idx - rr * NQ_G1;
        const int row = min(max(NQ_B * by - 3 + rr, 0), Hc - 1), col = min(max(NQ_B * bx - 3 + cc, 0), Wc - 1);
        gb[idx] = grey[(size_t)row * Wc + col];
      }
      __syncthreads();
      nq_mscn<NQ_B>(gb, x2, ms, w, t, ssig);
    } else {
      for (int idx = t; idx < NQ_G2 * NQ_G2; idx += NQ_THREADS) {
        const int rr = idx / NQ_G2, cc = idx - rr * NQ_G2;
        const int row = nq_reflect(NQ_B * by - 9 + rr, Hc), col = nq_reflect(NQ_B * bx - 9 + cc, Wc);
        gb[idx] = grey[(size_t)row * Wc + col];
      }
      __syncthreads();
      for (int idx = t; idx < NQ_X2 * NQ_X2; idx += NQ_THREADS) {
        const int ty = idx / NQ_X2, tx = idx - ty * NQ_X2;
        // the clamped sample of the half-size image, then its eight taps: tile row of source row 2i - 3
        const int iy = min(max(48 * by - 3 + ty, 0), Hc / 2 - 1), ix = min(max(48 * bx - 3 + tx, 0), Wc / 2 - 1);
        const unsigned char* s = gb + (2 * iy + 6 - NQ_B * by) * NQ_G2 + (2 * ix + 6 - NQ_B * bx);
        int S = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int ti = i == 0 || i == 7 ? -3 : i == 1 || i == 6 ? -9 : i == 2 || i == 5 ? 29 : 111;
          const unsigned char* q = s + i * NQ_G2;
          const int rs = -3 * (q[0] + q[7]) - 9 * (q[1] + q[6]) + 29 * (q[2] + q[5]) + 111 * (q[3] + q[4]);
          S += ti * rs;
        }
        x2[idx] = (float)S * (1.0f / 65536.0f);
      }
      __syncthreads();
      nq_mscn<NQ_B / 2>(gb, x2, ms, w, t, ssig);
    }
    __syncthreads();

    unsigned nn[5] = {0u, 0u, 0u, 0u, 0u}, np[5] = {0u, 0u, 0u, 0u, 0u};
    double s2n[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, s2p[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, sa[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int idx = t; idx < P * P; idx += NQ_THREADS) {
      const int y = idx / P, xx = idx - y * P;
      const int ym = y == 0 ? P - 1 : y - 1, xm = xx == 0 ? P - 1 : xx - 1, xp = xx == P - 1 ? 0 : xx + 1;
      const float m0 = ms[idx];
      const float v[5] = {m0, m0 * ms[y * P + xm], m0 * ms[ym * P + xx], m0 * ms[ym * P + xm], m0 * ms[ym * P + xp]};
#pragma unroll
      for (int f = 0; f < 5; ++f) {
        const float sq = v[f] * v[f];
        if (v[f] < 0.f) ++nn[f], s2n[f] += (double)sq;
        if (v[f] > 0.f) ++np[f], s2p[f] += (double)sq;
        sa[f] += (double)fabsf(v[f]);
      }
    }
#pragma unroll
    for (int f = 0; f < 5; ++f) {
      s2n[f] = nq_lanes_sum(s2n[f]);
      s2p[f] = nq_lanes_sum(s2p[f]);
      sa[f] = nq_lanes_sum(sa[f]);
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) nn[f] += __shfl_xor(nn[f], m), np[f] += __shfl_xor(np[f], m);
    }
    ssig = nq_lanes_sum(ssig);
    if (lane == 0) {
#pragma unroll
      for (int f = 0; f < 5; ++f) {
        wsum[3 * f][wave] = s2n[f], wsum[3 * f + 1][wave] = s2p[f], wsum[3 * f + 2][wave] = sa[f];
        wcnt[2 * f][wave] = nn[f], wcnt[2 * f + 1][wave] = np[f];
      }
      wsum[15][wave] = ssig;
    }
    __syncthreads();
    if (t < 16) {                                 // the waves in order
      double s = 0.0;
      for (int wv = 0; wv < NQ_WAVES; ++wv) s += wsum[t][wv];
      out_f[(size_t)u * 16 + t] = s;
    } else if (t >= 64 && t < 74) {
      unsigned c = 0u;
      for (int wv = 0; wv < NQ_WAVES; ++wv) c += wcnt[t - 64][wv];
      out_i[(size_t)u * 10 + t - 64] = (long long)c;
    }
    __syncthreads();                              // the next tile overwrites the staged levels, the samples and the partials
  }
}

// ---- the frame ------------------------------------------------------------------------------------------------------------------
// the AGGD fit of one field from its five sums -> alpha and (mean, bl, br); false: the fit has no value
__device__ __forceinline__ bool nq_fit(long long n_neg, long long n_pos, double s2n, double s2p, double sabs, double n,
                                       const double* __restrict__ r_gam, const double* __restrict__ c1, const double* __restrict__ c2,
                                       double* alpha, double* mean, double* bl, double* br) {
  if (n_neg <= 0 || n_pos <= 0) return false;
  const double l = sqrt(s2n / (double)n_neg), r = sqrt(s2p / (double)n_pos), gh = l / r;
  const double ma = sabs / n;
  const double rhat = ma * ma / ((s2n + s2p) / n);
  const double g2 = gh * gh + 1.0;
  const double rn = rhat * (gh * gh * gh + 1.0) * (gh + 1.0) / (g2 * g2);
  if (!(fabs(rn) < 1.0e300)) return false;        // not finite
  int lo = 0, hi = NQ_GRID;                       // the first entry that is not below rn
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (r_gam[mid] < rn) lo = mid + 1;
    else hi = mid;
  }
  int pos = lo;
  if (lo == NQ_GRID) pos = NQ_GRID - 1;
  else if (lo > 0) {
    const double da = r_gam[lo - 1] - rn, db = r_gam[lo] - rn;
    pos = da * da <= db * db ? lo - 1 : lo;
  }
  *alpha = 0.2 + 0.001 * (double)pos;
  *bl = l * c1[pos];
  *br = r * c1[pos];
  *mean = (*br - *bl) * c2[pos];
  return true;
}

// the 36 features of rows r0 .. r0 + rows - 1 into feat, and whether a row is valid
__device__ __forceinline__ void nq_rows(const long long* __restrict__ si, const double* __restrict__ sf, int nblk, int r0, int rows,
                                        const double* __restrict__ r_gam, const double* __restrict__ c1, const double* __restrict__ c2,
                                        double (*feat)[NQ_NF], int* valid, int t) {
  const double nan = __builtin_nan("");
  for (int task = t; task < rows * 10; task += NQ_F_THREADS) {
    const int row = task / 10, fit = task - row * 10, scale = fit / 5, f = fit - scale * 5;
    const size_t b = (size_t)scale * nblk + r0 + row;
    const long long* ci = si + b * 10 + 2 * f;
    const double* cf = sf + b * 16 + 3 * f;
    double alpha = nan, mean = nan, bl = nan, br = nan;
    nq_fit(ci[0], ci[1], cf[0], cf[1], cf[2], scale ? 2304.0 : 9216.0, r_gam, c1, c2, &alpha, &mean, &bl, &br);
    double* o = feat[row] + 18 * scale;
    if (f == 0) o[0] = alpha, o[1] = (bl + br) / 2.0;
    else o[4 * f - 2] = alpha, o[4 * f - 1] = mean, o[4 * f] = bl, o[4 * f + 1] = br;
  }
  __syncthreads();
  if (t < rows) {
    int ok = 1;
    for (int c = 0; c < NQ_NF; ++c) ok &= fabs(feat[t][c]) < 1.0e300 ? 1 : 0;
    valid[t] = ok;
  }
  __syncthreads();
}

__global__ void __launch_bounds__(NQ_F_THREADS) nq_frame_kernel(const long long* __restrict__ si, const double* __restrict__ sf, int nblk,
                                                               const double* __restrict__ r_gam, const double* __restrict__ c1,
                                                               const double* __restrict__ c2, long long* __restrict__ out_i,
                                                               double* __restrict__ out_f) {
  __shared__ double feat[NQ_CHUNK][NQ_NF];
  __shared__ int valid[NQ_CHUNK];
  __shared__ double mean[NQ_NF];
  __shared__ long long nv_s;
  const int t = threadIdx.x;
  double colsum = 0.0, vsum = 0.0;
  long long cnt = 0, nv = 0;
  for (int r0 = 0; r0 < nblk; r0 += NQ_CHUNK) {   // the means first, so that nothing cancels in the scatter
    const int rows = min(NQ_CHUNK, nblk - r0);
    nq_rows(si, sf, nblk, r0, rows, r_gam, c1, c2, feat, valid, t);
    if (t < NQ_NF) {
      for (int r = 0; r < rows; ++r) {
        const double v = feat[r][t];
        if (fabs(v) < 1.0e300) colsum += v, ++cnt;
        if (valid[r]) vsum += v;
      }
    } else if (t == 64) {
      for (int r = 0; r < rows; ++r) nv += valid[r];
    }
    __syncthreads();
  }
  if (t < NQ_NF) mean[t] = vsum;
  if (t == 64) nv_s = nv;
  __syncthreads();
  nv = nv_s;
  if (t < NQ_NF) {
    mean[t] = nv ? mean[t] / (double)nv : 0.0;
    out_i[2 + t] = cnt;
    out_f[t] = colsum;
    out_f[NQ_NF + t] = mean[t];
  }
  if (t == 64) out_i[0] = nblk, out_i[1] = nv;
  __syncthreads();

  int pi = 0, pj = 0;                             // pair t of the upper triangle, row-major
  if (t < NQ_NP) {
    int p = t;
    while (p >= NQ_NF - pi) p -= NQ_NF - pi, ++pi;
    pj = pi + p;
  }
  double acc = 0.0;
  for (int r0 = 0; r0 < nblk; r0 += NQ_CHUNK) {
    const int rows = min(NQ_CHUNK, nblk - r0);
    nq_rows(si, sf, nblk, r0, rows, r_gam, c1, c2, feat, valid, t);
    if (t < NQ_NP)
      for (int r = 0; r < rows; ++r)
        if (valid[r]) acc += (feat[r][pi] - mean[pi]) * (feat[r][pj] - mean[pj]);
    __syncthreads();
  }
  if (t < NQ_NP) out_f[2 * NQ_NF + t] = acc;
}

bool nq_size(int H, int W) { return H >= NQ_B && W >= NQ_B && (long long)H * W < (1ll << 31); }

}  // namespace

extern "C" int zt_niqe_ws_bytes(int H, int W, size_t* bytes) {
  ZT_REQUIRE(bytes && nq_size(H, W));
  *bytes = ((size_t)(H / NQ_B * NQ_B) * (size_t)(W / NQ_B * NQ_B) + 15) & ~(size_t)15;
  return ZT_OK;
}

extern "C" int zt_niqe_block_sums_f32(const float* x, int H, int W, const float* win, int max_workgroups, void* ws, size_t ws_bytes,
                                      long long* out_i, double* out_f, hipStream_t stream) {
  ZT_REQUIRE(x && win && ws && out_i && out_f && nq_size(H, W) && max_workgroups >= 0);
  ZT_REQUIRE((((uintptr_t)x | (uintptr_t)win | (uintptr_t)ws) & 3) == 0 && (((uintptr_t)out_i | (uintptr_t)out_f) & 7) == 0);
  const int Hc = H / NQ_B * NQ_B, Wc = W / NQ_B * NQ_B;
  ZT_REQUIRE(ws_bytes >= (size_t)Hc * Wc);
  const int units = 2 * (Hc / NQ_B) * (Wc / NQ_B);
  const int vec = W % 4 == 0 && ((uintptr_t)x & 15) == 0;
  const long long quads = (long long)Hc * (Wc / 4);
  hipLaunchKernelGGL(nq_grey_kernel, dim3((unsigned)min(zt_cdivl(quads, 256), 4096ll)), dim3(256), 0, stream, x, H, W, Hc, Wc, vec,
                     static_cast<unsigned*>(ws));
  ZT_LAUNCH_CHECK();
  hipLaunchKernelGGL(nq_block_kernel, dim3(min(units, max_workgroups ? max_workgroups : NQ_DEFAULT_WG)), dim3(NQ_THREADS), 0, stream,
                     static_cast<const unsigned char*>(ws), Hc, Wc, win, out_i, out_f);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}

extern "C" int zt_niqe_frame_f32(const long long* sums_i, const double* sums_f, int nblk, const double* r_gam, const double* c1,
                                 const double* c2, long long* out_i, double* out_f, hipStream_t stream) {
  ZT_REQUIRE(sums_i && sums_f && r_gam && c1 && c2 && out_i && out_f && nblk >= 1);
  ZT_REQUIRE((((uintptr_t)sums_i | (uintptr_t)sums_f | (uintptr_t)r_gam | (uintptr_t)c1 | (uintptr_t)c2 | (uintptr_t)out_i |
               (uintptr_t)out_f) & 7) == 0);
  hipLaunchKernelGGL(nq_frame_kernel, dim3(1), dim3(NQ_F_THREADS), 0, stream, sums_i, sums_f, nblk, r_gam, c1, c2, out_i, out_f);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}
