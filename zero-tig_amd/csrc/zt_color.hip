// No-reference colour grading of evals.py --color 1: UIQM (UICM / UISM / UIConM), UCIQE and Hasler-Suesstrunk
// colourfulness of one frame, from ONE read of the frame.
//   cl_frame_kernel: a workgroup takes work units in a loop.  A unit is a band of B rows (a row of blocks; the rows left over
//         form one more band that has no blocks) times a run of whole blocks (the last run takes the columns left over).  The
//         unit's 8-bit levels are staged once in LDS as bytes with a one-pixel halo, frame borders replicated.  The thread that
//         stages an own pixel of the unit also counts it in the workgroup's private table of six histograms (3301 counters of
//         32 bits) and takes it through the two tables to CIELAB for the three fp64 sums.  Then the waves take the unit's blocks:
//         Sobel on the staged levels, the extrema per block and channel, and the block's four logarithm terms, which the thread
//         that took the logarithm keeps adding up.  At the end the workgroup adds its non-zero counters to the table in memory
//         and writes its seven sums.
//   cl_finish_kernel: one workgroup: the moments, the trimmed sums and the quantiles off the histograms (block-wide scans) and
//         the workgroups' sums in index order.
// Integers are exact; every fp64 sum has an order that depends on the launch geometry only, so the same frame gives the same bits.
#include "zt_common.h"

namespace {

constexpr int CL_THREADS = 1024;
constexpr int CL_WAVES = CL_THREADS / 64;
constexpr int CL_TILE = 16384;                    // bytes of LDS per channel of the staged unit, halo included
constexpr int CL_ITEMS = 128;                     // (block, slice) items of one unit
constexpr int CL_SLICE = 256;                     // pixels of a block one wave takes at most
constexpr int CL_MAX_WG = 1024;                   // rows of the workgroups' sums in the workspace
constexpr int CL_DEFAULT_WG = 256;
constexpr int CL_SUMS = 7;                        // fp64 sums a workgroup writes: C, C^2, S, the terms of E_R, E_G, E_B and of A
// the six histograms in one table: R, G, B (256 each), R - G + 255 (511), R + G - 2B + 510 (1021), the lightness key (1001)
constexpr int CL_HG = 256, CL_HB = 512, CL_HRG = 768, CL_HYB = 1279, CL_HL = 2300, CL_BINS = 3301;
constexpr int CL_CNT = 3304;                      // behind the histograms: the blocks with a zero minimum (R, G, B), the flat blocks
constexpr int CL_BINS_PAD = 3328;

struct ClGeom {
  int H, W, B;
  int k1, k2;                                     // blocks per row of blocks, rows of blocks
  int nbands, nruns, run;                         // bands, runs of blocks per band, blocks per run
  int slices, per_slice;                          // waves' slices of one block, pixels of a slice
  int nwg;
};

__device__ __forceinline__ unsigned long long cl_shfl_xor64(unsigned long long v, int m) {
  const unsigned lo = __shfl_xor((unsigned)v, m), hi = __shfl_xor((unsigned)(v >> 32), m);
  return ((unsigned long long)hi << 32) | lo;
}

// a fixed butterfly over the lanes that differ in the bits from STOP up: the lanes of a group end with the same bits
template <int STOP>
__device__ __forceinline__ double cl_lanes_sum(double v) {
#pragma unroll
  for (int m = 32; m >= STOP; m >>= 1) {
    unsigned long long u;
    __builtin_memcpy(&u, &v, 8);
    u = cl_shfl_xor64(u, m);
    double o;
    __builtin_memcpy(&o, &u, 8);
    v += o;
  }
  return v;
}

__global__ void __launch_bounds__(CL_THREADS) cl_frame_kernel(const float* __restrict__ x, ClGeom g, const unsigned* __restrict__ lin16,
                                                             const float* __restrict__ flut, unsigned* __restrict__ hist,
                                                             double* __restrict__ part) {
  __shared__ uint4 tile4[3 * CL_TILE / 16];
  __shared__ unsigned lh[CL_BINS_PAD];
  __shared__ unsigned lin[256];
  __shared__ unsigned long long imax[CL_ITEMS][3], imin[CL_ITEMS][3];
  __shared__ unsigned icm[CL_ITEMS];              // cmax << 8 | cmin
  __shared__ double wsum[CL_SUMS][CL_WAVES];
  __shared__ unsigned wcnt[4][CL_WAVES];
  unsigned char* tile = reinterpret_cast<unsigned char*>(tile4);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  for (int d = t; d < CL_BINS_PAD; d += CL_THREADS) lh[d] = 0u;
  if (t < 256) lin[t] = lin16[t];
  __syncthreads();

  const int H = g.H, W = g.W, B = g.B;
  const size_t plane = (size_t)H * W;
  const int units = g.nbands * g.nruns;
  const int u0 = (int)((long long)units * blockIdx.x / g.nwg), u1 = (int)((long long)units * (blockIdx.x + 1) / g.nwg);
  double sc = 0.0, sc2 = 0.0, ss = 0.0;
  double tsum = 0.0;                              // of term t & 3 of the blocks this thread takes the logarithm of, unit after unit
  unsigned tcnt = 0u;                             // the blocks among them that have no term

  for (int u = u0; u < u1; ++u) {
    const int band = u / g.nruns, q = u - band * g.nruns;
    const bool blocks = band < g.k2;
    const int r0 = band * B, r1 = blocks ? r0 + B : H;
    const int c0 = q * g.run * B, c1 = q == g.nruns - 1 ? W : c0 + g.run * B;
    const int th = r1 - r0 + 2, tw = c1 - c0 + 2;

    for (int idx = t; idx < th * tw; idx += CL_THREADS) {
      const int rr = idx / tw, cc = idx - rr * tw;
      const int row = min(max(r0 - 1 + rr, 0), H - 1), col = min(max(c0 - 1 + cc, 0), W - 1);
      const size_t p = (size_t)row * W + col;
      const int R = zt_quant_u8(x[p], 1), G = zt_quant_u8(x[plane + p], 1), Bl = zt_quant_u8(x[2 * plane + p], 1);
      tile[idx] = (unsigned char)R;
      tile[CL_TILE + idx] = (unsigned char)G;
      tile[2 * CL_TILE + idx] = (unsigned char)Bl;
      if (rr >= 1 && rr < th - 1 && cc >= 1 && cc < tw - 1) {             // an own pixel of the unit: counted exactly once
        const unsigned lr = lin[R], lg = lin[G], lb = lin[Bl];
        const unsigned X16 = (28440u * lr + 24655u * lg + 12441u * lb + 32768u) >> 16;
        const unsigned Y16 = (13938u * lr + 46868u * lg + 4730u * lb + 32768u) >> 16;
        const unsigned Z16 = (1164u * lr + 7174u * lg + 57198u * lb + 32768u) >> 16;
        const float fx = flut[X16], fy = flut[Y16], fz = flut[Z16];
        const float L = 116.f * fy - 16.f;
        const float a = 500.f * (fx - fy);
        const float b = 200.f * (fy - fz);
        const float C = sqrtf(a * a + b * b);
        const float D = sqrtf(C * C + L * L);
        const float S = D > 0.f ? C / D : 0.f;
        const int kL = min(max((int)floorf(L * 10.f), 0), 1000);
        atomicAdd(&lh[R], 1u);
        atomicAdd(&lh[CL_HG + G], 1u);
        atomicAdd(&lh[CL_HB + Bl], 1u);
        atomicAdd(&lh[CL_HRG + R - G + 255], 1u);
        atomicAdd(&lh[CL_HYB + R + G - 2 * Bl + 510], 1u);
        atomicAdd(&lh[CL_HL + kL], 1u);
        sc += (double)C;
        sc2 += (double)C * (double)C;
        ss += (double)S;
      }
    }
    __syncthreads();

    if (blocks) {
      const int j0 = q * g.run, nb = min(g.run, g.k1 - j0);               // the unit's blocks: columns j0 .. j0 + nb - 1
      for (int item = wave; item < nb * g.slices; item += CL_WAVES) {
        const int jb = item / g.slices, s = item - jb * g.slices;
        const int p1 = min((s + 1) * g.per_slice, B * B);
        unsigned long long emax[3] = {0ull, 0ull, 0ull}, emin[3] = {~0ull, ~0ull, ~0ull};
        unsigned cmax = 0u, cmin = 255u;
        for (int p = s * g.per_slice + lane; p < p1; p += 64) {
          const int py = p / B, px = p - py * B;
          const unsigned char* c = tile + (py + 1) * tw + jb * B + px + 1;
#pragma unroll
          for (int ch = 0; ch < 3; ++ch, c += CL_TILE) {
            const int nw = c[-tw - 1], n = c[-tw], ne = c[-tw + 1], w = c[-1], v = c[0], e = c[1], sw = c[tw - 1], so = c[tw],
                      se = c[tw + 1];
            const int gx = (ne + 2 * e + se) - (nw + 2 * w + sw), gy = (sw + 2 * so + se) - (nw + 2 * n + ne);
            const unsigned long long e2 = (unsigned long long)(unsigned)(gx * gx + gy * gy) * (unsigned)(v * v);
            emax[ch] = e2 > emax[ch] ? e2 : emax[ch];
            emin[ch] = e2 < emin[ch] ? e2 : emin[ch];
            cmax = max(cmax, (unsigned)v);
            cmin = min(cmin, (unsigned)v);
          }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) {
            const unsigned long long om = cl_shfl_xor64(emax[ch], m), on = cl_shfl_xor64(emin[ch], m);
            emax[ch] = om > emax[ch] ? om : emax[ch];
            emin[ch] = on < emin[ch] ? on : emin[ch];
          }
          cmax = max(cmax, __shfl_xor(cmax, m));
          cmin = min(cmin, __shfl_xor(cmin, m));
        }
        if (lane < 3) {
          imax[item][lane] = emax[lane];
          imin[item][lane] = emin[lane];
        }
        if (lane == 3) icm[item] = cmax << 8 | cmin;
      }
      __syncthreads();

      if (t < 4 * nb) {                           // thread (block jb, term k): the slices in order, then the block's logarithm
        const int jb = t >> 2, k = t & 3;
        if (k < 3) {
          unsigned long long hi = 0ull, lo = ~0ull;
          for (int s = 0; s < g.slices; ++s) {
            const unsigned long long a = imax[jb * g.slices + s][k], b = imin[jb * g.slices + s][k];
            hi = a > hi ? a : hi;
            lo = b < lo ? b : lo;
          }
          if (lo == 0ull) ++tcnt;
          else tsum += log((double)hi / (double)lo);
        } else {
          unsigned hi = 0u, lo = 255u;
          for (int s = 0; s < g.slices; ++s) {
            const unsigned v = icm[jb * g.slices + s];
            hi = max(hi, v >> 8);
            lo = min(lo, v & 255u);
          }
          if (hi == lo) ++tcnt;
          else {
            const double r = (double)(hi - lo) / (double)(hi + lo);
            tsum += r * log(r);
          }
        }
      }
    }
    __syncthreads();                              // the next unit overwrites the tile and the items
  }

  for (int d = t; d < CL_BINS; d += CL_THREADS)
    if (lh[d]) atomicAdd(&hist[d], lh[d]);

  sc = cl_lanes_sum<1>(sc);
  sc2 = cl_lanes_sum<1>(sc2);
  ss = cl_lanes_sum<1>(ss);
  tsum = cl_lanes_sum<4>(tsum);                   // over the lanes of one term: lane l ends with the wave's sum of term l & 3
#pragma unroll
  for (int m = 32; m >= 4; m >>= 1) tcnt += __shfl_xor(tcnt, m);
  if (lane == 0) {
    wsum[0][wave] = sc;
    wsum[1][wave] = sc2;
    wsum[2][wave] = ss;
  }
  if (lane < 4) {
    wsum[3 + lane][wave] = tsum;
    wcnt[lane][wave] = tcnt;
  }
  __syncthreads();
  if (t < CL_SUMS) {                              // the waves in order
    double s = 0.0;
    for (int w = 0; w < CL_WAVES; ++w) s += wsum[t][w];
    part[CL_SUMS * blockIdx.x + t] = s;
  } else if (t < CL_SUMS + 4) {
    unsigned c = 0u;
    for (int w = 0; w < CL_WAVES; ++w) c += wcnt[t - CL_SUMS][w];
    if (c) atomicAdd(&hist[CL_CNT + t - CL_SUMS], c);
  }
}

// inclusive scan of one value per thread over the workgroup, in thread order
__device__ __forceinline__ unsigned cl_scan(unsigned v, unsigned* wtot, int lane, int wave) {
  unsigned inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned up = __shfl(inc, (lane - d) & 63);
    if (lane >= d) inc += up;
  }
  __syncthreads();                                // the last scan's readers are done with wtot
  if (lane == 63) wtot[wave] = inc;
  __syncthreads();
  unsigned base = 0u;
  for (int w = 0; w < wave; ++w) base += wtot[w];
  return inc + base;
}

// the trimmed share of a bin that holds the sorted positions [excl, incl): those in [TL, N - TR)
__device__ __forceinline__ long long cl_kept(unsigned excl, unsigned incl, long long TL, long long hiN) {
  const long long lo = max((long long)excl, TL), hi = min((long long)incl, hiN);
  return hi > lo ? hi - lo : 0ll;
}

__global__ void __launch_bounds__(CL_THREADS) cl_finish_kernel(const unsigned* __restrict__ hist, const double* __restrict__ part, int nwg,
                                                              long long N, long long nblk, long long* __restrict__ out_i,
                                                              double* __restrict__ out_f) {
  __shared__ unsigned wtot[CL_WAVES];
  __shared__ unsigned long long acc[16];          // 0-2 sum R G B, 3-5 S1 S2 T of rg, 6-8 of yb, 9 k01, 10 k99
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (t < 16) acc[t] = 0ull;
  __syncthreads();
  const long long TL = (N + 9) / 10, TR = N / 10, hiN = N - TR;

  if (t < 256) {
    atomicAdd(&acc[0], (unsigned long long)hist[t] * (unsigned)t);
    atomicAdd(&acc[1], (unsigned long long)hist[CL_HG + t] * (unsigned)t);
    atomicAdd(&acc[2], (unsigned long long)hist[CL_HB + t] * (unsigned)t);
  }
  // negative values: the sums wrap in 64 unsigned bits and come out right as signed
  {
    const unsigned h = t < 511 ? hist[CL_HRG + t] : 0u;
    const unsigned incl = cl_scan(h, wtot, lane, wave);
    const long long v = t - 255;
    if (h) {
      atomicAdd(&acc[3], (unsigned long long)((long long)h * v));
      atomicAdd(&acc[4], (unsigned long long)((long long)h * v * v));
      atomicAdd(&acc[5], (unsigned long long)(cl_kept(incl - h, incl, TL, hiN) * v));
    }
  }
  {
    const unsigned h = t < 1021 ? hist[CL_HYB + t] : 0u;
    const unsigned incl = cl_scan(h, wtot, lane, wave);
    const long long v = t - 510;
    if (h) {
      atomicAdd(&acc[6], (unsigned long long)((long long)h * v));
      atomicAdd(&acc[7], (unsigned long long)((long long)h * v * v));
      atomicAdd(&acc[8], (unsigned long long)(cl_kept(incl - h, incl, TL, hiN) * v));
    }
  }
  {
    const unsigned h = t < 1001 ? hist[CL_HL + t] : 0u;
    const unsigned incl = cl_scan(h, wtot, lane, wave);
    const long long q01 = (N + 99) / 100, q99 = (99 * N + 99) / 100;      // the one bin whose share of positions holds the target
    if ((long long)(incl - h) < q01 && (long long)incl >= q01) acc[9] = (unsigned long long)t;
    if ((long long)(incl - h) < q99 && (long long)incl >= q99) acc[10] = (unsigned long long)t;
  }

  __syncthreads();

  if (t < CL_SUMS) {                              // the workgroups in order
    double e = 0.0;
    for (int w = 0; w < nwg; ++w) e += part[CL_SUMS * w + t];
    out_f[t] = e;
  }
  if (t == 64) {
    out_i[0] = N;
    out_i[1] = nblk;
    for (int k = 0; k < 9; ++k) out_i[2 + k] = (long long)acc[k];
    out_i[11] = N - TL - TR;
    out_i[12] = (long long)acc[9];
    out_i[13] = (long long)acc[10];
    for (int k = 0; k < 4; ++k) out_i[14 + k] = (long long)hist[CL_CNT + k];
  }
}

// the geometry of a launch, or false when the arguments are outside what the kernels take
bool cl_geometry(int H, int W, int B, int max_workgroups, ClGeom* g) {
  if (H < 1 || W < 1 || B < 4 || B > 64 || max_workgroups < 0 || (long long)H * W >= (1ll << 31)) return false;
  g->H = H, g->W = W, g->B = B;
  g->k1 = W / B, g->k2 = H / B;
  g->nbands = g->k2 + (H % B != 0 ? 1 : 0);
  g->slices = (B * B + CL_SLICE - 1) / CL_SLICE;
  g->per_slice = (B * B + g->slices - 1) / g->slices;
  // a unit of `run` blocks is at most run * B + B - 1 columns and B rows, plus the halo, in CL_TILE bytes a channel
  g->run = min((CL_TILE / (B + 2) - B - 1) / B, CL_ITEMS / g->slices);
  g->nruns = max(1, (g->k1 + g->run - 1) / g->run);
  const int units = g->nbands * g->nruns;
  int cap = max_workgroups ? min(max_workgroups, CL_MAX_WG) : CL_DEFAULT_WG;
  cap = min(cap, units);
  g->nwg = (units + (units + cap - 1) / cap - 1) / ((units + cap - 1) / cap);      // the fewest workgroups with as deep a loop
  return g->run >= 1;
}

constexpr size_t CL_WS_BYTES = CL_BINS_PAD * sizeof(unsigned) + CL_SUMS * CL_MAX_WG * sizeof(double);

}  // namespace

extern "C" int zt_color_ws_bytes(int H, int W, int block, size_t* bytes) {
  ClGeom g;
  ZT_REQUIRE(bytes && cl_geometry(H, W, block, 0, &g));
  *bytes = CL_WS_BYTES;
  return ZT_OK;
}

extern "C" int zt_color_stats_f32(const float* x, int H, int W, int block, const unsigned* lin16, const float* flut, int max_workgroups,
                                  void* ws, size_t ws_bytes, long long* out_i, double* out_f, hipStream_t stream) {
  ClGeom g;
  ZT_REQUIRE(x && lin16 && flut && ws && out_i && out_f);
  ZT_REQUIRE(cl_geometry(H, W, block, max_workgroups, &g));
  ZT_REQUIRE((((uintptr_t)x | (uintptr_t)lin16 | (uintptr_t)flut) & 3) == 0);
  ZT_REQUIRE((((uintptr_t)ws | (uintptr_t)out_i | (uintptr_t)out_f) & 7) == 0 && ws_bytes >= CL_WS_BYTES);
  unsigned* hist = static_cast<unsigned*>(ws);
  double* part = reinterpret_cast<double*>(hist + CL_BINS_PAD);
  hipError_t e = hipMemsetAsync(hist, 0, CL_BINS_PAD * sizeof(unsigned), stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(cl_frame_kernel, dim3(g.nwg), dim3(CL_THREADS), 0, stream, x, g, lin16, flut, hist, part);
  ZT_LAUNCH_CHECK();
  hipLaunchKernelGGL(cl_finish_kernel, dim3(1), dim3(CL_THREADS), 0, stream, hist, part, g.nwg, (long long)H * W,
                     (long long)g.k1 * g.k2, out_i, out_f);
  ZT_LAUNCH_CHECK();
  return ZT_OK;
}
