// TSGBench statistics (MDD, ACD, SD, KD) for gfx950: the device halves of
// timevqvae/evaluation/stat_metrics.py.
//
// Reference: timevqvae/evaluation/stat_metrics.py:5-60 runs scipy.stats.gaussian_kde (100
// grid points against every sample), np.correlate(s, s, "full") per series and
// scipy.stats.skew / kurtosis on one host core.  Here, all in float64:
//
//   tvq_stat_moments   {min, max, mean, m2, m3, m4} of a flat array in two passes, as scipy's
//                      _moment: the mean first, then the central powers about that mean
//                      ((d d) d and (d d)(d d), unfused, scipy's exponentiation by squares).
//   tvq_stat_kde       the Gaussian KDE at G grid points: blocks split the samples
//                      (blockIdx.x) and the grid (blockIdx.y, KDE_GT points per thread in
//                      registers); one exp per (sample, grid point).
//   tvq_stat_acf_mean  the mean raw autocorrelation over N series: a block owns ACF_KT
//                      consecutive lags and a chunk of series; a series is staged in LDS once,
//                      each thread owns ACF_R consecutive lags and slides a register window
//                      over t, so one LDS read of s[t] (broadcast) and one of s[t + k + R]
//                      feed ACF_R FMAs.
//
// Every kernel writes per-block partials and a second launch adds them in a fixed order: no
// float atomics, results are bitwise identical from run to run.
#include "tvq_eval.h"

namespace tvq {
namespace {

constexpr int ST_T = 256;          // threads per block, all kernels
constexpr int ST_MAX_BLOCKS = 1024;
constexpr int ST_PER_BLOCK = ST_T * 16;  // elements a block takes before the grid stops growing

int64_t stat_blocks(int64_t n) {
  const int64_t b = (n + ST_PER_BLOCK - 1) / ST_PER_BLOCK;
  return b < 1 ? 1 : (b > ST_MAX_BLOCKS ? ST_MAX_BLOCKS : b);
}

// ---- moments ---------------------------------------------------------------------------
// pass 1: ws[b] = block sum, ws[nb + b] = block min, ws[2 nb + b] = block (-max)
__global__ __launch_bounds__(ST_T) void stat_sum_kernel(const double* __restrict__ x, int64_t n,
                                                        double* __restrict__ ws) {
#pragma clang fp contract(off)
  __shared__ double red[ST_T];
  const int64_t nb = gridDim.x, step = nb * ST_T;
  double s = 0.0, lo = INFINITY, nhi = INFINITY;
  for (int64_t i = (int64_t)blockIdx.x * ST_T + threadIdx.x; i < n; i += step) {
    const double v = x[i];
    s += v;
    lo = fmin(lo, v);
    nhi = fmin(nhi, -v);
  }
  s = block_tree_sum_d<ST_T>(s, red);
  lo = block_tree_min_d<ST_T>(lo, red);
  nhi = block_tree_min_d<ST_T>(nhi, red);
  if (threadIdx.x == 0) {
    ws[blockIdx.x] = s;
    ws[nb + blockIdx.x] = lo;
    ws[2 * nb + blockIdx.x] = nhi;
  }
}

// one block: out6[0..2] = {min, max, sum / n} from the nb block partials, in block order
__global__ __launch_bounds__(ST_T) void stat_sum_finish_kernel(const double* __restrict__ ws,
                                                               int64_t nb, int64_t n,
                                                               double* __restrict__ out6) {
#pragma clang fp contract(off)
  __shared__ double red[ST_T];
  double s = 0.0, lo = INFINITY, nhi = INFINITY;
  for (int64_t b = threadIdx.x; b < nb; b += ST_T) {
    s += ws[b];
    lo = fmin(lo, ws[nb + b]);
    nhi = fmin(nhi, ws[2 * nb + b]);
  }
  s = block_tree_sum_d<ST_T>(s, red);
  lo = block_tree_min_d<ST_T>(lo, red);
  nhi = block_tree_min_d<ST_T>(nhi, red);
  if (threadIdx.x == 0) {
    out6[0] = lo;
    out6[1] = -nhi;
    out6[2] = s / (double)n;
  }
}

// pass 2: ws[b], ws[nb + b], ws[2 nb + b] = block sums of d^2, d^3, d^4, d = x - out6[2]
__global__ __launch_bounds__(ST_T) void stat_central_kernel(const double* __restrict__ x,
                                                            int64_t n,
                                                            const double* __restrict__ out6,
                                                            double* __restrict__ ws) {
#pragma clang fp contract(off)
  __shared__ double red[ST_T];
  const int64_t nb = gridDim.x, step = nb * ST_T;
  const double mean = out6[2];
  double s2 = 0.0, s3 = 0.0, s4 = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * ST_T + threadIdx.x; i < n; i += step) {
    const double d = x[i] - mean;
    const double d2 = d * d;
    s2 += d2;
    s3 += d2 * d;
    s4 += d2 * d2;
  }
  s2 = block_tree_sum_d<ST_T>(s2, red);
  s3 = block_tree_sum_d<ST_T>(s3, red);
  s4 = block_tree_sum_d<ST_T>(s4, red);
  if (threadIdx.x == 0) {
    ws[blockIdx.x] = s2;
    ws[nb + blockIdx.x] = s3;
    ws[2 * nb + blockIdx.x] = s4;
  }
}

__global__ __launch_bounds__(ST_T) void stat_central_finish_kernel(const double* __restrict__ ws,
                                                                   int64_t nb, int64_t n,
                                                                   double* __restrict__ out6) {
#pragma clang fp contract(off)
  __shared__ double red[ST_T];
  double s2 = 0.0, s3 = 0.0, s4 = 0.0;
  for (int64_t b = threadIdx.x; b < nb; b += ST_T) {
    s2 += ws[b];
    s3 += ws[nb + b];
    s4 += ws[2 * nb + b];
  }
  s2 = block_tree_sum_d<ST_T>(s2, red);
  s3 = block_tree_sum_d<ST_T>(s3, red);
  s4 = block_tree_sum_d<ST_T>(s4, red);
  if (threadIdx.x == 0) {
    out6[3] = s2 / (double)n;
    out6[4] = s3 / (double)n;
    out6[5] = s4 / (double)n;
  }
}

// ---- Gaussian KDE ----------------------------------------------------------------------
constexpr int KDE_GT = 10;  // grid points per thread (registers); blockIdx.y tiles the grid

// ws[blockIdx.x * G + g] = sum over this block's samples of exp(-(grid[g]/s - x[i]/s)^2 / 2)
__global__ __launch_bounds__(ST_T) void kde_partial_kernel(const double* __restrict__ x, int64_t n,
                                                           const double* __restrict__ grid,
                                                           int64_t G, double s,
                                                           double* __restrict__ ws) {
  __shared__ double red[ST_T / 64][KDE_GT];
  const int64_t g0 = (int64_t)blockIdx.y * KDE_GT;
  double gw[KDE_GT], acc[KDE_GT];
#pragma unroll
  for (int j = 0; j < KDE_GT; ++j) {
    gw[j] = g0 + j < G ? grid[g0 + j] / s : 0.0;
    acc[j] = 0.0;
  }
  const int64_t step = (int64_t)gridDim.x * ST_T;
  for (int64_t i = (int64_t)blockIdx.x * ST_T + threadIdx.x; i < n; i += step) {
    const double xi = x[i] / s;
#pragma unroll
    for (int j = 0; j < KDE_GT; ++j) {
      const double d = gw[j] - xi;
      acc[j] += exp(-0.5 * (d * d));
    }
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < KDE_GT; ++j) {
    const double v = wave_sum_d(acc[j]);
    if (lane == 0) red[wid][j] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < KDE_GT && g0 + threadIdx.x < G) {
    double t = 0.0;
    for (int w = 0; w < ST_T / 64; ++w) t += red[w][threadIdx.x];
    ws[(int64_t)blockIdx.x * G + g0 + threadIdx.x] = t;
  }
}

// out[g] = norm * sum_b ws[b * G + g], blocks in order
__global__ __launch_bounds__(ST_T) void kde_finish_kernel(const double* __restrict__ ws,
                                                          int64_t nb, int64_t G, double norm,
                                                          double* __restrict__ out) {
  const int64_t g = (int64_t)blockIdx.x * ST_T + threadIdx.x;
  if (g >= G) return;
  double t = 0.0;
  for (int64_t b = 0; b < nb; ++b) t += ws[b * G + g];
  out[g] = t * norm;
}

// ---- mean autocorrelation ----------------------------------------------------------------
constexpr int ACF_R = 8;               // consecutive lags per thread
constexpr int ACF_KT = ST_T * ACF_R;   // lags per block (2048)
constexpr int ACF_PAD = 16;            // zeros past L + ACF_KT the unrolled window may read
constexpr int64_t ACF_MAX_L = 8192;
// Blocks asked for.  A block's time is its first wave's (series per chunk) x (L - k0) steps,
// so few series per chunk keep the longest block short; up to three blocks share a CU.
constexpr int64_t ACF_TARGET_BLOCKS = 4096;
static_assert(ACF_R == 8, "the LDS layout below splits an index into (m & 7, m >> 3)");

// LDS layout: element m of the staged series sits at (m & 7) * P + (m >> 3).  A wave's
// window reads are m = c + 8 lane (same plane, consecutive slots): conflict-free, where the
// plain layout would put 16 lanes on one bank pair.
__device__ __forceinline__ int acf_at(int m, int P) { return (m & 7) * P + (m >> 3); }

int acf_plane(int64_t L) { return (int)((L + ACF_KT + ACF_PAD + 7) / 8) | 1; }

// ws[chunk * L + k] = sum over the chunk's series n of sum_t x[n ld + t] x[n ld + t + k]
__global__ __launch_bounds__(ST_T) void acf_partial_kernel(const double* __restrict__ x, int64_t N,
                                                           int64_t ld, int L, int P, int spc,
                                                           double* __restrict__ ws) {
  extern __shared__ double S[];  // 8 * P doubles
  const int k0 = blockIdx.x * ACF_KT;         // first lag of the block
  const int kb = k0 + threadIdx.x * ACF_R;    // first lag of the thread
  // t = 0 .. T-1 reach the wave's first lag: the trip count is uniform within a wave, and a
  // wave of high lags stops early instead of multiplying the zeros behind the series
  const int T = L - (kb - (int)(threadIdx.x & 63) * ACF_R);
  const int64_t n0 = (int64_t)blockIdx.y * spc;
  const int64_t n1 = n0 + spc < N ? n0 + spc : N;
  // zeros behind the series: the window of a lag near L, and the last unrolled step, read them
  for (int m = L + threadIdx.x; m < 8 * P; m += ST_T) S[acf_at(m, P)] = 0.0;
  double acc[ACF_R];
#pragma unroll
  for (int j = 0; j < ACF_R; ++j) acc[j] = 0.0;
  for (int64_t n = n0; n < n1; ++n) {
    __syncthreads();  // the previous series is consumed
    const double* __restrict__ row = x + n * ld;
    for (int m = threadIdx.x; m < L; m += ST_T) S[acf_at(m, P)] = row[m];
    __syncthreads();
    if (kb < L) {
      double sa[ACF_R], w[ACF_R];
#pragma unroll
      for (int j = 0; j < ACF_R; ++j) {
        sa[j] = 0.0;
        w[j] = S[acf_at(kb + j, P)];
      }
      // step t: w[(u + j) & 7] holds s[t + kb + j]; slot u is then refilled with s[t + kb + 8].
      // Highest index read, kw the wave's first lag: (L - kw + 6) + (kw + 504) + 8 = L + 518
      // < L + ACF_KT + ACF_PAD.
      // The 16 LDS reads of a round of 8 steps are issued ahead of its 64 FMAs, so one read
      // latency is paid per round, not one per step.
      for (int t0 = 0; t0 < T; t0 += ACF_R) {
        double a[ACF_R], wn[ACF_R];
#pragma unroll
        for (int u = 0; u < ACF_R; ++u) {
          a[u] = S[acf_at(t0 + u, P)];
          wn[u] = S[acf_at(t0 + u + kb + ACF_R, P)];
        }
#pragma unroll
        for (int u = 0; u < ACF_R; ++u) {
#pragma unroll
          for (int j = 0; j < ACF_R; ++j) sa[j] = fma(a[u], w[(u + j) & 7], sa[j]);
          w[u] = wn[u];
        }
      }
#pragma unroll
      for (int j = 0; j < ACF_R; ++j) acc[j] += sa[j];
    }
  }
#pragma unroll
  for (int j = 0; j < ACF_R; ++j)
    if (kb + j < L) ws[(int64_t)blockIdx.y * L + kb + j] = acc[j];
}

// out[k] = (sum_c ws[c * L + k]) / N: chunks in order within groups of 32, then the groups in
// order, so the rounding error grows with 32 + chunks / 32 additions, not with chunks
__global__ __launch_bounds__(ST_T) void acf_finish_kernel(const double* __restrict__ ws,
                                                          int64_t chunks, int64_t L, int64_t N,
                                                          double* __restrict__ out) {
  const int64_t k = (int64_t)blockIdx.x * ST_T + threadIdx.x;
  if (k >= L) return;
  double t = 0.0;
  for (int64_t c0 = 0; c0 < chunks; c0 += 32) {
    const int64_t c1 = c0 + 32 < chunks ? c0 + 32 : chunks;
    double g = 0.0;
    for (int64_t c = c0; c < c1; ++c) g += ws[c * L + k];
    t += g;
  }
  out[k] = t / (double)N;
}

// series per chunk: (lag tiles x chunks) reaches ACF_TARGET_BLOCKS when N allows it
int64_t acf_spc(int64_t N, int64_t L) {
  const int64_t tiles = (L + ACF_KT - 1) / ACF_KT;
  int64_t chunks = (ACF_TARGET_BLOCKS + tiles - 1) / tiles;
  if (chunks > N) chunks = N;
  return (N + chunks - 1) / chunks;
}

}  // namespace
}  // namespace tvq

using namespace tvq;

extern "C" int64_t tvq_stat_moments_workspace(int64_t n) { return n > 0 ? 3 * stat_blocks(n) : 0; }

extern "C" int tvq_stat_moments(const double* x, int64_t n, double* out6, double* workspace,
                                tvq_stream_t stream) {
  TVQ_CHECK_ARG(x && out6 && workspace && n >= 1, "tvq_stat_moments: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  const int64_t nb = stat_blocks(n);
  hipLaunchKernelGGL(stat_sum_kernel, dim3((unsigned)nb), dim3(ST_T), 0, st, x, n, workspace);
  hipLaunchKernelGGL(stat_sum_finish_kernel, dim3(1), dim3(ST_T), 0, st, workspace, nb, n, out6);
  hipLaunchKernelGGL(stat_central_kernel, dim3((unsigned)nb), dim3(ST_T), 0, st, x, n, out6,
                     workspace);
  hipLaunchKernelGGL(stat_central_finish_kernel, dim3(1), dim3(ST_T), 0, st, workspace, nb, n,
                     out6);
  return launch_status("tvq_stat_moments");
}

extern "C" int64_t tvq_stat_kde_workspace(int64_t n, int64_t G) {
  return n > 0 && G > 0 ? stat_blocks(n) * G : 0;
}

extern "C" int tvq_stat_kde(const double* x, int64_t n, const double* grid, int64_t G, double s,
                            double* out, double* workspace, tvq_stream_t stream) {
  TVQ_CHECK_ARG(x && grid && out && workspace && n >= 1 && G >= 1, "tvq_stat_kde: bad arguments");
  TVQ_CHECK_ARG(s > 0.0 && s < INFINITY, "tvq_stat_kde: the bandwidth must be positive and finite");
  TVQ_CHECK_ARG(G <= 65535 * (int64_t)KDE_GT, "tvq_stat_kde: G too large");
  hipStream_t st = (hipStream_t)stream;
  const int64_t nb = stat_blocks(n);
  const int64_t gt = (G + KDE_GT - 1) / KDE_GT;
  hipLaunchKernelGGL(kde_partial_kernel, dim3((unsigned)nb, (unsigned)gt), dim3(ST_T), 0, st, x, n,
                     grid, G, s, workspace);
  const double norm = 1.0 / ((double)n * s * 2.5066282746310002);  // sqrt(2 pi)
  hipLaunchKernelGGL(kde_finish_kernel, dim3((unsigned)((G + ST_T - 1) / ST_T)), dim3(ST_T), 0, st,
                     workspace, nb, G, norm, out);
  return launch_status("tvq_stat_kde");
}

extern "C" int64_t tvq_stat_acf_max_len(void) { return ACF_MAX_L; }

extern "C" int64_t tvq_stat_acf_workspace(int64_t N, int64_t L) {
  if (N < 1 || L < 1 || L > ACF_MAX_L) return 0;
  const int64_t spc = acf_spc(N, L);
  return (N + spc - 1) / spc * L;
}

extern "C" int tvq_stat_acf_mean(const double* x, int64_t N, int64_t ld, int64_t L, double* out,
                                 double* workspace, tvq_stream_t stream) {
  TVQ_CHECK_ARG(x && out && workspace && N >= 1 && L >= 1, "tvq_stat_acf_mean: bad arguments");
  TVQ_CHECK_ARG(L <= ACF_MAX_L, "tvq_stat_acf_mean: L = %lld exceeds the limit of %lld",
                (long long)L, (long long)ACF_MAX_L);
  TVQ_CHECK_ARG(ld >= L, "tvq_stat_acf_mean: row stride %lld < L", (long long)ld);
  hipStream_t st = (hipStream_t)stream;
  const int P = acf_plane(L);
  const size_t lds = (size_t)8 * P * sizeof(double);  // <= 82.3 KiB at L = 8192
  // above 64 KiB of dynamic LDS a kernel has to opt in (a gfx950 CU has 160 KiB)
  static bool attr = [] {
    (void)hipFuncSetAttribute((const void*)acf_partial_kernel,
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)((size_t)8 * acf_plane(ACF_MAX_L) * sizeof(double)));
    return true;
  }();
  (void)attr;
  const int64_t spc = acf_spc(N, L);
  const int64_t chunks = (N + spc - 1) / spc;
  const int64_t tiles = (L + ACF_KT - 1) / ACF_KT;
  hipLaunchKernelGGL(acf_partial_kernel, dim3((unsigned)tiles, (unsigned)chunks), dim3(ST_T), lds,
                     st, x, N, ld, (int)L, P, (int)spc, workspace);
  hipLaunchKernelGGL(acf_finish_kernel, dim3((unsigned)((L + ST_T - 1) / ST_T)), dim3(ST_T), 0, st,
                     workspace, chunks, L, N, out);
  return launch_status("tvq_stat_acf_mean");
}
