// FID on the device for gfx950, float64 throughout: the feature moments
// (tvq_fid_moments), and the whole distance with tr sqrtm(sigma1 sigma2) as a sum of singular
// values by one-sided Jacobi (tvq_fid_device, tvq_jacobi_sv).
//
// Reference: timevqvae/evaluation/eval_utils.py:56-81 calculate_fid: mu = z.mean(0),
// sigma = np.cov(z, rowvar=False) (float64, divisor N-1), then
//   fid = |mu1 - mu2|^2 + tr(sigma1 + sigma2 - 2 sqrtm(sigma1 sigma2)).
// tvq_fid_moments gives mu and sigma and leaves the D x D square root to the host
// (scipy.linalg.sqrtm, as the reference), see timevqvae/evaluation/eval_utils.py.
// For tvq_fid_device, with A_i = (z_i - mu_i) / sqrt(N_i - 1), sigma_i = A_i^T A_i; the non-zero
// eigenvalues of sigma1 sigma2 are the squared singular values of A1 A2^T, so the trace of the square root is
// the nuclear norm T = sum_k s_k(A1 A2^T) and nothing is squared on the way.
//
//   few  (min(N1, N2) <= D): W = A1 A2^T, the min(N1, N2) vectors as rows; Jacobi; T = sum of
//        the row norms.
//   many (min(N1, N2) > D):  Jacobi on the rows of [sigma_i | I] (decisions on the sigma half)
//        leaves |lambda_j| v_j on the left and v_j on the right; F_i = rows sqrt(lambda_j)
//        v_j^T has F_i^T F_i = sigma_i; W = F1 F2^T (D x D); Jacobi; T = sum of the row norms.
//
//   fid_mean_kernel      mu[d] = (sum_n z[n, d]) / N, one thread per column, rows in order
//   fid_centre_kernel    the same mu, A = (z - mu) / sqrt(N - 1) and the column sums of A^2
//   fid_cov_kernel       one block per upper-triangular 64 x 64 tile (ti <= tj) of the
//                        covariance: the centred rows of both column panels staged 32 at a
//                        time, the sums scaled by 1 / (N - 1), the tile written to (ti, tj) and
//                        mirrored to (tj, ti)
//   fid_abt_kernel       C = A B^T (A M x K, B Nn x K, row-major), K staged 32 at a time
//                        Both are tvq_eval.h's tile64_d (4 x 4 fp64 FMA sub-tiles, edge tiles
//                        zero-filled) with their own stage loader and epilogue.  The bound is
//                        the fp64 FMA rate (covariance: 2 N D^2 flop, the N x D input is read
//                        D/64 times from L2).  (z - mu) summed and then scaled and
//                        (z - mu) / sqrt(N - 1) multiplied are different arithmetic: "many"
//                        keeps the first, "few" the second.
//   jacobi_round_kernel  one round of the round-robin tournament: one workgroup per pair
//                        (p, q), alpha / beta / gamma by a fixed tree, the Hestenes rotation
//                        over the whole vectors.  One launch per round: the launch boundary
//                        is the only synchronisation between rounds.  Rotations are counted
//                        in the next sweep's counter (an integer atomic: no result bit depends
//                        on it); a round whose sweep's own counter is zero returns at once, so
//                        every sweep can be enqueued up front with no host read.
//   fid_stack / fid_factor / jacobi_norms / fid_finish   glue, fixed-order sums.
// No float atomics anywhere: two runs give the same bits.
#include "tvq_eval.h"

namespace tvq {

constexpr int JS_T = 256;         // threads per pair
constexpr int JS_R = 8;           // entries of each vector a thread keeps in registers
constexpr int JS_MAX_SWEEPS = 64;
constexpr int JS_CTR = 128;       // int32 counters per Jacobi run (>= JS_MAX_SWEEPS + 1)
constexpr int64_t JS_MAX_N = 16384, JS_MAX_M = 16384;
constexpr int64_t FIDS_MAX_D = 2048, FIDS_MAX_N = 16384;

// sum_n z[n, d], rows in order
__device__ __forceinline__ double fid_col_sum(const double* __restrict__ z, int64_t N, int64_t D,
                                              int64_t d) {
  double s = 0.0;
  for (int64_t n = 0; n < N; ++n) s += z[n * D + d];
  return s;
}

__global__ __launch_bounds__(256) void fid_mean_kernel(const double* __restrict__ z, int64_t N,
                                                       int64_t D, double* __restrict__ mu) {
  const int64_t d = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (d >= D) return;
  mu[d] = fid_col_sum(z, N, D, d) / (double)N;
}

__global__ __launch_bounds__(256) void fid_centre_kernel(const double* __restrict__ z, int64_t N,
                                                         int64_t D, double* __restrict__ mu,
                                                         double* __restrict__ A,
                                                         double* __restrict__ colsq) {
  const int64_t d = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (d >= D) return;
  const double m = fid_col_sum(z, N, D, d) / (double)N;
  mu[d] = m;
  const double sc = sqrt((double)(N - 1));
  double q = 0.0;
  for (int64_t n = 0; n < N; ++n) {
    const double v = (z[n * D + d] - m) / sc;
    A[n * D + d] = v;
    q = fma(v, v, q);
  }
  colsq[d] = q;
}

__global__ __launch_bounds__(256) void fid_cov_kernel(const double* __restrict__ z, int64_t N,
                                                      int64_t D, const double* __restrict__ mu,
                                                      double* __restrict__ cov, int nt) {
  // blockIdx.x -> (ti, tj), ti <= tj, row-major over the upper triangle
  int t = blockIdx.x, ti = 0;
  while (t >= nt - ti) {
    t -= nt - ti;
    ++ti;
  }
  const int tj = ti + t;
  const int64_t i0 = (int64_t)ti * ET_T, j0 = (int64_t)tj * ET_T;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  double acc[4][4] = {};
  // a stage is ET_K centred rows of the two column panels, row-major as z itself
  tile64_d(N, tx, ty, [&](int64_t n0, auto& As, auto& Bs) {
    for (int e = threadIdx.x; e < ET_K * ET_T; e += 256) {
      const int r = e / ET_T, c = e - r * ET_T;
      const int64_t n = n0 + r;
      const int64_t ci = i0 + c, cj = j0 + c;
      As[r][c] = (n < N && ci < D) ? z[n * D + ci] - mu[ci] : 0.0;
      Bs[r][c] = (n < N && cj < D) ? z[n * D + cj] - mu[cj] : 0.0;
    }
  }, acc);
  const double inv = 1.0 / (double)(N - 1);
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int64_t i = i0 + ty + 16 * u, j = j0 + tx + 16 * v;
      if (i < D && j < D) {
        const double c = acc[u][v] * inv;
        cov[i * D + j] = c;
        if (ti != tj) cov[j * D + i] = c;
      }
    }
}

__global__ __launch_bounds__(256) void fid_abt_kernel(const double* __restrict__ A, int64_t M,
                                                      const double* __restrict__ B, int64_t Nn,
                                                      int64_t K, double* __restrict__ C) {
  const int64_t i0 = (int64_t)blockIdx.y * ET_T, j0 = (int64_t)blockIdx.x * ET_T;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  double acc[4][4] = {};
  // a stage is ET_K entries of ET_T rows of A and of B, transposed on the way in
  tile64_d(K, tx, ty, [&](int64_t k0, auto& As, auto& Bs) {
    for (int e = threadIdx.x; e < ET_K * ET_T; e += 256) {
      const int r = e / ET_K, kk = e - r * ET_K;
      const int64_t k = k0 + kk, i = i0 + r, j = j0 + r;
      As[kk][r] = (k < K && i < M) ? A[i * K + k] : 0.0;
      Bs[kk][r] = (k < K && j < Nn) ? B[j * K + k] : 0.0;
    }
  }, acc);
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int64_t i = i0 + ty + 16 * u, j = j0 + tx + 16 * v;
      if (i < M && j < Nn) C[i * Nn + j] = acc[u][v];
    }
}

// counters c[0 .. JS_CTR): c[s] = rotations of sweep s - 1 (c[0] = 1 starts sweep 0)
__global__ void jacobi_init_kernel(int* __restrict__ c) {
  if (threadIdx.x < JS_CTR) c[threadIdx.x] = threadIdx.x == 0 ? 1 : 0;
}

// Round `round` of the tournament on ne = ne1 + 1 players (ne even; player ne1 >= n is the
// bye of an odd n): pair 0 is (ne1, round), pair k is (round + k, round - k) mod ne1.
__global__ __launch_bounds__(JS_T) void jacobi_round_kernel(double* __restrict__ a, int n, int ne1,
                                                            int64_t m_all, int64_t m_dot,
                                                            int round, const int* prev, int* cur) {
  if (ld_wt(prev) == 0) return;  // the sweep before rotated nothing: converged
  __shared__ double red[3][JS_T / 64];
  const int k = blockIdx.x;
  int p, q;
  if (k == 0) {
    p = ne1;
    q = round;
  } else {
    p = (round + k) % ne1;
    q = (round - k + ne1) % ne1;
  }
  if (p >= n || q >= n) return;
  double* __restrict__ ap = a + (int64_t)p * m_all;
  double* __restrict__ aq = a + (int64_t)q * m_all;
  const int tid = threadIdx.x;
  double xp[JS_R], xq[JS_R];
  double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
  for (int u = 0; u < JS_R; ++u) {
    const int64_t i = tid + u * JS_T;
    xp[u] = i < m_all ? ap[i] : 0.0;
    xq[u] = i < m_all ? aq[i] : 0.0;
    if (i < m_dot) {
      al = fma(xp[u], xp[u], al);
      be = fma(xq[u], xq[u], be);
      ga = fma(xp[u], xq[u], ga);
    }
  }
  for (int64_t i = tid + JS_R * JS_T; i < m_dot; i += JS_T) {
    const double vp = ap[i], vq = aq[i];
    al = fma(vp, vp, al);
    be = fma(vq, vq, be);
    ga = fma(vp, vq, ga);
  }
  const double alpha = block_wave_sum_d(al, red[0]);
  const double beta = block_wave_sum_d(be, red[1]);
  const double gamma = block_wave_sum_d(ga, red[2]);
  // the same bits in every thread, so the whole block takes one decision
  if (alpha == 0.0 || beta == 0.0) return;
  if (fabs(gamma) <= 0x1p-52 * sqrt((double)m_dot) * (sqrt(alpha) * sqrt(beta))) return;
  const double zeta = (beta - alpha) / (2.0 * gamma);
  // hypot: 1 + zeta^2 overflows for vectors of very different scale
  const double t = zeta == 0.0 ? 1.0 : copysign(1.0, zeta) / (fabs(zeta) + hypot(1.0, zeta));
  // c x_p - s x_q, s x_p + c x_q in Rutishauser's form x_p - s (x_q + tau x_p),
  // x_q + s (x_p - tau x_q), tau = s / (1 + c): for a small angle c rounds to 1, always
  // upwards, and the plain form inflates every norm by a few ulps a sweep (measured +20 ulps
  // on each singular value after 11 sweeps; this form: within 1)
  const double c = 1.0 / sqrt(1.0 + t * t), s = c * t, tau = s / (1.0 + c);
  if (tid == 0) atomicAdd(cur, 1);
#pragma unroll
  for (int u = 0; u < JS_R; ++u) {
    const int64_t i = tid + u * JS_T;
    if (i < m_all) {
      ap[i] = fma(-s, fma(tau, xp[u], xq[u]), xp[u]);
      aq[i] = fma(s, fma(-tau, xq[u], xp[u]), xq[u]);
    }
  }
  for (int64_t i = tid + JS_R * JS_T; i < m_all; i += JS_T) {
    const double vp = ap[i], vq = aq[i];
    ap[i] = fma(-s, fma(tau, vp, vq), vp);
    aq[i] = fma(s, fma(-tau, vq, vp), vq);
  }
}

// sigma[j] = |a_j| over the first m_dot entries (NaN when the last sweep still rotated);
// block 0 also writes info = {sweeps that ran, converged}
__global__ __launch_bounds__(256) void jacobi_norms_kernel(const double* __restrict__ a,
                                                           int64_t m_all, int64_t m_dot,
                                                           int max_sweeps, const int* c,
                                                           double* __restrict__ sigma,
                                                           int* __restrict__ info) {
  __shared__ double red[4];
  const double* v = a + (int64_t)blockIdx.x * m_all;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < m_dot; i += blockDim.x) s = fma(v[i], v[i], s);
  s = block_wave_sum_d(s, red);
  const bool conv = ld_wt(c + max_sweeps) == 0;
  if (threadIdx.x == 0) {
    sigma[blockIdx.x] = conv ? sqrt(s) : __builtin_nan("");
    if (blockIdx.x == 0 && info) {
      int ran = 0;
      for (int w = 0; w < max_sweeps; ++w) ran += ld_wt(c + w) != 0;
      info[0] = ran;
      info[1] = conv ? 1 : 0;
    }
  }
}

// S (D x 2D) = [cov | I]; diag[j] = cov[j][j]
__global__ __launch_bounds__(256) void fid_stack_kernel(const double* __restrict__ cov, int64_t D,
                                                        double* __restrict__ S,
                                                        double* __restrict__ diag) {
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= 2 * D * D) return;
  const int64_t j = e / (2 * D), i = e - j * 2 * D;
  S[e] = i < D ? cov[j * D + i] : (i - D == j ? 1.0 : 0.0);
  if (i == j) diag[j] = cov[j * D + j];
}

// F[j] = sqrt(lambda_j) v_j with lambda_j = |S[j][0 .. D)| and v_j = S[j][D .. 2D)
__global__ __launch_bounds__(256) void fid_factor_kernel(const double* __restrict__ S, int64_t D,
                                                         double* __restrict__ F) {
  __shared__ double red[4];
  const double* row = S + (int64_t)blockIdx.x * 2 * D;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < D; i += blockDim.x) s = fma(row[i], row[i], s);
  const double f = sqrt(sqrt(block_wave_sum_d(s, red)));
  for (int64_t i = threadIdx.x; i < D; i += blockDim.x)
    F[(int64_t)blockIdx.x * D + i] = f * row[D + i];
}

// out = {fid, |mu1 - mu2|^2, tr sigma1, tr sigma2, T}; info = {form, sweeps x 3, converged}.
// One block; ca / cb (null for "few") and cw are the runs' counters.
__global__ __launch_bounds__(256) void fid_finish_kernel(const double* __restrict__ mu1,
                                                         const double* __restrict__ mu2,
                                                         const double* __restrict__ tr1v,
                                                         const double* __restrict__ tr2v,
                                                         int64_t D, const double* __restrict__ sigma,
                                                         int64_t nvec, int form, int max_sweeps,
                                                         const int* ca, const int* cb,
                                                         const int* cw, double* __restrict__ out,
                                                         int* __restrict__ info) {
  __shared__ double red[4];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < D; i += blockDim.x) {
    const double d = mu1[i] - mu2[i];
    s = fma(d, d, s);
  }
  const double ss = block_wave_sum_d(s, red);
  const double tr1 = block_sum_strided(tr1v, D, 1, red);
  const double tr2 = block_sum_strided(tr2v, D, 1, red);
  const double T = block_sum_strided(sigma, nvec, 1, red);
  if (threadIdx.x != 0) return;
  const int* cs[3] = {ca, cb, cw};
  bool conv = true;
  info[0] = form;
  for (int r = 0; r < 3; ++r) {
    int ran = 0;
    if (cs[r]) {
      for (int w = 0; w < max_sweeps; ++w) ran += ld_wt(cs[r] + w) != 0;
      conv = conv && ld_wt(cs[r] + max_sweeps) == 0;
    }
    info[1 + r] = ran;
  }
  info[4] = conv ? 1 : 0;
  const double nan = __builtin_nan("");
  out[0] = conv ? ((ss + tr1) + tr2) - 2.0 * T : nan;
  out[1] = ss;
  out[2] = tr1;
  out[3] = tr2;
  out[4] = conv ? T : nan;
}

// Enqueue max_sweeps sweeps on the n vectors of a; c = this run's JS_CTR counters.
static void jacobi_enqueue(double* a, int64_t n, int64_t m_all, int64_t m_dot, int max_sweeps,
                           int* c, hipStream_t st) {
  hipLaunchKernelGGL(jacobi_init_kernel, dim3(1), dim3(JS_CTR), 0, st, c);
  if (n < 2) return;
  const int ne = (int)(n + (n & 1));
  for (int s = 0; s < max_sweeps; ++s)
    for (int r = 0; r < ne - 1; ++r)
      hipLaunchKernelGGL(jacobi_round_kernel, dim3(ne / 2), dim3(JS_T), 0, st, a, (int)n, ne - 1,
                         m_all, m_dot, r, c + s, c + s + 1);
}

// mu = z.mean(0) and cov = np.cov(z, rowvar=False) of z (N x D)
static void moments_enqueue(const double* z, int64_t N, int64_t D, double* mu, double* cov,
                            hipStream_t st) {
  hipLaunchKernelGGL(fid_mean_kernel, dim3((unsigned)((D + 255) / 256)), dim3(256), 0, st, z, N,
                     D, mu);
  const int nt = (int)((D + ET_T - 1) / ET_T);
  const int64_t tiles = (int64_t)nt * (nt + 1) / 2;
  hipLaunchKernelGGL(fid_cov_kernel, dim3((unsigned)tiles), dim3(256), 0, st, z, N, D, mu, cov,
                     nt);
}

static void abt_enqueue(const double* A, int64_t M, const double* B, int64_t Nn, int64_t K,
                        double* C, hipStream_t st) {
  hipLaunchKernelGGL(fid_abt_kernel,
                     dim3((unsigned)((Nn + ET_T - 1) / ET_T), (unsigned)((M + ET_T - 1) / ET_T)),
                     dim3(256), 0, st, A, M, B, Nn, K, C);
}

// form 0 (by shape) / 1 (few) / 2 (many) -> 1 / 2, or 0 with the error set
static int fid_form(const char* what, int64_t N1, int64_t N2, int64_t D, int64_t form,
                    int64_t max_sweeps) {
  const bool ok = N1 >= 2 && N2 >= 2 && N1 <= FIDS_MAX_N && N2 <= FIDS_MAX_N && D >= 1 &&
                  D <= FIDS_MAX_D && form >= 0 && form <= 2 && max_sweeps >= 1 &&
                  max_sweeps <= JS_MAX_SWEEPS;
  if (!ok) {
    set_error("%s: need 2 <= N1, N2 <= 16384, 1 <= D <= 2048, form 0 / 1 / 2 and "
              "1 <= max_sweeps <= 64 (got N1 %lld N2 %lld D %lld form %lld max_sweeps %lld)",
              what, (long long)N1, (long long)N2, (long long)D, (long long)form,
              (long long)max_sweeps);
    return 0;
  }
  const int64_t nmin = N1 < N2 ? N1 : N2;
  const int f = form ? (int)form : (nmin <= D ? 1 : 2);
  if (f == 1 && nmin > FIDS_MAX_D) {
    set_error("%s: the \"few\" form needs min(N1, N2) <= 2048 (got %lld)", what, (long long)nmin);
    return 0;
  }
  return f;
}

// workspace: 3 x JS_CTR counters, then doubles: mu1, mu2, t1, t2 (D each), sigma (nvec), and
//   few:  A1 (N1 D), A2 (N2 D), W (nmin nmax)
//   many: C1, C2 (D D each: cov_i, then F_i), S (D 2D), W (D D)
struct FidLayout {
  int64_t nvec, head, bytes;
};
static FidLayout fid_layout(int f, int64_t N1, int64_t N2, int64_t D) {
  FidLayout L;
  const int64_t nmin = N1 < N2 ? N1 : N2, nmax = N1 < N2 ? N2 : N1;
  L.nvec = f == 1 ? nmin : D;
  L.head = 4 * D + ((L.nvec + 1) & ~(int64_t)1);
  const int64_t body = f == 1 ? (N1 + N2) * D + nmin * nmax : 5 * D * D;
  L.bytes = 3 * JS_CTR * (int64_t)sizeof(int) + (L.head + body) * (int64_t)sizeof(double);
  return L;
}

}  // namespace tvq

using namespace tvq;

// mu (D) and the sample covariance (D x D, divisor N-1) of the rows of z (N x D, float64,
// row-major), as numpy's z.mean(0) / np.cov(z, rowvar=False).
extern "C" int tvq_fid_moments(const double* z, int64_t N, int64_t D, double* mu, double* cov,
                               tvq_stream_t stream) {
  TVQ_CHECK_ARG(z && mu && cov && N >= 2 && D >= 1, "tvq_fid_moments: bad arguments");
  TVQ_CHECK_ARG(D <= (1 << 20), "tvq_fid_moments: D too large");
  moments_enqueue(z, N, D, mu, cov, (hipStream_t)stream);
  return launch_status("tvq_fid_moments");
}

extern "C" int64_t tvq_jacobi_sv_workspace(int64_t n) {
  if (n < 1 || n > JS_MAX_N) {
    set_error("tvq_jacobi_sv_workspace: need 1 <= n <= 16384 (got %lld)", (long long)n);
    return -1;
  }
  return JS_CTR * (int64_t)sizeof(int);
}

extern "C" int tvq_jacobi_sv(double* a, int64_t n, int64_t m_all, int64_t m_dot,
                             int64_t max_sweeps, double* sigma, int32_t* info, void* workspace,
                             tvq_stream_t stream) {
  TVQ_CHECK_ARG(a && sigma && info && workspace, "tvq_jacobi_sv: null pointer");
  TVQ_CHECK_ARG(n >= 1 && n <= JS_MAX_N && m_dot >= 1 && m_dot <= m_all && m_all <= JS_MAX_M &&
                    max_sweeps >= 1 && max_sweeps <= JS_MAX_SWEEPS,
                "tvq_jacobi_sv: need 1 <= n <= 16384, 1 <= m_dot <= m_all <= 16384 and "
                "1 <= max_sweeps <= 64 (got n %lld m_all %lld m_dot %lld max_sweeps %lld)",
                (long long)n, (long long)m_all, (long long)m_dot, (long long)max_sweeps);
  hipStream_t st = (hipStream_t)stream;
  int* c = (int*)workspace;
  jacobi_enqueue(a, n, m_all, m_dot, (int)max_sweeps, c, st);
  hipLaunchKernelGGL(jacobi_norms_kernel, dim3((unsigned)n), dim3(256), 0, st, a, m_all, m_dot,
                     (int)max_sweeps, c, sigma, info);
  return launch_status("tvq_jacobi_sv");
}

extern "C" int64_t tvq_fid_device_workspace(int64_t N1, int64_t N2, int64_t D, int64_t form) {
  const int f = fid_form("tvq_fid_device_workspace", N1, N2, D, form, 1);
  if (!f) return -1;
  return fid_layout(f, N1, N2, D).bytes;
}

extern "C" int tvq_fid_device(const double* z1, int64_t N1, const double* z2, int64_t N2,
                              int64_t D, int64_t form, int64_t max_sweeps, double* out,
                              int32_t* info, void* workspace, tvq_stream_t stream) {
  TVQ_CHECK_ARG(z1 && z2 && out && info && workspace, "tvq_fid_device: null pointer");
  TVQ_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "tvq_fid_device: workspace not 16-byte aligned");
  const int f = fid_form("tvq_fid_device", N1, N2, D, form, max_sweeps);
  if (!f) return TVQ_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const FidLayout L = fid_layout(f, N1, N2, D);
  int* ctr = (int*)workspace;
  double* w = (double*)(ctr + 3 * JS_CTR);
  double *mu1 = w, *mu2 = w + D, *t1 = w + 2 * D, *t2 = w + 3 * D, *sigma = w + 4 * D;
  double* body = w + L.head;
  const int ms = (int)max_sweeps;
  const unsigned colblocks = (unsigned)((D + 255) / 256);
  if (f == 1) {
    double *A1 = body, *A2 = A1 + N1 * D, *W = A2 + N2 * D;
    hipLaunchKernelGGL(fid_centre_kernel, dim3(colblocks), dim3(256), 0, st, z1, N1, D, mu1, A1, t1);
    hipLaunchKernelGGL(fid_centre_kernel, dim3(colblocks), dim3(256), 0, st, z2, N2, D, mu2, A2, t2);
    const int64_t nmin = L.nvec, nmax = N1 < N2 ? N2 : N1;
    if (N1 <= N2)
      abt_enqueue(A1, N1, A2, N2, D, W, st);
    else
      abt_enqueue(A2, N2, A1, N1, D, W, st);
    jacobi_enqueue(W, nmin, nmax, nmax, ms, ctr + 2 * JS_CTR, st);
    hipLaunchKernelGGL(jacobi_norms_kernel, dim3((unsigned)nmin), dim3(256), 0, st, W, nmax, nmax,
                       ms, ctr + 2 * JS_CTR, sigma, (int*)nullptr);
    hipLaunchKernelGGL(fid_finish_kernel, dim3(1), dim3(256), 0, st, mu1, mu2, t1, t2, D, sigma,
                       nmin, 1, ms, (const int*)nullptr, (const int*)nullptr,
                       (const int*)(ctr + 2 * JS_CTR), out, info);
  } else {
    double* C[2] = {body, body + D * D};
    double *S = body + 2 * D * D, *W = body + 4 * D * D;
    const double* z[2] = {z1, z2};
    const int64_t N[2] = {N1, N2};
    double* mu[2] = {mu1, mu2};
    double* t[2] = {t1, t2};
    for (int i = 0; i < 2; ++i) {
      moments_enqueue(z[i], N[i], D, mu[i], C[i], st);
      hipLaunchKernelGGL(fid_stack_kernel, dim3((unsigned)((2 * D * D + 255) / 256)), dim3(256), 0,
                         st, C[i], D, S, t[i]);
      jacobi_enqueue(S, D, 2 * D, D, ms, ctr + i * JS_CTR, st);
      hipLaunchKernelGGL(fid_factor_kernel, dim3((unsigned)D), dim3(256), 0, st, S, D, C[i]);
    }
    abt_enqueue(C[0], D, C[1], D, D, W, st);
    jacobi_enqueue(W, D, D, D, ms, ctr + 2 * JS_CTR, st);
    hipLaunchKernelGGL(jacobi_norms_kernel, dim3((unsigned)D), dim3(256), 0, st, W, D, D, ms,
                       ctr + 2 * JS_CTR, sigma, (int*)nullptr);
    hipLaunchKernelGGL(fid_finish_kernel, dim3(1), dim3(256), 0, st, mu1, mu2, t1, t2, D, sigma, D,
                       2, ms, (const int*)ctr, (const int*)(ctr + JS_CTR),
                       (const int*)(ctr + 2 * JS_CTR), out, info);
  }
  return launch_status("tvq_fid_device");
}
