// VQ codebook health: k-means initialisation and dead-code expiry for gfx950
// (reference timevqvae/models/vq.py:67-106 sample_vectors / kmeans, 170-195 init_embed_ /
// replace / expire_codes_).
//
// Row draw: sample_vectors picks K rows of the M token rows, distinct (randperm(M)[:K]) when
// M >= K and i.i.d. uniform (randint) otherwise.  The distinct draw is the first K values of
// a keyed pseudo-random permutation of [0, M): a keyed bijection of [0, 2^b), 2^b >= M > 2^(b-1),
// walked along its cycle until it lands below M (cycle-walking: the restriction of a
// permutation to a subset, expected < 2 steps).  O(K), no sort, no scratch, and a pure
// function of (device seed, offset, k), so the expiry kernel draws its own rows and a captured
// graph redraws on every replay.
//
// k-means (Lloyd): the assignment is the product's own fp32-MFMA assign kernel, the per-code
// counts and row sums the deterministic group-by / segmented row sum behind tvq_vq_stats; new
// here are the gathers and the mean update.  No float atomics anywhere: the same inputs and
// the same drawn rows give the same bits on every run.
#include <limits.h>

#include "tvq_common.h"
#include "tvq_reduce.h"

namespace tvq {

constexpr int DRAW_ROUNDS = 4;

// keyed bijection of [0, 2^b): DRAW_ROUNDS rounds of (odd multiply + add mod 2^b, xorshift by
// b/2), each step invertible on b bits; the round keys are counter hashes of the stream key
__device__ __forceinline__ uint32_t draw_permute(uint32_t v, int b, uint32_t mask, uint64_t key) {
  const int s = b > 1 ? b >> 1 : 1;
#pragma unroll
  for (int r = 0; r < DRAW_ROUNDS; ++r) {
    const uint32_t ka = hash_u32(key + (uint64_t)(2 * r));
    const uint32_t kb = hash_u32(key + (uint64_t)(2 * r + 1));
    v = (v * (ka | 1u) + kb) & mask;
    v ^= v >> s;
  }
  return v;
}

// row index of draw k (0 <= k < K) among M rows
__device__ __forceinline__ int draw_row(int64_t M, int64_t K, uint64_t seed, int k) {
  const uint64_t key = seed * 0xD1B54A32D192ED03ull;
  if (M < K)  // with replacement (vq.py:73): floor(u * M), u a 32-bit counter hash
    return (int)(((uint64_t)hash_u32(key + 0x100ull + (uint64_t)k) * (uint64_t)M) >> 32);
  int b = 1;
  while (((int64_t)1 << b) < M) ++b;
  const uint32_t mask = b >= 32 ? 0xFFFFFFFFu : ((1u << b) - 1u);
  uint32_t v = (uint32_t)k;  // k < K <= M: the walk stays on k's cycle, which re-enters [0, M)
  do {
    v = draw_permute(v, b, mask, key);
  } while ((int64_t)v >= M);
  return (int)v;
}

__global__ void vq_draw_rows_kernel(int64_t M, int64_t K, const int64_t* __restrict__ seed_ptr,
                                    uint64_t offset, int32_t* __restrict__ sel) {
  const int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (k >= K) return;
  sel[k] = draw_row(M, K, mix_seed(seed_ptr, offset), (int)k);
}

// embed[k, :] = x[row sel[k], :] for every k with cluster_size[k] < threshold (vq.py:181-195);
// one 64-thread block per code.  A row index outside [0, M) (a bad injected sel) writes
// nothing.  n_expired (optional): the number of expired codes, by block 0.
__global__ __launch_bounds__(64) void vq_expire_kernel(
    const float* __restrict__ x, int64_t M, int64_t N, int D, int64_t sB, int64_t sN, int64_t sD,
    const int32_t* __restrict__ sel, const int64_t* __restrict__ seed_ptr, uint64_t offset,
    const float* __restrict__ cluster_size, float threshold, int K, float* __restrict__ embed,
    int32_t* __restrict__ n_expired) {
  const int k = blockIdx.x;
  if (n_expired && k == 0) {
    int c = 0;
    for (int j = threadIdx.x; j < K; j += 64) c += cluster_size[j] < threshold ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (threadIdx.x == 0) n_expired[0] = c;
  }
  if (!(cluster_size[k] < threshold)) return;
  const int64_t m = sel ? (int64_t)sel[k] : (int64_t)draw_row(M, K, mix_seed(seed_ptr, offset), k);
  if (m < 0 || m >= M) return;
  const int64_t b = m / N, n = m - b * N;
  const float* xr = x + b * sB + n * sN;
  for (int d = threadIdx.x; d < D; d += 64) embed[(int64_t)k * D + d] = xr[(int64_t)d * sD];
}

// rows[m, :] = x[m / N, m % N, :] token-major (the fit then reads contiguous rows whatever
// the layout of x, so a strided view and its token-major copy give the same bits)
__global__ __launch_bounds__(256) void vq_rows_kernel(const float* __restrict__ x, int64_t M,
                                                      int64_t N, int D, int64_t sB, int64_t sN,
                                                      int64_t sD, float* __restrict__ rows) {
  const int64_t total = M * (int64_t)D;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t m = e / D;
    const int d = (int)(e - m * D);
    const int64_t b = m / N, n = m - b * N;
    rows[e] = x[b * sB + n * sN + (int64_t)d * sD];
  }
}

// means[k, :] = rows[sel[k], :] (vq.py:81 sample_vectors); an index outside [0, M) gives zeros
__global__ __launch_bounds__(64) void vq_gather_means_kernel(const float* __restrict__ rows,
                                                             int64_t M, int D,
                                                             const int32_t* __restrict__ sel,
                                                             float* __restrict__ means) {
  const int k = blockIdx.x;
  const int64_t m = sel[k];
  const bool ok = m >= 0 && m < M;
  for (int d = threadIdx.x; d < D; d += 64)
    means[(int64_t)k * D + d] = ok ? rows[m * D + d] : 0.f;
}

// Lloyd update (vq.py:93-104): means = where(bins == 0, means, sums / max(bins, 1))
__global__ __launch_bounds__(64) void vq_kmeans_update_kernel(const float* __restrict__ sums,
                                                              const int32_t* __restrict__ counts,
                                                              int D, float* __restrict__ means) {
  const int k = blockIdx.x;
  const int c = counts[k];
  if (c == 0) return;
  const float cf = (float)c;
  for (int d = threadIdx.x; d < D; d += 64)
    means[(int64_t)k * D + d] = sums[(int64_t)k * D + d] / cf;
}

// workspace layout of tvq_vq_kmeans, in 4-byte words (every part a multiple of 4 words)
struct KmeansWs {
  int64_t rows, quant, idx, idx32, ee, counts, sums, stats, total;
};
static int64_t al4(int64_t n) { return ((n + 3) / 4) * 4; }
static KmeansWs kmeans_ws(int64_t M, int64_t K, int64_t D) {
  KmeansWs w;
  int64_t o = 0;
  w.rows = o;   o += al4(M * D);
  w.quant = o;  o += al4(M * D);  // the assign kernel's mandatory E[idx] output (unused)
  w.idx = o;    o += al4(2 * M);  // int64
  w.idx32 = o;  o += al4(M);
  w.ee = o;     o += al4(K);
  w.counts = o; o += al4(K);
  w.sums = o;   o += al4(K * D);
  w.stats = o;  o += al4(tvq_vq_stats_workspace(M, K));
  w.total = o;
  return w;
}

}  // namespace tvq

using namespace tvq;

extern "C" int tvq_vq_draw_rows(int64_t M, int64_t K, const int64_t* seed_ptr, uint64_t offset,
                                int32_t* sel, tvq_stream_t stream) {
  TVQ_CHECK_ARG(M > 0 && M < INT_MAX && K > 0 && K < INT_MAX && seed_ptr && sel,
                "tvq_vq_draw_rows: bad arguments");
  hipLaunchKernelGGL(vq_draw_rows_kernel, dim3((unsigned)((K + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, M, K, seed_ptr, offset, sel);
  return launch_status("tvq_vq_draw_rows");
}

extern "C" int tvq_vq_expire(const float* x, int64_t B, int64_t N, int64_t D, int64_t sB,
                             int64_t sN, int64_t sD, const int32_t* sel, const int64_t* seed_ptr,
                             uint64_t offset, const float* cluster_size, float threshold,
                             int64_t K, float* embed, int32_t* n_expired, tvq_stream_t stream) {
  TVQ_CHECK_ARG(x && cluster_size && embed && B > 0 && N > 0 && D > 0 && D < INT_MAX && K > 0 &&
                    K < INT_MAX && B * N < INT_MAX, "tvq_vq_expire: bad arguments");
  TVQ_CHECK_ARG(sel || seed_ptr, "tvq_vq_expire: needs injected rows or a device seed");
  hipLaunchKernelGGL(vq_expire_kernel, dim3((unsigned)K), dim3(64), 0, (hipStream_t)stream, x,
                     B * N, N, (int)D, sB, sN, sD, sel, seed_ptr, offset, cluster_size, threshold,
                     (int)K, embed, n_expired);
  return launch_status("tvq_vq_expire");
}

extern "C" int64_t tvq_vq_kmeans_workspace(int64_t M, int64_t K, int64_t D) {
  if (M <= 0 || K <= 0 || D <= 0) return 0;
  return kmeans_ws(M, K, D).total;
}

extern "C" int tvq_vq_kmeans(const float* x, int64_t B, int64_t N, int64_t D, int64_t sB,
                             int64_t sN, int64_t sD, const int32_t* sel, int64_t K, int64_t iters,
                             float* means, float* bins, int32_t* workspace, tvq_stream_t stream) {
  TVQ_CHECK_ARG(x && sel && means && bins && workspace && B > 0 && N > 0 && K > 0 && K < INT_MAX &&
                    B * N < INT_MAX, "tvq_vq_kmeans: bad arguments");
  TVQ_CHECK_ARG(iters >= 1, "tvq_vq_kmeans: iters must be >= 1 (bins belong to an assignment)");
  if (D != 32 && D != 64 && D != 128) {
    set_error("tvq_vq_kmeans: unsupported codebook dim %lld (32/64/128)", (long long)D);
    return TVQ_ERR_ARG;
  }
  const int64_t M = B * N;
  hipStream_t st = (hipStream_t)stream;
  const KmeansWs w = kmeans_ws(M, K, D);
  float* rows = (float*)(workspace + w.rows);
  float* quant = (float*)(workspace + w.quant);
  int64_t* idx = (int64_t*)(workspace + w.idx);
  int32_t* idx32 = workspace + w.idx32;
  float* ee = (float*)(workspace + w.ee);
  int32_t* counts = workspace + w.counts;
  float* sums = (float*)(workspace + w.sums);
  int32_t* stats_ws = workspace + w.stats;
  TVQ_PLAN("vq_kmeans M%lld K%lld D%lld iters%lld", (long long)M, (long long)K, (long long)D,
           (long long)iters);
  const int64_t nb = (M * D + 255) / 256;
  hipLaunchKernelGGL(vq_rows_kernel, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(256), 0, st, x,
                     M, N, (int)D, sB, sN, sD, rows);
  hipLaunchKernelGGL(vq_gather_means_kernel, dim3((unsigned)K), dim3(64), 0, st, rows, M, (int)D,
                     sel, means);
  int rc = launch_status("tvq_vq_kmeans");
  for (int64_t it = 0; it < iters && rc == TVQ_OK; ++it) {
    rc = tvq_vq_sqnorm(means, K, D, ee, stream);
    if (rc == TVQ_OK)
      rc = tvq_vq_assign(rows, 1, M, D, M * D, D, 1, means, ee, K, 0, quant, idx, idx32, nullptr,
                         stream);
    // bins = the per-code counts of this assignment, as float (vq.py:93); the last
    // iteration's stay (vq.py:106)
    if (rc == TVQ_OK)
      rc = tvq_vq_stats(rows, 1, M, D, M * D, D, 1, idx32, K, counts, bins, sums, stats_ws, stream);
    if (rc == TVQ_OK) {
      hipLaunchKernelGGL(vq_kmeans_update_kernel, dim3((unsigned)K), dim3(64), 0, st, sums, counts,
                         (int)D, means);
      rc = launch_status("tvq_vq_kmeans");
    }
  }
  return rc;
}
