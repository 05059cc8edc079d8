// fp64 helpers of the evaluation kernels (tvq_stat, tvq_traj, tvq_traj_frechet, tvq_fid), once
// each.  These kernels promise the same bits from run to run and from batch to batch, so the
// order of every sum below is part of its contract: do not reassociate.
#pragma once
#include "tvq_common.h"

namespace tvq {

// xor butterfly over the 64 lanes; the total in every lane
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- block reductions: two orders, not interchangeable -------------------------------------
struct SumD {
  __device__ static double op(double a, double b) { return a + b; }
};
struct MinD {
  __device__ static double op(double a, double b) { return fmin(a, b); }
};
struct MaxD {
  __device__ static double op(double a, double b) { return fmax(a, b); }
};

// LDS tree over NT = blockDim.x threads (a power of two): slot t takes op(slot t, slot t + o)
// for o = NT / 2, NT / 4, ..., 1.  The result in every thread.  `red` holds NT doubles; the
// leading barrier lets one `red` serve several reductions in a row.
template <int NT, class Op>
__device__ __forceinline__ double block_tree_d(double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = NT / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = Op::op(red[threadIdx.x], red[threadIdx.x + o]);
    __syncthreads();
  }
  return red[0];
}
template <int NT>
__device__ __forceinline__ double block_tree_sum_d(double v, double* red) {
  return block_tree_d<NT, SumD>(v, red);
}
template <int NT>
__device__ __forceinline__ double block_tree_min_d(double v, double* red) {
  return block_tree_d<NT, MinD>(v, red);
}
template <int NT>
__device__ __forceinline__ double block_tree_max_d(double v, double* red) {
  return block_tree_d<NT, MaxD>(v, red);
}

// Wave first: wave_sum_d's butterfly inside each wave, then the wave totals added serially in
// wave order starting from wave 0's.  The result in every thread.  `red` holds blockDim.x / 64
// doubles (blockDim.x a multiple of 64).
__device__ __forceinline__ double block_wave_sum_d(double v, double* red) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  v = wave_sum_d(v);
  __syncthreads();
  if (lane == 0) red[wid] = v;
  __syncthreads();
  double t = red[0];
  for (int i = 1; i < nw; ++i) t += red[i];
  return t;
}

// sum_{i < n} x[i * stride] over the block: strided per-thread partials, then block_wave_sum_d
__device__ __forceinline__ double block_sum_strided(const double* x, int64_t n, int64_t stride,
                                                    double* red) {
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += blockDim.x) s += x[i * stride];
  return block_wave_sum_d(s, red);
}

// ---- planar geometry -------------------------------------------------------------------------
__device__ __forceinline__ double dist2d(double ax, double ay, double bx, double by) {
#pragma clang fp contract(off)
  const double dx = ax - bx, dy = ay - by;
  return sqrt(dx * dx + dy * dy);
}

// basic_euclidean.point_to_seg; the end-point case is Python's min(dps1, dps2)
__device__ __forceinline__ double point_to_seg(double px, double py, double p1x, double p1y,
                                               double p2x, double p2y, double dps1, double dps2,
                                               double segl) {
#pragma clang fp contract(off)
  if (p1x == p2x && p1y == p2y) return dps1;
  const double xd = p2x - p1x, yd = p2y - p1y;
  const double u1 = ((px - p1x) * xd) + ((py - p1y) * yd);
  const double u = u1 / (segl * segl);
  if ((u < 0.00001) || (u > 1.0)) return dps2 < dps1 ? dps2 : dps1;
  const double ix = p1x + u * xd, iy = p1y + u * yd;
  return dist2d(px, py, ix, iy);
}

// ---- 64 x 64 fp64 output tile ------------------------------------------------------------------
constexpr int ET_T = 64;  // output tile edge: 16 x 16 threads, a 4 x 4 sub-tile each
constexpr int ET_K = 32;  // reduction entries staged per step

// acc[u][v] = sum_k As[k][ty + 16 u] Bs[k][tx + 16 v] over k = 0 .. K - 1, ascending, one fma
// per term.  load(k0, As, Bs) is called by all 256 threads and fills both stages for
// k0 .. k0 + ET_K - 1, zeros past the operands' edges; the barriers are here.
template <class Load>
__device__ __forceinline__ void tile64_d(int64_t K, int tx, int ty, Load load,
                                         double (&acc)[4][4]) {
  __shared__ double As[ET_K][ET_T + 1];
  __shared__ double Bs[ET_K][ET_T + 1];
  for (int64_t k0 = 0; k0 < K; k0 += ET_K) {
    load(k0, As, Bs);
    __syncthreads();
#pragma unroll 4
    for (int kk = 0; kk < ET_K; ++kk) {
      double a[4], b[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        a[u] = As[kk][ty + 16 * u];
        b[u] = Bs[kk][tx + 16 * u];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = fma(a[u], b[v], acc[u][v]);
    }
    __syncthreads();
  }
}

// ---- ragged pair batches, host side ----------------------------------------------------------
// Lengths of every pair from the host copy of the offsets; false (error set) for a negative
// offset or a length outside [nmin, nmax].  each(n0, n1) sees every accepted pair in order.
template <class Each>
inline bool check_ragged_pairs(const char* what, const int64_t* h0, const int64_t* h1, int64_t P,
                               int64_t nmin, int64_t nmax, Each each) {
  for (int64_t p = 0; p < P; ++p) {
    const int64_t n0 = h0[p + 1] - h0[p], n1 = h1[p + 1] - h1[p];
    if (h0[p] < 0 || h1[p] < 0 || n0 < nmin || n1 < nmin) {
      set_error("%s: pair %lld has %lld and %lld points, at least %lld each are needed", what,
                (long long)p, (long long)n0, (long long)n1, (long long)nmin);
      return false;
    }
    if (n0 > nmax || n1 > nmax) {
      set_error("%s: pair %lld has %lld and %lld points, the limit is %lld", what, (long long)p,
                (long long)n0, (long long)n1, (long long)nmax);
      return false;
    }
    each(n0, n1);
  }
  return true;
}

}  // namespace tvq
