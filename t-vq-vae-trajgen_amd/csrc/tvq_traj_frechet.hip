// The continuous Frechet distance of the flyability evaluation for gfx950: the device form of
// timevqvae/evaluation/flyability_utils/trajectory_distances/frechet.py (Alt & Godau as
// traj-dist states it), the 14th distance of calculate_trajectory_distances.
//
// Reference, per pair (P of p points, Q of q points): the set of critical values {end_point}
// + point_to_seg of every cell's two edges that exceed end_point, sorted; a binary search
// over that list whose every probe decides reachability in the free-space diagram with a pure
// Python loop over all cells (LF_BF, LR_BR).  Here a ragged batch of pairs (packed as for
// csrc/tvq_traj.hip) runs in float64 through three stages, all on the device:
//
//   1 fr_critical_kernel   a thread per cell writes Lij and Bij as their bit patterns (a value
//                          not above end_point is written as end_point, which the set holds
//                          anyway); element 0 is end_point, the tail up to a whole number of
//                          sort tiles is padded with all-ones.
//   2 fr_tile_sort_kernel  bitonic sort of 4096-value tiles in LDS (non-negative doubles
//     fr_merge_kernel      order as unsigned integers), then merge passes between the two
//     fr_unique_kernel     workspace halves: every element finds its rank in the partner run by
//                          binary search (lower bound from the left run, upper bound from the
//                          right one, so the merge is stable and writes every slot once); then
//                          flag / ballot-scan / compact to the unique values and their count.
//   3 fr_search_kernel     one workgroup per pair runs every probe.  The search state (first
//                          index and length of the live slice, the last eps) lives in
//                          registers; the probe loop is bounded by ceil(log2 V) + 1.  A probe
//                          works through bands of rows: all four waves evaluate free_line of
//                          the cells' left and bottom edges and ballot the "not [-1, -1]"
//                          flags into two LDS bitmaps (a word = 64 columns); wave 0 then walks
//                          the band's rows, lane w owning word w of the row: reach(i, j) =
//                          seed(i, j) | pass(i, j) & reach(i, j - 1) with seed = reach(i - 1, j)
//                          & BF(i, j) and pass = LF(i, j) is a carry chain, resolved inside a
//                          word by a 6-step parallel prefix, across the row's words by the
//                          same prefix over two ballot masks (word generates / word passes).
//                          The interval end points are evaluated only where the reference
//                          reads them: the four corner cells, column 0 and row 0.
//
// The distances (mdist, P_dist, Q_dist of the reference) are never stored: dist2d recomputes
// them in stages 1 and 3 alike, and both stages call the one point_to_seg, so a critical
// value probed as eps sees `point_to_seg > eps` false in its own cell, exactly.  No atomics,
// a pair's value depends on that pair alone.  This file must not be built with fast-math.
#include "tvq_eval.h"

namespace tvq {
namespace {

constexpr int FR_T = 256;                 // threads per block, every kernel
constexpr int FR_TILE = 4096;             // values per LDS sort tile (32 KiB)
constexpr int FR_WORDS = 1024;            // 64-column words of the two band bitmaps (2 x 4 KiB)
constexpr unsigned long long FR_PAD = ~0ull;
typedef unsigned long long u64;

struct FrIv {
  double lo, hi;
};

__host__ __device__ inline int64_t fr_cap(int64_t n0, int64_t n1) {
  const int64_t v = (n0 < 2 || n1 < 2) ? 1 : 2 * (n0 - 1) * (n1 - 1) + 1;
  return (v + FR_TILE - 1) / FR_TILE * FR_TILE;
}

// frechet.free_line with basic_euclidean.circle_line_intersection inlined
__device__ __forceinline__ FrIv fr_free_line(double px, double py, double s1x, double s1y,
                                             double s2x, double s2y, double dps1, double dps2,
                                             double ds, double eps) {
#pragma clang fp contract(off)
  const FrIv none = {-1.0, -1.0};
  if (s1x == s2x && s1y == s2y) {
    if (dps1 > eps) return none;
    return FrIv{0.0, 1.0};
  }
  if (point_to_seg(px, py, s1x, s1y, s2x, s2y, dps1, dps2, ds) > eps) return none;
  const double segl2 = ds * ds;
  double x1, y1, x2, y2;
  if (s2x == s1x) {
    const double rac = sqrt((eps * eps) - ((s1x - px) * (s1x - px)));
    x1 = x2 = s1x;
    y1 = py + rac;
    y2 = py - rac;
  } else {
    const double m = (s2y - s1y) / (s2x - s1x);
    const double c = s2y - m * s2x;
    const double A = m * m + 1.0;
    const double B = 2.0 * (((m * c) - (m * py)) - px);
    const double C = ((((py * py) - (eps * eps)) + (px * px)) - ((2.0 * c) * py)) + (c * c);
    const double delta = (B * B) - ((4.0 * A) * C);
    if (delta <= 0.0) {
      x1 = x2 = (-B) / (2.0 * A);
      y1 = y2 = m * x1 + c;
    } else {
      const double sd = sqrt(delta);
      x1 = ((-B) + sd) / (2.0 * A);
      y1 = m * x1 + c;
      x2 = ((-B) - sd) / (2.0 * A);
      y2 = m * x2 + c;
    }
  }
  if (x1 != x2 || y1 != y2) {
    const double u1 = (((x1 - s1x) * (s2x - s1x)) + ((y1 - s1y) * (s2y - s1y))) / segl2;
    const double u2 = (((x2 - s1x) * (s2x - s1x)) + ((y2 - s1y) * (s2y - s1y))) / segl2;
    // sorted((0, 1, u1, u2))[1:3]: the two middle values of the sorted pairs (0, 1), (c, d)
    const double c = u2 < u1 ? u2 : u1, d = u2 < u1 ? u1 : u2;
    const double a = c > 0.0 ? c : 0.0, b = d < 1.0 ? d : 1.0;
    return b < a ? FrIv{b, a} : FrIv{a, b};
  }
  if (px == s1x && py == s1y) return FrIv{0.0, 0.0};
  if (px == s2x && py == s2y) return FrIv{1.0, 1.0};
  const double u1 = (((x1 - s1x) * (s2x - s1x)) + ((y1 - s1y) * (s2y - s1y))) / segl2;
  if (0.0 <= u1 && u1 <= 1.0) return FrIv{u1, u1};
  return none;
}

__device__ __forceinline__ bool fr_some(FrIv v) { return !(v.lo == -1.0 && v.hi == -1.0); }
__device__ __forceinline__ bool fr_full(FrIv v) { return v.lo == 0.0 && v.hi == 1.0; }

// One pair: P (p points) and Q (q points), row-major (n, 2).  The four functions below are the
// only places a distance is formed, always as dist2d(point of P or segment start, ...).
struct FrPair {
  const double* __restrict__ P;
  const double* __restrict__ Q;
  int p, q;
};

// Lij: point_to_seg(Q[j], P[i], P[i + 1], mdist[i, j], mdist[i + 1, j], P_dist[i])
__device__ __forceinline__ double fr_L(const FrPair& t, int i, int j) {
  const double ax = t.P[2 * i], ay = t.P[2 * i + 1], bx = t.P[2 * i + 2], by = t.P[2 * i + 3];
  const double qx = t.Q[2 * j], qy = t.Q[2 * j + 1];
  return point_to_seg(qx, qy, ax, ay, bx, by, dist2d(ax, ay, qx, qy), dist2d(bx, by, qx, qy),
                      dist2d(ax, ay, bx, by));
}
// Bij: point_to_seg(P[i], Q[j], Q[j + 1], mdist[i, j], mdist[i, j + 1], Q_dist[j])
__device__ __forceinline__ double fr_B(const FrPair& t, int i, int j) {
  const double ax = t.Q[2 * j], ay = t.Q[2 * j + 1], bx = t.Q[2 * j + 2], by = t.Q[2 * j + 3];
  const double px = t.P[2 * i], py = t.P[2 * i + 1];
  return point_to_seg(px, py, ax, ay, bx, by, dist2d(px, py, ax, ay), dist2d(px, py, bx, by),
                      dist2d(ax, ay, bx, by));
}
// LF[(i, j)]: the free part of segment [P[i], P[i + 1]] seen from Q[j]; i <= p - 2, j <= q - 1
__device__ __forceinline__ FrIv fr_LF(const FrPair& t, int i, int j, double eps) {
  const double ax = t.P[2 * i], ay = t.P[2 * i + 1], bx = t.P[2 * i + 2], by = t.P[2 * i + 3];
  const double qx = t.Q[2 * j], qy = t.Q[2 * j + 1];
  return fr_free_line(qx, qy, ax, ay, bx, by, dist2d(ax, ay, qx, qy), dist2d(bx, by, qx, qy),
                      dist2d(ax, ay, bx, by), eps);
}
// BF[(i, j)]: the free part of segment [Q[j], Q[j + 1]] seen from P[i]; i <= p - 1, j <= q - 2
__device__ __forceinline__ FrIv fr_BF(const FrPair& t, int i, int j, double eps) {
  const double ax = t.Q[2 * j], ay = t.Q[2 * j + 1], bx = t.Q[2 * j + 2], by = t.Q[2 * j + 3];
  const double px = t.P[2 * i], py = t.P[2 * i + 1];
  return fr_free_line(px, py, ax, ay, bx, by, dist2d(px, py, ax, ay), dist2d(px, py, bx, by),
                      dist2d(ax, ay, bx, by), eps);
}

__device__ __forceinline__ bool fr_load_pair(const double* pts0, const int64_t* off0,
                                             const double* pts1, const int64_t* off1, int64_t pr,
                                             int64_t max_len, FrPair* t) {
  const int64_t a0 = off0[pr], a1 = off1[pr];
  const int64_t n0 = off0[pr + 1] - a0, n1 = off1[pr + 1] - a1;
  if (a0 < 0 || a1 < 0 || n0 < 1 || n1 < 1 || n0 > max_len || n1 > max_len) return false;
  t->P = pts0 + 2 * a0;
  t->Q = pts1 + 2 * a1;
  t->p = (int)n0;
  t->q = (int)n1;
  return true;
}

// ---- stage 0: where each pair's values live ----------------------------------------------
// voff[p] = sum of fr_cap over the pairs before p, voff[P] the total; one block.  If the device
// offsets do not add up to the total the host sized the workspace for, every pair gets no room
// (all zeros) and the later kernels leave it alone.
__global__ __launch_bounds__(FR_T) void fr_layout_kernel(const int64_t* __restrict__ off0,
                                                         const int64_t* __restrict__ off1,
                                                         int64_t P, int64_t total,
                                                         int64_t* __restrict__ voff) {
  __shared__ int64_t part[FR_T];
  __shared__ int agree;
  const int t = threadIdx.x;
  const int64_t K = (P + FR_T - 1) / FR_T;
  const int64_t b = t * K < P ? t * K : P, e = b + K < P ? b + K : P;
  int64_t s = 0;
  for (int64_t p = b; p < e; ++p) s += fr_cap(off0[p + 1] - off0[p], off1[p + 1] - off1[p]);
  part[t] = s;
  __syncthreads();
  if (t == 0) {
    int64_t run = 0;
    for (int k = 0; k < FR_T; ++k) {
      const int64_t v = part[k];
      part[k] = run;
      run += v;
    }
    agree = run == total;
    voff[P] = agree ? run : 0;
  }
  __syncthreads();
  s = part[t];
  for (int64_t p = b; p < e; ++p) {
    voff[p] = agree ? s : 0;
    s += fr_cap(off0[p + 1] - off0[p], off1[p + 1] - off1[p]);
  }
}

// ---- stage 1: critical values ------------------------------------------------------------
__global__ __launch_bounds__(FR_T) void fr_critical_kernel(
    const double* __restrict__ pts0, const int64_t* __restrict__ off0,
    const double* __restrict__ pts1, const int64_t* __restrict__ off1, int64_t max_len,
    const int64_t* __restrict__ voff, u64* __restrict__ buf) {
  FrPair t;
  const int64_t pr = blockIdx.x;
  if (!fr_load_pair(pts0, off0, pts1, off1, pr, max_len, &t)) return;
  const int64_t cap = voff[pr + 1] - voff[pr];
  const int64_t cols = t.q - 1;
  const int64_t cells = (int64_t)(t.p - 1) * cols;
  const int64_t V = 2 * cells + 1;
  if (cap != fr_cap(t.p, t.q)) return;  // the layout is this pair's own
  u64* dst = buf + voff[pr];
  const double origin = dist2d(t.P[0], t.P[1], t.Q[0], t.Q[1]);
  const double end = dist2d(t.P[2 * (t.p - 1)], t.P[2 * (t.p - 1) + 1], t.Q[2 * (t.q - 1)],
                            t.Q[2 * (t.q - 1) + 1]);
  const double end_point = end > origin ? end : origin;
  int64_t n = cells > cap - V ? cells : cap - V;
  if (n < 1) n = 1;
  for (int64_t c = (int64_t)blockIdx.y * FR_T + threadIdx.x; c < n; c += (int64_t)gridDim.y * FR_T) {
    if (c == 0) dst[0] = (u64)__double_as_longlong(end_point);
    if (c < cells) {
      const int i = (int)(c / cols), j = (int)(c % cols);
      const double L = fr_L(t, i, j), B = fr_B(t, i, j);
      dst[1 + 2 * c] = (u64)__double_as_longlong(L > end_point ? L : end_point);
      dst[2 + 2 * c] = (u64)__double_as_longlong(B > end_point ? B : end_point);
    }
    if (V + c < cap) dst[V + c] = FR_PAD;
  }
}

// ---- stage 2: sort and unique ------------------------------------------------------------
__global__ __launch_bounds__(FR_T) void fr_tile_sort_kernel(const int64_t* __restrict__ voff,
                                                            u64* __restrict__ buf) {
  __shared__ u64 s[FR_TILE];
  const int64_t pr = blockIdx.x;
  const int64_t cap = voff[pr + 1] - voff[pr];
  const int64_t base = (int64_t)blockIdx.y * FR_TILE;
  if (base + FR_TILE > cap) return;  // uniform: cap is a whole number of tiles
  u64* v = buf + voff[pr] + base;
  for (int k = threadIdx.x; k < FR_TILE; k += FR_T) s[k] = v[k];
  __syncthreads();
  for (int k = 2; k <= FR_TILE; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < FR_TILE / 2; t += FR_T) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
        const u64 a = s[lo], b = s[hi];
        const bool asc = (lo & k) == 0;
        if ((a > b) == asc) {
          s[lo] = b;
          s[hi] = a;
        }
      }
      __syncthreads();
    }
  }
  for (int k = threadIdx.x; k < FR_TILE; k += FR_T) v[k] = s[k];
}

// One merge pass: runs of `run` sorted values in src pair up into runs of 2 * run in dst.
__global__ __launch_bounds__(FR_T) void fr_merge_kernel(const int64_t* __restrict__ voff,
                                                        const u64* __restrict__ src,
                                                        u64* __restrict__ dst, int64_t run) {
  const int64_t pr = blockIdx.x;
  const int64_t cap = voff[pr + 1] - voff[pr];
  const u64* a = src + voff[pr];
  u64* d = dst + voff[pr];
  for (int64_t k = (int64_t)blockIdx.y * FR_T + threadIdx.x; k < cap;
       k += (int64_t)gridDim.y * FR_T) {
    const int64_t base = k / (2 * run) * (2 * run);
    const int64_t mid = base + run < cap ? base + run : cap;
    const int64_t end = base + 2 * run < cap ? base + 2 * run : cap;
    const u64 x = a[k];
    int64_t lo, hi;
    if (k < mid) {  // left run: the count of right values below x
      lo = mid, hi = end;
      while (lo < hi) {
        const int64_t m = lo + ((hi - lo) >> 1);
        if (a[m] < x) lo = m + 1; else hi = m;
      }
      d[k + (lo - mid)] = x;
    } else {  // right run: the count of left values not above x
      lo = base, hi = mid;
      while (lo < hi) {
        const int64_t m = lo + ((hi - lo) >> 1);
        if (a[m] <= x) lo = m + 1; else hi = m;
      }
      d[(k - mid) + lo] = x;
    }
  }
}

// The unique values of a pair's sorted list (padding dropped) to dst, their count to ucnt.
__global__ __launch_bounds__(FR_T) void fr_unique_kernel(const int64_t* __restrict__ voff,
                                                         const u64* __restrict__ src,
                                                         u64* __restrict__ dst,
                                                         int64_t* __restrict__ ucnt) {
  __shared__ int wsum[FR_T / 64];
  const int64_t pr = blockIdx.x;
  const int64_t cap = voff[pr + 1] - voff[pr];
  const u64* a = src + voff[pr];
  u64* d = dst + voff[pr];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t kept = 0;
  for (int64_t base = 0; base < cap; base += FR_T) {
    const int64_t k = base + threadIdx.x;
    u64 x = 0;
    bool f = false;
    if (k < cap) {
      x = a[k];
      f = x != FR_PAD && (k == 0 || x != a[k - 1]);
    }
    const u64 mask = __ballot(f);
    if (lane == 0) wsum[wave] = __popcll(mask);
    __syncthreads();
    int before = __popcll(mask & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
    for (int w = 0; w < FR_T / 64; ++w) {
      if (w < wave) before += wsum[w];
      total += wsum[w];
    }
    if (f) d[kept + before] = x;
    kept += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) ucnt[pr] = kept;
}

// ---- stage 3: search and decision --------------------------------------------------------
// g[j] |= p[j] & g[j - 1] resolved for all 64 bits (bit 0 has no carry in)
__device__ __forceinline__ u64 fr_carry(u64 g, u64 p) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    g |= p & (g << d);
    p &= p << d;
  }
  return g;
}

// frechet.decision_problem for one eps; every thread of the block returns the same answer.
__device__ bool fr_decide(const FrPair& t, double eps, u64* lfb, u64* bfb, int* s_rep) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = t.p, q = t.q;
  // LR_BR's four corner tests ([-1, -1] passes the two `<= 0` ones, as in the reference)
  if (!(fr_LF(t, 0, 0, eps).lo <= 0.0 && fr_BF(t, 0, 0, eps).lo <= 0.0 &&
        fr_LF(t, p - 2, q - 1, eps).hi >= 1.0 && fr_BF(t, p - 1, q - 2, eps).hi >= 1.0))
    return false;
  const int rows = p - 1, cols = q - 1;  // cells
  const int W = (cols + 63) >> 6;        // <= 64 words: a lane of wave 0 per word
  const int R = (FR_WORDS / 2) / W;      // rows per band, >= 8
  u64 prev = 0, row0 = 0;                // wave 0: reach of the row above; BR[(0, j)]
  if (wave == 0) {
    for (int w = 0; w < W; ++w) {
      const int j = w * 64 + lane;
      bool b = false;
      if (j < cols)
        b = j == 0 || (fr_some(fr_BF(t, 0, j, eps)) && fr_full(fr_BF(t, 0, j - 1, eps)));
      const u64 m = __ballot(b);
      if (lane == w) row0 = m;
    }
  }
  for (int i0 = 0; i0 < rows; i0 += R) {
    const int nr = rows - i0 < R ? rows - i0 : R;
    __syncthreads();  // the band before is consumed
    for (int item = wave; item < nr * W; item += FR_T / 64) {
      const int r = item / W, w = item - r * W;
      const int i = i0 + r, j = w * 64 + lane;
      bool lf = false, bf = false;
      if (j < cols) {
        lf = fr_some(fr_LF(t, i, j, eps));
        bf = fr_some(fr_BF(t, i, j, eps));
      }
      const u64 ml = __ballot(lf), mb = __ballot(bf);
      if (lane == 0) {
        lfb[item] = ml;
        bfb[item] = mb;
      }
    }
    __syncthreads();
    if (wave == 0) {
      for (int c0 = 0; c0 < nr; c0 += 64) {
        // LR[(i, 0)] of up to 64 rows, a lane each
        const int ic = i0 + c0 + lane;
        bool b = false;
        if (c0 + lane < nr)
          b = ic == 0 || (fr_some(fr_LF(t, ic, 0, eps)) && fr_full(fr_LF(t, ic - 1, 0, eps)));
        const u64 col0 = __ballot(b);
        const int nc = nr - c0 < 64 ? nr - c0 : 64;
        for (int rr = 0; rr < nc; ++rr) {
          const int r = c0 + rr;
          const u64 lf = lane < W ? lfb[r * W + lane] : 0ull;
          const u64 bf = lane < W ? bfb[r * W + lane] : 0ull;
          const u64 seed = i0 + r == 0 ? row0 : (prev & bf);
          const u64 pass = lf | (lane == 0 ? 1ull : 0ull);  // column 0 takes LR[(i, 0)] as carry
          const u64 cin0 = (col0 >> rr) & 1ull;
          const u64 r0 = fr_carry(seed, pass);  // reach with no carry into the word
          const u64 gm = __ballot(lane < W && (r0 >> 63) != 0);
          const u64 pm = __ballot(lane < W && pass == ~0ull);
          const u64 outc = fr_carry(gm | (pm & cin0), pm);  // bit w: carry out of word w
          const u64 inc = (outc << 1) | cin0;
          const bool ci = ((inc >> lane) & 1ull) != 0;
          prev = r0 | (ci ? (pass & (pass ^ (pass + 1ull))) : 0ull);
        }
      }
    }
  }
  if (wave == 0) {
    const u64 fin = __shfl(prev, (cols - 1) >> 6, 64);
    if (lane == 0) *s_rep = (int)((fin >> ((cols - 1) & 63)) & 1ull);
  }
  __syncthreads();
  const bool rep = *s_rep != 0;
  __syncthreads();
  return rep;
}

__global__ __launch_bounds__(FR_T) void fr_search_kernel(
    const double* __restrict__ pts0, const int64_t* __restrict__ off0,
    const double* __restrict__ pts1, const int64_t* __restrict__ off1, int64_t max_len,
    const int64_t* __restrict__ voff, const u64* __restrict__ uniq,
    const int64_t* __restrict__ ucnt, double* __restrict__ out) {
  __shared__ u64 lfb[FR_WORDS / 2], bfb[FR_WORDS / 2];
  __shared__ int s_rep;
  FrPair t;
  const int64_t pr = blockIdx.x;
  if (!fr_load_pair(pts0, off0, pts1, off1, pr, max_len, &t)) return;
  const int64_t cap = voff[pr + 1] - voff[pr];
  const int64_t U = ucnt[pr];
  if (U < 1 || U > cap) return;
  const u64* cc = uniq + voff[pr];
  // cc = cc[first : first + len]; the reference's `while len(cc) != 1`, bounded by the count
  int64_t first = 0, len = U;
  double eps = __longlong_as_double((long long)cc[0]);
  int bound = 1;
  while (bound < 64 && (1ll << (bound - 1)) < U) ++bound;  // ceil(log2 U) + 1
  if (t.p < 2 || t.q < 2) bound = 0;
  for (int it = 0; it < bound; ++it) {
    if (len == 1) break;
    const int64_t m = (len >> 1) - 1;  // int(len / 2 - 1)
    eps = __longlong_as_double((long long)cc[first + m]);
    if (fr_decide(t, eps, lfb, bfb, &s_rep)) {
      len = m + 1;
    } else {
      first += m + 1;
      len -= m + 1;
    }
  }
  if (threadIdx.x == 0) out[pr] = eps;
}

constexpr int64_t FR_MAX_PAIRS = 65536;

// From the host offsets: the total of fr_cap, the largest one and the most cells of a pair.
// False (error set) for a pair outside [1, max_len].
bool fr_sizes(const char* what, const int64_t* h0, const int64_t* h1, int64_t P, int64_t max_len,
              int64_t* total, int64_t* cap_max, int64_t* cells_max) {
  *total = *cap_max = *cells_max = 0;
  return check_ragged_pairs(what, h0, h1, P, 1, max_len, [&](int64_t n0, int64_t n1) {
    const int64_t cap = fr_cap(n0, n1), cells = (n0 - 1) * (n1 - 1);
    *total += cap;
    if (cap > *cap_max) *cap_max = cap;
    if (cells > *cells_max) *cells_max = cells;
  });
}

int64_t fr_head_bytes(int64_t P) { return ((2 * P + 1) * (int64_t)sizeof(int64_t) + 255) / 256 * 256; }

}  // namespace
}  // namespace tvq

using namespace tvq;

extern "C" int64_t tvq_traj_frechet_workspace(const int64_t* host_off0, const int64_t* host_off1,
                                              int64_t P) {
  if (P < 0 || P > FR_MAX_PAIRS || (P > 0 && (!host_off0 || !host_off1))) {
    set_error("tvq_traj_frechet_workspace: bad arguments (at most %lld pairs a call)",
              (long long)FR_MAX_PAIRS);
    return -1;
  }
  if (P == 0) return 0;
  int64_t total, cap_max, cells_max;
  if (!fr_sizes("tvq_traj_frechet_workspace", host_off0, host_off1, P, tvq_traj_max_len(), &total,
                &cap_max, &cells_max))
    return -1;
  return fr_head_bytes(P) + 2 * total * (int64_t)sizeof(u64);
}

extern "C" int tvq_traj_frechet_stages(const double* pts0, const int64_t* off0,
                                       const double* pts1, const int64_t* off1,
                                       const int64_t* host_off0, const int64_t* host_off1,
                                       int64_t P, double* out, void* workspace,
                                       int64_t workspace_bytes, int stages, tvq_stream_t stream) {
  TVQ_CHECK_ARG(P >= 0 && P <= FR_MAX_PAIRS, "tvq_traj_frechet: bad pair count (at most %lld a call)",
                (long long)FR_MAX_PAIRS);
  TVQ_CHECK_ARG(stages >= 1 && stages <= 7, "tvq_traj_frechet: stages is a mask of 1, 2 and 4");
  if (P == 0) return TVQ_OK;
  TVQ_CHECK_ARG(pts0 && off0 && pts1 && off1 && host_off0 && host_off1 && out && workspace,
                "tvq_traj_frechet: bad arguments");
  const int64_t max_len = tvq_traj_max_len();
  int64_t total, cap_max, cells_max;
  if (!fr_sizes("tvq_traj_frechet", host_off0, host_off1, P, max_len, &total, &cap_max, &cells_max))
    return TVQ_ERR_ARG;
  const int64_t need = fr_head_bytes(P) + 2 * total * (int64_t)sizeof(u64);
  TVQ_CHECK_ARG(workspace_bytes >= need && ((uintptr_t)workspace & 7) == 0,
                "tvq_traj_frechet: the workspace has %lld bytes (8-aligned), %lld are needed",
                (long long)workspace_bytes, (long long)need);
  hipStream_t st = (hipStream_t)stream;
  int64_t* voff = (int64_t*)workspace;
  int64_t* ucnt = voff + P + 1;
  u64* a = (u64*)((char*)workspace + fr_head_bytes(P));
  u64* b = a + total;
  const auto blocks = [](int64_t n) {
    const int64_t g = (n + FR_T - 1) / FR_T;
    return (unsigned)(g < 1 ? 1 : g > 4096 ? 4096 : g);
  };
  hipLaunchKernelGGL(fr_layout_kernel, dim3(1), dim3(FR_T), 0, st, off0, off1, P, total, voff);
  if (stages & 1) {
    const int64_t fill = cells_max > FR_TILE ? cells_max : FR_TILE;
    hipLaunchKernelGGL(fr_critical_kernel, dim3((unsigned)P, blocks(fill)), dim3(FR_T), 0, st, pts0,
                       off0, pts1, off1, max_len, voff, a);
  }
  if (stages & 2)
    hipLaunchKernelGGL(fr_tile_sort_kernel, dim3((unsigned)P, (unsigned)(cap_max / FR_TILE)),
                       dim3(FR_T), 0, st, voff, a);
  // the sorted list ends in the half the number of merge passes leaves it in
  for (int64_t run = FR_TILE; run < cap_max; run *= 2) {
    if (stages & 2)
      hipLaunchKernelGGL(fr_merge_kernel, dim3((unsigned)P, blocks(cap_max)), dim3(FR_T), 0, st,
                         voff, a, b, run);
    u64* s = a;
    a = b;
    b = s;
  }
  if (stages & 2)
    hipLaunchKernelGGL(fr_unique_kernel, dim3((unsigned)P), dim3(FR_T), 0, st, voff, a, b, ucnt);
  if (stages & 4)
    hipLaunchKernelGGL(fr_search_kernel, dim3((unsigned)P), dim3(FR_T), 0, st, pts0, off0, pts1,
                       off1, max_len, voff, b, ucnt, out);
  return launch_status("tvq_traj_frechet");
}

extern "C" int tvq_traj_frechet(const double* pts0, const int64_t* off0, const double* pts1,
                                const int64_t* off1, const int64_t* host_off0,
                                const int64_t* host_off1, int64_t P, double* out, void* workspace,
                                int64_t workspace_bytes, tvq_stream_t stream) {
  return tvq_traj_frechet_stages(pts0, off0, pts1, off1, host_off0, host_off1, P, out, workspace,
                                 workspace_bytes, 7, stream);
}
