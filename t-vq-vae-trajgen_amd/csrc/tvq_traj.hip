// Trajectory distances of the flyability evaluation for gfx950: the device halves of
// timevqvae/evaluation/flyability_utils/trajectory_distances (SSPD, DTW, Hausdorff, LCSS, ERP
// and EDR in Euclidean and spherical geometry, and the discrete Frechet distance).
//
// Reference: every distance is a pure-Python double loop over an n0 x n1 table, the spherical
// ones with a math.sin / cos / atan2 chain per cell.  Here a ragged batch of P pairs (points
// packed as (sum n, 2) float64, int64 offsets) is scored in float64 by two kernels:
//
//   traj_table_kernel    DTW e/s, ERP e/s, EDR e/s, LCSS e/s, discrete Frechet: nine recurrences
//                        over the same (n0 + 1) x (n1 + 1) table.  One wave per (pair, geometry)
//                        (grid P x 2) sweeps the table by anti-diagonals in bands of 64 rows: a
//                        lane owns a row, step s puts lane l on column s - l.  Of the three
//                        diagonals a cell reads, the lane's own last value (left) and the value
//                        its upper neighbour held two steps ago (diagonal) are in registers, the
//                        neighbour's last value (up) comes by a lane shift.  LDS holds what
//                        crosses bands and columns: the last row of the band above, the gap
//                        distances and cos(rad lat) of t1.  The cost of a cell is computed once
//                        and feeds every recurrence of its geometry; neither the table nor the
//                        pairwise distances reach global memory.
//   traj_segment_kernel  SSPD e/s and Hausdorff e/s: one block per pair, a thread per point, the
//                        other trajectory's segments staged through LDS in tiles (end points,
//                        cos / sin of the latitudes, segment lengths and bearings computed once
//                        per tile).  The per-point minima are added per thread in point order
//                        and then by a fixed tree.
//
// No atomics: a pair's row is a function of that pair alone and is bitwise the same in any
// batch.  Every comparison keeps the reference's form (a NaN along-track distance takes the
// cross-track branch); this file must not be built with fast-math.
#include "tvq_eval.h"

namespace tvq {
namespace {

constexpr int TJ_W = 64;          // table family: threads per block = rows per band
constexpr int TJ_ST = 256;        // segment family: threads per block
constexpr int TJ_TILE = 256;      // segment family: segments staged per tile
// LDS of a table wave: 4 doubles + one uint32 per column of t1 = 36 B; 4096 columns take
// 144 KiB of the CU's 160 KiB.
constexpr int64_t TJ_MAX_LEN = 4096;
constexpr int TJ_COL_BYTES = 4 * (int)sizeof(double) + (int)sizeof(uint32_t);
constexpr double TJ_R = 6378137.0;
constexpr double TJ_RAD = 3.14159265358979323846 / 180.0;
constexpr int TJ_COLS = 13;

// great_circle_distance(lon1, lat1, lon2, lat2) with c1 = cos(rad lat1), c2 = cos(rad lat2)
__device__ __forceinline__ double tj_hav(double lon1, double lat1, double c1, double lon2,
                                         double lat2, double c2) {
#pragma clang fp contract(off)
  const double dlat = TJ_RAD * (lat2 - lat1);
  const double dlon = TJ_RAD * (lon2 - lon1);
  const double sa = sin(dlat / 2.0), so = sin(dlon / 2.0);
  const double a = sa * sa + c1 * c2 * so * so;
  const double c = 2.0 * atan2(sqrt(a), sqrt(1.0 - a));
  return TJ_R * c;
}

__device__ __forceinline__ double tj_min3(double a, double b, double c) {
  return fmin(fmin(a, b), c);
}
__device__ __forceinline__ int tj_imin3(int a, int b, int c) {
  const int m = a < b ? a : b;
  return m < c ? m : c;
}

// ---- the table family --------------------------------------------------------------------
// Real-valued recurrences of a geometry: d[0] DTW, d[1] ERP, d[2] discrete Frechet (Euclidean
// only); counts c[0] EDR, c[1] LCSS.  lds: gap1[n1] | bnd[0][n1] | bnd[1][n1] |
// (SPH ? cos1 : bnd[2])[n1] | packed counts uint32[n1].
template <bool SPH>
__device__ void tj_table_sweep(const double* __restrict__ t0, int n0,
                               const double* __restrict__ t1, int n1, double g0, double g1,
                               double eps_edr, double eps_lcss, double* __restrict__ orow,
                               double* lds) {
#pragma clang fp contract(off)
  constexpr int ND = SPH ? 2 : 3;
  const int lane = threadIdx.x;
  double* gap1 = lds;
  double* bnd = lds + n1;
  double* cos1 = lds + 3 * (size_t)n1;
  uint32_t* bcnt = reinterpret_cast<uint32_t*>(lds + 4 * (size_t)n1);
  const double cg = SPH ? cos(TJ_RAD * g1) : 0.0;

  // gap distances of t1 (and cos(rad lat)) once per pair; both totals in a fixed order
  double s1 = 0.0, s0 = 0.0;
  for (int j = lane; j < n1; j += TJ_W) {
    const double x = t1[2 * j], y = t1[2 * j + 1];
    double gp;
    if (SPH) {
      const double c = cos(TJ_RAD * y);
      cos1[j] = c;
      gp = tj_hav(g0, g1, cg, x, y, c);
    } else {
      gp = dist2d(g0, g1, x, y);
    }
    gap1[j] = gp;
    s1 += gp;
  }
  for (int i = lane; i < n0; i += TJ_W) {
    const double x = t0[2 * i], y = t0[2 * i + 1];
    s0 += SPH ? tj_hav(g0, g1, cg, x, y, cos(TJ_RAD * y)) : dist2d(g0, g1, x, y);
  }
  const double total1 = wave_sum_d(s1), total0 = wave_sum_d(s0);
  __syncthreads();

  // border values C[i >= 1][0] and C[0][j >= 1] of the real-valued recurrences
  double col0[ND], row0[ND];
  col0[0] = row0[0] = INFINITY;
  col0[1] = total0;
  row0[1] = total1;
  if constexpr (!SPH) col0[ND - 1] = row0[ND - 1] = INFINITY;

  const int nb = (n0 + TJ_W - 1) / TJ_W;
  for (int b = 0; b < nb; ++b) {
    const int i = b * TJ_W + lane + 1;  // this lane's row, 1-based
    const bool rowok = i <= n0;
    const int ic = (rowok ? i : n0) - 1;
    const double x0 = t0[2 * ic], y0 = t0[2 * ic + 1];
    const double c0 = SPH ? cos(TJ_RAD * y0) : 0.0;
    const double gp0 = SPH ? tj_hav(x0, y0, c0, g0, g1, cg) : dist2d(g0, g1, x0, y0);
    const int rows = n0 - b * TJ_W < TJ_W ? n0 - b * TJ_W : TJ_W;
    const bool feeds = b + 1 < nb && lane == TJ_W - 1;  // the band below reads this row

    double cur_d[ND], up_d[ND];
    int cur_c[2] = {0, 0}, up_c[2] = {0, 0};
#pragma unroll
    for (int k = 0; k < ND; ++k) cur_d[k] = up_d[k] = 0.0;

    for (int s = 0; s < n1 + rows - 1; ++s) {
      const int j = s - lane + 1;  // this lane's column, 1-based
      const bool colok = j >= 1 && j <= n1;
      // C[i - 1][j]: what the lane above computed in the previous step
      double nu_d[ND];
      int nu_c[2];
#pragma unroll
      for (int k = 0; k < ND; ++k) nu_d[k] = __shfl_up(cur_d[k], 1, TJ_W);
      nu_c[0] = __shfl_up(cur_c[0], 1, TJ_W);
      nu_c[1] = __shfl_up(cur_c[1], 1, TJ_W);
      if (lane == 0) {
        if (b == 0) {
#pragma unroll
          for (int k = 0; k < ND; ++k) nu_d[k] = row0[k];
          nu_c[0] = nu_c[1] = 0;
        } else if (colok) {
#pragma unroll
          for (int k = 0; k < ND; ++k) nu_d[k] = bnd[(size_t)k * n1 + (j - 1)];
          const uint32_t pk = bcnt[j - 1];
          nu_c[0] = (int)(pk & 0xffffu);
          nu_c[1] = (int)(pk >> 16);
        }
      }
      if (rowok && colok) {
        double dg_d[ND], lf_d[ND];
        int dg_c[2], lf_c[2];
        if (j == 1) {
#pragma unroll
          for (int k = 0; k < ND; ++k) {
            dg_d[k] = i == 1 ? 0.0 : col0[k];
            lf_d[k] = col0[k];
          }
          dg_c[0] = dg_c[1] = lf_c[0] = lf_c[1] = 0;
        } else {
#pragma unroll
          for (int k = 0; k < ND; ++k) {
            dg_d[k] = up_d[k];
            lf_d[k] = cur_d[k];
          }
          dg_c[0] = up_c[0];
          dg_c[1] = up_c[1];
          lf_c[0] = cur_c[0];
          lf_c[1] = cur_c[1];
        }
        const double x1 = t1[2 * (j - 1)], y1 = t1[2 * (j - 1) + 1];
        const double cost = SPH ? tj_hav(x0, y0, c0, x1, y1, cos1[j - 1]) : dist2d(x0, y0, x1, y1);
        cur_d[0] = cost + tj_min3(lf_d[0], dg_d[0], nu_d[0]);
        cur_d[1] = tj_min3(nu_d[1] + gp0, lf_d[1] + gap1[j - 1], dg_d[1] + cost);
        if constexpr (!SPH)
          cur_d[ND - 1] = fmax(cost, tj_min3(lf_d[ND - 1], dg_d[ND - 1], nu_d[ND - 1]));
        cur_c[0] = tj_imin3(lf_c[0] + 1, nu_c[0] + 1, dg_c[0] + (cost < eps_edr ? 0 : 1));
        cur_c[1] = cost < eps_lcss ? dg_c[1] + 1 : (lf_c[1] > nu_c[1] ? lf_c[1] : nu_c[1]);
        if (feeds) {
#pragma unroll
          for (int k = 0; k < ND; ++k) bnd[(size_t)k * n1 + (j - 1)] = cur_d[k];
          bcnt[j - 1] = (uint32_t)cur_c[0] | ((uint32_t)cur_c[1] << 16);
        }
        if (i == n0 && j == n1) {
          const double nmax = (double)(n0 > n1 ? n0 : n1), nmin = (double)(n0 < n1 ? n0 : n1);
          const int o = SPH ? 1 : 0;
          orow[2 + o] = cur_d[0];
          orow[8 + o] = cur_d[1];
          orow[10 + o] = (double)cur_c[0] / nmax;
          orow[6 + o] = 1.0 - (double)cur_c[1] / nmin;
          if constexpr (!SPH) orow[12] = cur_d[ND - 1];
        }
      }
#pragma unroll
      for (int k = 0; k < ND; ++k) up_d[k] = nu_d[k];
      up_c[0] = nu_c[0];
      up_c[1] = nu_c[1];
    }
    __syncthreads();  // the row this band left is complete before the next band reads it
  }
}

__global__ __launch_bounds__(TJ_W) void traj_table_kernel(
    const double* __restrict__ pts0, const int64_t* __restrict__ off0,
    const double* __restrict__ pts1, const int64_t* __restrict__ off1, double g0, double g1,
    double eps, double eps_lcss_s, double eps_edr_s, int cap, double* __restrict__ out) {
  extern __shared__ double tj_lds[];
  const int64_t p = blockIdx.x;
  const int64_t a0 = off0[p], a1 = off1[p];
  const int64_t n0 = off0[p + 1] - a0, n1 = off1[p + 1] - a1;
  if (n0 < 1 || n1 < 1 || n1 > cap || n0 > TJ_MAX_LEN) return;  // the host refused these already
  double* orow = out + p * TJ_COLS;
  if (blockIdx.y == 0)
    tj_table_sweep<false>(pts0 + 2 * a0, (int)n0, pts1 + 2 * a1, (int)n1, g0, g1, eps, eps, orow,
                          tj_lds);
  else
    tj_table_sweep<true>(pts0 + 2 * a0, (int)n0, pts1 + 2 * a1, (int)n1, g0, g1, eps_edr_s,
                         eps_lcss_s, orow, tj_lds);
}

// ---- the segment family ------------------------------------------------------------------
// basic_spherical.point_to_path; th12 the segment's initial bearing, (c1, s1) = cos / sin of
// rad lat1, (c3, s3) of rad lat3
__device__ __forceinline__ double tj_point_to_path(double lon1, double c1, double s1, double th12,
                                                   double d12, double lon3, double c3, double s3,
                                                   double d13, double d23) {
#pragma clang fp contract(off)
  const double dlon = TJ_RAD * (lon3 - lon1);
  const double y = sin(dlon) * c3;
  const double x = c1 * s3 - s1 * c3 * cos(dlon);
  const double th13 = atan2(y, x);
  const double crt = asin(sin(d13 / TJ_R) * sin(th13 - th12)) * TJ_R;
  const double cc = cos(crt / TJ_R);
  const double d1p = acos(cos(d13 / TJ_R) / cc) * TJ_R;
  const double d2p = acos(cos(d23 / TJ_R) / cc) * TJ_R;
  // a NaN d1p / d2p compares false and takes |crt|, as in the reference
  if ((d1p > d12) || (d2p > d12)) return fmin(d13, d23);
  return fabs(crt);
}

__global__ __launch_bounds__(TJ_ST) void traj_segment_kernel(
    const double* __restrict__ pts0, const int64_t* __restrict__ off0,
    const double* __restrict__ pts1, const int64_t* __restrict__ off1,
    double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double sx[TJ_TILE + 1], sy[TJ_TILE + 1], sc[TJ_TILE + 1], ss[TJ_TILE + 1];
  __shared__ double sds[TJ_TILE], sd12[TJ_TILE], sth[TJ_TILE];
  __shared__ double red[TJ_ST];
  const int64_t p = blockIdx.x;
  const int64_t a0 = off0[p], a1 = off1[p];
  const int64_t m0 = off0[p + 1] - a0, m1 = off1[p + 1] - a1;
  if (m0 < 2 || m1 < 2 || m0 > TJ_MAX_LEN || m1 > TJ_MAX_LEN) return;  // refused by the host
  const int tid = threadIdx.x;
  double mean_e[2], mean_s[2], max_e[2], max_s[2];

  // dir 0: the points of t0 against the segments of t1; dir 1: the other way round
  for (int dir = 0; dir < 2; ++dir) {
    const double* __restrict__ A = dir == 0 ? pts0 + 2 * a0 : pts1 + 2 * a1;
    const double* __restrict__ B = dir == 0 ? pts1 + 2 * a1 : pts0 + 2 * a0;
    const int nA = (int)(dir == 0 ? m0 : m1), nB = (int)(dir == 0 ? m1 : m0);
    double sum_e = 0.0, sum_s = 0.0, top_e = 0.0, top_s = 0.0;
    for (int base = 0; base < nA; base += TJ_ST) {
      const int k = base + tid;
      const bool valid = k < nA;
      const int kc = valid ? k : nA - 1;
      const double px = A[2 * kc], py = A[2 * kc + 1];
      const double cp = cos(TJ_RAD * py), sp = sin(TJ_RAD * py);
      double me = INFINITY, ms = 9e100;
      for (int t0 = 0; t0 < nB - 1; t0 += TJ_TILE) {
        const int nseg = nB - 1 - t0 < TJ_TILE ? nB - 1 - t0 : TJ_TILE;
        __syncthreads();  // the previous tile is consumed
        for (int m = tid; m <= nseg; m += TJ_ST) {
          const double x = B[2 * (t0 + m)], y = B[2 * (t0 + m) + 1];
          sx[m] = x;
          sy[m] = y;
          sc[m] = cos(TJ_RAD * y);
          ss[m] = sin(TJ_RAD * y);
        }
        __syncthreads();
        for (int m = tid; m < nseg; m += TJ_ST) {
          sds[m] = dist2d(sx[m], sy[m], sx[m + 1], sy[m + 1]);
          sd12[m] = tj_hav(sx[m], sy[m], sc[m], sx[m + 1], sy[m + 1], sc[m + 1]);
          // initial_bearing(segment start -> segment end)
          const double dlon = TJ_RAD * (sx[m + 1] - sx[m]);
          const double y = sin(dlon) * sc[m + 1];
          const double x = sc[m] * ss[m + 1] - ss[m] * sc[m + 1] * cos(dlon);
          sth[m] = atan2(y, x);
        }
        __syncthreads();
        if (valid) {
          // the pairwise distances are those of (t0 point, t1 point) in both directions
          double dps1 = dir == 0 ? dist2d(px, py, sx[0], sy[0]) : dist2d(sx[0], sy[0], px, py);
          double d13 = dir == 0 ? tj_hav(px, py, cp, sx[0], sy[0], sc[0])
                                : tj_hav(sx[0], sy[0], sc[0], px, py, cp);
          for (int m = 0; m < nseg; ++m) {
            const double qx = sx[m + 1], qy = sy[m + 1], qc = sc[m + 1];
            const double dps2 = dir == 0 ? dist2d(px, py, qx, qy) : dist2d(qx, qy, px, py);
            const double d23 = dir == 0 ? tj_hav(px, py, cp, qx, qy, qc)
                                        : tj_hav(qx, qy, qc, px, py, cp);
            me = fmin(me, point_to_seg(px, py, sx[m], sy[m], qx, qy, dps1, dps2, sds[m]));
            ms = fmin(ms, tj_point_to_path(sx[m], sc[m], ss[m], sth[m], sd12[m], px, cp, sp, d13,
                                           d23));
            dps1 = dps2;
            d13 = d23;
          }
        }
      }
      if (valid) {
        sum_e += me;
        sum_s += ms;
        top_e = fmax(top_e, me);
        top_s = fmax(top_s, ms);
      }
    }
    mean_e[dir] = block_tree_sum_d<TJ_ST>(sum_e, red) / (double)nA;
    mean_s[dir] = block_tree_sum_d<TJ_ST>(sum_s, red) / (double)nA;
    max_e[dir] = block_tree_max_d<TJ_ST>(top_e, red);
    max_s[dir] = block_tree_max_d<TJ_ST>(top_s, red);
  }
  if (tid == 0) {
    double* orow = out + p * TJ_COLS;
    orow[0] = (mean_e[0] + mean_e[1]) / 2.0;
    orow[1] = mean_s[1] + mean_s[0];  // s_sspd does not halve
    orow[4] = fmax(max_e[0], max_e[1]);
    orow[5] = fmax(max_s[1], max_s[0]);
  }
}

}  // namespace
}  // namespace tvq

using namespace tvq;

extern "C" int64_t tvq_traj_max_len(void) { return TJ_MAX_LEN; }

extern "C" int tvq_traj_table_distances(const double* pts0, const int64_t* off0,
                                        const double* pts1, const int64_t* off1,
                                        const int64_t* host_off0, const int64_t* host_off1,
                                        int64_t P, double g0, double g1, double eps,
                                        double eps_lcss_spherical, double eps_edr_spherical,
                                        double* out, tvq_stream_t stream) {
  TVQ_CHECK_ARG(P >= 0 && P <= 0x7fffffffLL, "tvq_traj_table_distances: bad pair count");
  if (P == 0) return TVQ_OK;
  TVQ_CHECK_ARG(pts0 && off0 && pts1 && off1 && host_off0 && host_off1 && out,
                "tvq_traj_table_distances: bad arguments");
  int64_t max1 = 0;  // the longest t1 sizes the LDS
  if (!check_ragged_pairs("tvq_traj_table_distances", host_off0, host_off1, P, 1, TJ_MAX_LEN,
                          [&](int64_t, int64_t n1) { max1 = n1 > max1 ? n1 : max1; }))
    return TVQ_ERR_ARG;
  // above 64 KiB of dynamic LDS a kernel has to opt in (a gfx950 CU has 160 KiB)
  static bool attr = [] {
    (void)hipFuncSetAttribute((const void*)traj_table_kernel,
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(TJ_MAX_LEN * TJ_COL_BYTES));
    return true;
  }();
  (void)attr;
  const size_t lds = (size_t)max1 * TJ_COL_BYTES;
  hipLaunchKernelGGL(traj_table_kernel, dim3((unsigned)P, 2), dim3(TJ_W), lds, (hipStream_t)stream,
                     pts0, off0, pts1, off1, g0, g1, eps, eps_lcss_spherical, eps_edr_spherical,
                     (int)max1, out);
  return launch_status("tvq_traj_table_distances");
}

extern "C" int tvq_traj_segment_distances(const double* pts0, const int64_t* off0,
                                          const double* pts1, const int64_t* off1,
                                          const int64_t* host_off0, const int64_t* host_off1,
                                          int64_t P, double* out, tvq_stream_t stream) {
  TVQ_CHECK_ARG(P >= 0 && P <= 0x7fffffffLL, "tvq_traj_segment_distances: bad pair count");
  if (P == 0) return TVQ_OK;
  TVQ_CHECK_ARG(pts0 && off0 && pts1 && off1 && host_off0 && host_off1 && out,
                "tvq_traj_segment_distances: bad arguments");
  if (!check_ragged_pairs("tvq_traj_segment_distances", host_off0, host_off1, P, 2, TJ_MAX_LEN,
                          [](int64_t, int64_t) {}))
    return TVQ_ERR_ARG;
  hipLaunchKernelGGL(traj_segment_kernel, dim3((unsigned)P), dim3(TJ_ST), 0, (hipStream_t)stream,
                     pts0, off0, pts1, off1, out);
  return launch_status("tvq_traj_segment_distances");
}
