// The transformer's row norms over the last dim, forward and backward:
//
//  rmsnorm     x-transformers RMSNorm: F.normalize(x) * sqrt(D) * g
//  layernorm   LayerNorm (gamma [+ beta]), eps given
//
// Four kernel templates, each taking the operator as a policy type (RmsNorm, LayerNorm):
//
//  norm_fwd_kernel<Op>           one wave per row, any D
//  norm_fwd_vec_kernel<Op, L>    D = 4L: one float4 per lane, 64 / L rows per wave
//  norm_bwd_loop_kernel<Op>      one wave per row, any D (the path for D > 256)
//  norm_bwd_kernel<Op, LR, ND>   the row in registers: LR lanes per row, ND elements per lane
//
// y = Op's normalised x * gain [+ shift], gain and shift per-column parameters (either may be
// null: RMSNorm has no shift).  A policy holds the operator's other arguments and supplies
//   Stat, NRED, NP       the per-row statistics, the number of row reductions of the backward
//                        and of parameter-gradient slabs
//   OPT_GAIN, SHIFT      whether the gain may be null (then 1); whether it takes a shift
//   HALF                 whether D <= 32 takes the backward's 32-lanes-per-row form
//   stats(row view, D)   forward: the statistics from the row's sum / sum of squares
//   y(x, gain, st), save(row, st)
//   stat(row)            backward: the saved statistics
//   terms, finish        a column's addends to the NRED row sums; the sums -> the row's scalars
//   dx, dparam           a column's input gradient (last argument: the loop form) and its NP
//                        parameter-gradient addends
//   res(offset)          the residual path's gradient (RMSNorm only; 0 otherwise)
#include <math.h>

#include "tvq_common.h"
#include "tvq_reduce.h"

namespace tvq {

struct RmsNorm {
  static constexpr int NRED = 1, NP = 1;
  static constexpr bool OPT_GAIN = false, SHIFT = false, HALF = true;
  static constexpr const char* NAME = "rmsnorm";
  struct Stat {
    float inv;
  };
  float scale;
  float* inv_norm;
  const float* dres;

  template <class Row>
  __device__ __forceinline__ Stat stats(const Row& r, int) const {
    return {1.0f / fmaxf(sqrtf(r.sumsq(0.f)), 1e-12f)};
  }
  __device__ __forceinline__ float y(float x, float gn, const Stat& st) const {
    return x * st.inv * scale * gn;
  }
  __device__ __forceinline__ void save(int64_t row, const Stat& st) const { inv_norm[row] = st.inv; }

  __device__ __forceinline__ Stat stat(int64_t row) const { return {inv_norm[row]}; }
  __device__ __forceinline__ float res(int64_t o) const { return dres ? dres[o] : 0.f; }
  // y = x * inv * scale * g ; norm = 1/inv (assumes ||x|| > 1e-12)
  __device__ __forceinline__ void terms(float x, float dy, float gn, const Stat&,
                                        float (&s)[NRED]) const {
    s[0] += dy * gn * x;
  }
  __device__ __forceinline__ void finish(float (&s)[NRED], const Stat& st, int) const {
    s[0] = s[0] * scale * st.inv * st.inv * st.inv;
  }
  __device__ __forceinline__ float dx(float x, float dy, float gn, float r, const Stat& st,
                                      const float (&s)[NRED], bool) const {
    const float v = dy * gn * scale * st.inv - x * s[0];
    return dres ? v + r : v;  // + the residual path's gradient
  }
  __device__ __forceinline__ void dparam(float x, float dy, const Stat& st, float (&p)[NP]) const {
    p[0] = dy * x * st.inv * scale;
  }
};

struct LayerNorm {
  static constexpr int NRED = 2, NP = 2;  // slabs: dgamma, dbeta
  static constexpr bool OPT_GAIN = true, SHIFT = true, HALF = false;
  static constexpr const char* NAME = "layernorm";
  struct Stat {
    float mean, rstd;
  };
  float eps;
  float* mean;
  float* rstd;

  template <class Row>
  __device__ __forceinline__ Stat stats(const Row& r, int D) const {
    const float mu = r.sum() / (float)D;
    const float var = r.sumsq(mu) / (float)D;
    return {mu, 1.0f / sqrtf(var + eps)};
  }
  __device__ __forceinline__ float y(float x, float gn, const Stat& st) const {
    return (x - st.mean) * st.rstd * gn;
  }
  __device__ __forceinline__ void save(int64_t row, const Stat& st) const {
    mean[row] = st.mean;
    rstd[row] = st.rstd;
  }

  __device__ __forceinline__ Stat stat(int64_t row) const { return {mean[row], rstd[row]}; }
  __device__ __forceinline__ float res(int64_t) const { return 0.f; }
  __device__ __forceinline__ void terms(float x, float dy, float gn, const Stat& st,
                                        float (&s)[NRED]) const {
    const float xh = (x - st.mean) * st.rstd;
    const float gg = dy * gn;
    s[0] += gg;
    s[1] += gg * xh;
  }
  __device__ __forceinline__ void finish(float (&s)[NRED], const Stat&, int D) const {
    s[0] = s[0] / (float)D;
    s[1] = s[1] / (float)D;
  }
  // loop: the one-wave-per-row form rounds dy * gain - s[0] once (it has always compiled to
  // an fma there), the register form twice; each form keeps its results
  __device__ __forceinline__ float dx(float x, float dy, float gn, float, const Stat& st,
                                      const float (&s)[NRED], bool loop) const {
    const float xh = (x - st.mean) * st.rstd;
    const float t = loop ? fmaf(dy, gn, -s[0]) : dy * gn - s[0];
    return st.rstd * (t - xh * s[1]);
  }
  __device__ __forceinline__ void dparam(float x, float dy, const Stat& st, float (&p)[NP]) const {
    p[0] = dy * ((x - st.mean) * st.rstd);
    p[1] = dy;
  }
};

// the row sum over its L lanes by xor shuffles; L = 64 is wave_sum's order
template <int L>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = L / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <class Op>
__device__ __forceinline__ float gain_at(const float* gain, int d) {
  return !Op::OPT_GAIN || gain ? gain[d] : 1.f;
}

// ------------------------------------------------------------------ forward
// A lane's view of its row for the statistics: sum() and sumsq(c) = sum (x - c)^2.
struct LoopRow {  // lanes stride the row
  const float* xr;
  int D, lane;
  __device__ __forceinline__ float sum() const {
    float s = 0.f;
    for (int d = lane; d < D; d += 64) s += xr[d];
    return wave_sum(s);
  }
  __device__ __forceinline__ float sumsq(float c) const {
    float v = 0.f;
    for (int d = lane; d < D; d += 64) {
      const float t = xr[d] - c;
      v += t * t;
    }
    return wave_sum(v);
  }
};

template <int L>
struct VecRow {  // one float4 of a 4L-wide row
  float4 v;
  __device__ __forceinline__ float sum() const { return group_sum<L>((v.x + v.y) + (v.z + v.w)); }
  __device__ __forceinline__ float sumsq(float c) const {
    const float t0 = v.x - c, t1 = v.y - c, t2 = v.z - c, t3 = v.w - c;
    float q = t0 * t0;
    q = fmaf(t1, t1, q);
    q = fmaf(t2, t2, q);
    q = fmaf(t3, t3, q);
    return group_sum<L>(q);
  }
};

// one wave per row
template <class Op>
__global__ void norm_fwd_kernel(const float* __restrict__ x, int64_t M, int D,
                                const float* __restrict__ gain, const float* __restrict__ shift,
                                Op op, float* __restrict__ y) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= M) return;
  const float* xr = x + row * D;
  const typename Op::Stat st = op.stats(LoopRow{xr, D, lane}, D);
  for (int d = lane; d < D; d += 64) {
    float t = op.y(xr[d], gain_at<Op>(gain, d), st);
    if (Op::SHIFT && shift) t += shift[d];
    y[row * D + d] = t;
  }
  if (lane == 0) op.save(row, st);
}

// Narrow rows (D = 4L, L in {8, 16, 32, 64} lanes): one float4 per lane, 64 / L rows per
// wave, the row sum over its L lanes by xor shuffles.  The one-wave-per-row form above
// left half to 7/8 of the lanes idle on the HF prior's D = 32 rows and issued one 4-B load
// per element (42 us for 1024 x 97 rows while sampling, ~0.3 TB/s).
template <class Op, int L>
__global__ __launch_bounds__(256) void norm_fwd_vec_kernel(const float4* __restrict__ x, int64_t M,
                                                           const float* __restrict__ gain,
                                                           const float* __restrict__ shift, Op op,
                                                           float4* __restrict__ y) {
  const int lane = threadIdx.x & 63, sub = lane % L;
  const int64_t row = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * (64 / L) + lane / L;
  const bool ok = row < M;
  const float4 v = ok ? x[row * L + sub] : make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 gn = !Op::OPT_GAIN || gain ? *reinterpret_cast<const float4*>(gain + 4 * sub)
                                         : make_float4(1.f, 1.f, 1.f, 1.f);
  const typename Op::Stat st = op.stats(VecRow<L>{v}, 4 * L);
  if (!ok) return;
  float4 o = make_float4(op.y(v.x, gn.x, st), op.y(v.y, gn.y, st), op.y(v.z, gn.z, st),
                         op.y(v.w, gn.w, st));
  if (Op::SHIFT && shift) {
    const float4 sh = *reinterpret_cast<const float4*>(shift + 4 * sub);
    o.x += sh.x; o.y += sh.y; o.z += sh.z; o.w += sh.w;
  }
  y[row * L + sub] = o;
  if (sub == 0) op.save(row, st);
}

// ----------------------------------------------------------------- backward
// dx, and per-block partial parameter gradients: part[k][block][D], k < Op::NP, each the
// block's rows summed per slot in row order, then the slots in index order (deterministic;
// the blocks are reduced by reduce_rows / param_rows_finish)
template <class Op>
__device__ __forceinline__ void norm_bwd_zero(float* sh, int nslot, int D) {
  for (int i = threadIdx.x; i < nslot * Op::NP * D; i += blockDim.x) sh[i] = 0.f;
}

template <class Op>
__device__ __forceinline__ void norm_bwd_slabs(const float* sh, int nslot, int D,
                                               float* __restrict__ part) {
  for (int i = threadIdx.x; i < Op::NP * D; i += blockDim.x) {
    const int k = Op::NP == 1 ? 0 : i / D, d = i - k * D;
    float s = 0.f;
    for (int w = 0; w < nslot; ++w) s += sh[(w * Op::NP + k) * D + d];
    part[((int64_t)k * gridDim.x + blockIdx.x) * D + d] = s;
  }
}

// one wave per row
template <class Op>
__global__ void norm_bwd_loop_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                     int64_t M, int D, const float* __restrict__ gain, Op op,
                                     float* __restrict__ dx, float* __restrict__ part,
                                     int rows_per_block) {
  extern __shared__ float sh[];  // [waves][NP][D] parameter-gradient partials
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  norm_bwd_zero<Op>(sh, nw, D);
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  for (int64_t row = r0 + wid; row < min(M, r0 + rows_per_block); row += nw) {
    const float* xr = x + row * D;
    const float* gr = dy + row * D;
    const typename Op::Stat st = op.stat(row);
    float s[Op::NRED] = {};
    for (int d = lane; d < D; d += 64) op.terms(xr[d], gr[d], gain_at<Op>(gain, d), st, s);
#pragma unroll
    for (int k = 0; k < Op::NRED; ++k) s[k] = wave_sum(s[k]);
    op.finish(s, st, D);
    for (int d = lane; d < D; d += 64) {
      dx[row * D + d] =
          op.dx(xr[d], gr[d], gain_at<Op>(gain, d), op.res(row * D + d), st, s, true);
      float p[Op::NP];
      op.dparam(xr[d], gr[d], st, p);
#pragma unroll
      for (int k = 0; k < Op::NP; ++k) sh[(wid * Op::NP + k) * D + d] += p[k];
    }
  }
  __syncthreads();
  norm_bwd_slabs<Op>(sh, nw, D, part);
}

// The same backward with each row held in registers (D <= LR ND): LR lanes take a row, a
// lane owning d = lane % LR + LR j, so a wave runs 64 / LR rows at a time (LR = 32 for the
// HF prior's D <= 32: the one-row form left half of every wave idle), and a slot -- a
// wave's group of LR lanes -- loads its next row while it reduces and stores the current
// one (the loop above pays two dependent load round trips per row).  Every sum has the
// loop above's order: the parameter gradients are bitwise equal, and dx but for
// LayerNorm::dx's one rounding.
template <class Op, int LR, int ND>
__global__ __launch_bounds__(256) void norm_bwd_kernel(const float* __restrict__ dy,
                                                       const float* __restrict__ x, int64_t M,
                                                       int D, const float* __restrict__ gain,
                                                       Op op, float* __restrict__ dx,
                                                       float* __restrict__ part,
                                                       int rows_per_block) {
  extern __shared__ float sh[];  // [slots][NP][D] parameter-gradient partials
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int sub = lane % LR, grp = lane / LR;
  const int slot = (64 / LR) * wid + grp, nslot = (64 / LR) * (blockDim.x >> 6);
  norm_bwd_zero<Op>(sh, nslot, D);
  float gn[ND];
#pragma unroll
  for (int j = 0; j < ND; ++j) {
    const int d = sub + LR * j;
    gn[j] = d < D ? gain_at<Op>(gain, d) : 1.f;
  }
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = min(M, r0 + rows_per_block);
  struct Row {
    float x[ND], dy[ND], r[ND];
    typename Op::Stat st;
  } cur, nxt;
  auto load = [&](int64_t row, Row& v) {
    const int64_t rr = row < r1 ? row : r0;  // past the block's rows: a valid row, unused
#pragma unroll
    for (int j = 0; j < ND; ++j) {
      const int d = sub + LR * j;
      const int64_t o = rr * D + (d < D ? d : 0);
      v.x[j] = x[o];
      v.dy[j] = dy[o];
      v.r[j] = op.res(o);
    }
    v.st = op.stat(rr);
  };
  int64_t row = r0 + slot;
  if (row - grp < r1) load(row, cur);
  for (; row - grp < r1; row += nslot) {  // a wave's slots iterate together (wave-uniform trip)
    load(row + nslot, nxt);
    const bool live = row < r1;
    float s[Op::NRED] = {};
#pragma unroll
    for (int j = 0; j < ND; ++j)
      if (live && sub + LR * j < D) op.terms(cur.x[j], cur.dy[j], gn[j], cur.st, s);
#pragma unroll
    for (int k = 0; k < Op::NRED; ++k) s[k] = group_sum<LR>(s[k]);
    op.finish(s, cur.st, D);
#pragma unroll
    for (int j = 0; j < ND; ++j) {
      const int d = sub + LR * j;
      if (live && d < D) {
        dx[row * D + d] = op.dx(cur.x[j], cur.dy[j], gn[j], cur.r[j], cur.st, s, false);
        float p[Op::NP];
        op.dparam(cur.x[j], cur.dy[j], cur.st, p);
#pragma unroll
        for (int k = 0; k < Op::NP; ++k) sh[(slot * Op::NP + k) * D + d] += p[k];
      }
    }
    cur = nxt;
  }
  __syncthreads();
  norm_bwd_slabs<Op>(sh, nslot, D, part);
}

static bool a16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static int norm_rows_per_block(int64_t M) {
  // ~256 blocks of rows for the deterministic partial-sum backward
  int64_t r = (M + 255) / 256;
  return (int)(r < 4 ? 4 : r);
}

// the vec form for D in {32, 64, 128, 256} with 16-byte-aligned operands, else the loop form
template <class Op>
static void norm_fwd(const float* x, int64_t M, int64_t D, const float* gain, const float* shift,
                     const Op& op, float* y, hipStream_t st) {
  if ((D == 32 || D == 64 || D == 128 || D == 256) && a16(x) && a16(y) && a16(gain) &&
      a16(shift)) {
    const int L = (int)(D / 4), rows = 4 * (64 / L);
    const dim3 grid((unsigned)((M + rows - 1) / rows));
    TVQ_PLAN("%s_fwd_vec D%lld", Op::NAME, (long long)D);
#define NF_(LV)                                                                                 \
  hipLaunchKernelGGL((norm_fwd_vec_kernel<Op, LV>), grid, dim3(256), 0, st, (const float4*)x, M, \
                     gain, shift, op, (float4*)y)
    if (L == 8) NF_(8); else if (L == 16) NF_(16); else if (L == 32) NF_(32); else NF_(64);
#undef NF_
    return;
  }
  hipLaunchKernelGGL(norm_fwd_kernel<Op>, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, x, M,
                     (int)D, gain, shift, op, y);
}

// LR = 32 for D <= 32 where the operator has that arm (Op::HALF), ND = 1 / 2 / 4 for
// D <= 64 / 128 / 256, the loop form above; per-block slabs into the workspace
template <class Op>
static int norm_bwd(const float* dy, const float* x, int64_t M, int64_t D, const float* gain,
                    const Op& op, float* dx, float* workspace, hipStream_t st) {
  const int rpb = norm_rows_per_block(M);
  const int nb = (int)((M + rpb - 1) / rpb);
  const size_t lds = 4 * Op::NP * D * sizeof(float);  // 4 waves' slots
#define NB_(LR, ND)                                                                             \
  do {                                                                                          \
    TVQ_PLAN("%s_bwd LR%d ND%d", Op::NAME, LR, ND);                                             \
    hipLaunchKernelGGL((norm_bwd_kernel<Op, LR, ND>), dim3(nb), dim3(256), (64 / LR) * lds, st, \
                       dy, x, M, (int)D, gain, op, dx, workspace, rpb);                         \
  } while (0)
  if (Op::HALF && D <= 32) {
    if constexpr (Op::HALF) NB_(32, 1);  // instantiated only for an operator that takes it
  } else if (D <= 64) {
    NB_(64, 1);
  } else if (D <= 128) {
    NB_(64, 2);
  } else if (D <= 256) {
    NB_(64, 4);
  } else {
    TVQ_PLAN("%s_bwd loop", Op::NAME);
    hipLaunchKernelGGL(norm_bwd_loop_kernel<Op>, dim3(nb), dim3(256), lds, st, dy, x, M, (int)D, gain,
                       op, dx, workspace, rpb);
  }
#undef NB_
  return nb;
}

}  // namespace tvq

using namespace tvq;

extern "C" int tvq_rmsnorm_fwd(const float* x, int64_t M, int64_t D, const float* g, float scale,
                               float* y, float* inv_norm, tvq_stream_t stream) {
  TVQ_CHECK_ARG(x && g && y && inv_norm && M > 0 && D > 0, "tvq_rmsnorm_fwd: bad arguments");
  norm_fwd(x, M, D, g, nullptr, RmsNorm{scale, inv_norm, nullptr}, y, (hipStream_t)stream);
  return launch_status("tvq_rmsnorm_fwd");
}

extern "C" int64_t tvq_norm_bwd_workspace(int64_t M, int64_t D) {
  const int rpb = norm_rows_per_block(M);
  const int64_t nb = (M + rpb - 1) / rpb;
  return nb * 2 * D + 2 * reduce_rows_scratch(nb, D);
}

extern "C" int tvq_rmsnorm_bwd(const float* dy, const float* x, int64_t M, int64_t D,
                               const float* g, float scale, const float* inv_norm,
                               const float* dres, float* dx, float* dg, int64_t accumulate,
                               float* workspace, tvq_stream_t stream) {
  TVQ_CHECK_ARG(dy && x && g && inv_norm && dx && dg && workspace, "tvq_rmsnorm_bwd: bad args");
  hipStream_t st = (hipStream_t)stream;
  // the backward only reads the statistics
  const RmsNorm op{scale, const_cast<float*>(inv_norm), dres};
  const int nb = norm_bwd(dy, x, M, D, g, op, dx, workspace, st);
  // the gain gradient: into the flat gradient (accumulate) it joins an open deferral scope
  if (accumulate)
    param_rows_finish(workspace, nb, D, dg, 1, workspace + (int64_t)nb * 2 * D, st);
  else
    reduce_rows(workspace, nb, D, D, dg, nullptr, 0, 0, workspace + (int64_t)nb * 2 * D, st);
  return launch_status("tvq_rmsnorm_bwd");
}

extern "C" int tvq_layernorm_fwd(const float* x, int64_t M, int64_t D, const float* gamma,
                                 const float* beta, float eps, float* y, float* mean, float* rstd,
                                 tvq_stream_t stream) {
  TVQ_CHECK_ARG(x && y && mean && rstd && M > 0 && D > 0, "tvq_layernorm_fwd: bad arguments");
  norm_fwd(x, M, D, gamma, beta, LayerNorm{eps, mean, rstd}, y, (hipStream_t)stream);
  return launch_status("tvq_layernorm_fwd");
}

extern "C" int tvq_layernorm_bwd(const float* dy, const float* x, int64_t M, int64_t D,
                                 const float* gamma, const float* mean, const float* rstd,
                                 float* dx, float* dgamma, float* dbeta, int64_t accumulate,
                                 float* workspace, tvq_stream_t stream) {
  TVQ_CHECK_ARG(dy && x && mean && rstd && dx && workspace, "tvq_layernorm_bwd: bad args");
  hipStream_t st = (hipStream_t)stream;
  // the backward only reads the statistics
  const LayerNorm op{0.f, const_cast<float*>(mean), const_cast<float*>(rstd)};
  const int nb = norm_bwd(dy, x, M, D, gamma, op, dx, workspace, st);
  // workspace [gamma | beta][nb][D]: two slabs of contiguous rows; into the flat gradient
  // (accumulate) they join an open deferral scope
  float* rs = workspace + (int64_t)nb * 2 * D;
  float* rs2 = rs + reduce_rows_scratch(nb, D);
  if (accumulate) {
    if (dgamma) param_rows_finish(workspace, nb, D, dgamma, 1, rs, st);
    if (dbeta) param_rows_finish(workspace + (int64_t)nb * D, nb, D, dbeta, 1, rs2, st);
  } else {
    if (dgamma) reduce_rows(workspace, nb, D, D, dgamma, nullptr, 0, 0, rs, st);
    if (dbeta) reduce_rows(workspace + (int64_t)nb * D, nb, D, D, dbeta, nullptr, 0, 0, rs2, st);
  }
  return launch_status("tvq_layernorm_bwd");
}
