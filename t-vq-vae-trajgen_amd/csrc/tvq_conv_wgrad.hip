// Weight gradients of the conv engine: the tvq_conv2d_wgrad / tvq_convT2d_wgrad entry points,
// the one dispatcher that picks a kernel family for each (wgrad_ladder), the workspace size
// of either (conv_wgrad_ws), and conv_wgrad_kernel, the split GEMM that takes every shape.
// The family files are listed in tvq_conv_core.h.
#include "tvq_conv_core.h"
#include "tvq_reduce.h"

#include <algorithm>

namespace tvq {

// Weight gradient: rows = n (channels of G), cols = k' = (c, kh, kw), reduction over
// positions.  blockIdx.z = split index over positions; partial results go to
// slab[z][n][k'] and are summed in split order (conv_wgrad_finish).
template <int KH, int KW, int SW, bool REPL, int TN, int TK, int WN, int WK>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(const float* __restrict__ G,
                                                        const float* __restrict__ in,
                                                        float* __restrict__ slab, ConvGeom g,
                                                        int pos_per_split, int kcols) {
  // kcols = Kred (+1: a column of ones whose result is the bias gradient sum_m G[n, m])
  constexpr int BK = 16;  // positions per K-step
  constexpr int KK = KH * KW;
  constexpr int FN = TN / WN / 16;
  constexpr int FK = TK / WK / 16;
  constexpr int SA = ((TN + 31) / 32) * 32 + 16;
  constexpr int SB = ((TK + 31) / 32) * 32 + 16;
  constexpr int A_PER = TN * BK / 256;
  constexpr int B_PER = TK * BK / 256;
  static_assert(A_PER >= 1 && B_PER >= 1, "tile too small");
  __shared__ float As[BK * SA];
  __shared__ float Bs[BK * SB];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wn = wid % WN, wk = wid / WN;
  const int n0 = blockIdx.y * TN;
  const int kp0 = blockIdx.x * TK;
  const int p_begin = blockIdx.z * pos_per_split;
  const int p_end = min(g.Mpos, p_begin + pos_per_split);

  const int kk_t = tid % BK;  // each thread owns one position slot of the K-step
  const int a_nbase = tid / BK;
  const int b_kbase = tid / BK;
  // the thread's k' columns are fixed for the whole launch: decompose them once
  int bc_off[B_PER], bkh[B_PER], bkw[B_PER];
  unsigned bmask = 0u, bones = 0u;
#pragma unroll
  for (int j = 0; j < B_PER; ++j) {
    const int kp = kp0 + b_kbase + j * 16;
    const int c = kp / KK, r = kp - c * KK;
    bkh[j] = r / KW - g.oph;
    bkw[j] = r - (r / KW) * KW - g.opw;
    bc_off[j] = (kp < g.Kred) ? c * g.Hin * g.Win : 0;
    if (kp < g.Kred) bmask |= 1u << j;
    if (kp == g.Kred && kp < kcols) bones |= 1u << j;
  }

  float ra[A_PER], rb[B_PER];
  auto load_tile = [&](int p0) {
    const int p = p0 + kk_t;
    const bool pv = p < p_end;
    int b = 0, h = 0, w = 0;
    if (pv) {
      const uint32_t bh = fdiv((uint32_t)p, g.fd_wo);
      w = p - (int)bh * g.Wo;
      b = (int)fdiv((uint32_t)p, g.fd_hwo);
      h = (int)bh - b * g.Hout;
    }
    const float* gb = G + (((int64_t)b * g.N) * g.Hout + h) * g.Wo + w;
#pragma unroll
    for (int j = 0; j < A_PER; ++j) {
      const int n = n0 + a_nbase + j * 16;
      ra[j] = (pv && n < g.N) ? gb[(int64_t)n * g.Hout * g.Wo] : 0.f;
    }
    const float* inb = in + (int64_t)b * g.C * g.Hin * g.Win;
#pragma unroll
    for (int j = 0; j < B_PER; ++j) {
      float v = (pv && (bones >> j & 1u)) ? 1.0f : 0.f;
      if (pv && (bmask >> j & 1u)) {
        int hi = h + bkh[j], wi = w * SW + bkw[j];
        bool ok = true;
        if (REPL) {
          hi = hi < 0 ? 0 : (hi >= g.Hin ? g.Hin - 1 : hi);
          wi = wi < 0 ? 0 : (wi >= g.Win ? g.Win - 1 : wi);
        } else {
          ok = hi >= 0 && hi < g.Hin && wi >= 0 && wi < g.Win;
        }
        if (ok) v = inb[bc_off[j] + (int64_t)hi * g.Win + wi];
      }
      rb[j] = v;
    }
  };
  // rows of 16 positions, columns XOR-swizzled by (row & 14) as in gemm_kernel: the row
  // pitches are 16 mod 32 store banks, so unswizzled a half-wave's stores land on 16
  // banks (and with (row & 12) still 2-way).  Layout only (same k order, same results).
  auto store_tile = [&]() {
#pragma unroll
    for (int j = 0; j < A_PER; ++j) As[kk_t * SA + ((a_nbase + j * 16) ^ (kk_t & 14))] = ra[j];
#pragma unroll
    for (int j = 0; j < B_PER; ++j) Bs[kk_t * SB + ((b_kbase + j * 16) ^ (kk_t & 14))] = rb[j];
  };

  floatx4 acc[FN][FK];
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FK; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
  const int r16 = lane & 15, g4 = lane >> 4;
  if (p_begin < p_end) {
    load_tile(p_begin);
    for (int p0 = p_begin; p0 < p_end; p0 += BK) {
      __syncthreads();
      store_tile();
      __syncthreads();
      if (p0 + BK < p_end) load_tile(p0 + BK);
#pragma unroll
      for (int kk = 0; kk < BK; kk += 4) {
        float af[FN], bf[FK];
        const int swz = r16 ^ ((kk & 12) | (g4 & 2));  // sw(kk + g4)
#pragma unroll
        for (int i = 0; i < FN; ++i) af[i] = As[(kk + g4) * SA + (wn * FN + i) * 16 + swz];
#pragma unroll
        for (int j = 0; j < FK; ++j) bf[j] = Bs[(kk + g4) * SB + (wk * FK + j) * 16 + swz];
#pragma unroll
        for (int i = 0; i < FN; ++i)
#pragma unroll
          for (int j = 0; j < FK; ++j) acc[i][j] = mfma16x16x4(af[i], bf[j], acc[i][j]);
      }
    }
  }
  float* sl = slab + (int64_t)blockIdx.z * g.N * kcols;
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FK; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + (wn * FN + i) * 16 + 4 * g4 + r;
        const int kp = kp0 + (wk * FK + j) * 16 + r16;
        if (n < g.N && kp < kcols) sl[(int64_t)n * kcols + kp] = acc[i][j][r];
      }
}

template <int KH, int KW, int SW, bool REPL>
static void launch_wgrad(const float* G, const float* in, float* slab, int splits, int pps,
                         const ConvGeom& g, int kcols, hipStream_t st) {
  if (g.N <= 16) {
    dim3 grid((kcols + 63) / 64, (g.N + 15) / 16, splits);
    hipLaunchKernelGGL((conv_wgrad_kernel<KH, KW, SW, REPL, 16, 64, 1, 4>), grid, dim3(256), 0, st,
                       G, in, slab, g, pps, kcols);
  } else {
    dim3 grid((kcols + 63) / 64, (g.N + 63) / 64, splits);
    hipLaunchKernelGGL((conv_wgrad_kernel<KH, KW, SW, REPL, 64, 64, 2, 2>), grid, dim3(256), 0, st,
                       G, in, slab, g, pps, kcols);
  }
}

struct WSplitPlan {
  int S, pps;  // splits of the positions, positions per split
};
static WSplitPlan wsplit_plan(int64_t N, int64_t Kred, int64_t Mpos) {
  const int64_t kc = Kred + 1;
  const int tiles = (int)(((kc + 63) / 64) * ((N + (N <= 16 ? 15 : 63)) / (N <= 16 ? 16 : 64)));
  const int M = (int)Mpos;
  // aim for ~1024 blocks, each with >= 512 positions
  int splits = (1024 + tiles - 1) / tiles;
  const int maxs = (M + 511) / 512;
  if (splits > maxs) splits = maxs;
  if (splits < 1) splits = 1;
  if (splits > 256) splits = 256;
  int per = (M + splits - 1) / splits;
  per = (per + 15) / 16 * 16;
  return {(M + per - 1) / per, per};
}

static int launch_wgrad_split(const WgradArgs& a) {
  const ConvGeom g = make_geom(a.B, a.C, a.Hin, a.Win, a.N, a.Hout, a.Wo, a.KH, a.KW, PH_OF(a.KH),
                               PW_OF(a.KW), (int64_t)a.C * a.KH * a.KW, a.KH * a.KW);
  const WSplitPlan pl = wsplit_plan(a.N, g.Kred, g.Mpos);
  TVQ_PLAN("conv_wgrad split=%d", pl.S);
#define M_(kh, kw, sw, r) launch_wgrad<kh, kw, sw, r>(a.G, a.in, a.slab, pl.S, pl.pps, g, a.kcols, a.st);
  TVQ_DISPATCH_KIND(a.kind, a.repl, M_)
#undef M_
  return pl.S;
}

static int launch_wgrad_s2(const WgradArgs& a) {
  if (!ws2_fits(a.C, a.Hin, a.N, a.KH, a.KW, a.SW)) return 0;
  return ws2_launch(a.G, a.in, a.slab, a.B, a.C, a.N, a.Win, a.Wo, a.kcols, a.repl, a.st);
}

// The families in the order they are tried; the first whose shape it is launches, and its S
// slab rows are summed into dw (+ db).  `what`: the entry points' launch_status labels.
enum { WG_S2 = 1, WG_T32 = 2, WG_W8 = 4, WG_HALO = 8, WG_SPLIT = 16 };
static const struct {
  int bit;
  int (*launch)(const WgradArgs&);
  const char* what[2];  // [transposed]
} WG_LADDER[] = {
    {WG_S2, launch_wgrad_s2, {"tvq_conv2d_wgrad(s2)", "tvq_convT2d_wgrad(s2)"}},
    {WG_T32, launch_wgrad_t32, {"tvq_conv2d_wgrad(t32)", "tvq_convT2d_wgrad(t32)"}},
    {WG_W8, launch_wgrad_w8, {"tvq_conv2d_wgrad(w8)", "tvq_convT2d_wgrad(w8)"}},
    {WG_HALO, launch_wgrad_halo, {"tvq_conv2d_wgrad(halo)", "tvq_convT2d_wgrad(halo)"}},
    {WG_SPLIT, launch_wgrad_split, {"tvq_conv2d_wgrad", "tvq_convT2d_wgrad"}},
};

static int wgrad_ladder(const WgradArgs& a, int allow, bool transposed, float* dw, float* db,
                        int accumulate) {
  for (const auto& f : WG_LADDER) {
    const int S = (allow & f.bit) ? f.launch(a) : 0;
    if (S == 0) continue;
    conv_wgrad_finish(a.slab, S, a.N, a.kcols, dw, db, accumulate, a.st);
    return launch_status(f.what[transposed]);
  }
  set_error("conv weight gradient: no kernel family allowed");  // the split GEMM takes every shape
  return TVQ_ERR_ARG;
}

// Workspace floats of either entry point: S slab rows [N][C*KK + 1] and the split sum's
// scratch behind them, for the largest S among the families the query cannot rule out (it is
// given no stride, pad mode or input width).
int64_t conv_wgrad_ws(int64_t N, int64_t C, int64_t KH, int64_t KW, int64_t B, int64_t Hout,
                      int64_t Wo) {
  const int64_t KK = KH * KW;
  int S = wsplit_plan(N, C * KK, B * Hout * Wo).S;
  S = std::max(S, whalo_split(N, C, (int)KK, B).S);
  if (KH == 3 && KW == 3) S = std::max(S, w8_splits(B));
  if (wt32_fits(B, C, Hout, Wo, N, Wo, KH, KW, 1, 0))
    S = std::max(S, wt32_plan(B, C, Hout, Wo, N, KK).S);
  const int64_t ws = wgrad_slab_floats(S, N, C, KK) + reduce_rows_scratch(S, N * (C * KK + 1));
  // conv_wgrad_s2 (Wo: the width of G)
  const int64_t s2 = (KH == 3 && KW == 4 && C <= 16 && N <= 16) ? ws2_ws(B, C, Wo, N) : 0;
  return std::max(ws, s2);
}

}  // namespace tvq

using namespace tvq;

// Conv2d weight (+bias) gradient: dW[co,ci,kh,kw] (+)= sum dY[b,co,h,wo] X[b,ci,h+kh-PH, wo*SW+kw-PW],
// db[co] (+)= sum dY[b,co,h,wo] (db may be NULL)
extern "C" int tvq_conv2d_wgrad(const float* x, int64_t B, int64_t Ci, int64_t H, int64_t Wi,
                                const float* dy, int64_t Co, int64_t Wo, int64_t KH, int64_t KW,
                                int64_t SW, int64_t replicate, float* dw, float* db,
                                int64_t accumulate, float* workspace, tvq_stream_t stream) {
  TVQ_CHECK_ARG(x && dy && dw && workspace, "tvq_conv2d_wgrad: bad arguments");
  const int kind = kind_of((int)KH, (int)KW, (int)SW);
  TVQ_CHECK_ARG(kind >= 0, "tvq_conv2d_wgrad: unsupported kernel");
  const int kcols = (int)(Ci * KH * KW) + (db ? 1 : 0);
  const WgradArgs a = {dy, x, workspace, (int)B, (int)Ci, (int)H, (int)Wi, (int)Co, (int)H, (int)Wo,
                       (int)KH, (int)KW, (int)SW, kind, replicate != 0, kcols, (hipStream_t)stream};
  return wgrad_ladder(a, WG_S2 | WG_T32 | WG_W8 | WG_HALO | WG_SPLIT, false, dw, db,
                      (int)accumulate);
}

// ConvTranspose2d weight gradient: dW[ci,co,kh,kw] (+)= sum X[b,ci,h,wi] dY[b,co,h+kh-PH, wi*SW+kw-PW]
extern "C" int tvq_convT2d_wgrad(const float* x, int64_t B, int64_t Ci, int64_t H, int64_t Wi,
                                 const float* dy, int64_t Co, int64_t Wo, int64_t KH, int64_t KW,
                                 int64_t SW, float* dw, int64_t accumulate, float* workspace,
                                 tvq_stream_t stream) {
  TVQ_CHECK_ARG(x && dy && dw && workspace, "tvq_convT2d_wgrad: bad arguments");
  const int kind = kind_of((int)KH, (int)KW, (int)SW);
  TVQ_CHECK_ARG(kind >= 0, "tvq_convT2d_wgrad: unsupported kernel");
  // G = X (N = Ci channels at X's positions), In = dY gathered F-style (C = Co); no bias
  // column.  The transpose shapes keep to the stride-2, halo and split kernels.
  const WgradArgs a = {x, dy, workspace, (int)B, (int)Co, (int)H, (int)Wo, (int)Ci, (int)H, (int)Wi,
                       (int)KH, (int)KW, (int)SW, kind, false, (int)(Co * KH * KW),
                       (hipStream_t)stream};
  return wgrad_ladder(a, WG_S2 | WG_HALO | WG_SPLIT, true, dw, nullptr, (int)accumulate);
}
