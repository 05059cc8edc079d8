// The conv engine's staged 16x16x4 implicit GEMMs: conv_gemm_kernel (flat K order, small
// channel counts), conv_tap_kernel (tap-major, C % 16 == 0, split-K) and its separate
// split-K epilogue.
//
// GEMM orientation: MFMA rows = output channels n (A = weights), MFMA columns =
// output positions (B = gathered input), so each accumulator register holds 16
// consecutive positions of one channel and the NCHW stores are 64-B segments.
// Tiles are staged global -> registers -> LDS with the next K-step's loads in
// flight during the current step's MFMAs.
#include "tvq_conv_core.h"

namespace tvq {

template <int MODE, int KH, int KW, int SW, bool REPL, int TN, int TM, int WN, int WM>
__global__ __launch_bounds__(256) void conv_gemm_kernel(const float* __restrict__ in,
                                                       const float* __restrict__ wt,
                                                       float* __restrict__ out, ConvGeom g,
                                                       Epi e) {
  constexpr int BK = 16;
  constexpr int KK = KH * KW;
  constexpr int FN = TN / WN / 16;  // MFMA tiles per wave along channels
  constexpr int FM = TM / WM / 16;  // along positions
  constexpr int SA = ((TN + 31) / 32) * 32 + 16;
  constexpr int SB = ((TM + 31) / 32) * 32 + 16;
  constexpr int A_PER = TN * BK / 256;  // weight elements per thread per K-step
  constexpr int B_PER = TM * BK / 256;  // input elements per thread per K-step
  static_assert(A_PER >= 1 && B_PER >= 1, "tile too small");
  __shared__ float As[BK * SA];
  __shared__ float Bs[BK * SB];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wn = wid % WN, wm = wid / WN;
  const int n0 = blockIdx.y * TN;
  const int m0 = blockIdx.x * TM;

  // per-thread fixed position for the B (input) loads
  const int bm_local = tid % TM;
  const int bk_base = tid / TM;
  constexpr int BK_STEP = 256 / TM;
  const int mpos = m0 + bm_local;
  const bool mvalid = mpos < g.Mpos;
  int pb = 0, ph = 0, pw = 0;
  if (mvalid) {
    const uint32_t bh = fdiv((uint32_t)mpos, g.fd_wo);
    pw = mpos - (int)bh * g.Wo;
    pb = (int)fdiv((uint32_t)mpos, g.fd_hwo);
    ph = (int)bh - pb * g.Hout;
  }
  const float* inb = in + (int64_t)pb * g.C * g.Hin * g.Win;
  // per-thread fixed channel for the A (weight) loads
  const int an_local = tid % TN;
  const int ak_base = tid / TN;
  constexpr int AK_STEP = 256 / TN;
  const int an = n0 + an_local;

  float ra[A_PER], rb[B_PER];
  auto load_tile = [&](int k0) {
#pragma unroll
    for (int j = 0; j < A_PER; ++j) {
      const int k = k0 + ak_base + j * AK_STEP;
      float v = 0.f;
      if (an < g.N && k < g.Kred) {
        const int c = k / KK, r = k - c * KK;
        v = wt[an * g.wsn + c * g.wsc + r * g.wst];
      }
      ra[j] = v;
    }
#pragma unroll
    for (int j = 0; j < B_PER; ++j) {
      const int k = k0 + bk_base + j * BK_STEP;
      rb[j] = (mvalid && k < g.Kred) ? gather_in<MODE, KH, KW, SW, REPL>(in, g, inb, ph, pw, k) : 0.f;
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int j = 0; j < A_PER; ++j) As[(ak_base + j * AK_STEP) * SA + an_local] = ra[j];
#pragma unroll
    for (int j = 0; j < B_PER; ++j) Bs[(bk_base + j * BK_STEP) * SB + bm_local] = rb[j];
  };

  floatx4 acc[FN][FM];
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FM; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

  const int r16 = lane & 15, g4 = lane >> 4;
  load_tile(0);
  for (int k0 = 0; k0 < g.Kred; k0 += BK) {
    __syncthreads();
    store_tile();
    __syncthreads();
    if (k0 + BK < g.Kred) load_tile(k0 + BK);
#pragma unroll
    for (int kk = 0; kk < BK; kk += 4) {
      float af[FN], bf[FM];
#pragma unroll
      for (int i = 0; i < FN; ++i) af[i] = As[(kk + g4) * SA + (wn * FN + i) * 16 + r16];
#pragma unroll
      for (int j = 0; j < FM; ++j) bf[j] = Bs[(kk + g4) * SB + (wm * FM + j) * 16 + r16];
#pragma unroll
      for (int i = 0; i < FN; ++i)
#pragma unroll
        for (int j = 0; j < FM; ++j) acc[i][j] = mfma16x16x4(af[i], bf[j], acc[i][j]);
    }
  }

  const uint64_t seed = e.drop_p > 0.f ? mix_seed(e.seed_ptr, e.offset) : 0ull;
  // epilogue: acc[i][j][r] -> channel n0 + (wn*FN+i)*16 + 4*g4 + r, position m0 + (wm*FM+j)*16 + r16
  const int nbase = n0 + wn * FN * 16 + 4 * g4;
  float bv[FN][4];
  epi_load_bias<FN>(bv, e.bias, nbase, g.N);
  const int64_t hw = (int64_t)g.Hout * g.Wo;
#pragma unroll
  for (int j = 0; j < FM; ++j) {
    const int m = m0 + (wm * FM + j) * 16 + r16;
    const bool pv = m < g.Mpos;
    const int mc = pv ? m : 0;
    const uint32_t bh = fdiv((uint32_t)mc, g.fd_wo);
    const int w = mc - (int)bh * g.Wo;
    const int b = (int)fdiv((uint32_t)mc, g.fd_hwo);
    const int h = (int)bh - b * g.Hout;
    floatx4 a[FN];
#pragma unroll
    for (int i = 0; i < FN; ++i) a[i] = acc[i][j];
    epi_store<FN>(out, e, seed, bv, a, ((int64_t)b * g.N * g.Hout + h) * g.Wo + w, hw, nbase, g.N,
                  pv);
  }
}

// Tap-major variant for C % 16 == 0: the K loop runs over (tap, channel block), so a
// thread's spatial source (and its validity) is computed once per tap and every
// gathered element costs one multiply-add and one predicated load.
template <int MODE, int KH, int KW, int SW, bool REPL, int TN, int TM, int WN, int WM, int BK,
          bool POST = false>
__global__ __launch_bounds__(256) void conv_tap_kernel(const float* __restrict__ in,
                                                      const float* __restrict__ wt,
                                                      float* __restrict__ out, ConvGeom g, Epi e,
                                                      int steps_per_split, int64_t zstride,
                                                      int* __restrict__ cnt,
                                                      float* __restrict__ fout, Epi fe) {
  // split-K (gridDim.z > 1): block z covers K-steps [z*sps, (z+1)*sps) and stores raw
  // partial sums to out + z*zstride (the caller passes a slab and a raw Epi); with
  // `cnt` the last split block of the tile then sums the slabs in split order and
  // applies the real epilogue `fe` into `fout` (what conv_splitk_epi_kernel does)
  constexpr int KK = KH * KW;
  constexpr int FN = TN / WN / 16;
  constexpr int FM = TM / WM / 16;
  constexpr int SA = ((TN + 31) / 32) * 32 + 16;
  constexpr int SB = ((TM + 31) / 32) * 32 + 16;
  constexpr int A_PER = TN * BK / 256;
  constexpr int B_PER = TM * BK / 256;
  constexpr int BK_STEP = 256 / TM;
  constexpr int AK_STEP = 256 / TN;
  static_assert(A_PER >= 1 && B_PER >= 1 && BK_STEP >= 1 && AK_STEP >= 1, "tile");
  __shared__ float As[BK * SA];
  __shared__ float Bs[BK * SB];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wn = wid % WN, wm = wid / WN;
  const int n0 = blockIdx.y * TN;
  const int m0 = blockIdx.x * TM;
  const int bm_local = tid % TM, bk_base = tid / TM;
  const int mpos = m0 + bm_local;
  const bool mvalid = mpos < g.Mpos;
  int pb = 0, ph = 0, pw = 0;
  if (mvalid) {
    const uint32_t bh = fdiv((uint32_t)mpos, g.fd_wo);
    pw = mpos - (int)bh * g.Wo;
    pb = (int)fdiv((uint32_t)mpos, g.fd_hwo);
    ph = (int)bh - pb * g.Hout;
  }
  const int64_t plane = (int64_t)g.Hin * g.Win;
  const float* inb = in + (int64_t)pb * g.C * plane;
  float* const slab = out;
  const int an_local = tid % TN, ak_base = tid / TN;
  const int an = n0 + an_local;
  const float* wrow = wt + (int64_t)(an < g.N ? an : 0) * g.wsn;
  const int csteps = (g.C + BK - 1) / BK;
  const int kbeg = blockIdx.z * steps_per_split;
  const int nsteps = min(KK * csteps, kbeg + steps_per_split);
  out += (int64_t)blockIdx.z * zstride;

  float ra[A_PER], rb[B_PER];
  auto load_tile = [&](int step) {
    const int tap = step / csteps;
    const int c0 = (step - tap * csteps) * BK;
    const int kh = tap / KW, kw = tap - kh * KW;
    int hi, wi;
    bool ok = mvalid;
    if (MODE == GATHER_F) {
      hi = ph + kh - g.oph;
      wi = pw * SW + kw - g.opw;
      if (REPL) {
        hi = hi < 0 ? 0 : (hi >= g.Hin ? g.Hin - 1 : hi);
        wi = wi < 0 ? 0 : (wi >= g.Win ? g.Win - 1 : wi);
      } else {
        ok = ok && hi >= 0 && hi < g.Hin && wi >= 0 && wi < g.Win;
      }
    } else {
      hi = ph - kh + g.oph;
      const int wn_ = pw - kw + g.opw;
      ok = ok && hi >= 0 && hi < g.Hin && wn_ >= 0 && (SW == 1 || (wn_ & 1) == 0);
      wi = wn_ / SW;
      ok = ok && wi < g.Win;
    }
    const float* src = inb + (ok ? (int64_t)hi * g.Win + wi : 0);
#pragma unroll
    for (int j = 0; j < B_PER; ++j) {
      const int c = c0 + bk_base + j * BK_STEP;
      rb[j] = (ok && c < g.C) ? src[(int64_t)c * plane] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < A_PER; ++j) {
      const int c = c0 + ak_base + j * AK_STEP;
      ra[j] = (an < g.N && c < g.C) ? wrow[(int64_t)c * g.wsc + tap * g.wst] : 0.f;
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int j = 0; j < A_PER; ++j) As[(ak_base + j * AK_STEP) * SA + an_local] = ra[j];
#pragma unroll
    for (int j = 0; j < B_PER; ++j) Bs[(bk_base + j * BK_STEP) * SB + bm_local] = rb[j];
  };

  floatx4 acc[FN][FM];
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FM; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
  const int r16 = lane & 15, g4 = lane >> 4;
  if (kbeg < nsteps) load_tile(kbeg);
  for (int step = kbeg; step < nsteps; ++step) {
    __syncthreads();
    store_tile();
    __syncthreads();
    if (step + 1 < nsteps) load_tile(step + 1);
#pragma unroll
    for (int kk = 0; kk < BK; kk += 4) {
      float af[FN], bf[FM];
#pragma unroll
      for (int i = 0; i < FN; ++i) af[i] = As[(kk + g4) * SA + (wn * FN + i) * 16 + r16];
#pragma unroll
      for (int j = 0; j < FM; ++j) bf[j] = Bs[(kk + g4) * SB + (wm * FM + j) * 16 + r16];
#pragma unroll
      for (int i = 0; i < FN; ++i)
#pragma unroll
        for (int j = 0; j < FM; ++j) acc[i][j] = mfma16x16x4(af[i], bf[j], acc[i][j]);
    }
  }

  const uint64_t seed = e.drop_p > 0.f ? mix_seed(e.seed_ptr, e.offset) : 0ull;
  const int nbase = n0 + wn * FN * 16 + 4 * g4;
  float bv[FN][4];
  epi_load_bias<FN>(bv, e.bias, nbase, g.N);
  PostTile<FN> pt;
  if constexpr (POST) epi_load_post<FN>(pt, e, nbase, g.N);
  const int64_t hw = (int64_t)g.Hout * g.Wo;
#pragma unroll
  for (int j = 0; j < FM; ++j) {
    const int m = m0 + (wm * FM + j) * 16 + r16;
    const bool pv = m < g.Mpos;
    const int mc = pv ? m : 0;
    const uint32_t bh = fdiv((uint32_t)mc, g.fd_wo);
    const int w = mc - (int)bh * g.Wo;
    const int b = (int)fdiv((uint32_t)mc, g.fd_hwo);
    const int h = (int)bh - b * g.Hout;
    floatx4 a[FN];
#pragma unroll
    for (int i = 0; i < FN; ++i) a[i] = acc[i][j];
    epi_store<FN, POST>(out, e, seed, bv, a, ((int64_t)b * g.N * g.Hout + h) * g.Wo + w, hw, nbase,
                        g.N, pv, cnt != nullptr, &pt);
  }
  if (cnt && last_block(cnt + blockIdx.y * gridDim.x + blockIdx.x, (int)gridDim.z)) {
    const uint64_t fseed = fe.drop_p > 0.f ? mix_seed(fe.seed_ptr, fe.offset) : 0ull;
    for (int idx = tid; idx < TM * TN; idx += 256) {
      const int m = m0 + idx % TM, n = n0 + idx / TM;
      if (m >= g.Mpos || n >= g.N) continue;
      const uint32_t bh = fdiv((uint32_t)m, g.fd_wo);
      const int w = m - (int)bh * g.Wo;
      const int b = (int)fdiv((uint32_t)m, g.fd_hwo);
      const int h = (int)bh - b * g.Hout;
      const int64_t o = (((int64_t)b * g.N + n) * g.Hout + h) * g.Wo + w;
      float v = 0.f;
#pragma unroll 4
      for (int z = 0; z < (int)gridDim.z; ++z) v += ld_wt(slab + (int64_t)z * zstride + o);
      if (fe.bias) v += fe.bias[n];
      v = epi_post(fe, v, n);
      if (fe.drop_p > 0.f) v = uniform01(fseed, (uint64_t)o) >= fe.drop_p ? v * fe.drop_scale : 0.f;
      if (fe.residual) v += fe.residual[o];
      fout[o] = v;
    }
  }
}

// out[o] = epi(sum_z slab[z][o]) in split order; channel n = (o / HW) % N.  The dropout
// mask depends on (seed, offset, o) only, so it matches the unsplit epilogue exactly.
__global__ __launch_bounds__(256) void conv_splitk_epi_kernel(const float* __restrict__ slab,
                                                             int splits, int n_out, int N,
                                                             Div16 dhw, Epi e,
                                                             float* __restrict__ out) {
  const uint64_t seed = e.drop_p > 0.f ? mix_seed(e.seed_ptr, e.offset) : 0ull;
  // eval BN / Snake terms once per channel (N <= 256 here: tvq_conv2d_fwd_bn_eval's shapes)
  __shared__ PostCh pcs[256];
  const bool post = e.bn_rv != nullptr && N <= 256;
  if (post) {
    for (int n = threadIdx.x; n < N; n += 256) pcs[n] = epi_post_ch(e, n);
    __syncthreads();
  }
  for (int o = blockIdx.x * 256 + threadIdx.x; o < n_out; o += gridDim.x * 256) {
    float v = 0.f;
#pragma unroll 4
    for (int z = 0; z < splits; ++z) v += slab[(int64_t)z * n_out + o];
    const int n = div16(o, dhw) % N;
    if (e.bias) v += e.bias[n];
    if (post) v = epi_post_apply(pcs[n], v, e.gelu != 0);
    else v = epi_post(e, v, n);
    if (e.drop_p > 0.f) v = uniform01(seed, (uint64_t)o) >= e.drop_p ? v * e.drop_scale : 0.f;
    if (e.residual) v += e.residual[o];
    out[o] = v;
  }
}

static void tap_tile(int N, int* TN, int* TM) {
  if (N <= 16) { *TN = 16; *TM = 256; }
  else if (N <= 32) { *TN = 32; *TM = 128; }
  else { *TN = 64; *TM = 128; }
}

// split-K factor for the tap-major GEMM: only when the grid is small and K is deep
static int tap_splits(const ConvGeom& g, int KK, int* sps) {
  const int BK = g.C % 32 == 0 ? 32 : 16;
  int TN, TM;
  tap_tile(g.N, &TN, &TM);
  const int tiles = ((g.Mpos + TM - 1) / TM) * ((g.N + TN - 1) / TN);
  const int ksteps = KK * ((g.C + BK - 1) / BK);
  int s = 1;
  if (g.C % 16 == 0 && tiles < 512 && ksteps >= 8) {
    s = (1024 + tiles - 1) / tiles;
    if (s > ksteps / 4) s = ksteps / 4;
    if (s > 16) s = 16;
    if (s < 1) s = 1;
  }
  const int per = (ksteps + s - 1) / s;
  *sps = per;
  return (ksteps + per - 1) / per;
}

// returns whether the eval BN / Snake was applied (by the fused epilogue, or by the last split
// block's finish with `fe`)
template <int MODE, int KH, int KW, int SW, bool REPL, int BK>
static bool launch_tap_bk(const float* in, const float* wt, float* out, const ConvGeom& g,
                          const Epi& e, int splits, int sps, int64_t zstride, hipStream_t st,
                          int* cnt = nullptr, float* fout = nullptr, const Epi* fe = nullptr) {
  int TN, TM;
  tap_tile(g.N, &TN, &TM);
  dim3 grid((g.Mpos + TM - 1) / TM, (g.N + TN - 1) / TN, splits);
  const Epi fin = fe ? *fe : e;
  // the eval conv -> BN -> Snake shapes (ResBlock 3x3 / 1x1, DecBlock ConvT, Upscale Conv1d)
  // have epilogue-fused variants; the split-K finish applies `fin`'s BN itself
  constexpr bool post_kind = (MODE == GATHER_F && ((KH == 3 && KW == 3) || (KH == 1 && KW == 3 && !REPL) ||
                                                   (KH == 1 && KW == 1) ||
                                                   (KH == 3 && KW == 4 && SW == 2 && REPL))) ||
                             (MODE == GATHER_T && KH == 3 && KW == 4 && SW == 2);
  if constexpr (post_kind) {
    if (splits == 1 && e.bn_rv) {
      if (TN == 16)
        hipLaunchKernelGGL((conv_tap_kernel<MODE, KH, KW, SW, REPL, 16, 256, 1, 4, BK, true>), grid,
                           dim3(256), 0, st, in, wt, out, g, e, sps, zstride, cnt, fout, fin);
      else if (TN == 32)
        hipLaunchKernelGGL((conv_tap_kernel<MODE, KH, KW, SW, REPL, 32, 128, 2, 2, BK, true>), grid,
                           dim3(256), 0, st, in, wt, out, g, e, sps, zstride, cnt, fout, fin);
      else
        hipLaunchKernelGGL((conv_tap_kernel<MODE, KH, KW, SW, REPL, 64, 128, 2, 2, BK, true>), grid,
                           dim3(256), 0, st, in, wt, out, g, e, sps, zstride, cnt, fout, fin);
      return true;
    }
  }
  if (TN == 16)
    hipLaunchKernelGGL((conv_tap_kernel<MODE, KH, KW, SW, REPL, 16, 256, 1, 4, BK>), grid,
                       dim3(256), 0, st, in, wt, out, g, e, sps, zstride, cnt, fout, fin);
  else if (TN == 32)
    hipLaunchKernelGGL((conv_tap_kernel<MODE, KH, KW, SW, REPL, 32, 128, 2, 2, BK>), grid,
                       dim3(256), 0, st, in, wt, out, g, e, sps, zstride, cnt, fout, fin);
  else
    hipLaunchKernelGGL((conv_tap_kernel<MODE, KH, KW, SW, REPL, 64, 128, 2, 2, BK>), grid,
                       dim3(256), 0, st, in, wt, out, g, e, sps, zstride, cnt, fout, fin);
  return cnt && fin.bn_rv;
}

// floats of workspace launch_conv may use for this geometry (pack + split-K slab)
int64_t conv_gemm_ws(const ConvGeom& g, int KK) {
  if (g.C % 16 != 0) return 0;
  int sps;
  const int s = tap_splits(g, KK, &sps);
  return (int64_t)g.N * g.C * KK + (s > 1 ? (int64_t)s * g.N * g.Mpos : 0);
}

// tap-major GEMM (C % 16 == 0, packed or raw weights); `slab` (nullable) enables split-K with
// splits*N*Mpos floats of partials
template <int MODE, int KH, int KW, int SW, bool REPL>
static bool launch_tap_t(const float* in, const float* wt, float* out, const ConvGeom& g,
                         const Epi& e, float* slab, hipStream_t st) {
  int sps;
  const int splits = slab ? tap_splits(g, KH * KW, &sps) : 1;
  if (!slab) sps = KH * KW * ((g.C + 31) / 16);  // >= all K-steps
  TVQ_PLAN("conv_tap splits%d", splits);
  if (splits > 1) {
    const int64_t n_out = (int64_t)g.Mpos * g.N;
    const Epi raw = {nullptr, nullptr, 0.f, 1.f, nullptr, 0};
    int TN, TM;
    tap_tile(g.N, &TN, &TM);
    int* cnt = counters((int64_t)((g.Mpos + TM - 1) / TM) * ((g.N + TN - 1) / TN), FIN_CONV);
    const bool post =
        g.C % 32 == 0 ? launch_tap_bk<MODE, KH, KW, SW, REPL, 32>(in, wt, slab, g, raw, splits, sps,
                                                                  n_out, st, cnt, out, &e)
                      : launch_tap_bk<MODE, KH, KW, SW, REPL, 16>(in, wt, slab, g, raw, splits, sps,
                                                                  n_out, st, cnt, out, &e);
    if (cnt) return post;
    int blocks = (int)((n_out + 255) / 256);
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(conv_splitk_epi_kernel, dim3(blocks), dim3(256), 0, st, slab, splits,
                       (int)n_out, g.N, make_div16((int64_t)g.Hout * g.Wo), e, out);
    return e.bn_rv != nullptr;
  }
  return g.C % 32 == 0 ? launch_tap_bk<MODE, KH, KW, SW, REPL, 32>(in, wt, out, g, e, 1, sps, 0, st)
                       : launch_tap_bk<MODE, KH, KW, SW, REPL, 16>(in, wt, out, g, e, 1, sps, 0, st);
}

bool launch_tap(int mode, int kind, bool repl, const float* in, const float* wt, float* out,
                const ConvGeom& g, const Epi& e, float* slab, hipStream_t st) {
#define M_(m, a, b_, c, d) return launch_tap_t<m, a, b_, c, d>(in, wt, out, g, e, slab, st);
  TVQ_DISPATCH_CONV(mode, kind, repl, M_)
#undef M_
  return false;
}

template <int MODE, int KH, int KW, int SW, bool REPL>
static void launch_gemm_flat_t(const float* in, const float* wt, float* out, const ConvGeom& g,
                               const Epi& e, hipStream_t st) {
  // small channel counts: flat (c, kh, kw) K order keeps the K-steps full
  TVQ_PLAN("conv_gemm n%d", g.N);
  if (g.N <= 16) {
    dim3 grid((g.Mpos + 255) / 256, (g.N + 15) / 16);
    hipLaunchKernelGGL((conv_gemm_kernel<MODE, KH, KW, SW, REPL, 16, 256, 1, 4>), grid, dim3(256),
                       0, st, in, wt, out, g, e);
  } else if (g.N <= 32) {
    dim3 grid((g.Mpos + 127) / 128, (g.N + 31) / 32);
    hipLaunchKernelGGL((conv_gemm_kernel<MODE, KH, KW, SW, REPL, 32, 128, 2, 2>), grid, dim3(256),
                       0, st, in, wt, out, g, e);
  } else {
    dim3 grid((g.Mpos + 127) / 128, (g.N + 63) / 64);
    hipLaunchKernelGGL((conv_gemm_kernel<MODE, KH, KW, SW, REPL, 64, 128, 2, 2>), grid, dim3(256),
                       0, st, in, wt, out, g, e);
  }
}

void launch_gemm_flat(int mode, int kind, bool repl, const float* in, const float* wt, float* out,
                      const ConvGeom& g, const Epi& e, hipStream_t st) {
#define M_(m, a, b_, c, d) launch_gemm_flat_t<m, a, b_, c, d>(in, wt, out, g, e, st);
  TVQ_DISPATCH_CONV(mode, kind, repl, M_)
#undef M_
}

}  // namespace tvq
