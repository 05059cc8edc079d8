// Supervised FCN training kernels for gfx950: the tvq_fcn_* training entries of
// include/tvq_fcn.h.
//
// Reference: FCNBaseline (timevqvae/models/fcn.py) in training mode under CrossEntropyLoss
// (scripts/train_fcn.py:101-168).  Every sum below has a fixed order that does not depend on
// the grid's scheduling, and there are no float atomics: two runs give the same bits.
//
//   fcn_conv_kernel (tvq_fcn_core.h)  FC_EP_TRAIN: u = conv + bias and the fp64 partial sums of
//     u, u^2 per (channel, sample, position tile); FC_EP_PLAIN with left padding K-1-(K-1)/2 on
//     the flipped transpose of the weight (fcn_pack_t_kernel): the data gradient.
//   fcn_bn_finish_kernel   one block per channel adds the partials (strided per thread, xor
//     tree per wave, waves in order), writes mean / rstd / scale / shift and updates the
//     running statistics.
//   fcn_bn_relu_kernel     y = relu(fma(scale, u, shift)), one wave per (sample, channel) row;
//     the row's mean in the order of the eval kernel's pooled epilogue (L only).
//   fcn_head_ce_kernel     fcn_head_kernel plus the row's cross-entropy, dlogits and dfeat;
//     fcn_loss_mean_kernel adds the rows' losses; fcn_head_wgrad_kernel: dW, db, one thread
//     per entry over the batch in order.
//   fcn_bn_bwd_part / _finish / _apply   the BatchNorm + ReLU backward: v is recomputed as the
//     forward's fma(scale, u, shift), so the mask is the forward's bit for bit.
//   fcn_wgrad_kernel<K>    dw[co, ci, k] = sum_{b,l} du[b,co,l] h[b,ci,l+k-padL] on the matrix
//     cores with the positions as the reduction: a block owns 64 channels x 128 columns
//     r = ci K + k and a range of samples; per stage of 64 positions it keeps the du tile (row
//     stride 65: the 32 channel lanes hit 32 banks) and the h rows of its columns with their
//     halo (row stride 64 + K = K mod 32: the 32 column lanes hit 32 banks) in LDS, the next
//     stage's global loads in flight during the MFMAs.  The bias gradient is the row sums of
//     the staged du tile (four threads per row, 16 positions each, stages added in fp64).
//     The sample splits write slabs that reduce_rows (tvq_reduce.h) adds in its fixed order.
#include "../../include/tvq_fcn.h"
#include "tvq_common.h"
#include "tvq_eval.h"
#include "tvq_fcn_core.h"
#include "tvq_reduce.h"

namespace tvq {
namespace {

// wpt = the packed form (fcn_pack_kernel's order) of wT (Ci, Co, K), wT[ci][co][k'] =
// w[co][ci][K-1-k']: the data gradient's A operand, Ci rows of Co K taps.
__global__ __launch_bounds__(256) void fcn_pack_t_kernel(const float* __restrict__ w,
                                                         float* __restrict__ wp, int Co, int Ci,
                                                         int K, int64_t total) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int S = FC_CC * K / 2, nch = (Co + FC_CC - 1) / FC_CC;
  const int i = (int)(e & 31), h = (int)((e >> 5) & 1);
  int64_t q = e >> 6;
  const int s = (int)(q % S);
  q /= S;
  const int c = (int)(q % nch), t = (int)(q / nch);
  const int r = 2 * s + h, co = c * FC_CC + r / K, k = r % K, ci = 32 * t + i;
  wp[e] = co < Co ? w[((int64_t)co * Ci + ci) * K + (K - 1 - k)] : 0.f;
}

// ---- BatchNorm statistics ------------------------------------------------------------------
__global__ __launch_bounds__(256) void fcn_bn_finish_kernel(
    const double* __restrict__ part, int64_t P, double n, const float* __restrict__ gamma,
    const float* __restrict__ beta, double eps, double momentum, float* __restrict__ rmean,
    float* __restrict__ rvar, int64_t* __restrict__ nbt, float* __restrict__ stats, int C) {
  __shared__ double red[4];
  const int c = blockIdx.x;
  const double s1 = block_sum_strided(part + (int64_t)c * P, P, 1, red);
  const double s2 = block_sum_strided(part + ((int64_t)C + c) * P, P, 1, red);
  if (threadIdx.x != 0) return;
  const double mean = s1 / n, var = fmax(s2 / n - mean * mean, 0.0);
  const double rstd = 1.0 / sqrt(var + eps);
  const float scale = (float)((double)gamma[c] * rstd);
  stats[c] = (float)mean;
  stats[C + c] = (float)rstd;
  stats[2 * C + c] = scale;
  stats[3 * C + c] = (float)((double)beta[c] - mean * (double)scale);
  if (rmean) rmean[c] = (float)((1.0 - momentum) * (double)rmean[c] + momentum * mean);
  if (rvar) rvar[c] = (float)((1.0 - momentum) * (double)rvar[c] + momentum * var * n / (n - 1.0));
  if (nbt && c == 0) nbt[0] += 1;
}

__global__ __launch_bounds__(256) void fcn_bn_relu_kernel(const float* __restrict__ u,
                                                          const float* __restrict__ stats,
                                                          float* __restrict__ y,
                                                          float* __restrict__ gap, int64_t rows,
                                                          int C, int L) {
  const int lane = threadIdx.x & 63, j = lane & 31, wpos = lane >> 5;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;  // wave-uniform, no barrier below
  const int c = (int)(row % C);
  const float sc = stats[2 * C + c], sh = stats[3 * C + c];
  const float* ur = u + row * L;
  float acc = 0.f;
  for (int l0 = 0; l0 < L; l0 += FC_TL) {
    const int la = l0 + wpos * 64 + j, lb = la + 32;
    const float va = la < L ? fmaxf(fmaf(sc, ur[la], sh), 0.f) : 0.f;
    const float vb = lb < L ? fmaxf(fmaf(sc, ur[lb], sh), 0.f) : 0.f;
    if (y) {
      if (la < L) y[row * L + la] = va;
      if (lb < L) y[row * L + lb] = vb;
    }
    acc += va;
    acc += vb;
  }
  if (!gap) return;
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);  // the 32 columns of a half
  const float other = __shfl_xor(acc, 32, 64);
  if (lane == 0) gap[row] = (acc + other) / (float)L;
}

// ---- head with cross-entropy ---------------------------------------------------------------
constexpr int FH_WAVES = 4;
constexpr int FH_MAXC = 4096;  // 4 waves x 4096 floats = the 64 KiB a block may take

__global__ __launch_bounds__(64 * FH_WAVES) void fcn_head_ce_kernel(
    const float* __restrict__ feat, const float* __restrict__ w, const float* __restrict__ bias,
    const int64_t* __restrict__ target, float* __restrict__ logits, float* __restrict__ row_loss,
    float* __restrict__ dlogits, float* __restrict__ dfeat, int64_t B, int D, int C) {
  extern __shared__ float lg_all[];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  float* lg = lg_all + (int64_t)wid * C;
  const int64_t row = (int64_t)blockIdx.x * FH_WAVES + wid;
  const bool live = row < B;  // wave-uniform
  if (live) {
    const float* f = feat + row * D;
    for (int c = 0; c < C; ++c) {
      const float* wr = w + (int64_t)c * D;
      float v = 0.f;
      for (int d = lane; d < D; d += 64) v = fmaf(f[d], wr[d], v);
      v = wave_sum(v) + (bias ? bias[c] : 0.f);
      if (lane == 0) {
        lg[c] = v;
        logits[row * C + c] = v;
      }
    }
  }
  __syncthreads();
  float m = -INFINITY, s = 0.f;
  int64_t t = -1;
  if (live) {
    for (int c = lane; c < C; c += 64) m = fmaxf(m, lg[c]);
    m = wave_max(m);
    for (int c = lane; c < C; c += 64) s += expf(lg[c] - m);
    s = wave_sum(s);
    t = target[row];
    const bool ok = t >= 0 && t < C;  // a target outside the classes gives a NaN loss
    if (lane == 0) row_loss[row] = ok ? logf(s) + m - lg[t] : NAN;
  }
  __syncthreads();
  if (live) {
    const float inv_b = 1.f / (float)B;
    for (int c = lane; c < C; c += 64) {
      const float dl = (expf(lg[c] - m) / s - (c == t ? 1.f : 0.f)) * inv_b;
      lg[c] = dl;
      dlogits[row * C + c] = dl;
    }
  }
  __syncthreads();
  if (live) {
    for (int d = lane; d < D; d += 64) {
      float v = 0.f;
      for (int c = 0; c < C; ++c) v = fmaf(lg[c], w[(int64_t)c * D + d], v);
      dfeat[row * D + d] = v;
    }
  }
}

__global__ __launch_bounds__(256) void fcn_loss_mean_kernel(const float* __restrict__ row_loss,
                                                            int64_t B, float* __restrict__ loss) {
  __shared__ double red[4];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < B; i += 256) s += (double)row_loss[i];
  s = block_wave_sum_d(s, red);
  if (threadIdx.x == 0) loss[0] = (float)(s / (double)B);
}

__global__ __launch_bounds__(256) void fcn_head_wgrad_kernel(
    const float* __restrict__ dlogits, const float* __restrict__ feat, float* __restrict__ dw,
    float* __restrict__ db, int accumulate, int64_t B, int D, int C) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t nw = (int64_t)C * D;
  if (e >= nw + C) return;
  float v = 0.f;
  if (e < nw) {
    if (!dw) return;
    const int c = (int)(e / D), d = (int)(e % D);
    int64_t b = 0;
    for (; b + 8 <= B; b += 8) {  // the loads of 8 samples in flight, one fma chain in order
      float a[8], f[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        a[i] = dlogits[(b + i) * C + c];
        f[i] = feat[(b + i) * D + d];
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) v = fmaf(a[i], f[i], v);
    }
    for (; b < B; ++b) v = fmaf(dlogits[b * C + c], feat[b * D + d], v);
    dw[e] = accumulate ? dw[e] + v : v;
  } else {
    if (!db) return;
    const int c = (int)(e - nw);
    for (int64_t b = 0; b < B; ++b) v += dlogits[b * C + c];
    db[c] = accumulate ? db[c] + v : v;
  }
}

// ---- BatchNorm + ReLU backward -------------------------------------------------------------
// dv of one element: the upstream gradient where the forward's v = fma(scale, u, shift) > 0
__device__ __forceinline__ float fcn_dv(float uu, float sc, float sh, float g) {
  return fmaf(sc, uu, sh) > 0.f ? g : 0.f;
}

__global__ __launch_bounds__(256) void fcn_bn_bwd_part_kernel(
    const float* __restrict__ u, const float* __restrict__ dy, const float* __restrict__ dfeat,
    const float* __restrict__ stats, double* __restrict__ ws, int64_t B, int C, int L) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B * C) return;  // wave-uniform, no barrier below
  const int c = (int)(row % C);
  const int64_t b = row / C;
  const float mean = stats[c], rstd = stats[C + c], sc = stats[2 * C + c], sh = stats[3 * C + c];
  const float g0 = dfeat ? dfeat[row] / (float)L : 0.f;
  const float* ur = u + row * L;
  double s1 = 0.0, s2 = 0.0;
  for (int l = lane; l < L; l += 64) {
    const float uu = ur[l];
    const float dv = fcn_dv(uu, sc, sh, dy ? dy[row * L + l] : g0);
    const float xh = (uu - mean) * rstd;
    s1 += (double)dv;
    s2 += (double)dv * (double)xh;
  }
  s1 = wave_sum_d(s1);
  s2 = wave_sum_d(s2);
  if (lane == 0) {
    ws[(int64_t)c * B + b] = s1;
    ws[((int64_t)C + c) * B + b] = s2;
  }
}

__global__ __launch_bounds__(256) void fcn_bn_bwd_finish_kernel(double* __restrict__ ws, int64_t B,
                                                                int C, float* __restrict__ dgamma,
                                                                float* __restrict__ dbeta,
                                                                int accumulate) {
  __shared__ double red[4];
  const int c = blockIdx.x;
  const double s1 = block_sum_strided(ws + (int64_t)c * B, B, 1, red);
  const double s2 = block_sum_strided(ws + ((int64_t)C + c) * B, B, 1, red);
  if (threadIdx.x != 0) return;
  double* tot = ws + 2 * (int64_t)C * B;
  tot[c] = s1;
  tot[C + c] = s2;
  if (dbeta) dbeta[c] = accumulate ? dbeta[c] + (float)s1 : (float)s1;
  if (dgamma) dgamma[c] = accumulate ? dgamma[c] + (float)s2 : (float)s2;
}

__global__ __launch_bounds__(256) void fcn_bn_bwd_apply_kernel(
    const float* __restrict__ u, const float* __restrict__ dy, const float* __restrict__ dfeat,
    const float* __restrict__ stats, const double* __restrict__ ws, float* __restrict__ du,
    int64_t B, int C, int L) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B * C) return;
  const int c = (int)(row % C);
  const float mean = stats[c], rstd = stats[C + c], sc = stats[2 * C + c], sh = stats[3 * C + c];
  const double n = (double)B * (double)L;
  const double* tot = ws + 2 * (int64_t)C * B;
  const float c1 = (float)(tot[c] / n), c2 = (float)(tot[C + c] / n);
  const float g0 = dfeat ? dfeat[row] / (float)L : 0.f;
  const float* ur = u + row * L;
  for (int l = lane; l < L; l += 64) {
    const float uu = ur[l];
    const float dv = fcn_dv(uu, sc, sh, dy ? dy[row * L + l] : g0);
    const float xh = (uu - mean) * rstd;
    du[row * L + l] = sc * (dv - c1 - xh * c2);
  }
}

// ---- conv weight and bias gradient ---------------------------------------------------------
constexpr int WG_T = 256;    // 4 waves: 2 (channels) x 2 (column halves)
constexpr int WG_CO = 64;    // channels per block
constexpr int WG_R = 128;    // columns r = ci K + k per block
constexpr int WG_LT = 64;    // positions per stage
constexpr int WG_DS = WG_LT + 1;  // du tile row stride (odd)
constexpr int WG_MAXSPLIT = 256;  // reduce_rows adds up to 256 slabs in one level

template <int K>
struct WgShape {
  static constexpr int NR = (WG_R - 1) / K + 2 < WG_R ? (WG_R - 1) / K + 2 : WG_R;  // h rows of a tile
  static constexpr int HS = WG_LT + K;   // h row stride: = K (mod 32), >= the span
  static constexpr int SPAN = WG_LT + K - 1;
  static constexpr int NH = (NR * SPAN + WG_T - 1) / WG_T;
};

// the one plan for the launch and the workspace query: sample splits
inline int fcn_wgrad_splits(int64_t B, int64_t Ci, int64_t Co, int64_t K) {
  const int64_t tiles = ((Ci * K + WG_R - 1) / WG_R) * ((Co + WG_CO - 1) / WG_CO);
  int64_t s = (512 + tiles - 1) / tiles;
  if (s > WG_MAXSPLIT) s = WG_MAXSPLIT;
  if (s > B) s = B;
  return (int)(s < 1 ? 1 : s);
}

template <int K>
__global__ __launch_bounds__(WG_T, 2) void fcn_wgrad_kernel(
    const float* __restrict__ du, const float* __restrict__ hin, float* __restrict__ slab_w,
    float* __restrict__ slab_b, int B, int Ci, int L, int Co) {
  using Sh = WgShape<K>;
  constexpr int PADL = (K - 1) / 2;
  __shared__ float dus[WG_CO * WG_DS];
  __shared__ float hs[Sh::NR * Sh::HS];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int j = lane & 31, hh = lane >> 5, wco = wid & 1, wr = wid >> 1;
  const int N = Ci * K;
  const int r0 = blockIdx.x * WG_R, co0 = blockIdx.y * WG_CO, ci0 = r0 / K;
  const int split = blockIdx.z, nsplit = gridDim.z;
  const int b_lo = (int)((int64_t)B * split / nsplit), b_hi = (int)((int64_t)B * (split + 1) / nsplit);
  const int ntl = (L + WG_LT - 1) / WG_LT;
  const int nstage = (b_hi - b_lo) * ntl;
  const bool want_b = slab_b != nullptr && blockIdx.x == 0;  // block-uniform

  // a lane's two columns: fixed offsets into the staged h rows (a column past N reads row 0
  // and is not stored)
  int boff[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int r = r0 + wr * 64 + p * 32 + j;
    boff[p] = r < N ? (r / K - ci0) * Sh::HS + r % K : 0;
  }
  const int aoff = (wco * 32 + j) * WG_DS;

  floatx16 acc0, acc1;
#pragma unroll
  for (int g = 0; g < 16; ++g) acc0[g] = acc1[g] = 0.f;
  // bias gradient: thread (row = tid / 4, quarter = tid % 4) adds its 16 positions of the
  // staged du row in order, the quarters by a fixed xor tree, the stages in fp64
  double bsum = 0.0;
  const int boff_row = (tid >> 2) * WG_DS + (tid & 3) * (WG_LT / 4);
  // a wave whose columns lie past N multiplies nothing (wave-uniform)
  const bool act0 = r0 + wr * 64 < N, act1 = r0 + wr * 64 + 32 < N;

  float rd[16], rh[Sh::NH];
  auto load = [&](int stage) {
    const int b = b_lo + stage / ntl, l0 = (stage % ntl) * WG_LT;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int co = co0 + wid + 4 * i, l = l0 + lane;
      rd[i] = (co < Co && l < L) ? du[((int64_t)b * Co + co) * L + l] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < Sh::NH; ++i) {
      const int e = tid + WG_T * i, row = e / Sh::SPAN, t = e - row * Sh::SPAN;
      const int ci = ci0 + row, pos = l0 + t - PADL;
      const bool ok = row < Sh::NR && ci < Ci && pos >= 0 && pos < L;
      rh[i] = ok ? hin[((int64_t)b * Ci + ci) * L + pos] : 0.f;
    }
  };

  if (nstage > 0) load(0);
  for (int stage = 0; stage < nstage; ++stage) {
    __syncthreads();  // the previous stage's MFMAs have read the tiles
#pragma unroll
    for (int i = 0; i < 16; ++i) dus[(wid + 4 * i) * WG_DS + lane] = rd[i];
#pragma unroll
    for (int i = 0; i < Sh::NH; ++i) {
      const int e = tid + WG_T * i, row = e / Sh::SPAN, t = e - row * Sh::SPAN;
      if (row < Sh::NR) hs[row * Sh::HS + t] = rh[i];
    }
    __syncthreads();
    if (stage + 1 < nstage) load(stage + 1);
    if (want_b) {
      float v = 0.f;
#pragma unroll
      for (int i = 0; i < WG_LT / 4; ++i) v += dus[boff_row + i];
      v += __shfl_xor(v, 1, 64);
      v += __shfl_xor(v, 2, 64);
      bsum += (double)v;
    }
    if (act1) {
#pragma unroll 8
      for (int s = 0; s < WG_LT / 2; ++s) {
        const int lp = 2 * s + hh;
        const float a = dus[aoff + lp];
        const float b0 = hs[boff[0] + lp], b1 = hs[boff[1] + lp];
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc1, 0, 0, 0);
      }
    } else if (act0) {
#pragma unroll 8
      for (int s = 0; s < WG_LT / 2; ++s) {
        const int lp = 2 * s + hh;
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(dus[aoff + lp], hs[boff[0] + lp], acc0, 0, 0, 0);
      }
    }
  }

#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int co = co0 + wco * 32 + (g & 3) + 8 * (g >> 2) + 4 * hh;
    const int ra = r0 + wr * 64 + j, rb = ra + 32;
    if (co < Co) {
      float* row = slab_w + ((int64_t)split * Co + co) * N;
      if (ra < N) row[ra] = acc0[g];
      if (rb < N) row[rb] = acc1[g];
    }
  }
  if (want_b && (tid & 3) == 0) {
    const int co = co0 + (tid >> 2);
    if (co < Co) slab_b[(int64_t)split * Co + co] = (float)bsum;
  }
}

template <int K>
void fcn_wgrad_launch(const float* du, const float* h, float* slab_w, float* slab_b, int B, int Ci,
                      int L, int Co, int splits, hipStream_t st) {
  const dim3 grid((unsigned)((Ci * K + WG_R - 1) / WG_R), (unsigned)((Co + WG_CO - 1) / WG_CO),
                  (unsigned)splits);
  hipLaunchKernelGGL((fcn_wgrad_kernel<K>), grid, dim3(WG_T), 0, st, du, h, slab_w, slab_b, B, Ci,
                     L, Co);
}

bool fcn_conv_args(const char* what, int64_t B, int64_t Ci, int64_t L, int64_t Co, int64_t K) {
  if (!(Co >= 32 && Co % 32 == 0 && Co <= (1 << 20))) {
    set_error("%s: Co=%lld is not a multiple of 32", what, (long long)Co);
    return false;
  }
  if (!(K >= 1 && K <= FC_MAXK)) {
    set_error("%s: K=%lld outside [1, 8]", what, (long long)K);
    return false;
  }
  if (!(B >= 1 && B <= 0x7fffffffLL && Ci >= 1 && Ci <= (1 << 20) && L >= 1 && L <= (1 << 22))) {
    set_error("%s: B=%lld, Ci=%lld or L=%lld out of range", what, (long long)B, (long long)Ci,
              (long long)L);
    return false;
  }
  if (Co * ((Ci + 7) / 8 * 8) * K >= ((int64_t)1 << 31)) {
    set_error("%s: Co*Ci*K too large", what);
    return false;
  }
  return true;
}

#define TVQ_FCN_K_SWITCH(K, CALL)                                                    \
  switch ((int)(K)) {                                                                \
    case 1: { constexpr int KK = 1; CALL; } break;                                   \
    case 2: { constexpr int KK = 2; CALL; } break;                                   \
    case 3: { constexpr int KK = 3; CALL; } break;                                   \
    case 4: { constexpr int KK = 4; CALL; } break;                                   \
    case 5: { constexpr int KK = 5; CALL; } break;                                   \
    case 6: { constexpr int KK = 6; CALL; } break;                                   \
    case 7: { constexpr int KK = 7; CALL; } break;                                   \
    case 8: { constexpr int KK = 8; CALL; } break;                                   \
  }

}  // namespace
}  // namespace tvq

using namespace tvq;

extern "C" int64_t tvq_fcn_stats_size(int64_t B, int64_t L, int64_t Co) {
  if (B < 1 || L < 1 || Co < 1) return 0;
  return 2 * Co * B * ((L + FC_TL - 1) / FC_TL);
}

extern "C" int tvq_fcn_conv_train_fwd(const float* x, const float* wp, const float* bias, float* u,
                                      double* part, int64_t B, int64_t Ci, int64_t L, int64_t Co,
                                      int64_t K, tvq_stream_t stream) {
  TVQ_CHECK_ARG(x && wp && bias && u && part, "tvq_fcn_conv_train_fwd: null x, wp, bias, u or part");
  if (!fcn_conv_args("tvq_fcn_conv_train_fwd", B, Ci, L, Co, K)) return TVQ_ERR_ARG;
  const int nch = (int)((Ci + FC_CC - 1) / FC_CC), ntiles = (int)((L + FC_TL - 1) / FC_TL);
  const dim3 grid((unsigned)B, (unsigned)ntiles, (unsigned)((Co + FC_COT - 1) / FC_COT));
  TVQ_PLAN("fcn_conv_train K=%d nch=%d tiles=%d", (int)K, nch, ntiles);
  TVQ_FCN_K_SWITCH(K, hipLaunchKernelGGL(
      (fcn_conv_kernel<KK, (KK - 1) / 2, FC_EP_TRAIN, true, false>), grid, dim3(FC_T), 0,
      (hipStream_t)stream, x, wp, bias, (const float*)nullptr, u, (void*)part, (int)Ci, (int)L,
      (int)Co, nch))
  return launch_status("tvq_fcn_conv_train_fwd");
}

extern "C" int tvq_fcn_bn_finish(const double* part, int64_t P, int64_t n, const float* gamma,
                                 const float* beta, float eps, float momentum, float* running_mean,
                                 float* running_var, int64_t* num_batches_tracked, float* stats,
                                 int64_t C, tvq_stream_t stream) {
  TVQ_CHECK_ARG(part && gamma && beta && stats, "tvq_fcn_bn_finish: null part, gamma, beta or stats");
  TVQ_CHECK_ARG(C >= 1 && C <= (1 << 20) && P >= 1, "tvq_fcn_bn_finish: C=%lld or P=%lld out of range", (long long)C, (long long)P);
  TVQ_CHECK_ARG(n >= 2, "tvq_fcn_bn_finish: batch statistics need more than 1 value per channel (n=%lld)", (long long)n);
  hipLaunchKernelGGL(fcn_bn_finish_kernel, dim3((unsigned)C), dim3(256), 0, (hipStream_t)stream, part,
                     P, (double)n, gamma, beta, (double)eps, (double)momentum, running_mean,
                     running_var, num_batches_tracked, stats, (int)C);
  return launch_status("tvq_fcn_bn_finish");
}

extern "C" int tvq_fcn_bn_relu(const float* u, const float* stats, float* y, float* gap, int64_t B,
                               int64_t C, int64_t L, tvq_stream_t stream) {
  TVQ_CHECK_ARG(u && stats && (y || gap), "tvq_fcn_bn_relu: null u or stats, or y and gap both null");
  TVQ_CHECK_ARG(B >= 1 && C >= 1 && C <= (1 << 20) && L >= 1 && L <= (1 << 22) && B * C < ((int64_t)1 << 32),
                "tvq_fcn_bn_relu: B=%lld, C=%lld or L=%lld out of range", (long long)B, (long long)C, (long long)L);
  hipLaunchKernelGGL(fcn_bn_relu_kernel, dim3((unsigned)((B * C + 3) / 4)), dim3(256), 0,
                     (hipStream_t)stream, u, stats, y, gap, B * C, (int)C, (int)L);
  return launch_status("tvq_fcn_bn_relu");
}

extern "C" int64_t tvq_fcn_head_ce_workspace(int64_t B) { return B < 1 ? 0 : B; }

extern "C" int tvq_fcn_head_ce(const float* feat, const float* w, const float* bias,
                               const int64_t* target, float* logits, float* loss, float* dlogits,
                               float* dfeat, float* workspace, int64_t B, int64_t D,
                               int64_t classes, tvq_stream_t stream) {
  TVQ_CHECK_ARG(feat && w && target && logits && loss && dlogits && dfeat && workspace,
                "tvq_fcn_head_ce: null argument");
  TVQ_CHECK_ARG(B >= 1 && B <= 0x7fffffffLL, "tvq_fcn_head_ce: B=%lld outside [1, 2^31)", (long long)B);
  TVQ_CHECK_ARG(D >= 1 && D <= (1 << 20), "tvq_fcn_head_ce: D=%lld outside [1, 2^20]", (long long)D);
  TVQ_CHECK_ARG(classes >= 1 && classes <= FH_MAXC, "tvq_fcn_head_ce: classes=%lld outside [1, %d]", (long long)classes, FH_MAXC);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(fcn_head_ce_kernel, dim3((unsigned)((B + FH_WAVES - 1) / FH_WAVES)),
                     dim3(64 * FH_WAVES), (size_t)(FH_WAVES * classes * sizeof(float)), st, feat, w,
                     bias, target, logits, workspace, dlogits, dfeat, B, (int)D, (int)classes);
  hipLaunchKernelGGL(fcn_loss_mean_kernel, dim3(1), dim3(256), 0, st, workspace, B, loss);
  return launch_status("tvq_fcn_head_ce");
}

extern "C" int tvq_fcn_head_wgrad(const float* dlogits, const float* feat, float* dw, float* db,
                                  int64_t accumulate, int64_t B, int64_t D, int64_t classes,
                                  tvq_stream_t stream) {
  TVQ_CHECK_ARG(dlogits && feat && (dw || db), "tvq_fcn_head_wgrad: null dlogits or feat, or dw and db both null");
  TVQ_CHECK_ARG(B >= 1 && D >= 1 && D <= (1 << 20) && classes >= 1 && classes <= FH_MAXC,
                "tvq_fcn_head_wgrad: B=%lld, D=%lld or classes=%lld out of range", (long long)B, (long long)D, (long long)classes);
  const int64_t n = classes * D + classes;
  hipLaunchKernelGGL(fcn_head_wgrad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, dlogits, feat, dw, db, (int)accumulate, B, (int)D,
                     (int)classes);
  return launch_status("tvq_fcn_head_wgrad");
}

extern "C" int64_t tvq_fcn_bn_bwd_workspace(int64_t B, int64_t C) {
  return (B < 1 || C < 1) ? 0 : 2 * C * B + 2 * C;
}

extern "C" int tvq_fcn_bn_relu_bwd(const float* u, const float* dy, const float* dfeat,
                                   const float* stats, float* du, float* dgamma, float* dbeta,
                                   int64_t accumulate, double* workspace, int64_t B, int64_t C,
                                   int64_t L, tvq_stream_t stream) {
  TVQ_CHECK_ARG(u && stats && du && workspace, "tvq_fcn_bn_relu_bwd: null u, stats, du or workspace");
  TVQ_CHECK_ARG((dy != nullptr) != (dfeat != nullptr), "tvq_fcn_bn_relu_bwd: exactly one of dy and dfeat");
  TVQ_CHECK_ARG(B >= 1 && C >= 1 && C <= (1 << 20) && L >= 1 && L <= (1 << 22) && B * C < ((int64_t)1 << 32),
                "tvq_fcn_bn_relu_bwd: B=%lld, C=%lld or L=%lld out of range", (long long)B, (long long)C, (long long)L);
  hipStream_t st = (hipStream_t)stream;
  const dim3 rows((unsigned)((B * C + 3) / 4));
  hipLaunchKernelGGL(fcn_bn_bwd_part_kernel, rows, dim3(256), 0, st, u, dy, dfeat, stats, workspace,
                     B, (int)C, (int)L);
  hipLaunchKernelGGL(fcn_bn_bwd_finish_kernel, dim3((unsigned)C), dim3(256), 0, st, workspace, B,
                     (int)C, dgamma, dbeta, (int)accumulate);
  hipLaunchKernelGGL(fcn_bn_bwd_apply_kernel, rows, dim3(256), 0, st, u, dy, dfeat, stats,
                     (const double*)workspace, du, B, (int)C, (int)L);
  return launch_status("tvq_fcn_bn_relu_bwd");
}

extern "C" int tvq_fcn_pack_weight_t(const float* w, float* wpt, int64_t Co, int64_t Ci, int64_t K,
                                     tvq_stream_t stream) {
  TVQ_CHECK_ARG(w && wpt, "tvq_fcn_pack_weight_t: null w or wpt");
  TVQ_CHECK_ARG(Ci >= 32 && Ci % 32 == 0 && Ci <= (1 << 20), "tvq_fcn_pack_weight_t: Ci=%lld is not a multiple of 32", (long long)Ci);
  TVQ_CHECK_ARG(K >= 1 && K <= FC_MAXK, "tvq_fcn_pack_weight_t: K=%lld outside [1, 8]", (long long)K);
  TVQ_CHECK_ARG(Co >= 1 && Co <= (1 << 20), "tvq_fcn_pack_weight_t: Co=%lld outside [1, 2^20]", (long long)Co);
  const int64_t total = tvq_fcn_packed_size(Ci, Co, K);
  TVQ_CHECK_ARG(total < ((int64_t)1 << 31), "tvq_fcn_pack_weight_t: Co*Ci*K=%lld too large", (long long)total);
  hipLaunchKernelGGL(fcn_pack_t_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, w, wpt, (int)Co, (int)Ci, (int)K, total);
  return launch_status("tvq_fcn_pack_weight_t");
}

extern "C" int tvq_fcn_conv_dgrad(const float* du, const float* wpt, float* dh, int64_t B,
                                  int64_t Ci, int64_t L, int64_t Co, int64_t K,
                                  tvq_stream_t stream) {
  TVQ_CHECK_ARG(du && wpt && dh, "tvq_fcn_conv_dgrad: null du, wpt or dh");
  if (!fcn_conv_args("tvq_fcn_conv_dgrad", B, Co, L, Ci, K)) return TVQ_ERR_ARG;
  const int nch = (int)((Co + FC_CC - 1) / FC_CC), ntiles = (int)((L + FC_TL - 1) / FC_TL);
  const dim3 grid((unsigned)B, (unsigned)ntiles, (unsigned)((Ci + FC_COT - 1) / FC_COT));
  TVQ_PLAN("fcn_conv_dgrad K=%d padl=%d nch=%d tiles=%d", (int)K, (int)(K - 1 - (K - 1) / 2), nch, ntiles);
  TVQ_FCN_K_SWITCH(K, hipLaunchKernelGGL(
      (fcn_conv_kernel<KK, KK - 1 - (KK - 1) / 2, FC_EP_PLAIN, true, false>), grid, dim3(FC_T), 0,
      (hipStream_t)stream, du, wpt, (const float*)nullptr, (const float*)nullptr, dh,
      (void*)nullptr, (int)Co, (int)L, (int)Ci, nch))
  return launch_status("tvq_fcn_conv_dgrad");
}

extern "C" int64_t tvq_fcn_conv_wgrad_workspace(int64_t B, int64_t Ci, int64_t L, int64_t Co,
                                                int64_t K) {
  if (B < 1 || Ci < 1 || L < 1 || Co < 1 || K < 1 || K > FC_MAXK) return 0;
  const int64_t s = fcn_wgrad_splits(B, Ci, Co, K), n = Co * Ci * K;
  return s * (n + Co) + reduce_rows_scratch(s, n) + reduce_rows_scratch(s, Co);
}

extern "C" int tvq_fcn_conv_wgrad(const float* du, const float* h, float* dw, float* db,
                                  int64_t accumulate, float* workspace, int64_t B, int64_t Ci,
                                  int64_t L, int64_t Co, int64_t K, tvq_stream_t stream) {
  TVQ_CHECK_ARG(du && h && workspace && (dw || db), "tvq_fcn_conv_wgrad: null du, h or workspace, or dw and db both null");
  if (!fcn_conv_args("tvq_fcn_conv_wgrad", B, Ci, L, Co, K)) return TVQ_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int splits = fcn_wgrad_splits(B, Ci, Co, K);
  const int64_t n = Co * Ci * K;
  float* slab_w = workspace;
  float* slab_b = slab_w + (int64_t)splits * n;
  float* scr_w = slab_b + (int64_t)splits * Co;
  float* scr_b = scr_w + reduce_rows_scratch(splits, n);
  TVQ_PLAN("fcn_wgrad K=%d splits=%d cols=%lld", (int)K, splits, (long long)(Ci * K));
  TVQ_FCN_K_SWITCH(K, fcn_wgrad_launch<KK>(du, h, slab_w, db ? slab_b : nullptr, (int)B, (int)Ci,
                                           (int)L, (int)Co, splits, st))
  int rc = launch_status("tvq_fcn_conv_wgrad");
  if (rc != TVQ_OK) return rc;
  if (dw) reduce_rows(slab_w, splits, n, n, dw, nullptr, 0, (int)accumulate, scr_w, st);
  if (db) reduce_rows(slab_b, splits, Co, Co, db, nullptr, 0, (int)accumulate, scr_b, st);
  return launch_status("tvq_fcn_conv_wgrad");
}
