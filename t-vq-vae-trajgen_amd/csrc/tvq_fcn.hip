// Supervised FCN feature extractor (eval) for gfx950: include/tvq_fcn.h.
//
// Reference: FCNBaseline (timevqvae/models/fcn.py:65-101): ConvBlock(Ci,128,8) ->
// ConvBlock(128,256,5) -> ConvBlock(256,128,3), each Conv1dSamePadding -> BatchNorm1d -> ReLU,
// the mean over positions and nn.Linear(128, classes).  The conv engine of tvq_conv*.hip
// pads (K-1)/2 on both sides and has neither a ReLU nor a pooled epilogue, so this is its
// own implicit GEMM.
//
//   fcn_conv_kernel   tvq_fcn_core.h, the core shared with the training kernels; here its
//     FC_EP_EVAL epilogue with the reference's left padding (K-1)/2.
//   fcn_head_kernel   one wave per row: logits by a lane-strided dot and a fixed xor tree,
//     softmax with the row maximum subtracted over the wave's LDS copy of the logits.
#include "../../include/tvq_fcn.h"
#include "tvq_common.h"
#include "tvq_fcn_core.h"

namespace tvq {
namespace {

__global__ __launch_bounds__(256) void fcn_pack_kernel(const float* __restrict__ w,
                                                       float* __restrict__ wp, int Co, int Ci,
                                                       int K, int64_t total) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int S = FC_CC * K / 2, nch = (Ci + FC_CC - 1) / FC_CC;
  const int i = (int)(e & 31), h = (int)((e >> 5) & 1);
  int64_t q = e >> 6;
  const int s = (int)(q % S);
  q /= S;
  const int c = (int)(q % nch), t = (int)(q / nch);
  const int r = 2 * s + h, ci = c * FC_CC + r / K, k = r % K, co = 32 * t + i;
  wp[e] = ci < Ci ? w[((int64_t)co * Ci + ci) * K + k] : 0.f;
}

template <int K>
void fcn_conv_launch(const float* x, const float* wp, const float* scale, const float* shift,
                     float* y, float* gap, int64_t B, int Ci, int L, int Co, hipStream_t st) {
  const int nch = (Ci + FC_CC - 1) / FC_CC, ntiles = (L + FC_TL - 1) / FC_TL;
  const unsigned gz = (unsigned)((Co + FC_COT - 1) / FC_COT);
  TVQ_PLAN("fcn_conv K=%d y=%d gap=%d nch=%d tiles=%d", K, y != nullptr, gap != nullptr, nch, ntiles);
  if (gap && y)
    hipLaunchKernelGGL((fcn_conv_kernel<K, (K - 1) / 2, FC_EP_EVAL, true, true>), dim3((unsigned)B, 1, gz), dim3(FC_T), 0, st,
                       x, wp, scale, shift, y, gap, Ci, L, Co, nch);
  else if (gap)
    hipLaunchKernelGGL((fcn_conv_kernel<K, (K - 1) / 2, FC_EP_EVAL, false, true>), dim3((unsigned)B, 1, gz), dim3(FC_T), 0,
                       st, x, wp, scale, shift, y, gap, Ci, L, Co, nch);
  else
    hipLaunchKernelGGL((fcn_conv_kernel<K, (K - 1) / 2, FC_EP_EVAL, true, false>), dim3((unsigned)B, (unsigned)ntiles, gz),
                       dim3(FC_T), 0, st, x, wp, scale, shift, y, gap, Ci, L, Co, nch);
}

// ---- head --------------------------------------------------------------------------------
constexpr int FH_WAVES = 4;
constexpr int FH_MAXC = 4096;  // 4 waves x 4096 floats = the 64 KiB a block may take

__global__ __launch_bounds__(64 * FH_WAVES) void fcn_head_kernel(
    const float* __restrict__ feat, const float* __restrict__ w, const float* __restrict__ bias,
    float* __restrict__ logits, float* __restrict__ probs, int64_t B, int D, int C) {
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
  if (!live || !probs) return;
  float m = -INFINITY;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, lg[c]);
  m = wave_max(m);
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += expf(lg[c] - m);
  s = wave_sum(s);
  for (int c = lane; c < C; c += 64) probs[row * C + c] = expf(lg[c] - m) / s;
}

}  // namespace
}  // namespace tvq

using namespace tvq;

extern "C" int64_t tvq_fcn_packed_size(int64_t Co, int64_t Ci, int64_t K) {
  if (Co < 1 || Ci < 1 || K < 1) return 0;
  return Co * ((Ci + FC_CC - 1) / FC_CC * FC_CC) * K;
}

extern "C" int tvq_fcn_pack_weight(const float* w, float* wp, int64_t Co, int64_t Ci, int64_t K,
                                   tvq_stream_t stream) {
  TVQ_CHECK_ARG(w && wp, "tvq_fcn_pack_weight: null w or wp");
  TVQ_CHECK_ARG(Co >= 32 && Co % 32 == 0 && Co <= (1 << 20), "tvq_fcn_pack_weight: Co=%lld is not a multiple of 32", (long long)Co);
  TVQ_CHECK_ARG(K >= 1 && K <= FC_MAXK, "tvq_fcn_pack_weight: K=%lld outside [1, 8]", (long long)K);
  TVQ_CHECK_ARG(Ci >= 1 && Ci <= (1 << 20), "tvq_fcn_pack_weight: Ci=%lld outside [1, 2^20]", (long long)Ci);
  const int64_t total = tvq_fcn_packed_size(Co, Ci, K);
  TVQ_CHECK_ARG(total < ((int64_t)1 << 31), "tvq_fcn_pack_weight: Co*Ci*K=%lld too large", (long long)total);
  hipLaunchKernelGGL(fcn_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, w, wp, (int)Co, (int)Ci, (int)K, total);
  return launch_status("tvq_fcn_pack_weight");
}

extern "C" int tvq_fcn_conv_bn_relu(const float* x, const float* wp, const float* scale,
                                    const float* shift, float* y, float* gap, int64_t B, int64_t Ci,
                                    int64_t L, int64_t Co, int64_t K, tvq_stream_t stream) {
  TVQ_CHECK_ARG(x && wp && scale && shift, "tvq_fcn_conv_bn_relu: null x, wp, scale or shift");
  TVQ_CHECK_ARG(y || gap, "tvq_fcn_conv_bn_relu: y and gap are both null");
  TVQ_CHECK_ARG(Co >= 32 && Co % 32 == 0 && Co <= (1 << 20), "tvq_fcn_conv_bn_relu: Co=%lld is not a multiple of 32", (long long)Co);
  TVQ_CHECK_ARG(K >= 1 && K <= FC_MAXK, "tvq_fcn_conv_bn_relu: K=%lld outside [1, 8]", (long long)K);
  TVQ_CHECK_ARG(B >= 1 && B <= 0x7fffffffLL, "tvq_fcn_conv_bn_relu: B=%lld outside [1, 2^31)", (long long)B);
  TVQ_CHECK_ARG(Ci >= 1 && Ci <= (1 << 20), "tvq_fcn_conv_bn_relu: Ci=%lld outside [1, 2^20]", (long long)Ci);
  TVQ_CHECK_ARG(L >= 1 && L <= (1 << 22), "tvq_fcn_conv_bn_relu: L=%lld outside [1, 2^22]", (long long)L);
  TVQ_CHECK_ARG(tvq_fcn_packed_size(Co, Ci, K) < ((int64_t)1 << 31), "tvq_fcn_conv_bn_relu: Co*Ci*K too large");
  hipStream_t st = (hipStream_t)stream;
  switch ((int)K) {
#define TVQ_FCN_CASE(KK)                                                                     \
  case KK:                                                                                   \
    fcn_conv_launch<KK>(x, wp, scale, shift, y, gap, B, (int)Ci, (int)L, (int)Co, st);       \
    break;
    TVQ_FCN_CASE(1) TVQ_FCN_CASE(2) TVQ_FCN_CASE(3) TVQ_FCN_CASE(4)
    TVQ_FCN_CASE(5) TVQ_FCN_CASE(6) TVQ_FCN_CASE(7) TVQ_FCN_CASE(8)
#undef TVQ_FCN_CASE
  }
  return launch_status("tvq_fcn_conv_bn_relu");
}

extern "C" int tvq_fcn_head(const float* feat, const float* w, const float* bias, float* logits,
                            float* probs, int64_t B, int64_t D, int64_t classes,
                            tvq_stream_t stream) {
  TVQ_CHECK_ARG(feat && w && logits, "tvq_fcn_head: null feat, w or logits");
  TVQ_CHECK_ARG(B >= 1 && B <= 0x7fffffffLL, "tvq_fcn_head: B=%lld outside [1, 2^31)", (long long)B);
  TVQ_CHECK_ARG(D >= 1 && D <= (1 << 20), "tvq_fcn_head: D=%lld outside [1, 2^20]", (long long)D);
  TVQ_CHECK_ARG(classes >= 1 && classes <= FH_MAXC, "tvq_fcn_head: classes=%lld outside [1, %d]", (long long)classes, FH_MAXC);
  const int64_t nb = (B + FH_WAVES - 1) / FH_WAVES;
  hipLaunchKernelGGL(fcn_head_kernel, dim3((unsigned)nb), dim3(64 * FH_WAVES),
                     (size_t)(FH_WAVES * classes * sizeof(float)), (hipStream_t)stream, feat, w, bias,
                     logits, probs, B, (int)D, (int)classes);
  return launch_status("tvq_fcn_head");
}
