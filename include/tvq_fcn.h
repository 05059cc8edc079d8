/* tvq_fcn.h — the supervised FCN feature extractor of libtvq_hip.so (gfx950).
 *
 * Second public header of the library (include/tvq.h is the first; its conventions hold
 * here: raw device pointers, fp32 data, asynchronous on `stream`, no allocation, 0 or a
 * negative status with tvq_last_error()).
 *
 * Reference: FCNBaseline.forward (timevqvae/models/fcn.py:65-101) in eval mode: three
 * ConvBlocks (Conv1dSamePadding -> BatchNorm1d -> ReLU, fcn.py:11-62), the mean over
 * positions, and the final Linear.  One tvq_fcn_conv_bn_relu launch per ConvBlock (the third
 * with y == NULL: only the pooled features leave the kernel), then tvq_fcn_head.
 */
#ifndef TVQ_FCN_H
#define TVQ_FCN_H
#include "tvq.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Floats of the packed form of a (Co, Ci, K) weight: Co * roundup(Ci, 8) * K. */
int64_t tvq_fcn_packed_size(int64_t Co, int64_t Ci, int64_t K);

/* wp = the weight w (Co, Ci, K) in the order the conv kernel's matrix-core A operand reads
 * it: [Co / 32][chunk of 8 input channels][step s][half h][row i] = w[32 t + i][r], with
 * r = 2 s + h the flat (channel, tap) index inside the chunk; channels past Ci are zeros
 * (the reduction is padded to the MFMA's k step).  Co a multiple of 32, 1 <= K <= 8. */
int tvq_fcn_pack_weight(const float* w, float* wp, int64_t Co, int64_t Ci, int64_t K,
                        tvq_stream_t stream);

/* y[b,co,l] = relu(scale[co] * sum_{ci,k} w[co,ci,k] * x[b,ci,l+k-padL] + shift[co]) with
 * padL = (K-1)/2 rounded down and zeros outside [0, L): conv1d_same_padding (stride 1,
 * dilation 1; K = 8 pads 3 left, 4 right), eval BatchNorm1d folded into scale / shift, ReLU.
 * gap[b,co] = mean_l y[b,co,l], summed in an order that depends on L only (not on B, not on
 * whether y is written); no float atomics.  x (B,Ci,L), wp from tvq_fcn_pack_weight, y
 * (B,Co,L) or NULL, gap (B,Co) or NULL, not both NULL.  B, L, Ci >= 1, 1 <= K <= 8, Co a
 * multiple of 32. */
int tvq_fcn_conv_bn_relu(const float* x, const float* wp, const float* scale,
                         const float* shift, float* y, float* gap, int64_t B, int64_t Ci,
                         int64_t L, int64_t Co, int64_t K, tvq_stream_t stream);

/* logits[b,c] = sum_d feat[b,d] * w[c,d] + bias[c] (nn.Linear, fcn.py:93,101); probs (or
 * NULL) = softmax over c with the row maximum subtracted.  One wave per row, fixed order.
 * feat (B,D), w (classes,D), bias (classes) or NULL, 1 <= classes <= 4096. */
int tvq_fcn_head(const float* feat, const float* w, const float* bias, float* logits,
                 float* probs, int64_t B, int64_t D, int64_t classes, tvq_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TVQ_FCN_H */
