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

/* ---------------------------------------------------------------- training
 * FCNBaseline in training mode under CrossEntropyLoss (scripts/train_fcn.py:101-168), op by
 * op.  fp32 data, fp64 statistics, workspaces from the *_size / *_workspace queries, no float
 * atomics: every sum has a fixed order that does not depend on the grid's scheduling.
 * Per ConvBlock, n = B L:  u = conv1d_same(h, w) + b;  mean, var = biased batch statistics of
 * u over (b, l);  v = gamma (u - mean) / sqrt(var + eps) + beta;  y = relu(v). */

/* Doubles of the statistics partials of tvq_fcn_conv_train_fwd: 2 Co B ceil(L / 128). */
int64_t tvq_fcn_stats_size(int64_t B, int64_t L, int64_t Co);

/* u[b,co,l] = sum_{ci,k} w[co,ci,k] x[b,ci,l+k-padL] + bias[co] (the eval kernel's sum and
 * padding; a sample's row depends on neither the batch nor the grid), and part [2][Co][B]
 * [ceil(L / 128)]: the fp64 sums of u and of u^2 over each tile of 128 positions.  wp from
 * tvq_fcn_pack_weight.  Shapes as tvq_fcn_conv_bn_relu. */
int tvq_fcn_conv_train_fwd(const float* x, const float* wp, const float* bias, float* u,
                           double* part, int64_t B, int64_t Ci, int64_t L, int64_t Co, int64_t K,
                           tvq_stream_t stream);

/* Adds the P partials per channel of `part` ([2][C][P], P = B ceil(L / 128)) in one fixed
 * order and writes stats [4][C] = mean, rstd = 1 / sqrt(var + eps), scale = gamma rstd, shift
 * = beta - mean scale.  In place, each when non-NULL: running_mean = (1 - momentum)
 * running_mean + momentum mean, running_var likewise with var n / (n - 1),
 * num_batches_tracked += 1.  n = B L >= 2. */
int tvq_fcn_bn_finish(const double* part, int64_t P, int64_t n, const float* gamma,
                      const float* beta, float eps, float momentum, float* running_mean,
                      float* running_var, int64_t* num_batches_tracked, float* stats, int64_t C,
                      tvq_stream_t stream);

/* y = relu(fma(scale, u, shift)) (B,C,L) or NULL; gap[b,c] = mean_l y (or NULL, not both), in
 * the summation order of tvq_fcn_conv_bn_relu's gap (it depends on L only; the same bits with
 * and without y). */
int tvq_fcn_bn_relu(const float* u, const float* stats, float* y, float* gap, int64_t B,
                    int64_t C, int64_t L, tvq_stream_t stream);

/* tvq_fcn_head plus the mean cross-entropy: logits (B,classes); loss (1) = mean_b (logsumexp
 * - logit of target[b]), rows added in a fixed order; dlogits = (softmax - onehot) / B;
 * dfeat = dlogits w (B,D).  One wave per row, the row maximum subtracted.  target int64 in
 * [0, classes) (another value makes the loss NaN).  classes = 1: loss 0, zero gradients.
 * workspace: tvq_fcn_head_ce_workspace(B) floats. */
int64_t tvq_fcn_head_ce_workspace(int64_t B);
int tvq_fcn_head_ce(const float* feat, const float* w, const float* bias, const int64_t* target,
                    float* logits, float* loss, float* dlogits, float* dfeat, float* workspace,
                    int64_t B, int64_t D, int64_t classes, tvq_stream_t stream);

/* dw[c,d] (+)= sum_b dlogits[b,c] feat[b,d], db[c] (+)= sum_b dlogits[b,c], b ascending.
 * dw or db may be NULL. */
int tvq_fcn_head_wgrad(const float* dlogits, const float* feat, float* dw, float* db,
                       int64_t accumulate, int64_t B, int64_t D, int64_t classes,
                       tvq_stream_t stream);

/* Backward of y = relu(v), v = fma(scale, u, shift) with batch statistics.  The upstream
 * gradient is dy (B,C,L), or dfeat (B,C) standing for dy[b,c,l] = dfeat[b,c] / L (the pooled
 * layer); exactly one is non-NULL.  dv = dy where v > 0 (v recomputed as the forward did),
 * dbeta (+)= sum dv, dgamma (+)= sum dv xhat (fp64 sums; each may be NULL),
 * du = scale (dv - dbeta / n - xhat dgamma / n).  workspace: tvq_fcn_bn_bwd_workspace(B, C)
 * doubles. */
int64_t tvq_fcn_bn_bwd_workspace(int64_t B, int64_t C);
int tvq_fcn_bn_relu_bwd(const float* u, const float* dy, const float* dfeat, const float* stats,
                        float* du, float* dgamma, float* dbeta, int64_t accumulate,
                        double* workspace, int64_t B, int64_t C, int64_t L, tvq_stream_t stream);

/* wpt = the data gradient's A operand: wT (Ci, Co, K), wT[ci][co][k] = w[co][ci][K-1-k], in
 * tvq_fcn_pack_weight's order; tvq_fcn_packed_size(Ci, Co, K) floats.  Ci a multiple of 32. */
int tvq_fcn_pack_weight_t(const float* w, float* wpt, int64_t Co, int64_t Ci, int64_t K,
                          tvq_stream_t stream);

/* dh[b,ci,l] = sum_{co,k} w[co,ci,k] du[b,co,l-k+padL]: the conv kernel on wpt with the left
 * padding K-1-padL.  du (B,Co,L), dh (B,Ci,L), Ci a multiple of 32. */
int tvq_fcn_conv_dgrad(const float* du, const float* wpt, float* dh, int64_t B, int64_t Ci,
                       int64_t L, int64_t Co, int64_t K, tvq_stream_t stream);

/* dw[co,ci,k] (+)= sum_{b,l} du[b,co,l] h[b,ci,l+k-padL], db[co] (+)= sum_{b,l} du[b,co,l]
 * (dw or db may be NULL).  Sample splits write slabs that are added in a fixed order.
 * workspace: tvq_fcn_conv_wgrad_workspace floats. */
int64_t tvq_fcn_conv_wgrad_workspace(int64_t B, int64_t Ci, int64_t L, int64_t Co, int64_t K);
int tvq_fcn_conv_wgrad(const float* du, const float* h, float* dw, float* db, int64_t accumulate,
                       float* workspace, int64_t B, int64_t Ci, int64_t L, int64_t Co, int64_t K,
                       tvq_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TVQ_FCN_H */
