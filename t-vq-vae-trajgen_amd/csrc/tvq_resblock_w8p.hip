// The projection ResBlocks of the LF band's W = 8 maps (reference vq_vae.py:13-62 with
// in_channels != out_channels): the encoder's last block ResBlock(64, 128) and the decoder's
// first ResBlock(128, 64), both on (B, C, 3, 8) images,
//
//   y = proj(x) + Dropout_p(conv2(Snake_a2(BN(conv1(Snake_a1(x)) + b1))) + b2),
//   proj = the 1x1 Conv2d(Ci, Co) on the raw input.
//
// The scheme, the stage bodies and the host-side builders are tvq_resblock_w8_core.h's (shared
// with the identity block, tvq_resblock_w8.hip, whose header describes the launches); this
// file holds the w8p_*<CI, CO> kernels and the tvq_resblock_proj_* entry points.  The three
// weight gradients: conv2 (s2, g2) and conv1 (s1, dh) by the image-batched conv_wgrad_w8
// kernel, proj (x, dy) by the 1x1 weight-gradient path.
#include "tvq_resblock_w8_core.h"

namespace tvq {
namespace w8 {

template <int CI, int CO>
__global__ __launch_bounds__(T) void w8p_fwd1_kernel(Args a) {
  extern __shared__ float sm[];
  float wa[9][8];
  fwd1_body<CI, CO>(a, sm, wa, nullptr);
}

template <int CI, int CO>
__global__ __launch_bounds__(T) void w8p_fwd2_kernel(Args a) {
  extern __shared__ float sm[];
  float wa[9][8], y[CO / 16];
  fwd2_body<CI, CO>(a, sm, wa, y, nullptr);
}

template <int CI, int CO>
__global__ __launch_bounds__(T) void w8p_eval_kernel(Args a) {
  extern __shared__ float sm[];
  eval_body<CI, CO>(a, sm);
}

template <int CI, int CO>
__global__ __launch_bounds__(T) void w8p_bwd2_kernel(Args a) {
  extern __shared__ float sm[];
  float wa[9][8];
  bwd2_body<CI, CO>(a, sm, wa, nullptr);
}

template <int CI, int CO>
__global__ __launch_bounds__(T) void w8p_bwd1_kernel(Args a) {
  extern __shared__ float sm[];
  float wa[9][8], dx[CI / 16];
  bwd1_body<CI, CO>(a, sm, wa, dx, nullptr);
}

template <int CI, int CO>
static void set_lds() {
  static bool done = false;
  if (done) return;
  for (const void* k : {(const void*)&w8p_fwd1_kernel<CI, CO>, (const void*)&w8p_fwd2_kernel<CI, CO>,
                        (const void*)&w8p_eval_kernel<CI, CO>, (const void*)&w8p_bwd2_kernel<CI, CO>,
                        (const void*)&w8p_bwd1_kernel<CI, CO>})
    (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds_bytes<CI, CO>());
  done = true;
}

static bool proj_shape_ok(int64_t B, int64_t CI, int64_t CO, int64_t H, int64_t Wd) {
  return H == 3 && Wd == W && B >= 1 && ((CI == 64 && CO == 128) || (CI == 128 && CO == 64)) &&
         B * 128 * P < (1ll << 31);
}

// the body (variadic: it holds commas) for the two instantiated projection shapes
#define W8P_DISPATCH(CI_, CO_, ...)             \
  if ((CI_) == 64 && (CO_) == 128) {           \
    constexpr int CI = 64, CO = 128;           \
    __VA_ARGS__                                \
  } else {                                     \
    constexpr int CI = 128, CO = 64;           \
    __VA_ARGS__                                \
  }

}  // namespace w8
}  // namespace tvq

using namespace tvq;
using namespace tvq::w8;

extern "C" int64_t tvq_resblock_proj_workspace(int64_t B, int64_t Ci, int64_t Co, int64_t H,
                                               int64_t Wd) {
  if (!proj_shape_ok(B, Ci, Co, H, Wd)) return 0;
  return (int64_t)ws_layout(B, Ci, Co).total;
}

extern "C" int64_t tvq_resblock_proj_saved_floats(int64_t B, int64_t Ci, int64_t Co, int64_t H,
                                                  int64_t Wd) {
  if (!proj_shape_ok(B, Ci, Co, H, Wd)) return 0;
  return B * P * (2 * Co + Ci);  // h | s1 | s2
}

extern "C" int tvq_resblock_proj_train_fwd(
    const float* x, int64_t B, int64_t Ci, int64_t Co, int64_t H, int64_t Wd, const float* a1,
    const float* w1, const float* b1, const float* bn_w, const float* bn_b, float* running_mean,
    float* running_var, int64_t* nbt, float momentum, float eps, const float* a2, const float* w2,
    const float* b2, const float* wp, const float* bp, float drop_p, const int64_t* seed_ptr,
    uint64_t offset, float* saved, float* y, float* save, void* workspace, tvq_stream_t stream) {
  TVQ_CHECK_ARG(proj_shape_ok(B, Ci, Co, H, Wd), "tvq_resblock_proj_train_fwd: unsupported shape");
  TVQ_CHECK_ARG(x && a1 && w1 && b1 && running_mean && running_var && a2 && w2 && b2 && wp && bp &&
                    saved && y && save && workspace && (drop_p == 0.f || seed_ptr),
                "tvq_resblock_proj_train_fwd: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  const float* p[10] = {a1, w1, b1, bn_w, bn_b, a2, w2, b2, wp, bp};
  float* rs[2] = {running_mean, running_var};
  Fwd f = fwd_args(Ci, Co, x, B, p, rs, nbt, momentum, eps, drop_p, seed_ptr, offset, saved, y,
                   save, workspace, st);
  TVQ_PLAN("w8p_fwd Ci%lld Co%lld B%lld packed=%d", (long long)Ci, (long long)Co, (long long)B,
           (int)(f.a.w1.sn == 1));
  W8P_DISPATCH(Ci, Co, {
    set_lds<CI, CO>();
    f.a.s_out = f.s1;
    launch<CI, CO>(w8p_fwd1_kernel<CI, CO>, B, st, f.a);
    bn_stats_final_launch(f.a.part, f.fin, st);
    f.a.s_out = f.s2;
    launch<CI, CO>(w8p_fwd2_kernel<CI, CO>, B, st, f.a);
  })
  return launch_status("tvq_resblock_proj_train_fwd");
}

extern "C" int tvq_resblock_proj_eval_fwd(const float* x, int64_t B, int64_t Ci, int64_t Co,
                                          int64_t H, int64_t Wd, const float* a1, const float* w1,
                                          const float* b1, const float* bn_w, const float* bn_b,
                                          const float* running_mean, const float* running_var,
                                          float eps, const float* a2, const float* w2,
                                          const float* b2, const float* wp, const float* bp,
                                          float* y, tvq_stream_t stream) {
  TVQ_CHECK_ARG(proj_shape_ok(B, Ci, Co, H, Wd), "tvq_resblock_proj_eval_fwd: unsupported shape");
  TVQ_CHECK_ARG(x && a1 && w1 && b1 && running_mean && running_var && a2 && w2 && b2 && wp && bp &&
                    y, "tvq_resblock_proj_eval_fwd: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  const float* p[10] = {a1, w1, b1, bn_w, bn_b, a2, w2, b2, wp, bp};
  const Args a = eval_args(Ci, Co, x, B, p, running_mean, running_var, eps, y, st);
  TVQ_PLAN("w8p_eval Ci%lld Co%lld B%lld packed=%d", (long long)Ci, (long long)Co, (long long)B,
           (int)(a.w1.sn == 1));
  W8P_DISPATCH(Ci, Co, {
    set_lds<CI, CO>();
    launch<CI, CO>(w8p_eval_kernel<CI, CO>, B, st, a);
  })
  return launch_status("tvq_resblock_proj_eval_fwd");
}

extern "C" int tvq_resblock_proj_bwd(
    const float* dy, const float* x, const float* saved, int64_t B, int64_t Ci, int64_t Co,
    int64_t H, int64_t Wd, const float* a1, const float* w1, const float* bn_w, const float* save,
    const float* a2, const float* w2, const float* wp, float drop_p, const int64_t* seed_ptr,
    uint64_t offset, float* dx, float* da1, float* dw1, float* db1, float* dbn_w, float* dbn_b,
    float* da2, float* dw2, float* db2, float* dwp, float* dbp, int64_t accumulate,
    void* workspace, tvq_stream_t stream) {
  TVQ_CHECK_ARG(proj_shape_ok(B, Ci, Co, H, Wd), "tvq_resblock_proj_bwd: unsupported shape");
  TVQ_CHECK_ARG(dy && x && saved && a1 && w1 && save && a2 && w2 && wp && dx && da1 && dw1 &&
                    db1 && da2 && dw2 && db2 && dwp && dbp && workspace &&
                    (drop_p == 0.f || seed_ptr),
                "tvq_resblock_proj_bwd: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  const float* q[7] = {a1, w1, bn_w, save, a2, w2, wp};
  float* g[10] = {da1, dw1, db1, dbn_w, dbn_b, da2, dw2, db2, dwp, dbp};
  Bwd b = bwd_args(Ci, Co, dy, x, saved, B, q, drop_p, seed_ptr, offset, dx, g, accumulate,
                   workspace, st);
  TVQ_PLAN("w8p_bwd Ci%lld Co%lld B%lld", (long long)Ci, (long long)Co, (long long)B);
  W8P_DISPATCH(Ci, Co, {
    set_lds<CI, CO>();
    b.a.g_out = b.g2;
    launch<CI, CO>(w8p_bwd2_kernel<CI, CO>, B, st, b.a);
    bn_bwd_final_launch(b.a.part, b.bfin, st);
    b.a.g_out = b.dh;
    launch<CI, CO>(w8p_bwd1_kernel<CI, CO>, B, st, b.a);
  })
  int rc = launch_status("tvq_resblock_proj_bwd");
  if (rc) return rc;
  // weight gradients: conv2 (s2, g2), conv1 (s1, dh), proj (x, dy)
  rc = wgrad_3x3(b, Ci, Co, g, accumulate, st);
  if (rc) return rc;
  rc = tvq_conv2d_wgrad(x, B, Ci, 3, W, dy, Co, W, 1, 1, 1, 0, dwp, dbp, accumulate, b.wgp, st);
  if (rc) return rc;
  da1_finish(b, Ci, da1, accumulate, st);
  return launch_status("tvq_resblock_proj_bwd");
}
