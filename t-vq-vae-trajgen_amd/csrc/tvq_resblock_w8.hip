// Fused ResBlock(64, 64) of the LF band on its (B, 64, 3, 8) maps (reference
// vq_vae.py:13-62; the last two encoder and first two decoder ResBlocks of the LF VQ-VAE):
//
//   y = x + Dropout_p(conv2(Snake_a2(BN(conv1(Snake_a1(x)) + b1))) + b2)
//
// The small-channel fused ResBlocks (tvq_resblock.hip) keep the whole 3x3 weight panel in
// LDS; a 64-channel panel is 147 KB, so here the weights stream from L2 as the MFMA A operand
// while the image -- 64 channels x 3 x 8, a 20 KB halo-plane stack -- is staged in LDS once
// per conv.  The scheme, the stage bodies and the host-side builders are
// tvq_resblock_w8_core.h's, shared with the projection blocks (tvq_resblock_w8p.hip); this
// file holds the w8_* kernels and the w8_* entry points tvq_resblock.hip calls.
//
//   w8_fwd1, (bn_stats_final_kernel: 64 one-wave blocks reduce the per-image partials in a
//            fixed order to the batch mean / invstd / affine form and the running
//            statistics), w8_fwd2
//   w8_bwd2, (bn_bwd_final_kernel: those partials -> the BN backward coefficients, the BN
//            weight / bias and Snake a2 gradients), w8_bwd1
// Reducing the 256 images' partials in every consumer block (as the small-channel kernels
// do) read 256 KB of partials per block and held them in 128 VGPRs: 24 us per fwd2 / bwd1
// launch; the one-wave-per-channel finish launch is ~3 us.
//   weight gradients: (s2, g2) and (s1, dh) in one launch of the image-batched
//            conv_wgrad_w8 kernel (a 64 x 577 slab row per image would be 148 KB)
//   w8_eval  both convs in one launch with BN from the running statistics (the frozen
//            encoder of stage2, the LF decoder while sampling)
//   w8_fwd21 / w8_bwd12: two consecutive blocks' adjacent stages in one launch
//
// Replaces, per ResBlock: tvq_snake_fwd, two conv launches, the whole-channel BN kernel, and
// in the backward the dropout, snake and BN kernels and two data-gradient convs.  Arithmetic
// is the per-op kernels' (Snake, BN affine / backward formulas, the dropout hash at the flat
// NCHW index) up to the summation order, which is fixed.
#include "tvq_resblock_w8.h"

#include "tvq_resblock_w8_core.h"

namespace tvq {
namespace w8 {

constexpr int C = 64;  // the identity block

__global__ __launch_bounds__(T) void w8_fwd1_kernel(Args a) {
  extern __shared__ float sm[];
  float wa[9][8];
  fwd1_body<C, C>(a, sm, wa, nullptr);
}

__global__ __launch_bounds__(T) void w8_fwd2_kernel(Args a) {
  extern __shared__ float sm[];
  float wa[9][8], y[4];
  fwd2_body<C, C>(a, sm, wa, y, nullptr);
}

// fwd2 of ResBlock 1 and fwd1 of ResBlock 2 (its input = ResBlock 1's output) in one launch
__global__ __launch_bounds__(T) void w8_fwd21_kernel(Args a1, Args a2) {
  extern __shared__ float sm[];
  float wa[9][8], y[4];
  fwd2_body<C, C>(a1, sm, wa, y, &a2.w1);
  __syncthreads();  // LDS reused
  fwd1_body<C, C>(a2, sm, wa, &y);
}

__global__ __launch_bounds__(T) void w8_eval_kernel(Args a) {
  extern __shared__ float sm[];
  eval_body<C, C>(a, sm);
}

__global__ __launch_bounds__(T) void w8_bwd2_kernel(Args a) {
  extern __shared__ float sm[];
  float wa[9][8];
  bwd2_body<C, C>(a, sm, wa, nullptr);
}

__global__ __launch_bounds__(T) void w8_bwd1_kernel(Args a) {
  extern __shared__ float sm[];
  float wa[9][8], dx[4];
  bwd1_body<C, C>(a, sm, wa, dx, nullptr);
}

// bwd1 of ResBlock 2 and bwd2 of ResBlock 1 (its output gradient = ResBlock 2's input
// gradient) in one launch
__global__ __launch_bounds__(T) void w8_bwd12_kernel(Args a2, Args a1) {
  extern __shared__ float sm[];
  float wa[9][8], d[4];
  bwd1_body<C, C>(a2, sm, wa, d, &a1.w2);
  __syncthreads();  // LDS reused
  bwd2_body<C, C>(a1, sm, wa, &d);
}

static void set_lds() {
  static bool done = false;
  if (done) return;
  for (const void* k :
       {(const void*)&w8_fwd1_kernel, (const void*)&w8_fwd2_kernel, (const void*)&w8_eval_kernel,
        (const void*)&w8_bwd2_kernel, (const void*)&w8_bwd1_kernel, (const void*)&w8_fwd21_kernel,
        (const void*)&w8_bwd12_kernel})
    (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds_bytes<C, C>());
  done = true;
}

}  // namespace w8

using namespace w8;

bool w8_supported(int64_t B, int64_t C, int64_t H, int64_t W) {
  return C == w8::C && H == 3 && W == w8::W && B >= 1 && B * C * 3 * W < (1ll << 31);
}
int64_t w8_workspace(int64_t B) { return (int64_t)ws_layout(B, C, C).total; }
int64_t w8_saved_floats(int64_t B) { return 3 * B * C * P; }  // h | s1 | s2

int w8_train_fwd(const float* x, int64_t B, const float* a1, const float* w1, const float* b1,
                 const float* bn_w, const float* bn_b, float* running_mean, float* running_var,
                 int64_t* nbt, float momentum, float eps, const float* a2, const float* w2,
                 const float* b2, float drop_p, const int64_t* seed_ptr, uint64_t offset,
                 float* saved, float* y, float* save, void* workspace, hipStream_t st) {
  set_lds();
  const float* p[8] = {a1, w1, b1, bn_w, bn_b, a2, w2, b2};
  float* rs[2] = {running_mean, running_var};
  Fwd f = fwd_args(C, C, x, B, p, rs, nbt, momentum, eps, drop_p, seed_ptr, offset, saved, y, save,
                   workspace, st);
  TVQ_PLAN("w8_fwd1 C%d W%d B%lld", C, W, (long long)B);
  f.a.s_out = f.s1;
  launch<C, C>(w8_fwd1_kernel, B, st, f.a);
  bn_stats_final_launch(f.a.part, f.fin, st);
  TVQ_PLAN("w8_fwd2 C%d W%d B%lld", C, W, (long long)B);
  f.a.s_out = f.s2;
  launch<C, C>(w8_fwd2_kernel, B, st, f.a);
  return launch_status("tvq_resblock_train_fwd");
}

int w8_eval_fwd(const float* x, int64_t B, const float* a1, const float* w1, const float* b1,
                const float* bn_w, const float* bn_b, const float* running_mean,
                const float* running_var, float eps, const float* a2, const float* w2,
                const float* b2, float* y, hipStream_t st) {
  set_lds();
  const float* p[8] = {a1, w1, b1, bn_w, bn_b, a2, w2, b2};
  const Args a = eval_args(C, C, x, B, p, running_mean, running_var, eps, y, st);
  TVQ_PLAN("w8_eval C%d W%d B%lld packed=%d", C, W, (long long)B, (int)(a.w1.sn == 1));
  launch<C, C>(w8_eval_kernel, B, st, a);
  return launch_status("tvq_resblock_eval_fwd");
}

int w8_bwd(const float* dy, const float* x, const float* saved, int64_t B, const float* a1,
           const float* w1, const float* bn_w, const float* save, const float* a2,
           const float* w2, float drop_p, const int64_t* seed_ptr, uint64_t offset, float* dx,
           float* da1, float* dw1, float* db1, float* dbn_w, float* dbn_b, float* da2, float* dw2,
           float* db2, int64_t accumulate, void* workspace, hipStream_t st) {
  set_lds();
  const float* q[6] = {a1, w1, bn_w, save, a2, w2};
  float* g[8] = {da1, dw1, db1, dbn_w, dbn_b, da2, dw2, db2};
  Bwd b = bwd_args(C, C, dy, x, saved, B, q, drop_p, seed_ptr, offset, dx, g, accumulate,
                   workspace, st);
  TVQ_PLAN("w8_bwd2 C%d W%d B%lld", C, W, (long long)B);
  b.a.g_out = b.g2;
  launch<C, C>(w8_bwd2_kernel, B, st, b.a);
  int rc = launch_status("tvq_resblock_bwd");
  if (rc) return rc;
  bn_bwd_final_launch(b.a.part, b.bfin, st);
  TVQ_PLAN("w8_bwd1 C%d W%d B%lld", C, W, (long long)B);
  b.a.g_out = b.dh;
  launch<C, C>(w8_bwd1_kernel, B, st, b.a);
  rc = launch_status("tvq_resblock_bwd");
  if (rc) return rc;
  rc = wgrad_3x3(b, C, C, g, accumulate, st);
  if (rc) return rc;
  da1_finish(b, C, da1, accumulate, st);
  return launch_status("tvq_resblock_bwd");
}

// Two consecutive ResBlock(64, 64)s (tvq_resblock_pair_train_fwd / _bwd): 5 launches forward
// instead of 6 (w8_fwd21 = block 1's fwd2 + block 2's fwd1), 4 + weight gradients backward
// instead of 5.
int w8_pair_train_fwd(const float* x, int64_t B, const float* const* p1, const float* const* p2,
                      float* const* rs1, float* const* rs2, int64_t* nbt1, int64_t* nbt2,
                      float momentum, float eps, float drop_p, const int64_t* seed_ptr,
                      uint64_t off1, uint64_t off2, float* saved1, float* y1, float* save1,
                      float* saved2, float* y2, float* save2, void* ws1, void* ws2,
                      hipStream_t st) {
  set_lds();
  Fwd f1 = fwd_args(C, C, x, B, p1, rs1, nbt1, momentum, eps, drop_p, seed_ptr, off1, saved1, y1,
                    save1, ws1, st);
  Fwd f2 = fwd_args(C, C, y1, B, p2, rs2, nbt2, momentum, eps, drop_p, seed_ptr, off2, saved2, y2,
                    save2, ws2, st);
  TVQ_PLAN("w8_fwd1 C%d W%d B%lld", C, W, (long long)B);
  f1.a.s_out = f1.s1;
  launch<C, C>(w8_fwd1_kernel, B, st, f1.a);
  bn_stats_final_launch(f1.a.part, f1.fin, st);
  TVQ_PLAN("w8_fwd21 C%d W%d B%lld", C, W, (long long)B);
  f1.a.s_out = f1.s2;
  f2.a.s_out = f2.s1;
  launch<C, C>(w8_fwd21_kernel, B, st, f1.a, f2.a);
  bn_stats_final_launch(f2.a.part, f2.fin, st);
  TVQ_PLAN("w8_fwd2 C%d W%d B%lld", C, W, (long long)B);
  f2.a.s_out = f2.s2;
  launch<C, C>(w8_fwd2_kernel, B, st, f2.a);
  return launch_status("tvq_resblock_pair_train_fwd");
}

int w8_pair_bwd(const float* dy, const float* x, int64_t B, const float* const* q1,
                const float* const* q2, const float* saved1, const float* y1,
                const float* saved2, float drop_p, const int64_t* seed_ptr, uint64_t off1,
                uint64_t off2, float* dx, float* dy1, float* const* g1, float* const* g2,
                int64_t accumulate, void* ws1, void* ws2, hipStream_t st) {
  set_lds();
  // block 2 runs first
  Bwd b2 = bwd_args(C, C, dy, y1, saved2, B, q2, drop_p, seed_ptr, off2, dy1, g2, accumulate, ws2,
                    st);
  Bwd b1 = bwd_args(C, C, dy1, x, saved1, B, q1, drop_p, seed_ptr, off1, dx, g1, accumulate, ws1,
                    st);
  TVQ_PLAN("w8_bwd2 C%d W%d B%lld", C, W, (long long)B);
  b2.a.g_out = b2.g2;
  launch<C, C>(w8_bwd2_kernel, B, st, b2.a);
  int rc = launch_status("tvq_resblock_pair_bwd");
  if (rc) return rc;
  bn_bwd_final_launch(b2.a.part, b2.bfin, st);
  TVQ_PLAN("w8_bwd12 C%d W%d B%lld", C, W, (long long)B);
  b2.a.g_out = b2.dh;
  b1.a.g_out = b1.g2;
  launch<C, C>(w8_bwd12_kernel, B, st, b2.a, b1.a);
  rc = launch_status("tvq_resblock_pair_bwd");
  if (rc) return rc;
  bn_bwd_final_launch(b1.a.part, b1.bfin, st);
  TVQ_PLAN("w8_bwd1 C%d W%d B%lld", C, W, (long long)B);
  b1.a.g_out = b1.dh;
  launch<C, C>(w8_bwd1_kernel, B, st, b1.a);
  rc = launch_status("tvq_resblock_pair_bwd");
  if (rc) return rc;
  const Bwd* bs[2] = {&b2, &b1};
  float* const* gs[2] = {g2, g1};
  if (conv_wgrad_w8_fits(W, B, C, C)) {  // the pair's four weight gradients in one launch
    const float* xs[4];
    const float* dys[4];
    float* wsl[4];
    float* dw[4];
    float* db[4];
    for (int i = 0; i < 2; ++i) {
      const Bwd& b = *bs[i];
      xs[2 * i] = b.s2; dys[2 * i] = b.g2; wsl[2 * i] = b.wg2;  // conv2: (s2, g2)
      dw[2 * i] = gs[i][6]; db[2 * i] = gs[i][7];
      xs[2 * i + 1] = b.s1; dys[2 * i + 1] = b.dh; wsl[2 * i + 1] = b.wg1;  // conv1: (s1, dh)
      dw[2 * i + 1] = gs[i][1]; db[2 * i + 1] = gs[i][2];
    }
    conv_wgrad_w8_multi(W, 4, xs, dys, wsl, dw, db, B, C, C, (int)accumulate, st);
    for (int i = 0; i < 2; ++i) da1_finish(*bs[i], C, gs[i][0], accumulate, st);
    return launch_status("tvq_resblock_pair_bwd");
  }
  for (int i = 0; i < 2; ++i) {
    rc = wgrad_3x3(*bs[i], C, C, gs[i], accumulate, st);
    if (rc) return rc;
    da1_finish(*bs[i], C, gs[i][0], accumulate, st);
  }
  return launch_status("tvq_resblock_pair_bwd");
}

}  // namespace tvq
