// Implicit-GEMM convolutions over the (B, C, H, W) STFT image (H = 3, or 1 for
// Conv1d) on gfx950 fp32 MFMA (exact fp32 FMA chains): the forward / data-gradient entry
// points of the conv engine and the dispatcher that picks a kernel family for each launch.
// The gather forms, the shared types and the family files are listed in tvq_conv_core.h.
#include "tvq_conv_core.h"

namespace tvq {

static ConvConfig g_conv_cfg;
const ConvConfig& conv_config() { return g_conv_cfg; }

// Fold the gradient of a replicate-padded input (B,C,H+2PH,W+2PW) onto (B,C,H,W).
__global__ void replicate_fold_kernel(const float* __restrict__ dpad, int B, int C, int H, int W,
                                      int PH, int PW, float* __restrict__ dx) {
  const int Hp = H + 2 * PH, Wp = W + 2 * PW;
  const int64_t tot = (int64_t)B * C * H * W;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < tot;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int w = (int)(i % W);
    const int64_t t = i / W;
    const int h = (int)(t % H);
    const int64_t bc = t / H;
    const float* p = dpad + bc * Hp * Wp;
    const int hlo = h == 0 ? 0 : h + PH, hhi = h == H - 1 ? Hp - 1 : h + PH;
    const int wlo = w == 0 ? 0 : w + PW, whi = w == W - 1 ? Wp - 1 : w + PW;
    float s = 0.f;
    for (int hh = hlo; hh <= hhi; ++hh)
      for (int ww = wlo; ww <= whi; ++ww) s += p[hh * Wp + ww];
    dx[i] = s;
  }
}

// staged GEMM; `slab` (nullable) enables split-K with splits*N*Mpos floats of partials.
// Returns whether the path applied e's eval BN / Snake.
static bool launch_gemm(int mode, int kind, bool repl, const float* in, const float* wt,
                        float* out, const ConvGeom& g, const Epi& e, float* slab, hipStream_t st) {
  if (g.C % 16 != 0) {  // small channel counts: flat (c, kh, kw) K order
    launch_gemm_flat(mode, kind, repl, in, wt, out, g, e, st);
    return false;
  }
  bool post;
  if (launch_t32(mode, kind, repl, in, wt, out, g, e, st, &post)) return post;
  if (launch_d32(mode, kind, repl, in, wt, out, g, e, st)) {
    TVQ_PLAN("conv_d32");
    return e.bn_rv != nullptr;  // conv_d32_kernel's epilogue applies it
  }
  return launch_tap(mode, kind, repl, in, wt, out, g, e, slab, st);
}

// One F / T gather launch of a kind_of() kernel shape with KK = KH*KW taps: the stride-2,
// direct, few-output and halo kernels where the shape is theirs, else the staged GEMM.
// workspace (nullable) = [packed weight N*C*KK][split-K slab]; see conv_gemm_ws.
// Returns whether the path's epilogue applied e's eval BN / Snake (the *_bn_eval entry points
// run the standalone eval BN after a path that did not).
static bool launch_conv(int mode, int kind, bool repl, int KK, const float* in, const float* wt,
                        float* out, ConvGeom g, float* ws, const Epi& e, hipStream_t st) {
  if (kind == 0) {
    const int k2 = s2_kind(mode, g);
    if (k2) {
      launch_s2(k2, repl, in, wt, out, g, e, st);
      return e.bn_rv != nullptr;
    }
    if (mode == GATHER_T && !repl && s2m_t_fits(g, e)) {
      if (ws) wt = pack_weight(wt, g, KK, ws, st);
      launch_s2m_t(false, in, wt, e.bias, out, g, st);
      return false;
    }
  }
  if (launch_small(mode, kind, repl, in, wt, out, g, e, st)) return false;
  if (ws && n16_geom_ok(mode, kind, g)) {
    wt = pack_weight(wt, g, KK, ws, st);  // [tap][c][n]
    launch_n16(mode, kind, in, wt, out, g, e, st);
    return e.bn_rv != nullptr;
  }
  bool post;
  if (launch_halo(mode, kind, repl, in, wt, out, g, e, st, &post)) return post;
  float* slab = nullptr;
  if (ws && g.C % 16 == 0) {
    wt = pack_weight(wt, g, KK, ws, st);
    slab = ws + (int64_t)g.N * g.C * KK;
  }
  return launch_gemm(mode, kind, repl, in, wt, out, g, e, slab, st);
}

}  // namespace tvq

using namespace tvq;

static Epi make_epi(const float* bias, const float* residual, float drop_p,
                    const int64_t* seed_ptr, uint64_t offset) {
  Epi e = {};
  e.bias = bias;
  e.residual = residual;
  e.drop_p = drop_p;
  e.drop_scale = drop_p > 0.f ? 1.0f / (1.0f - drop_p) : 1.0f;
  e.seed_ptr = seed_ptr;
  e.offset = offset;
  return e;
}

extern "C" int tvq_conv_config(int64_t bits) {
  ConvConfig& c = g_conv_cfg;
  const int prev = c.halo | (c.t32 ? 0 : 8) | (c.s2 ? 0 : 512) | (c.ws2 ? 0 : 1024) |
                   (c.s2m ? 0 : 4096);
  if (bits >= 0) {
    const int64_t unknown = bits & ~(int64_t)(7 | 8 | 512 | 1024 | 4096);
    TVQ_CHECK_ARG(unknown == 0, "tvq_conv_config: unknown bit %lld",
                  (long long)(unknown & -unknown));
    c.halo = (int)(bits & 7);
    c.t32 = (bits & 8) ? 0 : 1;
    c.s2 = (bits & 512) ? 0 : 1;
    c.ws2 = (bits & 1024) ? 0 : 1;
    c.s2m = (bits & 4096) ? 0 : 1;
  }
  return prev;
}

extern "C" int tvq_conv_s2_cap(int64_t cap) {
  const int prev = g_conv_cfg.s2_cap;
  if (cap >= 0) g_conv_cfg.s2_cap = cap > (1 << 30) ? (1 << 30) : (int)cap;
  return prev;
}

extern "C" int tvq_conv_out_width(int64_t Win, int64_t KW, int64_t SW, int64_t transposed) {
  const int64_t PW = (KW - 1) / 2;
  return (int)(transposed ? (Win - 1) * SW - 2 * PW + KW : (Win + 2 * PW - KW) / SW + 1);
}

// ---- geometry of each op as one F/T gather launch
static ConvGeom geom_conv_fwd(int64_t B, int64_t Ci, int64_t H, int64_t Wi, int64_t Co, int64_t KH,
                              int64_t KW, int64_t SW) {
  const int Wo = tvq_conv_out_width(Wi, KW, SW, 0);
  return make_geom((int)B, (int)Ci, (int)H, (int)Wi, (int)Co, (int)H, Wo, (int)KH, (int)KW,
                   PH_OF(KH), PW_OF(KW), Ci * KH * KW, KH * KW);
}
// ConvTranspose2d weight (Ci, Co, KH, KW): reduction channel c = ci (first dim)
static ConvGeom geom_convT_fwd(int64_t B, int64_t Ci, int64_t H, int64_t Wi, int64_t Co,
                               int64_t KH, int64_t KW, int64_t SW) {
  const int Wo = tvq_conv_out_width(Wi, KW, SW, 1);
  return make_geom((int)B, (int)Ci, (int)H, (int)Wi, (int)Co, (int)H, Wo, (int)KH, (int)KW,
                   PH_OF(KH), PW_OF(KW), KH * KW, Co * KH * KW);
}
// conv weight (Co, Ci, KH, KW): reduction c = co, output channel n = ci.  Replicate pad:
// gradient of the padded canvas (H+2PH, Wi+2PW) with zero offsets, folded afterwards.
static ConvGeom geom_conv_dgrad(int64_t B, int64_t Ci, int64_t H, int64_t Wi, int64_t Co,
                                int64_t KH, int64_t KW, int64_t SW, int64_t replicate) {
  const int Wo = tvq_conv_out_width(Wi, KW, SW, 0);
  if (!replicate)
    return make_geom((int)B, (int)Co, (int)H, Wo, (int)Ci, (int)H, (int)Wi, (int)KH, (int)KW,
                     PH_OF(KH), PW_OF(KW), KH * KW, Ci * KH * KW);
  return make_geom((int)B, (int)Co, (int)H, Wo, (int)Ci, (int)H + 2 * PH_OF(KH),
                   (int)Wi + 2 * PW_OF(KW), (int)KH, (int)KW, 0, 0, KH * KW, Ci * KH * KW);
}
// F-gather of dY with weight (Ci, Co, KH, KW) indexed (n = ci, c = co)
static ConvGeom geom_convT_dgrad(int64_t B, int64_t Ci, int64_t H, int64_t Wi, int64_t Co,
                                 int64_t KH, int64_t KW, int64_t SW) {
  const int Wo = tvq_conv_out_width(Wi, KW, SW, 1);
  return make_geom((int)B, (int)Co, (int)H, Wo, (int)Ci, (int)H, (int)Wi, (int)KH, (int)KW,
                   PH_OF(KH), PW_OF(KW), Co * KH * KW, KH * KW);
}

static int64_t canvas_floats(const ConvGeom& g) { return (int64_t)g.B * g.N * g.Hout * g.Wo; }

static bool geom_ok(const ConvGeom& g) {
  return g.Wo > 0 && g.Win > 0 && (int64_t)g.B * g.Hout * g.Wo < (1 << 30) &&
         (int64_t)g.B * g.N * g.Hout * g.Wo < (1ll << 31);
}

extern "C" int tvq_conv2d_fwd(const float* x, int64_t B, int64_t Ci, int64_t H, int64_t Wi,
                              const float* w, const float* bias, int64_t Co, int64_t KH,
                              int64_t KW, int64_t SW, int64_t replicate, float* y,
                              const float* residual, float drop_p, const int64_t* seed_ptr,
                              uint64_t offset, float* workspace, tvq_stream_t stream) {
  TVQ_CHECK_ARG(x && w && y && B > 0 && Ci > 0 && Co > 0, "tvq_conv2d_fwd: bad arguments");
  const int kind = kind_of((int)KH, (int)KW, (int)SW);
  TVQ_CHECK_ARG(kind >= 0, "tvq_conv2d_fwd: unsupported kernel %lldx%lld s%lld", (long long)KH,
                (long long)KW, (long long)SW);
  ConvGeom g = geom_conv_fwd(B, Ci, H, Wi, Co, KH, KW, SW);
  TVQ_CHECK_ARG(geom_ok(g), "tvq_conv2d_fwd: bad geometry");
  Epi e = make_epi(bias, residual, drop_p, seed_ptr, offset);
  hipStream_t st = (hipStream_t)stream;
  launch_conv(GATHER_F, kind, replicate != 0, (int)(KH * KW), x, w, y, g, workspace, e, st);
  return launch_status("tvq_conv2d_fwd");
}

extern "C" int tvq_convT2d_fwd(const float* x, int64_t B, int64_t Ci, int64_t H, int64_t Wi,
                               const float* w, const float* bias, int64_t Co, int64_t KH,
                               int64_t KW, int64_t SW, float* y, const float* residual,
                               float* workspace, tvq_stream_t stream) {
  TVQ_CHECK_ARG(x && w && y && B > 0 && Ci > 0 && Co > 0, "tvq_convT2d_fwd: bad arguments");
  const int kind = kind_of((int)KH, (int)KW, (int)SW);
  TVQ_CHECK_ARG(kind >= 0, "tvq_convT2d_fwd: unsupported kernel");
  ConvGeom g = geom_convT_fwd(B, Ci, H, Wi, Co, KH, KW, SW);
  TVQ_CHECK_ARG(geom_ok(g), "tvq_convT2d_fwd: bad geometry");
  Epi e = make_epi(bias, residual, 0.f, nullptr, 0);
  hipStream_t st = (hipStream_t)stream;
  launch_conv(GATHER_T, kind, false, (int)(KH * KW), x, w, y, g, workspace, e, st);
  return launch_status("tvq_convT2d_fwd");
}

// The training EncBlock / DecBlock conv with its BatchNorm's statistics in the epilogue
// (reference vq_vae.py:65-121: Conv2d / ConvTranspose2d (3x4, stride (1,2)) -> BatchNorm2d):
// tvq_conv_bnstats_blocks gives the number of per-block partials per channel (0: this shape
// does not take the stride-2 kernels, use tvq_conv2d_fwd + tvq_bn_train_fwd); part holds
// Co x blocks x 2 doubles for tvq_bn_train_apply_part.
static bool bnstats_geom(int64_t B, int64_t Ci, int64_t H, int64_t Wi, int64_t Co, int64_t KH,
                         int64_t KW, int64_t SW, int64_t transposed, ConvGeom* gout) {
  if (B <= 0 || Ci <= 0 || Co <= 0 || Wi <= 0 || kind_of((int)KH, (int)KW, (int)SW) != 0)
    return false;
  const ConvGeom g = transposed ? geom_convT_fwd(B, Ci, H, Wi, Co, KH, KW, SW)
                                : geom_conv_fwd(B, Ci, H, Wi, Co, KH, KW, SW);
  if (!geom_ok(g) || s2_kind(transposed ? GATHER_T : GATHER_F, g) != (transposed ? 2 : 1))
    return false;
  *gout = g;
  return true;
}

extern "C" int64_t tvq_conv_bnstats_blocks(int64_t B, int64_t Ci, int64_t H, int64_t Wi,
                                           int64_t Co, int64_t KH, int64_t KW, int64_t SW,
                                           int64_t transposed) {
  ConvGeom g;
  if (!bnstats_geom(B, Ci, H, Wi, Co, KH, KW, SW, transposed, &g)) return 0;
  return s2_blocks(g);
}

extern "C" int tvq_conv2d_fwd_bnstats(const float* x, int64_t B, int64_t Ci, int64_t H,
                                      int64_t Wi, const float* w, const float* bias, int64_t Co,
                                      int64_t KH, int64_t KW, int64_t SW, int64_t replicate,
                                      int64_t transposed, float* y, double* part,
                                      tvq_stream_t stream) {
  ConvGeom g;
  TVQ_CHECK_ARG(x && w && y && part &&
                    bnstats_geom(B, Ci, H, Wi, Co, KH, KW, SW, transposed, &g) &&
                    !(transposed && replicate),
                "tvq_conv2d_fwd_bnstats: unsupported (see tvq_conv_bnstats_blocks)");
  Epi e = make_epi(bias, nullptr, 0.f, nullptr, 0);
  e.bn_part = part;
  hipStream_t st = (hipStream_t)stream;
  launch_s2(transposed ? 2 : 1, !transposed && replicate, x, w, y, g, e, st);
  return launch_status("tvq_conv2d_fwd_bnstats");
}

static void fill_bn_eval(Epi& e, const float* bn_w, const float* bn_b, const float* running_mean,
                         const float* running_var, float eps, const float* snake_a, bool gelu) {
  e.bn_w = bn_w;
  e.bn_b = bn_b;
  e.bn_rm = running_mean;
  e.bn_rv = running_var;
  e.bn_eps = eps;
  e.snake_a = snake_a;
  e.gelu = gelu;
}

// the conv path had no fused epilogue for this shape: (GELU and) the eval BN / Snake of `e`
// over y (B, Co, HW), in place
static int bn_eval_separate(const Epi& e, float* y, int64_t B, int64_t Co, int64_t HW,
                            tvq_stream_t stream) {
  TVQ_PLAN("bn_eval separate");
  if (e.gelu) {
    const int rg = tvq_gelu_fwd(y, B * Co * HW, y, stream);
    if (rg != TVQ_OK) return rg;
  }
  return tvq_bn_eval_fwd(y, B, Co, HW, e.bn_w, e.bn_b, e.bn_rm, e.bn_rv, e.bn_eps, e.snake_a, y, y,
                         stream);
}

// Eval-mode conv -> BatchNorm(running statistics) -> Snake in one launch: the BN affine
// and the Snake are the conv epilogue's (epi_post), no (B, Co, H, W) round trip through
// HBM between them.  The same function as tvq_conv2d_fwd + tvq_bn_eval_fwd within ~1e-7
// relative, not bit for bit: the epilogue's GELU is the branch-free A&S erf (gelu_as) and its
// Snake sin^2 a Cody-Waite / polynomial form, where the separate launches call erff / sinf
// (tests/test_conv_bn_eval.py: 1e-6 of the two-launch path).
extern "C" int tvq_conv2d_fwd_bn_eval(const float* x, int64_t B, int64_t Ci, int64_t H,
                                      int64_t Wi, const float* w, const float* bias, int64_t Co,
                                      int64_t KH, int64_t KW, int64_t SW, int64_t replicate,
                                      int64_t pre_gelu, const float* bn_w, const float* bn_b,
                                      const float* running_mean, const float* running_var,
                                      float eps, const float* snake_a, float* y,
                                      float* workspace, tvq_stream_t stream) {
  TVQ_CHECK_ARG(x && w && y && running_mean && running_var && B > 0 && Ci > 0 && Co > 0,
                "tvq_conv2d_fwd_bn_eval: bad arguments");
  const int kind = kind_of((int)KH, (int)KW, (int)SW);
  TVQ_CHECK_ARG(kind >= 0, "tvq_conv2d_fwd_bn_eval: unsupported kernel");
  ConvGeom g = geom_conv_fwd(B, Ci, H, Wi, Co, KH, KW, SW);
  TVQ_CHECK_ARG(geom_ok(g), "tvq_conv2d_fwd_bn_eval: bad geometry");
  Epi e = make_epi(bias, nullptr, 0.f, nullptr, 0);
  fill_bn_eval(e, bn_w, bn_b, running_mean, running_var, eps, snake_a, pre_gelu != 0);
  hipStream_t st = (hipStream_t)stream;
  TVQ_PLAN("conv_bn_eval");
  if (!launch_conv(GATHER_F, kind, replicate != 0, (int)(KH * KW), x, w, y, g, workspace, e, st)) {
    const int rc = bn_eval_separate(e, y, B, Co, (int64_t)g.Hout * g.Wo, stream);
    if (rc != TVQ_OK) return rc;
  }
  return launch_status("tvq_conv2d_fwd_bn_eval");
}

extern "C" int tvq_convT2d_fwd_bn_eval(const float* x, int64_t B, int64_t Ci, int64_t H,
                                       int64_t Wi, const float* w, const float* bias, int64_t Co,
                                       int64_t KH, int64_t KW, int64_t SW, const float* bn_w,
                                       const float* bn_b, const float* running_mean,
                                       const float* running_var, float eps,
                                       const float* snake_a, float* y, float* workspace,
                                       tvq_stream_t stream) {
  TVQ_CHECK_ARG(x && w && y && running_mean && running_var && B > 0 && Ci > 0 && Co > 0,
                "tvq_convT2d_fwd_bn_eval: bad arguments");
  const int kind = kind_of((int)KH, (int)KW, (int)SW);
  TVQ_CHECK_ARG(kind >= 0, "tvq_convT2d_fwd_bn_eval: unsupported kernel");
  ConvGeom g = geom_convT_fwd(B, Ci, H, Wi, Co, KH, KW, SW);
  TVQ_CHECK_ARG(geom_ok(g), "tvq_convT2d_fwd_bn_eval: bad geometry");
  Epi e = make_epi(bias, nullptr, 0.f, nullptr, 0);
  fill_bn_eval(e, bn_w, bn_b, running_mean, running_var, eps, snake_a, false);
  hipStream_t st = (hipStream_t)stream;
  TVQ_PLAN("convT_bn_eval");
  if (!launch_conv(GATHER_T, kind, false, (int)(KH * KW), x, w, y, g, workspace, e, st)) {
    const int rc = bn_eval_separate(e, y, B, Co, (int64_t)g.Hout * g.Wo, stream);
    if (rc != TVQ_OK) return rc;
  }
  return launch_status("tvq_convT2d_fwd_bn_eval");
}

// workspace: [replicate canvas][pack + split-K slab]; required when replicate
extern "C" int tvq_conv2d_dgrad(const float* dy, int64_t B, int64_t Co, int64_t H, int64_t Wo,
                                const float* w, int64_t Ci, int64_t KH, int64_t KW, int64_t SW,
                                int64_t replicate, float* dx, int64_t Wi, float* workspace,
                                tvq_stream_t stream) {
  TVQ_CHECK_ARG(dy && w && dx && B > 0 && Ci > 0 && Co > 0, "tvq_conv2d_dgrad: bad arguments");
  const int kind = kind_of((int)KH, (int)KW, (int)SW);
  TVQ_CHECK_ARG(kind >= 0, "tvq_conv2d_dgrad: unsupported kernel");
  TVQ_CHECK_ARG(tvq_conv_out_width(Wi, KW, SW, 0) == Wo, "tvq_conv2d_dgrad: Wi/Wo mismatch");
  hipStream_t st = (hipStream_t)stream;
  Epi e = make_epi(nullptr, nullptr, 0.f, nullptr, 0);
  ConvGeom g = geom_conv_dgrad(B, Ci, H, Wi, Co, KH, KW, SW, replicate);
  TVQ_CHECK_ARG(geom_ok(g), "tvq_conv2d_dgrad: bad geometry");
  if (!replicate) {
    launch_conv(GATHER_T, kind, false, (int)(KH * KW), dy, w, dx, g, workspace, e, st);
    return launch_status("tvq_conv2d_dgrad");
  }
  if (KH == 3 && KW == 4 && SW == 2 && s2_fold_fits(g)) {
    launch_s2_fold(dy, w, dx, g, st);
    return launch_status("tvq_conv2d_dgrad(replicate, s2)");
  }
  if (KH == 3 && KW == 4 && SW == 2 && s2m_fold_fits(g)) {
    // packed [tap][c][n] behind the canvas's place, where the staged path puts it: the same
    // pack-cache entry either way.  The canvas itself stays in LDS here, so its
    // tvq_conv_workspace share (op 2) is unused by this launch; it is still sized, because the
    // workspace is asked for by shape alone and bit 4096 sends the same shape to the staged path
    const float* wp = w;
    if (workspace) wp = pack_weight(w, g, (int)(KH * KW), workspace + canvas_floats(g), st);
    launch_s2m_t(true, dy, wp, nullptr, dx, g, st);
    return launch_status("tvq_conv2d_dgrad(replicate, s2m)");
  }
  TVQ_CHECK_ARG(workspace, "tvq_conv2d_dgrad: replicate needs a workspace");
  float* canvas = workspace;
  float* rest = workspace + canvas_floats(g);
  launch_conv(GATHER_T, kind, false, (int)(KH * KW), dy, w, canvas, g, rest, e, st);
  const int64_t tot = B * Ci * H * Wi;
  const int blocks = (int)((tot + 255) / 256 < 8192 ? (tot + 255) / 256 : 8192);
  hipLaunchKernelGGL(replicate_fold_kernel, dim3(blocks), dim3(256), 0, st, canvas, (int)B,
                     (int)Ci, (int)H, (int)Wi, PH_OF(KH), PW_OF(KW), dx);
  return launch_status("tvq_conv2d_dgrad(replicate)");
}

extern "C" int tvq_convT2d_dgrad(const float* dy, int64_t B, int64_t Co, int64_t H, int64_t Wo,
                                 const float* w, int64_t Ci, int64_t KH, int64_t KW, int64_t SW,
                                 float* dx, int64_t Wi, float* workspace, tvq_stream_t stream) {
  TVQ_CHECK_ARG(dy && w && dx && B > 0 && Ci > 0 && Co > 0, "tvq_convT2d_dgrad: bad arguments");
  const int kind = kind_of((int)KH, (int)KW, (int)SW);
  TVQ_CHECK_ARG(kind >= 0, "tvq_convT2d_dgrad: unsupported kernel");
  TVQ_CHECK_ARG(tvq_conv_out_width(Wi, KW, SW, 1) == Wo, "tvq_convT2d_dgrad: Wi/Wo mismatch");
  ConvGeom g = geom_convT_dgrad(B, Ci, H, Wi, Co, KH, KW, SW);
  TVQ_CHECK_ARG(geom_ok(g), "tvq_convT2d_dgrad: bad geometry");
  Epi e = make_epi(nullptr, nullptr, 0.f, nullptr, 0);
  hipStream_t st = (hipStream_t)stream;
  launch_conv(GATHER_F, kind, false, (int)(KH * KW), dy, w, dx, g, workspace, e, st);
  return launch_status("tvq_convT2d_dgrad");
}

// op: 0 conv2d fwd, 1 convT2d fwd, 2 conv2d dgrad, 3 convT2d dgrad, 4 conv2d wgrad,
// 5 convT2d wgrad.  (Ci, Co, Wi) are the layer's input channels, output channels and
// input width.  Returns floats (>= 1).
extern "C" int64_t tvq_conv_workspace(int64_t op, int64_t B, int64_t Ci, int64_t H, int64_t Wi,
                                      int64_t Co, int64_t KH, int64_t KW, int64_t SW,
                                      int64_t replicate) {
  int64_t r = 0;
  const int KK = (int)(KH * KW);
  switch (op) {
    case 0: r = conv_gemm_ws(geom_conv_fwd(B, Ci, H, Wi, Co, KH, KW, SW), KK); break;
    case 1: r = conv_gemm_ws(geom_convT_fwd(B, Ci, H, Wi, Co, KH, KW, SW), KK); break;
    case 2: {
      const ConvGeom g = geom_conv_dgrad(B, Ci, H, Wi, Co, KH, KW, SW, replicate);
      // the canvas share is sized for every replicate shape, also where conv_s2t's / conv_s2m_t's
      // fold form keeps the canvas in LDS: bit 512 / 4096 send the same shape to the staged path
      r = (replicate ? canvas_floats(g) : 0) + conv_gemm_ws(g, KK);
      break;
    }
    case 3: r = conv_gemm_ws(geom_convT_dgrad(B, Ci, H, Wi, Co, KH, KW, SW), KK); break;
    case 4:
      r = conv_wgrad_ws(Co, Ci, KH, KW, B, H, tvq_conv_out_width(Wi, KW, SW, 0));
      break;
    case 5: r = conv_wgrad_ws(Ci, Co, KH, KW, B, H, Wi); break;
    default: return -1;
  }
  return r > 0 ? r : 1;
}

