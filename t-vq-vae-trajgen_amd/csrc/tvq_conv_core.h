// Private to the conv engine (tvq_conv*.hip): the geometry and epilogue types, the device
// helpers shared by the kernel families, the engine's switches and the host launchers each
// family file exposes.  Other kernel files include tvq_conv_internal.h only.
//
// Every conv on the TimeVQVAE path has KH in {1,3} with PH = KH/2 (so H_out == H_in),
// a W stride SW in {1,2} and PW = (KW-1)/2.  Three gather forms cover all of them:
//
//  F  out[b,n,h,wo] = sum_{c,kh,kw} Wt(n,c,kh,kw) * In[b,c,h+kh-PH, wo*SW+kw-PW]
//       Conv2d fwd (zero or replicate pad), ConvTranspose2d dgrad
//  T  out[b,n,h,wo] = sum_{c,kh,kw} Wt(n,c,kh,kw) * In[b,c,h-kh+PH, (wo-kw+PW)/SW]
//       Conv2d dgrad, ConvTranspose2d fwd (terms with a fractional/out-of-range
//       source are zero)
//  W  dW(n,c,kh,kw) = sum_{b,h,w} G[b,n,h,w] * In[b,c,h+kh-PH, w*SW+kw-PW]
//       Conv2d / ConvTranspose2d weight gradients (split over positions,
//       deterministic slab reduction)
//
// Kernel templates live in the family files, one translation unit each:
//   tvq_conv.hip        ABI entry points, launch_conv (the F/T dispatcher), the switches
//   tvq_conv_tap.hip    conv_gemm / conv_tap / conv_splitk_epi (staged 16x16x4 GEMMs)
//   tvq_conv_t32.hip    conv_t32 (32x32x2 tile, wide channels)
//   tvq_conv_d32.hip    conv_d32 (narrow maps, no LDS staging)
//   tvq_conv_halo.hip   conv_halo / conv_small / conv_n16
//   tvq_conv_s2.hip     conv_s2f / conv_s2t (+ fold), conv_wgrad_s2
//   tvq_conv_s2m.hip    conv_s2m_t (+ fold): the same T gather at 32 / 64 reduction channels
//   tvq_conv_pack.hip   weight packing and the pack cache
// and the W form's, one per family as well:
//   tvq_conv_wgrad.hip       ABI entry points, wgrad_ladder (the W dispatcher), conv_wgrad_ws,
//                            conv_wgrad (the split GEMM that takes every shape)
//   tvq_conv_wgrad_t32.hip   conv_wgrad_t32 (wide maps, 32x32x2 tile)
//   tvq_conv_wgrad_w8.hip    conv_wgrad_w8 (narrow maps, image-batched, multi-problem)
//   tvq_conv_wgrad_halo.hip  conv_wgrad_halo (one image's halo tile per step)
//   (conv_wgrad_s2 lives in tvq_conv_s2.hip; the split sums every family ends in, and their
//   deferral scope, are tvq_reduce.hip's conv_wgrad_finish)
#pragma once
#include "tvq_common.h"

namespace tvq {

struct FastDiv {  // q = n / d for 0 <= n < 2^30, d >= 1
  uint32_t d;
  uint64_t magic;
  uint32_t shift;
};
static FastDiv make_fastdiv(uint32_t d) {
  FastDiv f;
  f.d = d;
  uint32_t s = 0;
  while ((1ull << s) < d) ++s;
  f.shift = 32 + s;
  f.magic = ((1ull << f.shift) + d - 1) / d;
  return f;
}
__device__ __forceinline__ uint32_t fdiv(uint32_t n, const FastDiv& f) {
  return (uint32_t)(((uint64_t)n * f.magic) >> f.shift);
}

// Geometry of one conv launch.  "In" is the gathered tensor (reduction channels C),
// "out"/"G" has N channels at positions (b, h, w) with w in [0, Wo).
struct ConvGeom {
  int B, C, Hin, Win;  // gathered tensor
  int N, Hout, Wo;     // output / G positions
  int oph, opw;        // pad offsets: F: hi = h+kh-oph, wi = wo*SW+kw-opw;  T: hi = h-kh+oph, wn = wo-kw+opw
  int64_t wsn, wsc, wst;  // weight strides for (n, c, tap = kh*KW + kw)
  FastDiv fd_wo, fd_hwo;
  int Kred;            // C*KH*KW
  int Mpos;            // B*Hout*Wo
};

enum { GATHER_F = 0, GATHER_T = 1 };

// gathered input value for reduction index k at output position (b, h, wo)
template <int MODE, int KH, int KW, int SW, bool REPL>
__device__ __forceinline__ float gather_in(const float* __restrict__ in, const ConvGeom& g,
                                           const float* inb, int h, int wo, int k) {
  constexpr int KK = KH * KW;
  const int c = k / KK;
  const int r = k - c * KK;
  const int kh = r / KW, kw = r - kh * KW;
  if (c >= g.C) return 0.f;
  int hi, wi;
  if (MODE == GATHER_F) {
    hi = h + kh - g.oph;
    wi = wo * SW + kw - g.opw;
    if (REPL) {
      hi = hi < 0 ? 0 : (hi >= g.Hin ? g.Hin - 1 : hi);
      wi = wi < 0 ? 0 : (wi >= g.Win ? g.Win - 1 : wi);
    } else if (hi < 0 || hi >= g.Hin || wi < 0 || wi >= g.Win) {
      return 0.f;
    }
  } else {
    hi = h - kh + g.oph;
    const int wn = wo - kw + g.opw;
    if (hi < 0 || hi >= g.Hin || wn < 0) return 0.f;
    if (SW == 2 && (wn & 1)) return 0.f;
    wi = wn / SW;
    if (wi >= g.Win) return 0.f;
  }
  return inb[((int64_t)c * g.Hin + hi) * g.Win + wi];
}

// Epilogue options for F/T launches
struct Epi {
  const float* bias;      // [N] or null
  const float* residual;  // same layout as out, or null: out = residual + v
  float drop_p;           // dropout on v (before the residual add)
  float drop_scale;
  const int64_t* seed_ptr;
  uint64_t offset;
  // eval-mode BatchNorm (+ Snake) applied to conv + bias before the dropout / residual
  // (VQVAEDecBlock / ResBlock's conv -> BN -> Snake while sampling; null: off)
  const float* bn_w;
  const float* bn_b;
  const float* bn_rm;
  const float* bn_rv;
  const float* snake_a;
  float bn_eps;
  int gelu;  // GELU (erf form) on conv + bias before the BN (Upscale: Conv1d -> GELU -> BN)
  // training BatchNorm statistics of the stored output (the stride-2 kernels' STATS form,
  // tvq_conv2d_fwd_bnstats): per-stage (sum, sum of squares) in fp64 at
  // bn_part[(n * stages + stage) * 2 + k], stage = (image, segment); null: off
  double* bn_part;
};

// bn_eval_snake_kernel's BN arithmetic (tvq_norm.hip) for channel n: v -> v sc + sh, then
// Snake (a = 0: none) with its sin^2 from sin2_cw (within ~1e-7 relative of sinf's)
struct PostCh {
  float sc, sh, a;
};
__device__ __forceinline__ PostCh epi_post_ch(const Epi& e, int n) {
  PostCh p;
  const float inv = 1.0f / sqrtf(e.bn_rv[n] + e.bn_eps);
  p.sc = (e.bn_w ? e.bn_w[n] : 1.f) * inv;
  p.sh = (e.bn_b ? e.bn_b[n] : 0.f) - e.bn_rm[n] * p.sc;
  p.a = e.snake_a ? e.snake_a[n] : 0.f;
  return p;
}
__device__ __forceinline__ float epi_post_apply(const PostCh& p, float v, bool gelu) {
  if (gelu) v = gelu_as(v);  // branch-free erf (tvq_common.h), ~1e-7 of tvq_gelu_fwd's
  float s = fmaf(v, p.sc, p.sh);
  if (p.a != 0.f) s = s + (1.0f / p.a) * sin2_cw(p.a * s);
  return s;
}
__device__ __forceinline__ float epi_post(const Epi& e, float v, int n) {
  return e.bn_rv ? epi_post_apply(epi_post_ch(e, n), v, e.gelu != 0) : v;
}

// Epilogue helpers.  Every global load here is unconditional (clamped index) so the
// compiler issues them together instead of one load + wait per element.
template <int FN>
__device__ __forceinline__ void epi_load_bias(float (&bv)[FN][4], const float* __restrict__ bias,
                                              int nbase, int N) {
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = min(nbase + i * 16 + r, N - 1);
      bv[i][r] = bias ? bias[n] : 0.f;
    }
}

// a[i][r]: channel nbase + i*16 + r at flat offset ob + n*hw (ob for a clamped position
// when !pv, so every address is in bounds)
// POST kernels: the per-channel BN / Snake terms of a lane's FN x 4 channels, loaded once
// before the epilogue's position loop (as epi_load_bias does for the bias)
template <int FN>
struct PostTile {
  PostCh c[FN][4];
};
template <int FN>
__device__ __forceinline__ void epi_load_post(PostTile<FN>& pt, const Epi& e, int nbase, int N) {
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) pt.c[i][r] = epi_post_ch(e, min(nbase + i * 16 + r, N - 1));
}

template <int FN, bool POST = false>
__device__ __forceinline__ void epi_store(float* __restrict__ out, const Epi& e, uint64_t seed,
                                          const float (&bv)[FN][4], const floatx4 (&a)[FN],
                                          int64_t ob, int64_t hw, int nbase, int N, bool pv,
                                          bool wt = false, const PostTile<FN>* pt = nullptr) {
  float v[FN][4];
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) v[i][r] = a[i][r] + bv[i][r];
  if constexpr (POST) {  // a separate instantiation: its terms would crowd every conv's epilogue
#pragma unroll
    for (int i = 0; i < FN; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) v[i][r] = epi_post_apply(pt->c[i][r], v[i][r], e.gelu != 0);
  }
  if (e.drop_p > 0.f) {
#pragma unroll
    for (int i = 0; i < FN; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint64_t o = (uint64_t)(ob + (int64_t)(nbase + i * 16 + r) * hw);
        v[i][r] = uniform01(seed, o) >= e.drop_p ? v[i][r] * e.drop_scale : 0.f;
      }
  }
  if (e.residual) {
    float rv[FN][4];
#pragma unroll
    for (int i = 0; i < FN; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        rv[i][r] = e.residual[ob + (int64_t)min(nbase + i * 16 + r, N - 1) * hw];
#pragma unroll
    for (int i = 0; i < FN; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) v[i][r] += rv[i][r];
  }
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = nbase + i * 16 + r;
      if (pv && n < N) {
        if (wt) st_wt(out + ob + (int64_t)n * hw, v[i][r]);  // split-K slab, last-block finish
        else out[ob + (int64_t)n * hw] = v[i][r];
      }
    }
}

static ConvGeom make_geom(int B, int C, int Hin, int Win, int N, int Hout, int Wo, int KH, int KW,
                          int oph, int opw, int64_t wsn, int64_t wsc) {
  ConvGeom g;
  g.B = B; g.C = C; g.Hin = Hin; g.Win = Win; g.N = N; g.Hout = Hout; g.Wo = Wo;
  g.oph = oph; g.opw = opw;
  g.wsn = wsn; g.wsc = wsc; g.wst = 1;
  g.fd_wo = make_fastdiv((uint32_t)Wo);
  g.fd_hwo = make_fastdiv((uint32_t)(Hout * Wo));
  g.Kred = C * KH * KW;
  g.Mpos = B * Hout * Wo;
  return g;
}

// one image's zero- / replicate-padded (or stride-dilated, T) halo planes into LDS: the
// load phase of conv_halo_kernel and conv_wgrad_halo_kernel
static constexpr int HALO_U = 8;  // loads in flight per thread in the load phase

template <int MODE, int KH, int KW, int SW, bool REPL>
__device__ __forceinline__ void halo_fill(float* __restrict__ Hs, const float* __restrict__ inb,
                                          int C, int Cp, int Hin, int Win, int HP, int WP, int PS,
                                          int oh, int ow, const Div16& dv_hw, const Div16& dv_wp,
                                          int tid) {
  const int hw = HP * WP;
  const int total = Cp * hw;
  for (int base = tid; base < total; base += 256 * HALO_U) {
    float v[HALO_U];
    int dst[HALO_U];
#pragma unroll
    for (int u = 0; u < HALO_U; ++u) {
      const int idx = base + u * 256;
      v[u] = 0.f;
      dst[u] = -1;
      if (idx < total) {
        const int c = div16(idx, dv_hw);
        const int r = idx - c * hw;
        const int hp = div16(r, dv_wp);
        const int wp = r - hp * WP;
        dst[u] = c * PS + r;
        if (c < C) {
          int hi = hp - oh;
          if (MODE == GATHER_F) {
            int wi = wp - ow;
            if (REPL) {
              hi = hi < 0 ? 0 : (hi >= Hin ? Hin - 1 : hi);
              wi = wi < 0 ? 0 : (wi >= Win ? Win - 1 : wi);
              v[u] = inb[((int64_t)c * Hin + hi) * Win + wi];
            } else if (hi >= 0 && hi < Hin && wi >= 0 && wi < Win) {
              v[u] = inb[((int64_t)c * Hin + hi) * Win + wi];
            }
          } else {
            const int wn = wp - ow;
            const int wi = wn / SW;
            if (hi >= 0 && hi < Hin && wn >= 0 && wn - wi * SW == 0 && wi < Win)
              v[u] = inb[((int64_t)c * Hin + hi) * Win + wi];
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < HALO_U; ++u)
      if (dst[u] >= 0) Hs[dst[u]] = v[u];
  }
}

static constexpr int HALO_LDS_MAX = 64 * 1024;

#define PH_OF(KH) ((int)(KH) / 2)
#define PW_OF(KW) (((int)(KW) - 1) / 2)

// kind: 0 = 3x4 s2 (EncBlock / ConvT), 1 = 3x3 s1, 2 = 1x1, 3 = 1x3 s1 (Conv1d k3).  The W
// launchers' dispatch, MACRO(KH, KW, SW, REPL); `kind` is a kind_of() value the entry point checked
#define TVQ_DISPATCH_KIND(kind, repl, MACRO)                                  \
  switch (kind) {                                                             \
    case 0: if (repl) { MACRO(3, 4, 2, true) } else { MACRO(3, 4, 2, false) } break; \
    case 1: MACRO(3, 3, 1, false) break;                                      \
    case 2: MACRO(1, 1, 1, false) break;                                      \
    case 3: if (repl) { MACRO(1, 3, 1, true) } else { MACRO(1, 3, 1, false) } break; \
    case 4: MACRO(1, 7, 1, false) break;                                      \
    case 5: MACRO(1, 4, 2, false) break;                                      \
  }

static int kind_of(int KH, int KW, int SW) {
  if (KH == 3 && KW == 4 && SW == 2) return 0;
  if (KH == 3 && KW == 3 && SW == 1) return 1;
  if (KH == 1 && KW == 1 && SW == 1) return 2;
  if (KH == 1 && KW == 3 && SW == 1) return 3;
  if (KH == 1 && KW == 7 && SW == 1) return 4;  // FidelityEnhancer init conv (k7, pad 3)
  if (KH == 1 && KW == 4 && SW == 2) return 5;  // FidelityEnhancer Downsample (k4, s2, pad 1)
  return -1;
}

// The F / T launchers' dispatch: M(MODE, KH, KW, SW, REPL) for the 14 combinations the entry
// points reach -- the F gather of every kind (replicate padding for kinds 0 and 3 only), the
// T gather of every kind with zero padding.  `kind` is a kind_of() value the entry point checked.
#define TVQ_DISPATCH_CONV(mode, kind, repl, M)                                           \
  if ((mode) == GATHER_F) {                                                              \
    switch (kind) {                                                                      \
      case 0: if (repl) { M(GATHER_F, 3, 4, 2, true) } else { M(GATHER_F, 3, 4, 2, false) } break; \
      case 1: M(GATHER_F, 3, 3, 1, false) break;                                         \
      case 2: M(GATHER_F, 1, 1, 1, false) break;                                         \
      case 3: if (repl) { M(GATHER_F, 1, 3, 1, true) } else { M(GATHER_F, 1, 3, 1, false) } break; \
      case 4: M(GATHER_F, 1, 7, 1, false) break;                                         \
      case 5: M(GATHER_F, 1, 4, 2, false) break;                                         \
    }                                                                                    \
  } else {                                                                               \
    switch (kind) {                                                                      \
      case 0: M(GATHER_T, 3, 4, 2, false) break;                                         \
      case 1: M(GATHER_T, 3, 3, 1, false) break;                                         \
      case 2: M(GATHER_T, 1, 1, 1, false) break;                                         \
      case 3: M(GATHER_T, 1, 3, 1, false) break;                                         \
      case 4: M(GATHER_T, 1, 7, 1, false) break;                                         \
      case 5: M(GATHER_T, 1, 4, 2, false) break;                                         \
    }                                                                                    \
  }

// The engine's switches (tvq_conv_config; the object lives in tvq_conv.hip): each selects a
// path some test uses as its reference.
struct ConvConfig {
  // bits: 1 = halo fwd/dgrad, 2 = halo wgrad, 4 = halo fwd/dgrad wherever it fits (ignore
  // halo_preferred; tests)
  int halo = 3;
  int t32 = 1;  // conv_t32 / conv_d32 enabled (bit 8 turns them off)
  int s2 = 1;   // conv_s2f / conv_s2t enabled (bit 512 turns them off)
  int ws2 = 1;  // conv_wgrad_s2_kernel enabled (bit 1024 turns it off)
  int s2m = 1;  // conv_s2m_t enabled (bit 4096 turns it off)
  int s2_cap = 0;  // conv_s2f / conv_s2t block cap (tvq_conv_s2_cap): 0 = the per-kernel default
};
const ConvConfig& conv_config();

// ---- the families' host launchers.  The F / T ones take (mode, kind, replicate) at run
// time and return false, with nothing launched, when the shape is not theirs.

// tvq_conv_pack.hip: `wt` packed [tap][c][n] into `ws` (N*C*KK floats) -- or served from the
// open pack cache -- with g's weight strides retargeted; a null `ws` leaves it unpacked
const float* pack_weight(const float* wt, ConvGeom& g, int KK, float* ws, hipStream_t st);

// tvq_conv_s2.hip
int s2_kind(int mode, const ConvGeom& g);  // 0 none, 1 F, 2 T (Hout 3), 3 T (Hout 5)
int64_t s2_blocks(const ConvGeom& g);      // stages = per-channel partials of the STATS form
void launch_s2(int k2, bool repl, const float* in, const float* wt, float* out, const ConvGeom& g,
               const Epi& e, hipStream_t st);
bool s2_fold_fits(const ConvGeom& g);
void launch_s2_fold(const float* in, const float* wt, float* dx, const ConvGeom& g, hipStream_t st);
bool ws2_fits(int64_t C, int64_t H, int64_t N, int64_t KH, int64_t KW, int64_t SW);
int64_t ws2_ws(int64_t B, int64_t C, int64_t Wo, int64_t N);
int ws2_launch(const float* G, const float* X, float* slab, int B, int C, int N, int Win, int Wo,
               int kcols, bool repl, hipStream_t st);

// tvq_conv_s2m.hip: the LF band's middle levels (32 / 64 reduction channels).  s2m_t_fits: the
// Hout 3 T form with a bias-only epilogue; s2m_fold_fits: the replicate canvas geometry, folded
// onto dx in the kernel
bool s2m_t_fits(const ConvGeom& g, const Epi& e);
bool s2m_fold_fits(const ConvGeom& g);
void launch_s2m_t(bool fold, const float* in, const float* wt, const float* bias, float* out,
                  const ConvGeom& g, hipStream_t st);

// tvq_conv_halo.hip (*post: the epilogue applied e's eval BN / Snake)
bool launch_small(int mode, int kind, bool repl, const float* in, const float* wt, float* out,
                  const ConvGeom& g, const Epi& e, hipStream_t st);
bool n16_geom_ok(int mode, int kind, const ConvGeom& g);
void launch_n16(int mode, int kind, const float* in, const float* wp, float* out,
                const ConvGeom& g, const Epi& e, hipStream_t st);
bool launch_halo(int mode, int kind, bool repl, const float* in, const float* wt, float* out,
                 const ConvGeom& g, const Epi& e, hipStream_t st, bool* post);

// tvq_conv_t32.hip / tvq_conv_d32.hip: packed weights, C % 16 == 0
bool launch_t32(int mode, int kind, bool repl, const float* in, const float* wt, float* out,
                const ConvGeom& g, const Epi& e, hipStream_t st, bool* post);
bool launch_d32(int mode, int kind, bool repl, const float* in, const float* wt, float* out,
                const ConvGeom& g, const Epi& e, hipStream_t st);

// tvq_conv_tap.hip: the staged GEMMs take every shape.  launch_tap (C % 16 == 0; `slab`,
// nullable, enables split-K) returns whether e's eval BN / Snake was applied.
bool launch_tap(int mode, int kind, bool repl, const float* in, const float* wt, float* out,
                const ConvGeom& g, const Epi& e, float* slab, hipStream_t st);
void launch_gemm_flat(int mode, int kind, bool repl, const float* in, const float* wt, float* out,
                      const ConvGeom& g, const Epi& e, hipStream_t st);
int64_t conv_gemm_ws(const ConvGeom& g, int KK);  // floats: pack + split-K slab

// ---- the weight-gradient (W form) families.  One problem: G (B, N, Hout, Wo) against In
// (B, C, Hin, Win) into `slab`, S rows of [N][kcols] that conv_wgrad_finish sums in order;
// kcols = C*KH*KW (+ 1: the bias column).  Each family has one plan function, which fixes its
// split count S from the shape; its launcher and conv_wgrad_ws both take S from there.
struct WgradArgs {
  const float* G;
  const float* in;
  float* slab;
  int B, C, Hin, Win, N, Hout, Wo;
  int KH, KW, SW, kind;  // kind: the kind_of() value the entry point checked
  bool repl;
  int kcols;
  hipStream_t st;
};
// floats of S slab rows [N][C*KK + 1]: the one place a split count becomes a size
inline int64_t wgrad_slab_floats(int64_t S, int64_t N, int64_t C, int64_t KK) {
  return S * N * (C * KK + 1);
}
// launch_wgrad_*: the launch's S, or 0 with nothing launched when the shape is not theirs

// tvq_conv_wgrad_t32.hip
struct WtSplit {
  int S, spr;  // splits of the 32-position stages, stages per split
};
bool wt32_fits(int64_t B, int64_t C, int64_t H, int64_t Wi, int64_t N, int64_t Wo, int64_t KH,
               int64_t KW, int64_t SW, int64_t replicate);
WtSplit wt32_plan(int64_t B, int64_t C, int64_t H, int64_t W, int64_t N, int64_t KK);
int launch_wgrad_t32(const WgradArgs& a);

// tvq_conv_wgrad_w8.hip.  w8_splits: one slab row per block of images, 0 when the batch is
// not whole blocks (the kernel's other conditions need the map, which conv_wgrad_ws is not given)
int w8_splits(int64_t B);
int launch_wgrad_w8(const WgradArgs& a);

// tvq_conv_wgrad_halo.hip.  The blocking and S depend on (N, C, KK, B) alone.
struct WHaloSplit {
  int FN, CB;      // 16-row n tiles per block, input channels per block
  int nblk, cblk;  // blocks over n and over c
  int S, ips;      // splits over images, images per split
};
WHaloSplit whalo_split(int64_t N, int64_t C, int KK, int64_t B);
int whalo_plane_stride(int hw, int KK, int KW, int WP, int SW, int CB);
int launch_wgrad_halo(const WgradArgs& a);

// tvq_conv_wgrad.hip: workspace floats of tvq_conv2d_wgrad / tvq_convT2d_wgrad
int64_t conv_wgrad_ws(int64_t N, int64_t C, int64_t KH, int64_t KW, int64_t B, int64_t Hout,
                      int64_t Wo);

}  // namespace tvq

