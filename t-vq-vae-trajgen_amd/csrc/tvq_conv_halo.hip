// The conv engine's LDS-resident small-shape kernels: conv_halo_kernel (image + weight panel
// in LDS), conv_small_kernel (direct, few channels on both sides) and conv_n16_kernel (few
// outputs, wide input).
#include "tvq_conv_core.h"

namespace tvq {

// ---------------------------------------------------------------- halo-tile path
// For convolutions whose padded input image (Cp x HP x WP) and a weight panel of NB
// output channels (K = Cp*KK columns) fit in LDS together -- the small-channel ResBlock,
// encoder and decoder convs -- one block takes one image b and NB channels: both
// tiles are loaded once (batched so many loads are in flight per thread, one sync),
// then every MFMA operand is an LDS read: A from the panel, B from the halo image at
// h*WP + w*SW + koff[k], koff[k] = c*PS + kh*WP + kw from a per-block table.  There is
// no per-K-step global round trip, which is what bounds the staged GEMM at these sizes
// (a few hundred positions per image, K <= 576).
//   F  out[n,h,w] = sum W(n,c,kh,kw) In[c, h+kh-oh, w*SW+kw-ow]         (halo = In, padded)
//   T  out[n,h,w] = sum W(n,c,kh,kw) D[c, h+KH-1-kh, w+KW-1-kw]          (D = In dilated by SW,
//      oh = KH-1-PH, ow = KW-1-PW: the transposed gather as a stride-1 conv, taps flipped)
// The weight panel keeps the raw (c, kh, kw) column order, so it is a straight copy of
// the weight rows.  KS = 4 splits K across the 4 waves when the image has <= 4 position
// tiles (partials reduced through LDS).
struct HaloGeom {
  Div16 dv_hw, dv_wp, dv_wo, dv_k;
  int C, Cp, Hin, Win, N, Hout, Wo;
  int oh, ow;          // halo (hp, wp) -> source row hp - oh, col (wp - ow) [/SW for T]
  int HP, WP, PS;      // halo rows / cols; channel-plane stride (== 16 mod 32)
  int P, MT;           // positions per image, 16-position tiles per image
  int KST;             // weight-panel row stride (== 2 mod 32)
  int64_t wsn, wsc;    // raw weight strides of (n, c); taps contiguous
};

template <int MODE, int KH, int KW, int SW, bool REPL, int FN, int KS, bool POST = false>
__global__ __launch_bounds__(256) void conv_halo_kernel(const float* __restrict__ in,
                                                       const float* __restrict__ wt,
                                                       float* __restrict__ out, HaloGeom g,
                                                       Epi e) {
  constexpr int KK = KH * KW;
  constexpr int NB = FN * 16;
  constexpr int CSW = MODE == GATHER_F ? SW : 1;  // position stride inside the halo
  extern __shared__ float smem[];
  const int K = g.Cp * KK;
  float* Hs = smem;                                  // [Cp][PS]
  float* As = Hs + g.Cp * g.PS;                      // [NB][KST], columns (c, kh, kw)
  int* koff = reinterpret_cast<int*>(As + NB * g.KST);  // [K]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int b = blockIdx.x;
  const int n0 = blockIdx.y * NB;

  // ---- load phase
  halo_fill<MODE, KH, KW, SW, REPL>(Hs, in + (int64_t)b * g.C * g.Hin * g.Win, g.C, g.Cp, g.Hin,
                                    g.Win, g.HP, g.WP, g.PS, g.oh, g.ow, g.dv_hw, g.dv_wp, tid);
  {
    // panel element (nn, k = c*KK + t); walk the raw weight in its contiguous order
    const bool n_inner = g.wsn < g.wsc;  // dgrad / convT layouts: (c, n, t)
    const int total = NB * K;
    for (int base = tid; base < total; base += 256 * HALO_U) {
      float v[HALO_U];
      int dst[HALO_U];
#pragma unroll
      for (int u = 0; u < HALO_U; ++u) {
        const int idx = base + u * 256;
        v[u] = 0.f;
        dst[u] = -1;
        if (idx < total) {
          int nn, c, t;
          if (n_inner) {
            t = idx % KK;
            const int r = idx / KK;
            c = r / NB;
            nn = r - c * NB;
          } else {
            nn = div16(idx, g.dv_k);
            const int k = idx - nn * K;
            c = k / KK;
            t = k - c * KK;
          }
          dst[u] = nn * g.KST + c * KK + t;
          const int n = n0 + nn;
          if (n < g.N && c < g.C) v[u] = wt[(int64_t)n * g.wsn + (int64_t)c * g.wsc + t];
        }
      }
#pragma unroll
      for (int u = 0; u < HALO_U; ++u)
        if (dst[u] >= 0) As[dst[u]] = v[u];
    }
    for (int k = tid; k < K; k += 256) {
      const int c = k / KK, t = k - c * KK;
      const int tl = MODE == GATHER_F ? t : KK - 1 - t;
      koff[k] = c * g.PS + (tl / KW) * g.WP + (tl % KW);
    }
  }
  __syncthreads();

  const int j = lane & 15, kq = lane >> 4;
  const int Q = K / 4;
  const uint64_t seed = e.drop_p > 0.f ? mix_seed(e.seed_ptr, e.offset) : 0ull;

  auto run = [&](int mt0, int mstep, int fa, int qs, int qe, floatx4 (&acc)[FN][4]) {
    int base[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const int p = (mt0 + f * mstep) * 16 + j;
      const int pp = p < g.P ? p : 0;
      const int h = div16(pp, g.dv_wo);
      const int w = pp - h * g.Wo;
      base[f] = h * g.WP + w * CSW;
    }
#pragma unroll
    for (int i = 0; i < FN; ++i)
#pragma unroll
      for (int f = 0; f < 4; ++f) acc[i][f] = floatx4{0.f, 0.f, 0.f, 0.f};
    const float* ap = As + j * g.KST + kq;
    for (int q = qs; q < qe; ++q) {
      const int ko = koff[q * 4 + kq];
      float af[FN];
#pragma unroll
      for (int i = 0; i < FN; ++i) af[i] = ap[i * 16 * g.KST + q * 4];
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        if (f < fa) {
          const float bf = Hs[base[f] + ko];
#pragma unroll
          for (int i = 0; i < FN; ++i) acc[i][f] = mfma16x16x4(af[i], bf, acc[i][f]);
        }
      }
    }
  };
  const int nbase = n0 + kq * 4;
  float bv[FN][4];
  epi_load_bias<FN>(bv, e.bias, nbase, g.N);
  PostTile<FN> pt;
  if constexpr (POST) epi_load_post<FN>(pt, e, nbase, g.N);
  const int64_t hwo = (int64_t)g.Hout * g.Wo;
  auto store = [&](int mt, const floatx4 (&a)[FN]) {
    const int p = mt * 16 + j;
    const bool pv = p < g.P;
    const int pp = pv ? p : 0;
    const int h = div16(pp, g.dv_wo);
    const int w = pp - h * g.Wo;
    epi_store<FN, POST>(out, e, seed, bv, a, ((int64_t)b * g.N * g.Hout + h) * g.Wo + w, hwo,
                        nbase, g.N, pv, false, &pt);
  };

  floatx4 acc[FN][4];
  if (KS == 1) {
    for (int mt0 = wid; mt0 < g.MT; mt0 += 16) {
      const int fa = min(4, (g.MT - mt0 + 3) / 4);
      run(mt0, 4, fa, 0, Q, acc);
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        if (f < fa) {
          floatx4 a[FN];
#pragma unroll
          for (int i = 0; i < FN; ++i) a[i] = acc[i][f];
          store(mt0 + 4 * f, a);
        }
      }
    }
  } else {
    // MT <= 4: every wave takes all position tiles over a quarter of K
    const int fa = g.MT;
    const int qs = wid * Q / 4, qe = (wid + 1) * Q / 4;
    run(0, 1, fa, qs, qe, acc);
    __syncthreads();  // all waves done with the tiles: reuse LDS for the partials
    floatx4* red = reinterpret_cast<floatx4*>(smem);
    if (wid > 0) {
#pragma unroll
      for (int i = 0; i < FN; ++i)
#pragma unroll
        for (int f = 0; f < 4; ++f)
          if (f < fa) red[(((wid - 1) * FN + i) * 4 + f) * 64 + lane] = acc[i][f];
    }
    __syncthreads();
    if (wid == 0) {
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        if (f < fa) {
          floatx4 a[FN];
#pragma unroll
          for (int i = 0; i < FN; ++i) {
            a[i] = acc[i][f];
#pragma unroll
            for (int wv = 0; wv < 3; ++wv) {
              const floatx4 t = red[((wv * FN + i) * 4 + f) * 64 + lane];
              a[i][0] += t[0]; a[i][1] += t[1]; a[i][2] += t[2]; a[i][3] += t[3];
            }
          }
          store(f, a);
        }
      }
    }
  }
}

// Direct convolution for few channels on both sides (C, N <= 16): the stride-2 encoder /
// decoder convs and the decoders' ConvTranspose tail (12 <-> 4 / 12 channels at W up to
// 512), where an MFMA tile would be mostly padding and the staged GEMMs are latency-bound.
// One thread owns two adjacent output positions for all N channels (32 fp32 accumulators),
// the weights sit in LDS as [c][tap][16 n] (float4 broadcast reads), the input is read
// through L1/L2; for the T gather (stride-2 transposed) the taps whose source is fractional
// are skipped per output parity with wave-uniform branches.  Same epilogue as epi_store.
constexpr int SMALL_NB = 16;
template <int MODE, int KH, int KW, int SW, bool REPL, int NB>
__global__ __launch_bounds__(256) void conv_small_kernel(const float* __restrict__ in,
                                                         const float* __restrict__ wt,
                                                         float* __restrict__ out, ConvGeom g,
                                                         Epi e) {
  constexpr int KK = KH * KW;
  __shared__ floatx4 ws4[SMALL_NB * KK * NB / 4];  // [c][t][n], c < C <= 12 (dispatch)
  float* ws = reinterpret_cast<float*>(ws4);
  for (int i = threadIdx.x; i < g.C * KK * NB; i += 256) {
    const int n = i % NB, ct = i / NB;
    const int c = ct / KK, t = ct - c * KK;
    ws[i] = n < g.N ? wt[(int64_t)n * g.wsn + (int64_t)c * g.wsc + t] : 0.f;
  }
  __syncthreads();
  const int wo2 = (g.Wo + 1) >> 1;
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (tid >= (int64_t)g.B * g.Hout * wo2) return;
  const int j = (int)(tid % wo2);
  const int64_t bh = tid / wo2;
  const int h = (int)(bh % g.Hout), b = (int)(bh / g.Hout);
  const int wo0 = 2 * j;
  float acc[2][NB];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int n = 0; n < NB; ++n) acc[p][n] = 0.f;
  const float* inb = in + (int64_t)b * g.C * g.Hin * g.Win;
  for (int c = 0; c < g.C; ++c) {
    const float* inc = inb + (int64_t)c * g.Hin * g.Win;
#pragma unroll
    for (int kh = 0; kh < KH; ++kh) {
      int hi = MODE == GATHER_F ? h + kh - g.oph : h - kh + g.oph;
      bool hv = hi >= 0 && hi < g.Hin;
      if (REPL) {
        hi = hi < 0 ? 0 : (hi >= g.Hin ? g.Hin - 1 : hi);
        hv = true;
      }
      const float* row = inc + (int64_t)(hv ? hi : 0) * g.Win;
#pragma unroll
      for (int kw = 0; kw < KW; ++kw) {
        const floatx4* w4 = ws4 + ((c * KK + kh * KW + kw) * NB) / 4;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          const int wo = wo0 + p;
          int wi;
          bool ok;
          if (MODE == GATHER_F) {
            wi = wo * SW + kw - g.opw;
            ok = wi >= 0 && wi < g.Win;
            if (REPL) {
              wi = wi < 0 ? 0 : (wi >= g.Win ? g.Win - 1 : wi);
              ok = true;
            }
          } else {
            const int wn = wo - kw + g.opw;
            if (SW == 2 && ((wn & 1) != 0)) continue;  // parity: uniform per (p, kw)
            wi = wn / SW;
            ok = wn >= 0 && wi < g.Win;
          }
          ok = ok && hv && wo < g.Wo;
          const float v = ok ? row[ok ? wi : 0] : 0.f;
#pragma unroll
          for (int q = 0; q < NB / 4; ++q) {
            const floatx4 w = w4[q];
            acc[p][4 * q + 0] = fmaf(w[0], v, acc[p][4 * q + 0]);
            acc[p][4 * q + 1] = fmaf(w[1], v, acc[p][4 * q + 1]);
            acc[p][4 * q + 2] = fmaf(w[2], v, acc[p][4 * q + 2]);
            acc[p][4 * q + 3] = fmaf(w[3], v, acc[p][4 * q + 3]);
          }
        }
      }
    }
  }
  const uint64_t seed = e.drop_p > 0.f ? mix_seed(e.seed_ptr, e.offset) : 0ull;
  const int64_t hw = (int64_t)g.Hout * g.Wo;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int wo = wo0 + p;
    if (wo >= g.Wo) continue;
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      if (n >= g.N) continue;
      const int64_t o = ((int64_t)b * g.N + n) * hw + (int64_t)h * g.Wo + wo;
      float v = acc[p][n] + (e.bias ? e.bias[n] : 0.f);
      if (e.drop_p > 0.f) v = uniform01(seed, (uint64_t)o) >= e.drop_p ? v * e.drop_scale : 0.f;
      if (e.residual) v += e.residual[o];
      out[o] = v;
    }
  }
}

struct HaloPlan {
  HaloGeom g;
  int FN, KS;
  size_t lds;
};

// mode F: (oh, ow) = (PH, PW) of the conv;  T: (KH-1-oph, KW-1-opw) of the T gather
static bool halo_plan(int mode, int B, int C, int Hin, int Win, int N, int Hout, int Wo, int KH,
                      int KW, int SW, int oh, int ow, int64_t wsn, int64_t wsc, HaloPlan* pl) {
  HaloGeom g;
  g.C = C; g.Cp = (C + 3) & ~3; g.Hin = Hin; g.Win = Win; g.N = N; g.Hout = Hout; g.Wo = Wo;
  g.oh = oh; g.ow = ow;
  g.HP = Hout + KH - 1;
  g.WP = mode == GATHER_F ? (Wo - 1) * SW + KW : Wo + KW - 1;
  const int hw = g.HP * g.WP;
  g.PS = hw + ((16 - hw % 32) + 32) % 32;
  g.P = Hout * Wo;
  g.MT = (g.P + 15) / 16;
  g.wsn = wsn; g.wsc = wsc;
  const int K = KH * KW * g.Cp;
  if (Wo < 2 || g.WP < 2 || K < 2 || g.P >= (1 << 16)) return false;
  g.dv_hw = make_div16(hw);
  g.dv_wp = make_div16(g.WP);
  g.dv_wo = make_div16(Wo);
  g.dv_k = make_div16(K);
  const int KST = K + ((2 - K % 32) + 32) % 32;
  const int fn_cover = N <= 16 ? 1 : (N <= 32 ? 2 : 4);
  for (int FN = fn_cover; FN >= 1; FN /= 2) {
    const int NB = FN * 16;
    if ((N + NB - 1) / NB > 4) break;  // the image would be re-staged by > 4 blocks
    const int KS = g.MT <= 4 ? 4 : 1;
    size_t fl = (size_t)g.Cp * g.PS + (size_t)NB * KST + K;
    const size_t red = KS > 1 ? (size_t)3 * FN * 4 * 64 * 4 : 0;
    if (red > fl) fl = red;
    if (fl * 4 <= (size_t)HALO_LDS_MAX) {
      g.KST = KST;
      pl->g = g;
      pl->FN = FN;
      pl->KS = KS;
      pl->lds = fl * 4;
      return true;
    }
  }
  (void)B;
  return false;
}

// returns whether the epilogue applied e's eval BN / Snake
template <int MODE, int KH, int KW, int SW, bool REPL>
static bool launch_halo_pl(const float* in, const float* wt, float* out, const HaloPlan& pl, int B,
                           const Epi& e, hipStream_t st) {
  const dim3 grid(B, (pl.g.N + pl.FN * 16 - 1) / (pl.FN * 16));
  // the eval EncBlock (replicate 3x4 stride-2 conv -> BN -> Snake): an epilogue-fused instance
  if constexpr (MODE == GATHER_F && KH == 3 && KW == 4 && SW == 2 && REPL) {
    if (e.bn_rv) {
#define HP_(FN_, KS_)                                                                             \
  hipLaunchKernelGGL((conv_halo_kernel<MODE, KH, KW, SW, REPL, FN_, KS_, true>), grid, dim3(256), \
                     pl.lds, st, in, wt, out, pl.g, e)
      if (pl.KS == 4) {
        if (pl.FN == 1) HP_(1, 4); else if (pl.FN == 2) HP_(2, 4); else HP_(4, 4);
      } else {
        if (pl.FN == 1) HP_(1, 1); else if (pl.FN == 2) HP_(2, 1); else HP_(4, 1);
      }
#undef HP_
      return true;
    }
  }
#define H_(FN_, KS_)                                                                          \
  hipLaunchKernelGGL((conv_halo_kernel<MODE, KH, KW, SW, REPL, FN_, KS_>), grid, dim3(256), \
                     pl.lds, st, in, wt, out, pl.g, e)
  if (pl.KS == 4) {
    if (pl.FN == 1) H_(1, 4); else if (pl.FN == 2) H_(2, 4); else H_(4, 4);
  } else {
    if (pl.FN == 1) H_(1, 1); else if (pl.FN == 2) H_(2, 1); else H_(4, 1);
  }
#undef H_
  return false;
}

// Measured per shape on MI355X (tools/conv_shapes_bench.py, halo vs staged GEMM at the
// step's shapes): the halo tile wins while the gathered channel count is small (its
// per-image restaging of the weight panel grows with C), loses to the tap-major GEMM
// for 1x1 convs, for C >= 32, and for the stride-2 transposed gathers.  A register-
// resident-weight variant (whole reduction row per wave in VGPRs) was 1.5-4x slower
// than both (1 wave/SIMD, uncoalesced weight loads) and was dropped.
static bool halo_preferred(int mode, int C, int KK, int SW, int N, int64_t Mpos) {
  if (conv_config().halo & 4) return true;
  if (KK == 1 || C >= 32) return false;
  // 16 / 48 channels into >= 128 on a full grid: the 32x32-MFMA tile with a 16-wide K stage
  if (conv_config().t32 && C % 16 == 0 && N % 128 == 0 && (Mpos + 95) / 96 * (N / 128) >= 192)
    return false;
  if (mode == GATHER_T && SW == 2) return false;
  return true;
}

// the halo path where it is on, preferred and the image + weight panel fit in LDS
template <int MODE, int KH, int KW, int SW, bool REPL>
static bool launch_halo_t(const float* in, const float* wt, float* out, const ConvGeom& g,
                          const Epi& e, hipStream_t st, bool* post) {
  HaloPlan pl;
  const int oh = MODE == GATHER_F ? g.oph : KH - 1 - g.oph;
  const int ow = MODE == GATHER_F ? g.opw : KW - 1 - g.opw;
  if (!((conv_config().halo & 1) && halo_preferred(MODE, g.C, KH * KW, SW, g.N, g.Mpos) &&
        halo_plan(MODE, g.B, g.C, g.Hin, g.Win, g.N, g.Hout, g.Wo, KH, KW, SW, oh, ow, g.wsn, g.wsc,
                  &pl)))
    return false;
  TVQ_PLAN("conv_halo");
  *post = launch_halo_pl<MODE, KH, KW, SW, REPL>(in, wt, out, pl, g.B, e, st);
  return true;
}

bool launch_halo(int mode, int kind, bool repl, const float* in, const float* wt, float* out,
                 const ConvGeom& g, const Epi& e, hipStream_t st, bool* post) {
  *post = false;
#define M_(m, a, b_, c, d) return launch_halo_t<m, a, b_, c, d>(in, wt, out, g, e, st, post);
  TVQ_DISPATCH_CONV(mode, kind, repl, M_)
#undef M_
  return false;
}

// measured per shape (tools/conv_shapes_bench.py, r02): the direct kernel wins for the
// stride-2 transposed gathers with <= 12 channels on both sides (the decoders' ConvT tail
// and DecBlocks 8->4, the EncBlocks' data gradients), loses to the halo / staged paths
// elsewhere
template <int MODE, int KH, int KW, int SW, bool REPL>
static bool launch_small_t(const float* in, const float* wt, float* out, const ConvGeom& g,
                           const Epi& e, hipStream_t st) {
  if (!(MODE == GATHER_T && SW == 2 && g.C <= 12 && g.N <= 12)) return false;
  const int64_t th = (int64_t)g.B * g.Hout * ((g.Wo + 1) / 2);
  // outputs per thread rounded up to 4 (every channel's sum in the same order)
  const dim3 grid((unsigned)((th + 255) / 256));
  TVQ_PLAN("conv_small n%d", g.N);
  if (g.N <= 4)
    hipLaunchKernelGGL((conv_small_kernel<MODE, KH, KW, SW, REPL, 4>), grid, dim3(256), 0, st, in, wt, out, g, e);
  else if (g.N <= 8)
    hipLaunchKernelGGL((conv_small_kernel<MODE, KH, KW, SW, REPL, 8>), grid, dim3(256), 0, st, in, wt, out, g, e);
  else if (g.N <= 12)
    hipLaunchKernelGGL((conv_small_kernel<MODE, KH, KW, SW, REPL, 12>), grid, dim3(256), 0, st, in, wt, out, g, e);
  else
    hipLaunchKernelGGL((conv_small_kernel<MODE, KH, KW, SW, REPL, 16>), grid, dim3(256), 0, st, in, wt, out, g, e);
  return true;
}

bool launch_small(int mode, int kind, bool repl, const float* in, const float* wt, float* out,
                  const ConvGeom& g, const Epi& e, hipStream_t st) {
#define M_(m, a, b_, c, d) return launch_small_t<m, a, b_, c, d>(in, wt, out, g, e, st);
  TVQ_DISPATCH_CONV(mode, kind, repl, M_)
#undef M_
  return false;
}

// ---------------------------------------------------------------- few outputs, wide input
// The HF band's 128 -> <= 16 channel convs on (B, 128, 3, 32): ResBlock(128, 16)'s 3x3 conv1
// and 1x1 projection forward (the decoder's first block), ResBlock(16, 128)'s data gradients
// (the encoder's last block) -- a 24,576 x 16 output with a 1,152- (or 128-) deep reduction.
// The tap-major GEMM gave them 96 blocks of a 16-row tile (0.11 of the fp32 peak, 51 us for
// the 3x3 at B = 256).  Here one 8-wave block owns one image: its C x 3 x 32 input is staged
// once into zero-padded LDS halo planes (C x 5 x 34), every B operand of the
// v_mfma_f32_16x16x4_f32 chains is an LDS read at an immediate offset from the lane's base
// (the reduction is tap-major, k = tap * C + c, so a step never crosses a tap), and the A
// operand comes straight from the [tap][c][n]-packed weight (a wave's 64 lanes read 256
// contiguous bytes per step).  Wave w takes input channels 32 (w & 3) .. for every tap (72
// steps for 3x3) and position tiles 3 (w >> 2) .. + 2 (3 chains sharing each weight value);
// the 4 channel splits are summed in LDS in split order.
constexpr int N16_H = 3, N16_W = 32, N16_P = 96, N16_WPD = 34, N16_PS = 176, N16_T = 512;
bool n16_geom_ok(int mode, int kind, const ConvGeom& g) {  // kind 1 (3x3) or 2 (1x1)
  const int KH = kind == 1 ? 3 : 1, KW = KH;
  return (kind == 1 || kind == 2) && g.N <= 16 && g.C == 128 && g.Hin == N16_H && g.Hout == N16_H &&
         g.Win == N16_W && g.Wo == N16_W && g.oph == KH / 2 && g.opw == (KW - 1) / 2 &&
         (mode == GATHER_F || mode == GATHER_T);
}
constexpr size_t N16_LDS = 4 * ((size_t)128 * N16_PS + 4 * 16 * N16_P);

template <int MODE, int KH, int KW, bool POST>
__global__ __launch_bounds__(N16_T) void conv_n16_kernel(const float* __restrict__ in,
                                                         const float* __restrict__ wp,
                                                         float* __restrict__ out, ConvGeom g,
                                                         Epi e) {
  constexpr int C = 128, KK = KH * KW, SPT = 8;  // 8 steps of 4 channels per tap and split
  extern __shared__ float n16_smem[];
  float* Pl = n16_smem;               // [C][PS] halo planes
  float* red = n16_smem + C * N16_PS;  // [4 splits][16 rows][96 positions]
  const int tid = threadIdx.x, lane = tid & 63, j = lane & 15, kq = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ks = w & 3, pg = w >> 2, b = blockIdx.x, N = g.N;
  // the image's values (24 per thread in flight) and this wave's weights
  const float* inb = in + (int64_t)b * C * N16_P;
  float xv[C * N16_P / N16_T];
#pragma unroll
  for (int i = 0; i < C * N16_P / N16_T; ++i) xv[i] = inb[tid + N16_T * i];
  const int nn = j < N ? j : N - 1;
  float a[KK][SPT];
#pragma unroll
  for (int t = 0; t < KK; ++t)
#pragma unroll
    for (int s = 0; s < SPT; ++s) a[t][s] = wp[((int64_t)t * C + 32 * ks + 4 * s + kq) * N + nn];
  for (int i = tid; i < C * N16_PS; i += N16_T) Pl[i] = 0.f;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < C * N16_P / N16_T; ++i) {
    const int el = tid + N16_T * i, c = el / N16_P, p = el - c * N16_P;
    Pl[c * N16_PS + (p / N16_W + 1) * N16_WPD + p % N16_W + 1] = xv[i];
  }
  __syncthreads();
  // lane base: channel 32 ks + kq, the window centre of position 16 tile + j of row tile / 2
  const float* sp = Pl + (32 * ks + kq) * N16_PS + N16_WPD + 1 + j;
  floatx4 acc[3];
#pragma unroll
  for (int f = 0; f < 3; ++f) acc[f] = floatx4{0.f, 0.f, 0.f, 0.f};
  int pb[3];
#pragma unroll
  for (int f = 0; f < 3; ++f) {
    const int tile = 3 * pg + f;  // 16 positions of row tile / 2
    pb[f] = (tile >> 1) * N16_WPD + 16 * (tile & 1);
  }
#pragma unroll
  for (int t = 0; t < KK; ++t) {
    const int kh = t / KW, kw = t % KW;
    const int dr = MODE == GATHER_F ? kh - KH / 2 : KH / 2 - kh;
    const int dc = MODE == GATHER_F ? kw - (KW - 1) / 2 : (KW - 1) / 2 - kw;
    const int off = dr * N16_WPD + dc;
#pragma unroll
    for (int s = 0; s < SPT; ++s)
#pragma unroll
      for (int f = 0; f < 3; ++f)
        acc[f] = mfma16x16x4(a[t][s], sp[pb[f] + 4 * s * N16_PS + off], acc[f]);
  }
#pragma unroll
  for (int f = 0; f < 3; ++f)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[(ks * 16 + 4 * kq + r) * N16_P + 16 * (3 * pg + f) + j] = acc[f][r];
  __syncthreads();
  const uint64_t seed = e.drop_p > 0.f ? mix_seed(e.seed_ptr, e.offset) : 0ull;
  for (int el = tid; el < N * N16_P; el += N16_T) {
    const int n = el / N16_P, p = el - n * N16_P;
    float v = red[n * N16_P + p];
#pragma unroll
    for (int k = 1; k < 4; ++k) v += red[(k * 16 + n) * N16_P + p];
    v += e.bias ? e.bias[n] : 0.f;
    if (POST) v = epi_post(e, v, n);
    const int64_t o = ((int64_t)b * N + n) * N16_P + p;
    if (e.drop_p > 0.f) v = uniform01(seed, (uint64_t)o) >= e.drop_p ? v * e.drop_scale : 0.f;
    if (e.residual) v += e.residual[o];
    out[o] = v;
  }
}

template <int MODE, int KH, int KW>
static void launch_n16_t(const float* in, const float* wt, float* out, const ConvGeom& g,
                         const Epi& e, hipStream_t st) {
  static bool attr = [] {
    (void)hipFuncSetAttribute((const void*)conv_n16_kernel<MODE, KH, KW, false>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)N16_LDS);
    (void)hipFuncSetAttribute((const void*)conv_n16_kernel<MODE, KH, KW, true>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)N16_LDS);
    return true;
  }();
  (void)attr;
  TVQ_PLAN("conv_n16 k%dx%d mode%d n%d", KH, KW, MODE, g.N);
  if (e.bn_rv) {
    hipLaunchKernelGGL((conv_n16_kernel<MODE, KH, KW, true>), dim3(g.B), dim3(N16_T), N16_LDS, st,
                       in, wt, out, g, e);
  } else {
    hipLaunchKernelGGL((conv_n16_kernel<MODE, KH, KW, false>), dim3(g.B), dim3(N16_T), N16_LDS,
                       st, in, wt, out, g, e);
  }
}

void launch_n16(int mode, int kind, const float* in, const float* wp, float* out,
                const ConvGeom& g, const Epi& e, hipStream_t st) {
  if (mode == GATHER_F) {
    if (kind == 1) launch_n16_t<GATHER_F, 3, 3>(in, wp, out, g, e, st);
    else launch_n16_t<GATHER_F, 1, 1>(in, wp, out, g, e, st);
  } else {
    if (kind == 1) launch_n16_t<GATHER_T, 3, 3>(in, wp, out, g, e, st);
    else launch_n16_t<GATHER_T, 1, 1>(in, wp, out, g, e, st);
  }
}

}  // namespace tvq
