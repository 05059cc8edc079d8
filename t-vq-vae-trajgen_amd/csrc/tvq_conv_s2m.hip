// Stride-2 convolutions of the LF band's middle levels (16 <-> 32 and 32 <-> 64 channels on
// H = 3 maps 8-32 wide): conv_s2m_t, the T gather of the 3x4 stride-(1,2) kernel -- the
// ConvTranspose forward (Hout 3) and the replicate conv's data gradient (Hout 5, folded onto
// dx inside the kernel).
#include "tvq_conv_core.h"

#include <type_traits>

namespace tvq {

// T: out[b,n,h,wo] = sum w(n,c,kh,kw) in[b,c,h-kh+oph,(wo-kw+opw)/2] over the integer sources.
// The outputs are split by column parity (wo = 2 m + par): a parity leaves two kw (q, q + 2
// with q = (par + opw) & 1) whose source columns are m + D and m + D - 1, D = (par+opw-q)/2, so
// K is c x kh x {two kw} with no zero terms.  A block takes one image (24-85 columns per
// parity); its columns are (h, m) flattened, 16 to a 16x16x4 MFMA tile.
//
// LDS holds the image's three real rows as [row][c][XR] with staged column j <-> source column
// j - 1 (zeros left of column 0 and from Win on), and ZR rows of zeros before and after them,
// so the row h - kh + oph of every tap exists and the address stays linear: lane base
// (h, m, c = g4) + a per-step constant (kh, c / 4, kw), which is an instruction immediate.
// An MFMA's K is the four channels 4 cg .. 4 cg + 3 of one tap, lane group g4 = c % 4.
//
// Order of the sums: the one conv_tap's split-K form has at these shapes, so the results are
// the staged path's bit for bit (a zero term adds nothing, leaving it out changes no bit).
// There a K-step is one tap x 32 channels, taps ascending, a split is 4 K-steps with its own
// accumulator, and the splits are added in order.  Per parity that is S chains of VT taps
// (64 channels: 6 chains of one tap; 32 channels: 3 chains, the two taps of one kh), each
// chain an MFMA chain over its taps' channels in ascending order starting from zero, then
// v = ((p0 + p1) + p2) ... + bias.  The equality holds where conv_tap runs 4 K-steps per split
// (tap_splits, a grid-size heuristic: splits6 / splits3 up to B ~ 290 at these shapes); were
// that retuned, this order would stay a fixed, equally accurate one, only no longer that
// path's.  Why it is kept: the bias gradient of a conv in front of a BatchNorm is
// rounding noise around zero that AdamW normalises to full-size updates, so another order
// here, though as accurate, moves those parameters by 1e-4 relative within 25 steps.
//
// Waves (8): parity = wid & 1; the next bit is the output-channel tile (N = 32) or the column
// tiles' interleave (N = 16); the last bit halves the chains, so a SIMD holds two waves and
// one's MFMA chain covers the other's LDS reads.  A wave's weights (16 rows x its chains' K)
// stay in registers, read once from the packed [tap][c][n] weight.  The lower wave's sum
// goes through LDS to the upper wave, which goes on adding its chains and runs the epilogue.
//
// FOLD (Hout 5, the replicate canvas of width Wx + 2): the tiles go to an LDS canvas and a
// second pass writes dx = rows 0+1 | 2 | 3+4, columns 0+1 | j | Wx + (Wx+1), summed row by row
// as replicate_fold_kernel does.
// Every sum has a fixed order; no atomics.
struct S2mGeom {
  int N, Win, Wo, MP, opw;
  int64_t wsn, wsc, wst;
};

extern __shared__ float s2m_lds[];

template <int C, int XR, int HO>
struct S2M {
  static constexpr int ZR = HO == 5 ? 2 : 1;
  static constexpr int RW = C * XR;            // one row of every channel
  static constexpr int XN = (3 + 2 * ZR) * RW;  // zeros | the three rows | zeros
  static constexpr int WC = 2 * (XR - 2);       // canvas row stride (FOLD)
  __host__ __device__ static constexpr int cv_floats(int N, bool fold) {
    return fold ? N * 5 * WC : 0;
  }
  static int lds_bytes(int N, bool fold, int TC) {
    return (XN + cv_floats(N, fold) + 4 * TC * 256) * 4;
  }
};

template <int C, int NT, int XR, int HO, bool FOLD, int TC>
__global__ __launch_bounds__(512) void conv_s2m_t_kernel(const float* __restrict__ in,
                                                         const float* __restrict__ wt,
                                                         const float* __restrict__ bias,
                                                         float* __restrict__ out, S2mGeom g) {
  using L = S2M<C, XR, HO>;
  constexpr int CG = C / 4;                  // MFMA steps of one tap
  constexpr int VT = C == 64 ? 1 : 2;        // the parity's taps per chain
  constexpr int S = 6 / VT, S0 = (S + 1) / 2;  // chains; the lower wave takes the first S0
  constexpr int THR = 512;
  constexpr int IMG = C * 3;     // rows of one image (x Win floats)
  static_assert(!FOLD || HO == 5, "fold: replicate canvas");
  float* const Xs = s2m_lds;
  const int tid = threadIdx.x, lane = tid & 63, r16 = lane & 15, g4 = lane >> 4;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int par = wid & 1, o = (wid >> 1) & 1, kh2 = wid >> 2;  // kh2: the wave's half of K
  const int nt = o % NT, tfirst = o / NT, tstep = 2 / NT;
  const int b0 = blockIdx.x;
  const int q = (par + g.opw) & 1, D = (par + g.opw - q) >> 1;

  // the image's rows: flat, coalesced; in flight while the weights load and the LDS is cleared
  constexpr int XPER_MAX = (IMG * (XR - 2) + THR - 1) / THR;  // Win <= XR - 2
  const int nin = IMG * g.Win;
  float xv[XPER_MAX];
#pragma unroll
  for (int u = 0; u < XPER_MAX; ++u) {
    const int i = tid + THR * u;
    xv[u] = in[(int64_t)b0 * IMG * g.Win + (i < nin ? i : 0)];
  }
  // weights of row n = 16 nt + r16, channel 4 cg + g4 of the wave's chains: chain z's tap j is
  // the parity's tap vt = z VT + j = (kh = vt / 2, kw = q + 2 (vt % 2))
  float af[S0 * VT * CG];
  auto load_w = [&](auto zb_) {
    constexpr int ZB = decltype(zb_)::value, NCH = ZB ? S - S0 : S0;
    const int n = 16 * nt + r16;
#pragma unroll
    for (int i = 0; i < NCH * VT; ++i) {
      const int vt = ZB * VT + i, kh = vt / 2, kw = q + 2 * (vt % 2);
#pragma unroll
      for (int cg = 0; cg < CG; ++cg)
        af[i * CG + cg] = wt[n * g.wsn + (4 * cg + g4) * g.wsc + (kh * 4 + kw) * g.wst];
    }
  };
  if (kh2 == 0) load_w(std::integral_constant<int, 0>{});
  else load_w(std::integral_constant<int, S0>{});
  for (int i = tid; i < L::XN / 4; i += THR)
    reinterpret_cast<floatx4*>(Xs)[i] = floatx4{0.f, 0.f, 0.f, 0.f};
  __syncthreads();
  {
    const int rw = 3 * g.Win;
#pragma unroll
    for (int u = 0; u < XPER_MAX; ++u) {
      const int i = tid + THR * u;
      if (i < nin) {
        const int c = i / rw, rr = i - c * rw, r = rr / g.Win, wi = rr - r * g.Win;
        Xs[(L::ZR + r) * L::RW + c * XR + 1 + wi] = xv[u];
      }
    }
  }
  __syncthreads();

  const int ncols = HO * g.MP, ntiles = (ncols + 15) >> 4;
  float* const Cv = Xs + L::XN;  // FOLD: [n][5][WC]
  floatx4* const Up = reinterpret_cast<floatx4*>(Cv + L::cv_floats(g.N, FOLD));
  float bv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) bv[r] = (!FOLD && bias) ? bias[16 * nt + 4 * g4 + r] : 0.f;

  const int niter = (ntiles + tstep * TC - 1) / (tstep * TC);  // the same for every wave
  for (int it = 0; it < niter; ++it) {
    const int t0 = tfirst + it * tstep * TC;
    const float* xb[TC];
    int ch[TC], cm[TC];
    bool cv[TC];
    floatx4 acc[TC];
#pragma unroll
    for (int u = 0; u < TC; ++u) {
      const int j = (t0 + u * tstep) * 16 + r16;
      cv[u] = j < ncols;
      const int jj = cv[u] ? j : 0;
      ch[u] = jj / g.MP;
      cm[u] = jj - ch[u] * g.MP;
      // row h - kh + oph of the staged block = h + kh' (oph + ZR - 2 = 0 for both forms)
      xb[u] = Xs + ch[u] * L::RW + g4 * XR + cm[u] + D;
      acc[u] = floatx4{0.f, 0.f, 0.f, 0.f};
    }
    // the wave's chains, each from zero: pc[i][u]
    floatx4 pc[S0][TC];
    auto chains = [&](auto zb_) {
      constexpr int ZB = decltype(zb_)::value, NCH = ZB ? S - S0 : S0;
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
#pragma unroll
        for (int u = 0; u < TC; ++u) pc[i][u] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < VT; ++j) {
          const int vt = (ZB + i) * VT + j, khp = 2 - vt / 2, ep = 1 - vt % 2;
#pragma unroll
          for (int cg = 0; cg < CG; ++cg)
#pragma unroll
            for (int u = 0; u < TC; ++u)
              pc[i][u] = mfma16x16x4(af[(i * VT + j) * CG + cg],
                                     xb[u][khp * L::RW + 4 * cg * XR + ep], pc[i][u]);
        }
      }
    };
    if (kh2 == 0) {
      chains(std::integral_constant<int, 0>{});
#pragma unroll
      for (int u = 0; u < TC; ++u) {
        acc[u] = pc[0][u];
#pragma unroll
        for (int i = 1; i < S0; ++i) acc[u] = acc[u] + pc[i][u];
        Up[(wid * TC + u) * 64 + lane] = acc[u];
      }
    } else {
      chains(std::integral_constant<int, S0>{});
    }
    __syncthreads();
    if (kh2 == 1) {
#pragma unroll
      for (int u = 0; u < TC; ++u) {
        acc[u] = Up[((wid & 3) * TC + u) * 64 + lane];
#pragma unroll
        for (int i = 0; i < S - S0; ++i) acc[u] = acc[u] + pc[i][u];
      }
    }
#pragma unroll
    for (int u = 0; u < TC; ++u) {
      const int wo = 2 * cm[u] + par;
      const bool pv = kh2 == 1 && cv[u] && wo < g.Wo;
      if constexpr (FOLD) {
        if (pv) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            Cv[((16 * nt + 4 * g4 + r) * 5 + ch[u]) * L::WC + wo] = acc[u][r];
        }
      } else {
        if (pv) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int n = 16 * nt + 4 * g4 + r;
            out[(((int64_t)b0 * g.N + n) * HO + ch[u]) * g.Wo + wo] = acc[u][r] + bv[r];
          }
        }
      }
    }
    if (it + 1 < niter) __syncthreads();  // the lower waves' sums have been read
  }
  if constexpr (FOLD) {
    __syncthreads();
    const int Wx = g.Wo - 2, tot = g.N * 3 * Wx;
    float* const dx = out + (int64_t)b0 * g.N * 3 * Wx;
    for (int i = tid; i < tot; i += THR) {
      const int x = i % Wx, t = i / Wx, h = t % 3, bn = t / 3;
      const float* p = Cv + bn * 5 * L::WC;
      const int hlo = h == 0 ? 0 : h + 1, hhi = h == 2 ? 4 : h + 1;
      const int wlo = x == 0 ? 0 : x + 1, whi = x == Wx - 1 ? Wx + 1 : x + 1;
      float v = 0.f;
      for (int hh = hlo; hh <= hhi; ++hh)
        for (int ww = wlo; ww <= whi; ++ww) v += p[hh * L::WC + ww];
      dx[i] = v;
    }
  }
}

// The shapes conv_s2m_t takes: 64 -> 32 channels with <= 10 output columns per parity, or
// 32 -> 16 with <= 18 (the LF band: output widths 16 / 32, canvases 18 / 34).  0 none, 1 the
// Hout 3 form (oph 1, opw 1), 2 the canvas form (Hout 5, oph 0, opw 0)
static int s2m_t_form(const ConvGeom& g) {
  if (!conv_config().s2m || g.Hin != 3 || g.Wo < 4) return 0;
  const int MP = (g.Wo + 1) / 2;
  if (!((g.C == 64 && g.N == 32 && MP <= 10) || (g.C == 32 && g.N == 16 && MP <= 18))) return 0;
  if (g.Win > MP || g.Win < 1) return 0;
  if (g.Hout == 3 && g.oph == 1 && g.opw == 1) return 1;
  if (g.Hout == 5 && g.oph == 0 && g.opw == 0) return 2;
  return 0;
}
bool s2m_t_fits(const ConvGeom& g, const Epi& e) {
  return s2m_t_form(g) == 1 && !e.residual && e.drop_p <= 0.f && !e.bn_rv && !e.bn_part;
}
bool s2m_fold_fits(const ConvGeom& g) { return s2m_t_form(g) == 2; }

template <int C, int NT, int XR>
static void launch_s2m_t_i(bool fold, const float* in, const float* wt, const float* bias,
                           float* out, const ConvGeom& g, hipStream_t st) {
  S2mGeom s;
  s.N = g.N; s.Win = g.Win; s.Wo = g.Wo; s.MP = (g.Wo + 1) / 2; s.opw = g.opw;
  s.wsn = g.wsn; s.wsc = g.wsc; s.wst = g.wst;
  // column tiles per wave and pass: an image is 45 / 85 columns per parity in the canvas form
  // (3 tiles a wave) and 24 / 48 in the Hout 3 form (2 tiles)
  const dim3 grid((unsigned)g.B);
  TVQ_PLAN("conv_s2m_t c%d n%d hout%d%s blocks=%u", C, 16 * NT, g.Hout, fold ? " fold" : "",
           grid.x);
  if (fold)
    hipLaunchKernelGGL((conv_s2m_t_kernel<C, NT, XR, 5, true, 3>), grid, dim3(512),
                       (S2M<C, XR, 5>::lds_bytes(g.N, true, 3)), st, in, wt, bias, out, s);
  else
    hipLaunchKernelGGL((conv_s2m_t_kernel<C, NT, XR, 3, false, 2>), grid, dim3(512),
                       (S2M<C, XR, 3>::lds_bytes(g.N, false, 2)), st, in, wt, bias, out, s);
}
// g's weight strides may be the packed view's (pack_weight) or the parameter's own
void launch_s2m_t(bool fold, const float* in, const float* wt, const float* bias, float* out,
                  const ConvGeom& g, hipStream_t st) {
  if (g.C == 64) launch_s2m_t_i<64, 2, 12>(fold, in, wt, bias, out, g, st);
  else launch_s2m_t_i<32, 1, 20>(fold, in, wt, bias, out, g, st);
}

}  // namespace tvq
