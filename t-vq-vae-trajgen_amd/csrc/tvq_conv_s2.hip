// Stride-2 small-channel convolutions of the conv engine: conv_s2f / conv_s2t (forward, data
// gradient, the fold form, the BN-statistics epilogue) and conv_wgrad_s2.
#include "tvq_conv_core.h"
#include "tvq_reduce.h"

namespace tvq {

// ---------------------------------------------------------------- stride-2 small-channel
// The 3x4 stride-2 convs with <= 16 channels on both sides at the bands' full widths: the
// EncBlock convs (F, replicate padding), the decoders' ConvTranspose tails (T) and the data
// gradients of both (T into the replicate canvas / F).  The staged GEMMs above ran them at
// 0.02-0.1 of peak: 9 K-steps of 16 with a branchy per-element gather and two barriers
// each.  Here a stage is one image's 64-wide output segment on every output row: the three
// input rows it reads (C x 3 x the segment's columns) are staged in LDS, column padding
// applied while staging, and each wave runs its 16-position tiles as 16x16x4 MFMA chains
// (rows = output channels, weights held in registers; columns = positions, read from the
// staged rows).  F: k = (c, kh) x kw on the lane groups, every tap of the window is a
// term.  T (stride-2 gather): the output parity fixes which two kw have an integer source,
// so each wave takes one parity and its K is c x kh x {two kw} (half the taps, no zero terms).
//
// Only the rows that exist are staged.  The padding rows (hi = -1, 3 of F; -2, -1, 3, 4 of T)
// are not loaded: a replicate tap reads the clamped row, a zero tap reads rows of zeros that
// are written once per block, so every MFMA of every chain keeps its operands and its place.
//
// A block takes a contiguous run of stages (grid = min(stages, cap), tvq_conv_s2_cap).  The
// rows go global -> LDS by global_load_lds (4-byte form: a 257-wide row is not 16-byte
// aligned; one wave instruction fills 64 consecutive floats from 64 per-lane addresses, so
// replicate padding is a clamped address and zero padding the address of a zero word), into
// two LDS buffers: while stage s multiplies and stores, stage s + 1 lands in the other one.
// No prefetched value lives in a register.  Order per stage: wait for the DMA, barrier,
// issue the next stage's DMA, MFMA chains, epilogue.  The one-shot launch (cap >= stages) is
// the same kernel with one buffer.
constexpr int S2_SEG = 64;                 // output positions per segment
constexpr int S2_XRF = 2 * S2_SEG + 2;     // F: staged columns (stride 2, 4 taps)
constexpr int S2_XRT = S2_SEG / 2 + 4;     // T: staged columns (source offsets -2..2)

extern __shared__ float s2_lds[];
static __device__ float s2_zero_word[4];  // never written: the source of a zero-padded cell

// one wave instruction: 64 floats from the lanes' `src` to dst_wave[0..63]
__device__ __forceinline__ void s2_glds(const float* src, float* dst_wave) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)dst_wave, 4, 0, 0);
}
// the block's DMA has landed and every wave is done with the buffer it will overwrite
__device__ __forceinline__ void s2_ring_sync() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

struct S2Run {
  int nst, spr;  // stages of the launch, stages per block
};

// STATS epilogue of the stride-2 kernels (4 waves): lane (r16, g4) holds its positions' sums
// of channels 4 g4 + r in s1 / s2 (fp64); the 16 lanes of a g4 group are combined by a fixed
// xor tree, the 4 waves in wave order, and each channel's partial of stage `slot` (of nslots)
// is written for bn_apply_part_kernel (tvq_norm.hip), which finishes the statistics in the
// consumer.  Replaces the BatchNorm's separate statistics pass over the conv output.
__device__ __forceinline__ void s2_bn_stats_block(double (&s1)[4], double (&s2)[4], int nbase,
                                                  int N, double* __restrict__ part, int slot,
                                                  int nslots) {
  __shared__ double red[4][16][2];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
      s1[r] += __shfl_xor(s1[r], o, 64);
      s2[r] += __shfl_xor(s2[r], o, 64);
    }
  if ((lane & 15) == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      red[wid][nbase + r][0] = s1[r];
      red[wid][nbase + r][1] = s2[r];
    }
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < 2 * N) {
    const int n = t >> 1, k = t & 1;
    part[((int64_t)n * nslots + slot) * 2 + k] =
        ((red[0][n][k] + red[1][n][k]) + red[2][n][k]) + red[3][n][k];
  }
}

// F: out[b,n,h,wo] = sum_{c,kh,kw} w(n,c,kh,kw) in[b,c,h+kh-1,2wo+kw-opw], H = 3
// LDS: [buffer][row 0..2][c][S2_XRF] (each buffer padded to whole wave instructions), then
// CS rows of zeros for the taps of a zero-padded row.
template <int CS>
struct S2F {
  static constexpr int RW = CS * S2_XRF;             // one input row of every channel
  static constexpr int XN = 3 * RW, XNP = (XN + 63) / 64 * 64;
  static constexpr int XPER = (XNP + 255) / 256;
  static int lds_bytes(bool repl, int nbuf) { return (nbuf * XNP + (repl ? 0 : RW)) * 4; }
};
template <bool REPL, int CS, bool POST = false, bool STATS = false>
__global__ __launch_bounds__(256) void conv_s2f_kernel(const float* __restrict__ in,
                                                       const float* __restrict__ wt,
                                                       float* __restrict__ out, ConvGeom g, Epi e,
                                                       S2Run run) {
  using L = S2F<CS>;
  constexpr int NS = 3 * CS;  // K-steps (c, kh)
  float* const Xs = s2_lds;
  const int tid = threadIdx.x, lane = tid & 63, r16 = lane & 15, g4 = lane >> 4;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int segs = (g.Wo + S2_SEG - 1) / S2_SEG;
  const int s_begin = blockIdx.x * run.spr, s_end = min(run.nst, s_begin + run.spr);
  float* const Zs = Xs + (run.spr > 1 ? 2 : 1) * L::XNP;  // rows of zeros (!REPL)
  // stage st's rows into buf: cell i = (row r, channel c, column j)
  auto stage = [&](int st, float* buf) {
    const int b = st / segs, w0 = (st - b * segs) * S2_SEG;
    const float* inb = in + (int64_t)b * g.C * 3 * g.Win;
#pragma unroll
    for (int u = 0; u < L::XPER; ++u) {
      if (256 * u + 64 * wid >= L::XNP) break;  // wave-uniform
      const int i = tid + 256 * u;
      const int rc = i / S2_XRF, j = i - rc * S2_XRF, r = rc / CS, c = rc - r * CS;
      int wi = 2 * w0 - g.opw + j;
      bool ok = i < L::XN && c < g.C;
      if (REPL) wi = wi < 0 ? 0 : (wi >= g.Win ? g.Win - 1 : wi);
      else ok = ok && wi >= 0 && wi < g.Win;
      s2_glds(ok ? inb + ((int64_t)c * 3 + r) * g.Win + wi : s2_zero_word, buf + 256 * u + 64 * wid);
    }
  };
  stage(s_begin, Xs);  // first: the weight, bias and BN loads below ride along with it
  // weights of row n = r16, tap kw = g4, step s = (c, kh)
  float af[NS];
  const int nr = r16 < g.N ? r16 : 0;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int c = s / 3, kh = s - 3 * c;
    const int cc = c < g.C ? c : 0;
    af[s] = wt[nr * g.wsn + cc * g.wsc + (kh * 4 + g4) * g.wst];
  }
  float bv[1][4];
  const int nbase = 4 * g4;
  epi_load_bias<1>(bv, e.bias, nbase, g.N);
  const uint64_t seed = e.drop_p > 0.f ? mix_seed(e.seed_ptr, e.offset) : 0ull;
  const int64_t hw = (int64_t)g.Hout * g.Wo;
  PostTile<1> pt;
  if constexpr (POST) epi_load_post<1>(pt, e, nbase, g.N);
  if (!REPL)
    for (int i = tid; i < L::RW; i += 256) Zs[i] = 0.f;
  for (int st = s_begin; st < s_end; ++st) {
    float* const cur = Xs + ((st - s_begin) & 1) * L::XNP;
    s2_ring_sync();
    if (st + 1 < s_end) stage(st + 1, Xs + ((st + 1 - s_begin) & 1) * L::XNP);
    const int b = st / segs, w0 = (st - b * segs) * S2_SEG;
    // 12 tiles (3 rows x 4 position groups of 16), 3 per wave; rb[t][kh]: the staged row of
    // output row h under tap kh (h + kh - 1, clamped or the zeros) at this lane's column
    floatx4 acc[3];
    const float* rb[3][3];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const int tile = wid * 3 + t, h = tile >> 2, p0 = (tile & 3) * 16;
      const int col = 2 * (p0 + r16) + g4;
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) {
        const int hi = h + kh - 1;
        if (REPL) rb[t][kh] = cur + (hi < 0 ? 0 : (hi > 2 ? 2 : hi)) * L::RW + col;
        else rb[t][kh] = (hi >= 0 && hi <= 2 ? cur + hi * L::RW : Zs) + col;
      }
      acc[t] = floatx4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int c = s / 3, kh = s - 3 * c;
#pragma unroll
      for (int t = 0; t < 3; ++t) acc[t] = mfma16x16x4(af[s], rb[t][kh][c * S2_XRF], acc[t]);
    }
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const int tile = wid * 3 + t, h = tile >> 2;
      const int wo = w0 + (tile & 3) * 16 + r16;
      const bool pv = wo < g.Wo;
      const floatx4 a[1] = {acc[t]};
      epi_store<1, POST>(out, e, seed, bv, a, ((int64_t)b * g.N * g.Hout + h) * g.Wo + (pv ? wo : 0),
                         hw, nbase, g.N, pv, false, &pt);
    }
    if constexpr (STATS) {  // (no dropout / residual on this path: the stored value is acc + b)
      double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const int tile = wid * 3 + t;
        if (w0 + (tile & 3) * 16 + r16 >= g.Wo) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double v = (double)(acc[t][r] + bv[0][r]);
          s1[r] += v;
          s2[r] += v * v;
        }
      }
      s2_bn_stats_block(s1, s2, nbase, g.N, e.bn_part, st, run.nst);
    }
  }
}

// T: out[b,n,h,wo] = sum w(n,c,kh,kw) in[b,c,h-kh+oph,(wo-kw+opw)/2] over the integer
// sources, Hin = 3, HO = Hout (3, or 5 for the replicate canvas).  FOLD (the data gradient
// of a replicate-padded conv): the canvas (5 rows, Wo = Wx + 2 columns) is folded onto
// out = dx (3 rows, Wx columns) in the epilogue -- rows 0+1, 2, 3+4; canvas columns 0 / Wx+1
// onto dx columns 0 / Wx-1 through LDS -- instead of a canvas store and a fold launch.
// The tap kh is the lane's (k = 4 s + g4), so the staged row must stay linear in h - kh:
// LDS is [row][c][S2_XRT] with ZR rows of zeros before, between and after the buffers' three
// real rows (ZR = 2 for HO = 5, 1 for HO = 3); neighbouring buffers share their zeros.
template <int CS, int HO>
struct S2T {
  static constexpr int ZR = HO == 5 ? 2 : 1;
  static constexpr int RW = CS * S2_XRT;
  static constexpr int XN = 3 * RW, XNP = (XN + 63) / 64 * 64;  // the tail lands in zeros
  static constexpr int XPER = (XNP + 255) / 256;
  static constexpr int PER = (3 + ZR) * RW;  // buffer k's real rows start at ZR * RW + k * PER
  static_assert(XNP - XN <= ZR * RW, "the DMA's tail must stay inside the zeros");
  static int lds_bytes(int nbuf) { return (nbuf * PER + ZR * RW) * 4; }
};
template <int CS, int HO, bool FOLD = false, bool POST = false, bool STATS = false>
__global__ __launch_bounds__(256) void conv_s2t_kernel(const float* __restrict__ in,
                                                       const float* __restrict__ wt,
                                                       float* __restrict__ out, ConvGeom g, Epi e,
                                                       S2Run run) {
  using L = S2T<CS, HO>;
  constexpr int NS = 6 * CS / 4;  // K-steps
  float* const Xs = s2_lds;
  const int tid = threadIdx.x, lane = tid & 63, r16 = lane & 15, g4 = lane >> 4;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int par = wid & 1, mb = wid >> 1;  // this wave's output parity and 16-column group
  const int segs = (g.Wo + S2_SEG - 1) / S2_SEG;
  const int s_begin = blockIdx.x * run.spr, s_end = min(run.nst, s_begin + run.spr);
  const int nbuf = run.spr > 1 ? 2 : 1;
  // stage st's rows into buf (its first real row): cell i = (row r, channel c, column j),
  // staged column j <-> source column m0 - 2 + j
  auto stage = [&](int st, float* buf) {
    const int b = st / segs, m0 = ((st - b * segs) * S2_SEG) >> 1;
    const float* inb = in + (int64_t)b * g.C * 3 * g.Win;
#pragma unroll
    for (int u = 0; u < L::XPER; ++u) {
      if (256 * u + 64 * wid >= L::XNP) break;  // wave-uniform
      const int i = tid + 256 * u;
      const int rc = i / S2_XRT, j = i - rc * S2_XRT, r = rc / CS, c = rc - r * CS;
      const int wi = m0 - 2 + j;
      const bool ok = i < L::XN && c < g.C && wi >= 0 && wi < g.Win;
      s2_glds(ok ? inb + ((int64_t)c * 3 + r) * g.Win + wi : s2_zero_word, buf + 256 * u + 64 * wid);
    }
  };
  stage(s_begin, Xs + L::ZR * L::RW);
  // step s, lane group g4: k = 4s + g4 = (c, kh, e), kw = q + 2e with q = (par + opw) & 1
  float af[NS];
  int soff[NS];
  const int nr = r16 < g.N ? r16 : 0, q = (par + g.opw) & 1;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int k = 4 * s + g4, c = k / 6, rem = k - 6 * c, kh = rem >> 1, kw = q + 2 * (rem & 1);
    const int cc = c < g.C ? c : 0;
    af[s] = wt[nr * g.wsn + cc * g.wsc + (kh * 4 + kw) * g.wst];
    soff[s] = (c - kh * CS) * S2_XRT + ((par + g.opw - kw) >> 1);
  }
  float bv[1][4];
  const int nbase = 4 * g4;
  epi_load_bias<1>(bv, e.bias, nbase, g.N);
  const uint64_t seed = e.drop_p > 0.f ? mix_seed(e.seed_ptr, e.offset) : 0ull;
  const int64_t hw = (int64_t)g.Hout * g.Wo;
  PostTile<1> pt;
  if constexpr (POST) epi_load_post<1>(pt, e, nbase, g.N);
  for (int i = tid; i < nbuf * L::PER + L::ZR * L::RW; i += 256)
    if ((i / L::RW) % (3 + L::ZR) < L::ZR) Xs[i] = 0.f;
  for (int st = s_begin; st < s_end; ++st) {
    float* const cur = Xs + ((st - s_begin) & 1) * L::PER;  // row hi = -ZR of this buffer
    s2_ring_sync();
    if (st + 1 < s_end) stage(st + 1, Xs + ((st + 1 - s_begin) & 1) * L::PER + L::ZR * L::RW);
    const int b = st / segs, w0 = (st - b * segs) * S2_SEG;
    floatx4 acc[HO];
    const float* xb = cur + (g.oph + L::ZR) * L::RW + mb * 16 + r16 + 2;
#pragma unroll
    for (int h = 0; h < HO; ++h) acc[h] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int h = 0; h < HO; ++h) acc[h] = mfma16x16x4(af[s], xb[h * L::RW + soff[s]], acc[h]);
    const int wo = w0 + 2 * (mb * 16 + r16) + par;
    if constexpr (FOLD) {
      static_assert(HO == 5, "fold: replicate canvas");
      __shared__ floatx4 ex[2][3][4];
      const int Wx = g.Wo - 2;
      floatx4 y[3] = {acc[0] + acc[1], acc[2], acc[3] + acc[4]};
      if (wo == 0 || wo == Wx + 1) {
#pragma unroll
        for (int h = 0; h < 3; ++h) ex[wo == 0 ? 0 : 1][h][g4] = y[h];
      }
      __syncthreads();
      if (wo == 1) {
#pragma unroll
        for (int h = 0; h < 3; ++h) y[h] = ex[0][h][g4] + y[h];
      } else if (wo == Wx) {
#pragma unroll
        for (int h = 0; h < 3; ++h) y[h] = y[h] + ex[1][h][g4];
      }
      const bool pv = wo >= 1 && wo <= Wx;
#pragma unroll
      for (int h = 0; h < 3; ++h)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int n = nbase + r;
          if (pv && n < g.N) out[(((int64_t)b * g.N + n) * 3 + h) * Wx + wo - 1] = y[h][r];
        }
    } else {
      const bool pv = wo < g.Wo;
#pragma unroll
      for (int h = 0; h < HO; ++h) {
        const floatx4 a[1] = {acc[h]};
        epi_store<1, POST>(out, e, seed, bv, a,
                           ((int64_t)b * g.N * g.Hout + h) * g.Wo + (pv ? wo : 0), hw, nbase, g.N,
                           pv, false, &pt);
      }
      if constexpr (STATS) {
        double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
        if (pv) {
#pragma unroll
          for (int h = 0; h < HO; ++h)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const double v = (double)(acc[h][r] + bv[0][r]);
              s1[r] += v;
              s2[r] += v * v;
            }
        }
        s2_bn_stats_block(s1, s2, nbase, g.N, e.bn_part, st, run.nst);
      }
    }
  }
}

// which stride-2 small-channel kernel takes this launch: 0 none, 1 F, 2 T (Hout 3), 3 T (5)
int s2_kind(int mode, const ConvGeom& g) {
  if (!conv_config().s2 || g.C > 16 || g.N > 16 || g.Hin != 3) return 0;
  if (mode == GATHER_F)
    return g.Hout == 3 && g.oph == 1 && g.opw >= 0 && g.opw <= 2 ? 1 : 0;
  if (g.opw < 0 || g.opw > 3) return 0;
  if (g.Hout == 3 && g.oph == 1) return 2;
  if (g.Hout == 5 && g.oph == 0) return 3;
  return 0;
}

int64_t s2_blocks(const ConvGeom& g) { return (int64_t)g.B * ((g.Wo + S2_SEG - 1) / S2_SEG); }

// Blocks of a launch: min(stages, cap), the stages dealt in contiguous runs of `spr`.
// S2_CAP_DEFAULT is the production cap (profiles/s2_ring_ab.txt).
constexpr int S2_CAP_DEFAULT = 768;
static S2Run s2_run(const ConvGeom& g, unsigned* grid) {
  const int64_t nst = s2_blocks(g);
  const int64_t cap = conv_config().s2_cap > 0 ? conv_config().s2_cap : S2_CAP_DEFAULT;
  const int64_t blocks = nst < cap ? nst : cap;
  S2Run r;
  r.nst = (int)nst;
  r.spr = (int)((nst + blocks - 1) / blocks);
  *grid = (unsigned)((nst + r.spr - 1) / r.spr);
  return r;
}

template <bool REPL>
static void launch_s2_r(int kind, const float* in, const float* wt, float* out, const ConvGeom& g,
                        const Epi& e, hipStream_t st) {
  unsigned blocks;
  const S2Run run = s2_run(g, &blocks);
  const dim3 grid(blocks);
  const int nbuf = run.spr > 1 ? 2 : 1;
  const int cs = (g.C + 3) / 4;
  TVQ_PLAN("conv_s2%s cs%d hout%d%s blocks=%u per=%d", kind == 1 ? "f" : "t", 4 * cs, g.Hout,
           e.bn_part ? " bnstats" : "", blocks, run.spr);
#define S2F(CSV)                                                                                  \
  do {                                                                                            \
    const int lds = S2F<CSV>::lds_bytes(REPL, nbuf);                                              \
    if (e.bn_part)                                                                                \
      hipLaunchKernelGGL((conv_s2f_kernel<REPL, CSV, false, true>), grid, dim3(256), lds, st, in,  \
                         wt, out, g, e, run);                                                     \
    else if (e.bn_rv)                                                                             \
      hipLaunchKernelGGL((conv_s2f_kernel<REPL, CSV, true>), grid, dim3(256), lds, st, in, wt,     \
                         out, g, e, run);                                                         \
    else                                                                                          \
      hipLaunchKernelGGL((conv_s2f_kernel<REPL, CSV>), grid, dim3(256), lds, st, in, wt, out, g,   \
                         e, run);                                                                 \
  } while (0)
#define S2T(CSV, HOV)                                                                              \
  do {                                                                                             \
    const int lds = S2T<CSV, HOV>::lds_bytes(nbuf);                                                \
    if (e.bn_part)                                                                                 \
      hipLaunchKernelGGL((conv_s2t_kernel<CSV, HOV, false, false, true>), grid, dim3(256), lds, st, \
                         in, wt, out, g, e, run);                                                  \
    else if (e.bn_rv)                                                                              \
      hipLaunchKernelGGL((conv_s2t_kernel<CSV, HOV, false, true>), grid, dim3(256), lds, st, in,    \
                         wt, out, g, e, run);                                                      \
    else                                                                                           \
      hipLaunchKernelGGL((conv_s2t_kernel<CSV, HOV>), grid, dim3(256), lds, st, in, wt, out, g, e,  \
                         run);                                                                     \
  } while (0)
  if (kind == 1) {
    if (cs == 1) S2F(4); else if (cs == 2) S2F(8); else if (cs == 3) S2F(12); else S2F(16);
    return;
  }
  if (kind == 2) {
    if (cs == 1) S2T(4, 3); else if (cs == 2) S2T(8, 3); else if (cs == 3) S2T(12, 3); else S2T(16, 3);
  } else {
    if (cs == 1) S2T(4, 5); else if (cs == 2) S2T(8, 5); else if (cs == 3) S2T(12, 5); else S2T(16, 5);
  }
#undef S2F
#undef S2T
}
void launch_s2(int k2, bool repl, const float* in, const float* wt, float* out, const ConvGeom& g,
               const Epi& e, hipStream_t st) {
  if (repl) launch_s2_r<true>(k2, in, wt, out, g, e, st);
  else launch_s2_r<false>(k2, in, wt, out, g, e, st);
}

// data gradient of a replicate-padded conv straight into dx (canvas geometry g, Wx = Wo - 2):
// the canvas columns Wx and Wx + 1 must share a segment
bool s2_fold_fits(const ConvGeom& g) {
  return s2_kind(GATHER_T, g) == 3 && g.Wo >= 4 && (g.Wo - 1) % S2_SEG != 0;
}
void launch_s2_fold(const float* in, const float* wt, float* dx, const ConvGeom& g,
                    hipStream_t st) {
  unsigned blocks;
  const S2Run run = s2_run(g, &blocks);
  const dim3 grid(blocks);
  const int nbuf = run.spr > 1 ? 2 : 1;
  const Epi e = {nullptr, nullptr, 0.f, 1.f, nullptr, 0};
  const int cs = (g.C + 3) / 4;
  TVQ_PLAN("conv_s2t_fold cs%d blocks=%u per=%d", 4 * cs, blocks, run.spr);
#define S2T(CSV)                                                                            \
  hipLaunchKernelGGL((conv_s2t_kernel<CSV, 5, true>), grid, dim3(256),                      \
                     (S2T<CSV, 5>::lds_bytes(nbuf)), st, in, wt, dx, g, e, run)
  if (cs == 1) S2T(4); else if (cs == 2) S2T(8); else if (cs == 3) S2T(12); else S2T(16);
#undef S2T
}

// Weight (+ bias) gradient of the same stride-2 small-channel convs, in the F-gather form
// both directions share (conv2d: G = dY, In = x;  ConvTranspose2d: G = x, In = dY):
//   dW[n][c,kh,kw] = sum_{b,h,w} G[b,n,h,w] In[b,c,h+kh-1,2w+kw-opw],  db[n] = sum G
// A block (8 waves) walks stages of one image's 64-wide G segment on all 3 rows: the G rows
// (16 x 192) and the three input rows they read (C x 3 x 130, column padding applied while
// staging) go through LDS with the next stage's loads in flight.  Wave w owns k' tiles w%4,
// w%4+4, ... of the N x (12C+1) slab row for half of the stage's positions (w/4), so a k-step
// is one G read shared by its tiles; each lane's column pointers are fixed once per G row the
// wave meets (window cell of row h + kh - 1, clamped or the zeros plane for a padding row; a
// ones plane for the bias column, the zeros plane past it).  The position halves are summed
// in order at the end; blocks write slab rows (<= 256, one deferred ordered sum).
constexpr int W2_T = 512, W2_GS = 3 * S2_SEG + 4, W2_KP = 2 * S2_XRF + 2 * S2_SEG + 8;
struct W2Geom {
  int B, C, N, Win, Wo, Kred, kcols, segs, spr, opw;
};

template <bool REPL, int CS>
__global__ __launch_bounds__(W2_T) void conv_wgrad_s2_kernel(const float* __restrict__ G,
                                                            const float* __restrict__ X,
                                                            float* __restrict__ slab, W2Geom g) {
  constexpr int RS = 3, XN = CS * RS * S2_XRF, XPER = (XN + W2_T - 1) / W2_T;
  constexpr int GN = 16 * 3 * S2_SEG, GPER = GN / W2_T;
  constexpr int KT = (12 * CS + 1 + 15) / 16, TPW = (KT + 3) / 4;
  constexpr int RED = 4 * TPW * 256;
  static_assert(XPER <= 32 && GN % W2_T == 0, "staging");
  __shared__ float Xs[XN > RED ? XN : RED];  // after the stages: the second half's tiles
  __shared__ float Gs[16 * W2_GS];
  __shared__ float K1[2 * W2_KP];  // ones | zeros
  const int tid = threadIdx.x, lane = tid & 63, r16 = lane & 15, g4 = lane >> 4;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tg = wid & 3, ph = wid >> 2;  // tile group, position half
  const int nst = g.B * g.segs, z = blockIdx.x;
  const int s_begin = z * g.spr, s_end = min(nst, s_begin + g.spr);
  for (int i = tid; i < 2 * W2_KP; i += W2_T) K1[i] = i < W2_KP ? 1.f : 0.f;
  // This half's 24 k-steps are positions p = 96 ph + 4 i + g4 (row p / 64, column p % 64):
  // steps 0-7 lie on G row ph, 8-15 on row 2 ph, 16-23 on row ph + 1.  A lane's column
  // pointer per tile and row group, the group's first column folded in so that step i reads
  // at 8 i (two input columns per position).
  const float* bp[3][TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int kc = (tg + 4 * t) * 16 + r16;
    const int k = kc < g.Kred ? kc : 0, c = k / 12, rem = k - 12 * c, kh = rem >> 2;
    const float* plane = (kc == g.Kred && g.kcols > g.Kred ? K1 : K1 + W2_KP) + 2 * g4;
    auto row = [&](int h) -> const float* {
      if (kc >= g.Kred) return plane;
      int hi = h + kh - 1;
      if (REPL) hi = hi < 0 ? 0 : (hi > 2 ? 2 : hi);
      else if (hi < 0 || hi > 2) return K1 + W2_KP + 2 * g4;
      return Xs + (c * RS + hi) * S2_XRF + (rem & 3) + 2 * g4;
    };
    bp[0][t] = row(ph) + 64 * ph;
    bp[1][t] = row(2 * ph) - 64 * ph;
    bp[2][t] = row(ph + 1) + 64 * ph - 128;
  }
  const float* ap = Gs + r16 * W2_GS + g4;
  float xv[XPER], gv[GPER];
  uint32_t okm = 0, gok = 0;
  auto load = [&](int s) {
    const int b = s / g.segs, w0 = (s - b * g.segs) * S2_SEG;
    const float* xb = X + (int64_t)b * g.C * 3 * g.Win;
#pragma unroll
    for (int u = 0; u < XPER; ++u) {
      const int i = tid + W2_T * u;
      const int ck = i / S2_XRF, j = i - ck * S2_XRF, c = ck / RS, hi = ck - RS * c;
      int wi = 2 * w0 - g.opw + j;
      bool ok = i < XN && c < g.C;
      if (REPL) wi = wi < 0 ? 0 : (wi >= g.Win ? g.Win - 1 : wi);
      else ok = ok && wi >= 0 && wi < g.Win;
      xv[u] = xb[ok ? ((int64_t)c * 3 + hi) * g.Win + wi : 0];
      okm = u == 0 ? (ok ? 1u : 0u) : (okm | (ok ? 1u : 0u) << u);
    }
    const float* gb = G + (int64_t)b * g.N * 3 * g.Wo;
#pragma unroll
    for (int u = 0; u < GPER; ++u) {
      const int i = tid + W2_T * u;
      const int n = i / (3 * S2_SEG), p = i - n * (3 * S2_SEG), h = p / S2_SEG, w = w0 + p - h * S2_SEG;
      const bool ok = n < g.N && w < g.Wo;
      gv[u] = gb[ok ? ((int64_t)n * 3 + h) * g.Wo + w : 0];
      gok = u == 0 ? (ok ? 1u : 0u) : (gok | (ok ? 1u : 0u) << u);
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int u = 0; u < XPER; ++u) {
      const int i = tid + W2_T * u;
      if (i < XN) Xs[i] = (okm >> u & 1u) ? xv[u] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < GPER; ++u) {
      const int i = tid + W2_T * u;
      const int n = i / (3 * S2_SEG), p = i - n * (3 * S2_SEG);
      Gs[n * W2_GS + p] = (gok >> u & 1u) ? gv[u] : 0.f;
    }
  };
  floatx4 acc[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t) acc[t] = floatx4{0.f, 0.f, 0.f, 0.f};
  if (s_begin < s_end) load(s_begin);
  for (int s = s_begin; s < s_end; ++s) {
    __syncthreads();  // the previous stage's reads are done
    store();
    __syncthreads();
    if (s + 1 < s_end) load(s + 1);  // in flight during this stage's chains
#pragma unroll
    for (int i = 0; i < 24; ++i) {
      const float a = ap[96 * ph + 4 * i];
#pragma unroll
      for (int t = 0; t < TPW; ++t) acc[t] = mfma16x16x4(a, bp[i >> 3][t][8 * i], acc[t]);
    }
  }
  __syncthreads();
  floatx4* red = reinterpret_cast<floatx4*>(Xs);
  if (ph == 1) {
#pragma unroll
    for (int t = 0; t < TPW; ++t) red[(tg * TPW + t) * 64 + lane] = acc[t];
  }
  __syncthreads();
  if (ph == 0) {
    float* sl = slab + (int64_t)z * g.N * g.kcols;
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      const floatx4 o = red[(tg * TPW + t) * 64 + lane];
      const int kc = (tg + 4 * t) * 16 + r16;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = 4 * g4 + r;
        const float v = acc[t][r] + o[r];
        if (n < g.N && kc < g.kcols) sl[(int64_t)n * g.kcols + kc] = v;
      }
    }
  }
}

bool ws2_fits(int64_t C, int64_t H, int64_t N, int64_t KH, int64_t KW, int64_t SW) {
  return conv_config().ws2 && KH == 3 && KW == 4 && SW == 2 && H == 3 && C <= 16 && N <= 16;
}
static void ws2_plan(int64_t B, int64_t Wo, int* S, int* spr) {
  const int64_t nst = B * ((Wo + S2_SEG - 1) / S2_SEG);
  const int64_t s = nst < RR_ONE_ROWS ? nst : RR_ONE_ROWS;
  const int64_t per = (nst + s - 1) / s;
  *spr = (int)per;
  *S = (int)((nst + per - 1) / per);
}
int64_t ws2_ws(int64_t B, int64_t C, int64_t Wo, int64_t N) {
  int S, spr;
  ws2_plan(B, Wo, &S, &spr);
  const int64_t kc = C * 12 + 1;
  return (int64_t)S * N * kc + reduce_rows_scratch(S, N * kc);
}
// G (B, N, 3, Wo) against In (B, C, 3, Win) -> slab rows; returns the row count
int ws2_launch(const float* G, const float* X, float* slab, int B, int C, int N, int Win, int Wo,
               int kcols, bool repl, hipStream_t st) {
  W2Geom w;
  w.B = B; w.C = C; w.N = N; w.Win = Win; w.Wo = Wo; w.Kred = 12 * C; w.kcols = kcols;
  w.segs = (Wo + S2_SEG - 1) / S2_SEG; w.opw = 1;
  int S;
  ws2_plan(B, Wo, &S, &w.spr);
  const int cs = (C + 3) / 4;
  TVQ_PLAN("conv_wgrad_s2 cs%d S=%d spr=%d", 4 * cs, S, w.spr);
#define W2L(R, CSV) hipLaunchKernelGGL((conv_wgrad_s2_kernel<R, CSV>), dim3(S), dim3(W2_T), 0, st, G, X, slab, w)
  if (repl) {
    if (cs == 1) W2L(true, 4); else if (cs == 2) W2L(true, 8); else if (cs == 3) W2L(true, 12); else W2L(true, 16);
  } else {
    if (cs == 1) W2L(false, 4); else if (cs == 2) W2L(false, 8); else if (cs == 3) W2L(false, 12); else W2L(false, 16);
  }
#undef W2L
  return S;
}

}  // namespace tvq
