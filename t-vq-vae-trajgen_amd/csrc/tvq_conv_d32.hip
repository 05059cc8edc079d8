// The conv engine's direct path: conv_d32_kernel.
#include "tvq_conv_core.h"

namespace tvq {

// Convolutions of narrow maps with >= 32 channels on both sides -- the LF band's 64 /
// 128-channel convs on (256, C, 3, 8), 6,144 positions, and their neighbours (the 1x1
// projections, the 32 -> 64 EncBlock, the 64 -> 32 DecBlock): the staged paths give them
// 48-96 blocks (so split-K + an epilogue launch, 21 + 5 us per 3x3 64-channel conv at 0.13
// of the fp32 MFMA peak).  Here a block owns a 32-channel x 32-position output tile and its
// NW waves split the reduction by input-channel ranges (each wave: its C / NW channels for
// every tap), so the LF 64-channel convs run as 384 blocks of short MFMA chains with no LDS
// staging: every operand goes global (L2) -> registers.  Per step a lane supplies one
// packed weight w[tap][c][n0 + l % 32] (coalesced) and one gathered input value at its
// position (gather_in's index rules: zero / replicate padding, the stride-2 transposed
// parity skip); the wave runs one v_mfma_f32_32x32x2_f32 per 2 channels.  Up to ~144
// floats of loads (every tap of a 64-channel 3x3 conv) are in flight before the first MFMA.  The partial tiles are added in
// LDS in a fixed pairwise order; bias, dropout (the same counter hash) and residual as
// epi_store.  Replaced: split-K tap + epilogue, 6.12 -> 5.92 ms per joint step.
template <int MODE, int KH, int KW, int SW, bool REPL, int CW, int NW>
__global__ __launch_bounds__(64 * NW) void conv_d32_kernel(const float* __restrict__ in,
                                                          const float* __restrict__ wt,
                                                          float* __restrict__ out, ConvGeom g,
                                                          Epi e, int mtiles) {
  constexpr int KK = KH * KW;
  __shared__ float red[NW][16][64];
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r32 = lane & 31, hl = lane >> 5;
  const int mt = (int)blockIdx.x % mtiles, nt = (int)blockIdx.x / mtiles;
  const int m0 = mt * 32, n0 = nt * 32;
  // this lane's output position (B operand column) and output channel (A operand row)
  const int m = m0 + r32;
  const bool pv = m < g.Mpos;
  const int mc = pv ? m : 0;
  const uint32_t bh = fdiv((uint32_t)mc, g.fd_wo);
  const int ww = mc - (int)bh * g.Wo;
  const int b = (int)fdiv((uint32_t)mc, g.fd_hwo);
  const int hh = (int)bh - b * g.Hout;
  const int HW = g.Hin * g.Win;
  const int c0 = wid * CW;  // this wave's input channels [c0, c0 + CW)
  const float* inb = in + ((int64_t)b * g.C + c0 + hl) * HW;
  const float* wl = wt + (int64_t)(c0 + hl) * g.wsc + min(n0 + r32, g.N - 1);
  floatx16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  constexpr int ST = CW / 2;  // MFMA steps per tap
  // PD taps' loads in flight (a ring of PD register buffers, ~144 floats): every tap of a
  // 64-channel conv is requested before the first MFMA, so the block pays one L2 round
  // trip instead of one per tap (9 x ~1 us with one tap of prefetch)
  constexpr int PD0 = 144 / CW, PD = PD0 < 1 ? 1 : (PD0 > KK ? KK : PD0);
  float fa[PD][ST], fb[PD][ST];
  auto load = [&](int buf, int tap) {
    const int kh = tap / KW, kw = tap - KW * kh;
    int hi, wi;
    bool ok = pv;
    if (MODE == GATHER_F) {
      hi = hh + kh - g.oph;
      wi = ww * SW + kw - g.opw;
      if (REPL) {
        hi = hi < 0 ? 0 : (hi >= g.Hin ? g.Hin - 1 : hi);
        wi = wi < 0 ? 0 : (wi >= g.Win ? g.Win - 1 : wi);
      } else {
        ok = ok && hi >= 0 && hi < g.Hin && wi >= 0 && wi < g.Win;
      }
    } else {
      hi = hh - kh + g.oph;
      const int wn = ww - kw + g.opw;
      ok = ok && hi >= 0 && hi < g.Hin && wn >= 0 && (SW == 1 || (wn & 1) == 0);
      wi = wn / SW;
      ok = ok && wi < g.Win;
    }
    const int o = ok ? hi * g.Win + wi : 0;
    const float* wtap = wl + (int64_t)tap * g.wst;
#pragma unroll
    for (int u = 0; u < ST; ++u) {
      fa[buf][u] = wtap[(int64_t)(2 * u) * g.wsc];
      const float v = inb[(int64_t)(2 * u) * HW + o];
      fb[buf][u] = ok ? v : 0.f;
    }
  };
#pragma unroll
  for (int t = 0; t < PD; ++t) load(t, t);
#pragma unroll
  for (int tap = 0; tap < KK; ++tap) {
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < ST; ++u)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[tap % PD][u], fb[tap % PD][u], acc, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    if (tap + PD < KK) load(tap % PD, tap + PD);
  }
  // partial tiles -> LDS, summed pairwise ((w0 + w1) + (w2 + w3)) + ...; thread t then owns
  // tile elements t, t + 64 NW, ... with the channel slowest (row-major [n][m]: the stores
  // coalesce along m)
#pragma unroll
  for (int r = 0; r < 16; ++r) red[wid][r][lane] = acc[r];
  __syncthreads();
  const uint64_t seed = e.drop_p > 0.f ? mix_seed(e.seed_ptr, e.offset) : 0ull;
#pragma unroll
  for (int q = 0; q < 1024 / (64 * NW); ++q) {
    const int el = tid + 64 * NW * q, nr = el >> 5, mr = el & 31;
    // acc r of lane l: row (n) 8 (r / 4) + 4 (l / 32) + r % 4, column (m) l % 32
    const int ln = mr + 32 * ((nr >> 2) & 1), r = (nr & 3) + 4 * (nr >> 3);
    float part[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) part[w] = red[w][r][ln];
#pragma unroll
    for (int span = 1; span < NW; span *= 2)
#pragma unroll
      for (int w = 0; w + span < NW; w += 2 * span) part[w] += part[w + span];
    const int n = n0 + nr, mm = m0 + mr;
    if (n >= g.N || mm >= g.Mpos) continue;
    const uint32_t bh2 = fdiv((uint32_t)mm, g.fd_wo);
    const int w2 = mm - (int)bh2 * g.Wo;
    const int b2 = (int)fdiv((uint32_t)mm, g.fd_hwo);
    const int h2 = (int)bh2 - b2 * g.Hout;
    const int64_t o = (((int64_t)b2 * g.N + n) * g.Hout + h2) * g.Wo + w2;
    float v = epi_post(e, part[0] + (e.bias ? e.bias[n] : 0.f), n);
    if (e.drop_p > 0.f) v = uniform01(seed, (uint64_t)o) >= e.drop_p ? v * e.drop_scale : 0.f;
    if (e.residual) v += e.residual[o];
    out[o] = v;
  }
}

// the largest position count the direct narrow-map conv takes (the LF maps, 6,144
// positions) and its waves per block
constexpr int D32_MAX_POS = 8192, D32_NW = 4;

template <int MODE, int KH, int KW, int SW, bool REPL>
static bool launch_d32_t(const float* in, const float* wt, float* out, const ConvGeom& g,
                         const Epi& e, hipStream_t st) {
  // off with the 32x32-MFMA tiles (tvq_conv_config bit 8: the tap kernel alone)
  if (!conv_config().t32 || g.Mpos > D32_MAX_POS) return false;
  if (g.wsn != 1 || g.N < 32 || g.C < 32 || g.C > 128) return false;
  if (g.C % (2 * D32_NW) != 0) return false;
  const int mtiles = (g.Mpos + 31) / 32, ntiles = (g.N + 31) / 32;
  const unsigned grid = (unsigned)(mtiles * ntiles);
#define TVQ_D32(CWV)                                                                         \
  hipLaunchKernelGGL((conv_d32_kernel<MODE, KH, KW, SW, REPL, CWV, D32_NW>), dim3(grid),    \
                     dim3(64 * D32_NW), 0, st, in, wt, out, g, e, mtiles);                    \
  return true;
  switch (g.C / D32_NW) {
    case 8: TVQ_D32(8)
    case 16: TVQ_D32(16)
    case 24: TVQ_D32(24)
    case 32: TVQ_D32(32)
    default: return false;
  }
#undef TVQ_D32
}

bool launch_d32(int mode, int kind, bool repl, const float* in, const float* wt, float* out,
                const ConvGeom& g, const Epi& e, hipStream_t st) {
#define M_(m, a, b_, c, d) return launch_d32_t<m, a, b_, c, d>(in, wt, out, g, e, st);
  TVQ_DISPATCH_CONV(mode, kind, repl, M_)
#undef M_
  return false;
}

}  // namespace tvq
