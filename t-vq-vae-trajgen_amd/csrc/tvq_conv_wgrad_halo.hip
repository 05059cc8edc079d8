// conv_wgrad_halo_kernel: the weight gradient that stages one image's G tile and halo planes
// per step (small C x N, short images), its plan and its launcher.
#include "tvq_conv_core.h"

namespace tvq {

// Halo-tile weight gradient: dW[n, c, tap] = sum_{b,h,w} G[b,n,h,w] In[b,c, h+kh-oh, w*SW+kw-ow]
// (+ a ones column for the bias gradient).  Block (s, nb, cb) loops over the images of
// split s; per image the G tile (NB x P) and the halo of CB input channels are loaded
// with all loads in flight, then the MFMAs reduce over the image's positions from LDS.
// Partials go to slab[s][n][kcols] and are summed in split order (conv_wgrad_finish).
struct WHaloGeom {
  Div16 dv_hw, dv_wp, dv_gst;
  int B, C, Hin, Win, N, Hout, Wo;
  int oh, ow, HP, WP, PS;
  int P, GST, CB;
  int Kred, kcols;   // kcols = Kred (+1: bias column)
  int ips;           // images per split
};

template <int KH, int KW, int SW, bool REPL, int FN>
__global__ __launch_bounds__(256) void conv_wgrad_halo_kernel(const float* __restrict__ G,
                                                             const float* __restrict__ in,
                                                             float* __restrict__ slab,
                                                             WHaloGeom g) {
  constexpr int KK = KH * KW;
  constexpr int NB = FN * 16;
  extern __shared__ float smem[];
  float* Gs = smem;                     // [NB][GST]
  float* Hs = smem + NB * g.GST;        // [CB][PS], then a plane of ones
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int s = blockIdx.x;
  const int n0 = blockIdx.y * NB;
  const int c0 = blockIdx.z * g.CB;
  const int cbn = min(g.CB, g.C - c0);
  const bool last_cb = c0 + g.CB >= g.C;
  const int kb = cbn * KK + ((last_cb && g.kcols > g.Kred) ? 1 : 0);  // columns of this block
  const int KT = (kb + 15) / 16;
  const int j = lane & 15, kq = lane >> 4;

  for (int idx = tid; idx < g.PS; idx += 256) Hs[g.CB * g.PS + idx] = 1.0f;
  int koff[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int kl = (wid + 4 * t) * 16 + j;
    const int c = kl / KK, tap = kl - c * KK;
    koff[t] = kl < cbn * KK ? c * g.PS + (tap / KW) * g.WP + (tap % KW) : g.CB * g.PS;
  }
  const int ktw = wid < KT ? (KT - wid + 3) / 4 : 0;  // k-tiles of this wave (<= 4)

  floatx4 acc[FN][4];
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[i][t] = floatx4{0.f, 0.f, 0.f, 0.f};

  const int b_begin = s * g.ips, b_end = min(g.B, b_begin + g.ips);
  for (int b = b_begin; b < b_end; ++b) {
    __syncthreads();  // previous image consumed
    const float* gb = G + ((int64_t)b * g.N + n0) * g.P;
    const int gtot = NB * g.GST;
    for (int base = tid; base < gtot; base += 256 * HALO_U) {
      float v[HALO_U];
#pragma unroll
      for (int u = 0; u < HALO_U; ++u) {
        const int idx = base + u * 256;
        const int nn = div16(idx, g.dv_gst), m = idx - nn * g.GST;
        v[u] = (idx < gtot && m < g.P && n0 + nn < g.N) ? gb[(int64_t)nn * g.P + m] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < HALO_U; ++u)
        if (base + u * 256 < gtot) Gs[base + u * 256] = v[u];
    }
    halo_fill<GATHER_F, KH, KW, SW, REPL>(Hs, in + ((int64_t)b * g.C + c0) * g.Hin * g.Win, cbn,
                                          cbn, g.Hin, g.Win, g.HP, g.WP, g.PS, g.oh, g.ow,
                                          g.dv_hw, g.dv_wp, tid);
    __syncthreads();
    // positions m0..m0+3 lie in one row (Wo % 4 == 0); lane group kq takes m0 + kq
    int h0 = 0, w0 = 0;
    for (int m0 = 0; m0 < g.P; m0 += 4) {
      const int base = h0 * g.WP + (w0 + kq) * SW;
      float af[FN];
#pragma unroll
      for (int i = 0; i < FN; ++i) af[i] = Gs[(i * 16 + j) * g.GST + m0 + kq];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (t < ktw) {
          const float bf = Hs[base + koff[t]];
#pragma unroll
          for (int i = 0; i < FN; ++i) acc[i][t] = mfma16x16x4(af[i], bf, acc[i][t]);
        }
      }
      w0 += 4;
      if (w0 == g.Wo) { w0 = 0; ++h0; }
    }
  }
  float* out = slab + (int64_t)s * g.N * g.kcols;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (t >= ktw) continue;
    const int kl = (wid + 4 * t) * 16 + j;
    int kg;
    if (kl < cbn * KK) kg = c0 * KK + kl;
    else if (kl == cbn * KK && kb > cbn * KK) kg = g.Kred;
    else continue;
#pragma unroll
    for (int i = 0; i < FN; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + i * 16 + kq * 4 + r;
        if (n < g.N) out[(int64_t)n * g.kcols + kg] = acc[i][t][r];
      }
  }
}

// Halo-plane stride of conv_wgrad_halo_kernel's image (>= hw): the B-operand read of a
// half-wave (lanes j = 0..15 over 16 consecutive reduction columns (c, tap), kq = 0..1 over
// 2 positions) is Hs[c*PS + toff(tap) + kq*SW + base]; its 32 addresses should fall on 32
// distinct (a/4) mod 32 banks.  The stride residue mod 32 that minimises the extra bank
// cycles over the kernel's column tiles is chosen on the host (layout only: same sums).
int whalo_plane_stride(int hw, int KK, int KW, int WP, int SW, int CB) {
  int best = hw + ((16 - hw % 32) + 32) % 32, best_cost = 1 << 30;
  const int ncols = CB * KK;
  for (int pad = 0; pad < 32; ++pad) {
    const int PS = hw + pad;
    int cost = 0;
    for (int t0 = 0; t0 < ncols; t0 += 16) {
      int hits[32][2];  // per bank: distinct addresses seen (up to 2 tracked) and count
      int cnt[32] = {0};
      for (int l = 0; l < 32; ++l) {
        const int j = l & 15, kq = l >> 4;
        const int kl = t0 + j;
        if (kl >= ncols) continue;
        const int c = kl / KK, tap = kl - c * KK;
        const int a = c * PS + (tap / KW) * WP + (tap % KW) + kq * SW;
        const int bank = ((a % 32) + 32) % 32;
        bool dup = false;
        for (int q = 0; q < cnt[bank] && q < 2; ++q) dup |= hits[bank][q] == a;
        if (dup) continue;
        if (cnt[bank] < 2) hits[bank][cnt[bank]] = a;
        ++cnt[bank];
      }
      int worst = 0;
      for (int b = 0; b < 32; ++b) worst = cnt[b] > worst ? cnt[b] : worst;
      cost += worst > 1 ? worst - 1 : 0;
    }
    if (cost < best_cost) {
      best_cost = cost;
      best = PS;
    }
  }
  return best;
}

// slab floats cap of the halo weight gradient (8M: LF 64-ch leg 26 vs 30 us at 4M)
constexpr int64_t WHALO_SLAB_MAX = 8 << 20;

WHaloSplit whalo_split(int64_t N, int64_t C, int KK, int64_t B) {
  WHaloSplit p;
  p.FN = N <= 16 ? 1 : (N <= 32 ? 2 : 4);
  int cb = 1;
  while (cb * 2 <= C && (cb * 2) * KK + 1 <= 256) cb *= 2;  // <= 16 k-tiles of 16
  p.CB = cb > C ? (int)C : cb;
  p.nblk = (int)((N + p.FN * 16 - 1) / (p.FN * 16));
  p.cblk = (int)((C + p.CB - 1) / p.CB);
  int64_t S = 1024 / (p.nblk * p.cblk);
  const int64_t cap = WHALO_SLAB_MAX / wgrad_slab_floats(1, N, C, KK);
  if (S > cap) S = cap;
  if (S > B) S = B;
  if (S < 1) S = 1;
  const int64_t per = (B + S - 1) / S;
  p.S = (int)((B + per - 1) / per);
  p.ips = (int)((B + p.S - 1) / p.S);
  return p;
}

struct WHaloPlan {
  WHaloGeom g;
  WHaloSplit sp;
  size_t lds;
};

static bool whalo_plan(const WgradArgs& a, WHaloPlan* pl) {
  if (a.Wo % 4 != 0) return false;
  // long images with many channels (the Upscale Conv1d) and the 128x128 ResBlock convs
  // run better on the split GEMM (tools/conv_shapes_bench.py: 148 vs 178 us at W 32)
  if (a.Hout * a.Wo > 128 && a.C > 64) return false;
  if ((int64_t)a.C * a.N >= 128 * 128) return false;
  WHaloGeom g;
  g.B = a.B; g.C = a.C; g.Hin = a.Hin; g.Win = a.Win; g.N = a.N; g.Hout = a.Hout; g.Wo = a.Wo;
  g.oh = PH_OF(a.KH); g.ow = PW_OF(a.KW);
  g.HP = a.Hout + a.KH - 1;
  g.WP = (a.Wo - 1) * a.SW + a.KW;
  const int hw = g.HP * g.WP;
  g.P = a.Hout * a.Wo;
  g.GST = g.P + ((2 - g.P % 32) + 32) % 32;
  if (g.WP < 2 || g.P >= (1 << 16)) return false;
  g.dv_hw = make_div16(hw);
  g.dv_wp = make_div16(g.WP);
  g.dv_gst = make_div16(g.GST);
  const int KK = a.KH * a.KW;
  const WHaloSplit sp = whalo_split(a.N, a.C, KK, a.B);
  g.PS = whalo_plane_stride(hw, KK, a.KW, g.WP, a.SW, sp.CB);
  g.CB = sp.CB;
  g.Kred = a.C * KK;
  g.kcols = a.kcols;
  g.ips = sp.ips;
  const size_t fl = (size_t)sp.FN * 16 * g.GST + (size_t)(sp.CB + 1) * g.PS;
  if (fl * 4 > (size_t)HALO_LDS_MAX) return false;
  pl->g = g;
  pl->sp = sp;
  pl->lds = fl * 4;
  return true;
}

template <int KH, int KW, int SW, bool REPL>
static void whalo_launch(const WgradArgs& a, const WHaloPlan& pl) {
  const dim3 grid(pl.sp.S, pl.sp.nblk, pl.sp.cblk);
#define W_(FN_)                                                                              \
  hipLaunchKernelGGL((conv_wgrad_halo_kernel<KH, KW, SW, REPL, FN_>), grid, dim3(256), pl.lds, \
                     a.st, a.G, a.in, a.slab, pl.g)
  if (pl.sp.FN == 1) W_(1); else if (pl.sp.FN == 2) W_(2); else W_(4);
#undef W_
}

int launch_wgrad_halo(const WgradArgs& a) {
  WHaloPlan pl;
  if (!(conv_config().halo & 2) || !whalo_plan(a, &pl)) return 0;
  TVQ_PLAN("conv_wgrad_halo S=%d", pl.sp.S);
#define M_(kh, kw, sw, r) whalo_launch<kh, kw, sw, r>(a, pl);
  TVQ_DISPATCH_KIND(a.kind, a.repl, M_)
#undef M_
  return pl.sp.S;
}

}  // namespace tvq
