// Weight gradients of the conv engine: conv_wgrad_kernel (split GEMM), conv_wgrad_halo_kernel,
// conv_wgrad_w8_kernel (narrow maps), conv_wgrad_t32_kernel (wide maps), their plans and
// workspace sizes, the deterministic split sums and their deferral scope
// (tvq_conv_wgrad_defer_*), the tvq_conv2d_wgrad / tvq_convT2d_wgrad entry points, and
// tvq_channel_sum.  (conv_wgrad_s2_kernel lives with the other stride-2 kernels.)
#include "tvq_conv_core.h"
#include "tvq_conv_internal.h"
#include "tvq_gemm.h"
#include "tvq_reduce.h"

#include <algorithm>
#include <vector>

namespace tvq {

// Weight gradient: rows = n (channels of G), cols = k' = (c, kh, kw), reduction over
// positions.  blockIdx.z = split index over positions; partial results go to
// slab[z][n][k'] and are summed in split order by wgrad_reduce_kernel.
template <int KH, int KW, int SW, bool REPL, int TN, int TK, int WN, int WK>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(const float* __restrict__ G,
                                                        const float* __restrict__ in,
                                                        float* __restrict__ slab, ConvGeom g,
                                                        int pos_per_split, int kcols) {
  // kcols = Kred (+1: a column of ones whose result is the bias gradient sum_m G[n, m])
  constexpr int BK = 16;  // positions per K-step
  constexpr int KK = KH * KW;
  constexpr int FN = TN / WN / 16;
  constexpr int FK = TK / WK / 16;
  constexpr int SA = ((TN + 31) / 32) * 32 + 16;
  constexpr int SB = ((TK + 31) / 32) * 32 + 16;
  constexpr int A_PER = TN * BK / 256;
  constexpr int B_PER = TK * BK / 256;
  static_assert(A_PER >= 1 && B_PER >= 1, "tile too small");
  __shared__ float As[BK * SA];
  __shared__ float Bs[BK * SB];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wn = wid % WN, wk = wid / WN;
  const int n0 = blockIdx.y * TN;
  const int kp0 = blockIdx.x * TK;
  const int p_begin = blockIdx.z * pos_per_split;
  const int p_end = min(g.Mpos, p_begin + pos_per_split);

  const int kk_t = tid % BK;  // each thread owns one position slot of the K-step
  const int a_nbase = tid / BK;
  const int b_kbase = tid / BK;
  // the thread's k' columns are fixed for the whole launch: decompose them once
  int bc_off[B_PER], bkh[B_PER], bkw[B_PER];
  unsigned bmask = 0u, bones = 0u;
#pragma unroll
  for (int j = 0; j < B_PER; ++j) {
    const int kp = kp0 + b_kbase + j * 16;
    const int c = kp / KK, r = kp - c * KK;
    bkh[j] = r / KW - g.oph;
    bkw[j] = r - (r / KW) * KW - g.opw;
    bc_off[j] = (kp < g.Kred) ? c * g.Hin * g.Win : 0;
    if (kp < g.Kred) bmask |= 1u << j;
    if (kp == g.Kred && kp < kcols) bones |= 1u << j;
  }

  float ra[A_PER], rb[B_PER];
  auto load_tile = [&](int p0) {
    const int p = p0 + kk_t;
    const bool pv = p < p_end;
    int b = 0, h = 0, w = 0;
    if (pv) {
      const uint32_t bh = fdiv((uint32_t)p, g.fd_wo);
      w = p - (int)bh * g.Wo;
      b = (int)fdiv((uint32_t)p, g.fd_hwo);
      h = (int)bh - b * g.Hout;
    }
    const float* gb = G + (((int64_t)b * g.N) * g.Hout + h) * g.Wo + w;
#pragma unroll
    for (int j = 0; j < A_PER; ++j) {
      const int n = n0 + a_nbase + j * 16;
      ra[j] = (pv && n < g.N) ? gb[(int64_t)n * g.Hout * g.Wo] : 0.f;
    }
    const float* inb = in + (int64_t)b * g.C * g.Hin * g.Win;
#pragma unroll
    for (int j = 0; j < B_PER; ++j) {
      float v = (pv && (bones >> j & 1u)) ? 1.0f : 0.f;
      if (pv && (bmask >> j & 1u)) {
        int hi = h + bkh[j], wi = w * SW + bkw[j];
        bool ok = true;
        if (REPL) {
          hi = hi < 0 ? 0 : (hi >= g.Hin ? g.Hin - 1 : hi);
          wi = wi < 0 ? 0 : (wi >= g.Win ? g.Win - 1 : wi);
        } else {
          ok = hi >= 0 && hi < g.Hin && wi >= 0 && wi < g.Win;
        }
        if (ok) v = inb[bc_off[j] + (int64_t)hi * g.Win + wi];
      }
      rb[j] = v;
    }
  };
  // rows of 16 positions, columns XOR-swizzled by (row & 14) as in gemm_kernel: the row
  // pitches are 16 mod 32 store banks, so unswizzled a half-wave's stores land on 16
  // banks (and with (row & 12) still 2-way).  Layout only (same k order, same results).
  auto store_tile = [&]() {
#pragma unroll
    for (int j = 0; j < A_PER; ++j) As[kk_t * SA + ((a_nbase + j * 16) ^ (kk_t & 14))] = ra[j];
#pragma unroll
    for (int j = 0; j < B_PER; ++j) Bs[kk_t * SB + ((b_kbase + j * 16) ^ (kk_t & 14))] = rb[j];
  };

  floatx4 acc[FN][FK];
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FK; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
  const int r16 = lane & 15, g4 = lane >> 4;
  if (p_begin < p_end) {
    load_tile(p_begin);
    for (int p0 = p_begin; p0 < p_end; p0 += BK) {
      __syncthreads();
      store_tile();
      __syncthreads();
      if (p0 + BK < p_end) load_tile(p0 + BK);
#pragma unroll
      for (int kk = 0; kk < BK; kk += 4) {
        float af[FN], bf[FK];
        const int swz = r16 ^ ((kk & 12) | (g4 & 2));  // sw(kk + g4)
#pragma unroll
        for (int i = 0; i < FN; ++i) af[i] = As[(kk + g4) * SA + (wn * FN + i) * 16 + swz];
#pragma unroll
        for (int j = 0; j < FK; ++j) bf[j] = Bs[(kk + g4) * SB + (wk * FK + j) * 16 + swz];
#pragma unroll
        for (int i = 0; i < FN; ++i)
#pragma unroll
          for (int j = 0; j < FK; ++j) acc[i][j] = mfma16x16x4(af[i], bf[j], acc[i][j]);
      }
    }
  }
  float* sl = slab + (int64_t)blockIdx.z * g.N * kcols;
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FK; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + (wn * FN + i) * 16 + 4 * g4 + r;
        const int kp = kp0 + (wk * FK + j) * 16 + r16;
        if (n < g.N && kp < kcols) sl[(int64_t)n * kcols + kp] = acc[i][j][r];
      }
}
// Per-channel sum over (B, HW) of a (B, C, HW) tensor: out[c] (+)= sum, deterministic.
// Stage 1: partial[c][chunk], chunk = `ipc` whole images of channel c (contiguous HW rows,
// float4 loads, 4 in flight per thread); stage 2 (fixed xor tree over <= 64 partials, one
// load per lane) in the last block of channel c when `cnt` is given, else
// chan_sum_final_kernel.
__device__ __forceinline__ void chan_sum_final_one(const float* part, int chunks, int c,
                                                   float* out, int accumulate) {
  float s = 0.f;
  for (int i = 0; i < chunks; ++i) s += ld_wt(part + (int64_t)c * chunks + i);
  out[c] = accumulate ? out[c] + s : s;
}
__global__ __launch_bounds__(256) void chan_sum_partial_kernel(const float* __restrict__ x, int B,
                                                               int C, int HW, int ipc, int chunks,
                                                               int vec, float* __restrict__ part,
                                                               int* __restrict__ cnt,
                                                               float* __restrict__ out,
                                                               int accumulate) {
  __shared__ float red[4];
  const int c = blockIdx.x, ch = blockIdx.y;
  const int b0 = ch * ipc, b1 = min(B, b0 + ipc);
  float s = 0.f;
  if (vec) {
    const int hw4 = HW >> 2, n4 = (b1 - b0) * hw4;
    for (int i0 = threadIdx.x; i0 < n4; i0 += 256 * 4) {
      floatx4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + u * 256;
        const int bb = b0 + (i < n4 ? i : 0) / hw4, q = (i < n4 ? i : 0) % hw4;
        v[u] = *reinterpret_cast<const floatx4*>(x + ((int64_t)bb * C + c) * HW + 4 * q);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (i0 + u * 256 < n4) s += (v[u][0] + v[u][1]) + (v[u][2] + v[u][3]);
    }
  } else {
    const int n = (b1 - b0) * HW;
    for (int i = threadIdx.x; i < n; i += 256) {
      const int bb = b0 + i / HW, p = i % HW;
      s += x[((int64_t)bb * C + c) * HW + p];
    }
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) st_wt(part + (int64_t)c * chunks + ch, s);
  if (cnt && last_block(cnt + c, chunks) && threadIdx.x < 64) {
    float t = threadIdx.x < chunks ? ld_wt(part + (int64_t)c * chunks + threadIdx.x) : 0.f;
    t = wave_sum(t);
    if (threadIdx.x == 0) out[c] = accumulate ? out[c] + t : t;
  }
}
__global__ void chan_sum_final_kernel(const float* __restrict__ part, int C, int chunks,
                                      float* __restrict__ out, int accumulate) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  chan_sum_final_one(part, chunks, c, out, accumulate);
}

// Halo-tile weight gradient: dW[n, c, tap] = sum_{b,h,w} G[b,n,h,w] In[b,c, h+kh-oh, w*SW+kw-ow]
// (+ a ones column for the bias gradient).  Block (s, nb, cb) loops over the images of
// split s; per image the G tile (NB x P) and the halo of CB input channels are loaded
// with all loads in flight, then the MFMAs reduce over the image's positions from LDS.
// Partials go to slab[s][n][kcols] and are summed in split order (wgrad_finish).
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

// Weight (+ bias) gradient of a 3x3, stride-1, zero-padded conv on narrow (B, C, 3, W)
// maps (instantiated for W = 8: the LF band's 64 / 128-channel ResBlock convs):
//   dW[n][c*9 + tap] (+ dB[n]) = sum_{b, p} dY[b, n, p] * X[b, c, window(p, tap)].
// conv_wgrad_halo_kernel staged one image per step and wrote one 64 x 577 slab per 1-3
// images (43 MB of HBM traffic per op for 3.3 MB of algorithmic bytes).  Here block
// (s, nb, cb) owns a 32-row x (CB*9 [+1]) column tile and W8_IMG images, walked in stages of
// 4 (one per wave) through two LDS buffers: stage s + 1's dY rows (16-B loads) and input
// halo rows are in registers while stage s multiplies, and are stored behind its MFMAs
// (round 5; loading all 16 images before the first MFMA left the MFMA pipe idle through the
// load and the memory idle through the MFMAs, one 86 KB block per CU).  Each wave reduces
// its images over all of the tile's columns (5 x 2 independent 16x16x4 MFMA chains), and
// the 4 partial tiles are summed in wave order through LDS.  One slab row per W8_IMG
// images: S = B / W8_IMG splits, summed in order by the deferred slab sum.
#ifndef TVQ_W8_IMG
#define TVQ_W8_IMG 16
#endif
constexpr int W8_IMG = TVQ_W8_IMG;
constexpr int W8_STG = 4;  // images per pipeline stage (one per wave)

// up to 4 problems of one shape in a launch, stacked on blockIdx.y (the fused ResBlocks'
// conv1 / conv2 weight gradients, tvq_resblock_w8.hip / tvq_resblock.hip)
struct W8Probs {
  const float* G[4];
  const float* X[4];
  float* slab[4];
};

template <int W, int CB>
__global__ __launch_bounds__(256) void conv_wgrad_w8_kernel(W8Probs pr, int B, int C, int N,
                                                           int kcols, int PS) {
  constexpr int P = 3 * W, WP = W + 2;
  constexpr int GST = P + 4;                         // dY row stride in LDS (16-B aligned)
  constexpr int KB = CB * 9 + 1, KT = (KB + 15) / 16;  // columns (+ bias), 16-col tiles
  constexpr int TW = KT * 16;                        // combine-buffer row length
  extern __shared__ float smem[];
  // W8_STG images per stage (one per wave), two stage buffers: stage s + 1's loads are in
  // registers while stage s multiplies, and its LDS stores follow the MFMAs
  constexpr int STG = W8_STG, NSTG = W8_IMG / STG;
  static_assert(STG == 4 && W8_IMG % STG == 0, "one image per wave and stage");
  const int hs_img = (CB + 1) * PS;
  const int gbuf = STG * 32 * GST, hbuf = STG * hs_img;
  float* Gs = smem;                                  // [2][STG][32][GST]
  float* Hs = smem + 2 * gbuf;                       // [2][STG][CB + 1][PS] (plane CB: ones)
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int j = lane & 15, kq = lane >> 4;
  // a multi-problem launch (conv_wgrad_w8_pair, conv_wgrad_wn_multi) stacks the problems of
  // the same shape on blockIdx.y
  const int nty = (N + 31) / 32, pb = (int)blockIdx.y / nty;
  const float* __restrict__ G = pr.G[pb];
  const float* __restrict__ X = pr.X[pb];
  float* __restrict__ slab = pr.slab[pb];
  const int s = blockIdx.x, n0 = ((int)blockIdx.y - pb * nty) * 32, c0 = blockIdx.z * CB;
  const bool bias = c0 + CB >= C && kcols > C * 9;   // this block also owns the bias column
  const int b0 = s * W8_IMG;
  const int ni = min(W8_IMG, B - b0);
  constexpr int GQ = P / 4, GN = STG * 32 * GQ, GU = (GN + 255) / 256;
  constexpr int XQ = W / 4, XN = STG * CB * 3 * XQ, XU = (XN + 255) / 256;
  float4 gv[GU], xv[XU];
  auto load = [&](int sg) {  // stage sg's dY rows and input rows into registers
#pragma unroll
    for (int u = 0; u < GU; ++u) {
      const int e = tid + u * 256;
      const int ii = e / (32 * GQ), r = (e / GQ) % 32, q = e % GQ, im = sg * STG + ii;
      gv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (e < GN && im < ni && n0 + r < N)
        gv[u] = *reinterpret_cast<const float4*>(G + ((int64_t)(b0 + im) * N + n0 + r) * P + 4 * q);
    }
#pragma unroll
    for (int u = 0; u < XU; ++u) {
      const int e = tid + u * 256;
      const int ii = e / (CB * 3 * XQ), c = (e / (3 * XQ)) % CB, hq = e % (3 * XQ), im = sg * STG + ii;
      xv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (e < XN && im < ni && c0 + c < C)
        xv[u] = *reinterpret_cast<const float4*>(X + ((int64_t)(b0 + im) * C + c0 + c) * P + 4 * hq);
    }
  };
  auto store = [&](int buf) {  // the registers into stage buffer buf (interior cells only)
#pragma unroll
    for (int u = 0; u < GU; ++u) {
      const int e = tid + u * 256;
      if (e < GN) {
        const int ii = e / (32 * GQ), r = (e / GQ) % 32, q = e % GQ;
        *reinterpret_cast<float4*>(Gs + buf * gbuf + (ii * 32 + r) * GST + 4 * q) = gv[u];
      }
    }
#pragma unroll
    for (int u = 0; u < XU; ++u) {
      const int e = tid + u * 256;
      if (e < XN) {
        const int ii = e / (CB * 3 * XQ), c = (e / (3 * XQ)) % CB, hq = e % (3 * XQ);
        const int h = hq / XQ, q = hq % XQ;
        float* d = Hs + buf * hbuf + ii * hs_img + c * PS + (h + 1) * WP + 1 + 4 * q;
        d[0] = xv[u].x; d[1] = xv[u].y; d[2] = xv[u].z; d[3] = xv[u].w;
      }
    }
  };
  load(0);
  // zero padding and the ones planes of both buffers (the stores only write interiors)
  for (int e = tid; e < 2 * hbuf; e += 256) Hs[e] = (e % hs_img) >= CB * PS ? 1.f : 0.f;
  __syncthreads();
  store(0);
  __syncthreads();
  int koff[KT];
#pragma unroll
  for (int t = 0; t < KT; ++t) {
    const int kl = t * 16 + j, c = kl / 9, tap = kl - 9 * c;
    koff[t] = kl < CB * 9 ? c * PS + (tap / 3) * WP + (tap % 3) : CB * PS;
  }
  floatx4 acc[2][KT];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int t = 0; t < KT; ++t) acc[i][t] = floatx4{0.f, 0.f, 0.f, 0.f};
  // wave w reduces images w, w + 4, ... (stage by stage), as the unstaged form did
  for (int sg = 0; sg < NSTG; ++sg) {
    const int cur = sg & 1;
    if (sg + 1 < NSTG) load(sg + 1);
    if (sg * STG + wid < ni) {
      const float* gb = Gs + cur * gbuf + wid * 32 * GST + j * GST + kq;
      const float* hb = Hs + cur * hbuf + wid * hs_img + kq;
#pragma unroll
      for (int m0 = 0; m0 < P; m0 += 4) {
        const int base = (m0 / W) * WP + (m0 % W);   // positions m0 .. m0+3: one row
        const float a0 = gb[m0], a1 = gb[16 * GST + m0];
#pragma unroll
        for (int t = 0; t < KT; ++t) {
          const float bv = hb[base + koff[t]];
          acc[0][t] = mfma16x16x4(a0, bv, acc[0][t]);
          acc[1][t] = mfma16x16x4(a1, bv, acc[1][t]);
        }
      }
    }
    // buffer cur ^ 1 was last read in stage sg - 1, before the previous barrier
    if (sg + 1 < NSTG) store(cur ^ 1);
    __syncthreads();
  }
  // the last stage's barrier: Gs / Hs reads done, the combine buffer aliases them
  float* red = smem;  // [4 waves][32 rows][TW]
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int t = 0; t < KT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[(wid * 32 + i * 16 + 4 * kq + r) * TW + t * 16 + j] = acc[i][t][r];
  __syncthreads();
  const int kb = CB * 9 + (bias ? 1 : 0);
  float* out = slab + (int64_t)s * N * kcols;
  for (int e = tid; e < 32 * kb; e += 256) {
    const int row = e / kb, col = e - row * kb;
    const int n = n0 + row;
    if (n >= N) continue;
    const float v = ((red[row * TW + col] + red[(32 + row) * TW + col]) +
                     red[(64 + row) * TW + col]) + red[(96 + row) * TW + col];
    const int kg = col < CB * 9 ? c0 * 9 + col : C * 9;
    out[(int64_t)n * kcols + kg] = v;
  }
}

template <int W, int CB>
static size_t w8_lds(int PS) {
  constexpr int P = 3 * W, GST = P + 4;
  const size_t a = (size_t)2 * W8_STG * 32 * GST + (size_t)2 * W8_STG * (CB + 1) * PS;
  const size_t red = (size_t)4 * 32 * (((CB * 9 + 1 + 15) / 16) * 16);
  return 4 * (a > red ? a : red);
}

// the shapes conv_wgrad_w8_kernel takes
static bool w8_fits(int64_t B, int64_t C, int64_t H, int64_t Wi, int64_t N, int64_t Wo, int64_t KH,
                    int64_t KW, int64_t SW, int64_t replicate) {
  return KH == 3 && KW == 3 && SW == 1 && !replicate && H == 3 && Wi == Wo &&
         Wi == 8 && N % 32 == 0 && C % 8 == 0 && B % W8_IMG == 0;
}
static int64_t w8_ws(int64_t B, int64_t N, int64_t C) {
  const int64_t S = B / W8_IMG, kc = C * 9 + 1;
  return S * N * kc + reduce_rows_scratch(S, N * kc);
}

// ---------------------------------------------------------------- wide-map weight gradient
// Weight (+ bias) gradient of stride-1 "same" 3x3 / 1x3 convs on maps whose rows are a
// multiple of 32 wide, with >= 64 output channels -- the HF band's 128 -> 128 and
// 16 -> 128 3x3 convs on (256, C, 3, 32) and the HF prior's Upscale Conv1d k3 on
// (256, C, 1, 96), 7.25 / 4.8 GFLOP each, where the split 16x16x4 kernel with 16-position
// LDS steps ran at ~0.3 of the fp32 MFMA peak.  A block owns a 128 (n) x 128 (k' = c*KK +
// tap) tile of one split of the positions; positions go in stages of one 32-wide row
// segment (b, h, w0 .. w0+31): the stage's dY rows (128 x 32, 16-B loads) and the input rows
// its k' columns need (channels k0/KK .. (k0+127)/KK, KH rows, 34 floats with the zero
// halo) are staged in LDS, double-buffered (the next stage's loads are in flight while this
// one multiplies), and each of the 8 waves runs 2 interleaved v_mfma_f32_32x32x2_f32 chains
// (32 n rows x 2 x 32 k' columns) over the stage's 16 position pairs.  The bias column
// (k' = Kred) is summed by the k0 = 0 blocks from the staged dY rows.  Slabs summed in
// split order (wgrad_finish).
constexpr int WT_T = 512, WT_AP = 128 + 4;  // threads; staged dY pitch ([p][n], n fastest)
template <int KH, int KW>
struct WtCfg {
  static constexpr int KK = KH * KW, NCH = 128 / KK + 2;  // channels a 128-column tile spans
  static constexpr int XROW = 34, XCH = KH * XROW;        // staged row, floats per channel
  static constexpr int AS = 32 * WT_AP, XS = NCH * XCH;   // floats per stage buffer
  static constexpr int XPER = (XS + WT_T - 1) / WT_T;     // input loads per thread
  static_assert(XPER <= 32, "staging mask");
};

struct WtGeom {
  int B, C, N, H, W, Kred, kcols;
  int segs;    // 32-wide segments per row (W / 32)
  int spr;     // stages per split
  int ntiles;  // 128-row n tiles
};

__device__ __forceinline__ int wt_crow(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

template <int KH, int KW>
struct WtRegs {  // one stage's global loads, in flight until stored to LDS
  float4 ga[2];
  float xv[WtCfg<KH, KW>::XPER];
  uint32_t ok;
};

template <int KH, int KW>
__global__ __launch_bounds__(WT_T) void conv_wgrad_t32_kernel(const float* __restrict__ G,
                                                             const float* __restrict__ X,
                                                             float* __restrict__ slab, WtGeom g,
                                                             int ktiles) {
  using R = WtCfg<KH, KW>;
  using Regs = WtRegs<KH, KW>;
  constexpr int PH = KH / 2, PW = (KW - 1) / 2;
  __shared__ float As[2][R::AS];
  __shared__ float Xs[2][R::XS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn = wid & 3, wk = wid >> 2;
  // XCD-aware map (tvq_gemm.h xcd_tile): the k' / n tiles of one position split share an
  // XCD, so its dY rows are fetched into one L2 and re-read from there
  int z, tile;
  xcd_tile((int)blockIdx.x, ktiles * g.ntiles, &z, &tile);
  const int nst = g.B * g.H * g.segs;
  const int s_begin = z * g.spr, s_end = min(nst, s_begin + g.spr);
  if (s_begin >= nst) return;  // padding block of the XCD map (no split)
  const int k0 = (tile % ktiles) * 128, n0 = (tile / ktiles) * 128;
  const int c_lo = k0 / R::KK;
  // this lane's B-operand offsets into a stage's Xs: columns k' = k0 + 64 wk + 32 j + l % 32
  // (past Kred: a valid column, never stored)
  int boff[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    int kp = k0 + wk * 64 + j * 32 + (lane & 31);
    kp = kp < g.Kred ? kp : g.Kred - 1;
    const int c = kp / R::KK, t = kp - c * R::KK, kh = t / KW, kw = t - kh * KW;
    boff[j] = (c - c_lo) * R::XCH + kh * R::XROW + kw;
  }
  auto load = [&](Regs& q, int s) {
    if (s >= s_end) return;
    const int row = s / g.segs, w0 = (s - row * g.segs) * 32;
    const int b = row / g.H, h = row - b * g.H;
#pragma unroll
    for (int j = 0; j < 2; ++j) {  // dY: 128 rows x 32 positions, 8 threads per row
      const int e = tid + j * WT_T, n = e >> 3, p4 = (e & 7) * 4;
      const int nn = n0 + n < g.N ? n0 + n : g.N - 1;
      q.ga[j] = *(const float4*)(G + ((int64_t)(b * g.N + nn) * g.H + h) * g.W + w0 + p4);
    }
    q.ok = 0u;
#pragma unroll
    for (int u = 0; u < R::XPER; ++u) {  // input rows: (channel, kh, 34 columns)
      const int e = tid + u * WT_T;
      const int c = e / R::XCH, r = e - c * R::XCH, kh = r / R::XROW, jj = r - kh * R::XROW;
      const int cc = c_lo + c, hi = h + kh - PH, wi = w0 - PW + jj;
      const bool ok = e < R::XS && cc < g.C && hi >= 0 && hi < g.H && wi >= 0 && wi < g.W;
      q.xv[u] = X[ok ? ((int64_t)(b * g.C + cc) * g.H + hi) * g.W + wi : 0];
      q.ok |= (ok ? 1u : 0u) << u;
    }
  };
  auto store = [&](const Regs& q, int buf) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int e = tid + j * WT_T, n = e >> 3, p4 = (e & 7) * 4;
      float* d = As[buf] + p4 * WT_AP + n;
      d[0] = q.ga[j].x;
      d[WT_AP] = q.ga[j].y;
      d[2 * WT_AP] = q.ga[j].z;
      d[3 * WT_AP] = q.ga[j].w;
    }
#pragma unroll
    for (int u = 0; u < R::XPER; ++u) {
      const int e = tid + u * WT_T;
      if (e < R::XS) Xs[buf][e] = (q.ok >> u & 1u) ? q.xv[u] : 0.f;
    }
  };
  floatx16 acc[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  float bsum = 0.f;  // bias partial of row n0 + tid (k0 == 0 blocks, tid < 128)
  // stage i: LDS buffer i & 1; two stages' loads in flight ahead of the one multiplying
  auto body = [&](int s, const Regs& next, Regs& free) {
    const int buf = (s - s_begin) & 1;
    load(free, s + 2);
    const float* as = As[buf] + wn * 32 + (lane & 31);
    const float* xs = Xs[buf];
#pragma unroll
    for (int st = 0; st < 16; ++st) {
      const int p = 2 * st + (lane >> 5);
      const float a = as[p * WT_AP];
#pragma unroll
      for (int j = 0; j < 2; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, xs[boff[j] + p], acc[j], 0, 0, 0);
    }
    if (k0 == 0 && tid < 128) {
#pragma unroll 8
      for (int p = 0; p < 32; ++p) bsum += As[buf][p * WT_AP + tid];
    }
    if (s + 1 < s_end) store(next, buf ^ 1);
    __syncthreads();
  };
  Regs r0, r1;
  load(r0, s_begin);
  load(r1, s_begin + 1);
  store(r0, 0);
  __syncthreads();
  for (int s = s_begin; s < s_end; s += 2) {
    body(s, r1, r0);                       // r1: stage s+1; r0 <- stage s+2
    if (s + 1 < s_end) body(s + 1, r0, r1);  // r0: stage s+2; r1 <- stage s+3
  }
  float* sl = slab + (int64_t)z * g.N * g.kcols;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int kp = k0 + wk * 64 + j * 32 + (lane & 31);
    if (kp >= g.Kred) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n = n0 + wn * 32 + wt_crow(r, lane >> 5);
      if (n < g.N) sl[(int64_t)n * g.kcols + kp] = acc[j][r];
    }
  }
  if (k0 == 0 && tid < 128 && g.kcols > g.Kred && n0 + tid < g.N)
    sl[(int64_t)(n0 + tid) * g.kcols + g.Kred] = bsum;
}

// the shapes the wide-map weight-gradient kernel takes
static bool wt32_fits(int64_t B, int64_t C, int64_t H, int64_t Wi, int64_t N, int64_t Wo,
                      int64_t KH, int64_t KW, int64_t SW, int64_t replicate) {
  return SW == 1 && !replicate && KW == 3 && (KH == 1 || KH == 3) && Wi == Wo &&
         Wi % 32 == 0 && N >= 64 && C >= 64 && B * C * H * Wi < (1ll << 31) &&
         B * N * H * Wo < (1ll << 31);
}
static void wt32_plan(int64_t B, int64_t C, int64_t H, int64_t W, int64_t N, int64_t KK,
                      int* S, int* spr) {
  const int64_t kt = (C * KK + 127) / 128, nt = (N + 127) / 128;
  const int64_t nst = B * H * (W / 32);
  int64_t s = (512 + kt * nt - 1) / (kt * nt);  // ~2 blocks per CU
  if (s > 256) s = 256;
  if (s > nst) s = nst;
  if (s < 1) s = 1;
  const int64_t per = (nst + s - 1) / s;
  *spr = (int)per;
  *S = (int)((nst + per - 1) / per);
}
static int64_t wt32_ws(int64_t B, int64_t C, int64_t H, int64_t W, int64_t N, int64_t KK) {
  int S, spr;
  wt32_plan(B, C, H, W, N, KK, &S, &spr);
  const int64_t kc = C * KK + 1;
  return (int64_t)S * N * kc + reduce_rows_scratch(S, N * kc);
}

struct WHaloPlan {
  WHaloGeom g;
  int FN, S, nblk, cblk;
  size_t lds;
};

// slab floats cap of the halo weight gradient (8M: LF 64-ch leg 26 vs 30 us at 4M)
static int64_t whalo_slab_max() { return (int64_t)(8 << 20); }

// split count depends only on (N, C, KK, B) so the workspace query can reproduce it
static int whalo_splits(int64_t N, int64_t C, int KK, int64_t B, int nblk, int cblk) {
  const int64_t kc = C * KK + 1;
  int64_t S = 1024 / (nblk * cblk);
  const int64_t cap = whalo_slab_max() / (N * kc);
  if (S > cap) S = cap;
  if (S > B) S = B;
  if (S < 1) S = 1;
  const int64_t ips = (B + S - 1) / S;
  return (int)((B + ips - 1) / ips);
}

static void whalo_blocking(int64_t N, int64_t C, int KK, int* FN, int* CB) {
  *FN = N <= 16 ? 1 : (N <= 32 ? 2 : 4);
  int cb = 1;
  while (cb * 2 <= C && (cb * 2) * KK + 1 <= 256) cb *= 2;  // <= 16 k-tiles of 16
  if (cb > C) cb = (int)C;
  *CB = cb;
}

// Halo-plane stride of conv_wgrad_halo_kernel's image (>= hw): the B-operand read of a
// half-wave (lanes j = 0..15 over 16 consecutive reduction columns (c, tap), kq = 0..1 over
// 2 positions) is Hs[c*PS + toff(tap) + kq*SW + base]; its 32 addresses should fall on 32
// distinct (a/4) mod 32 banks.  The stride residue mod 32 that minimises the extra bank
// cycles over the kernel's column tiles is chosen on the host (layout only: same sums).
static int whalo_plane_stride(int hw, int KK, int KW, int WP, int SW, int CB) {
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

static bool whalo_plan(int B, int C, int Hin, int Win, int N, int Hout, int Wo, int KH, int KW,
                       int SW, int oh, int ow, int kcols, WHaloPlan* pl) {
  if (Wo % 4 != 0) return false;
  // long images with many channels (the Upscale Conv1d) and the 128x128 ResBlock convs
  // run better on the split GEMM (tools/conv_shapes_bench.py: 148 vs 178 us at W 32)
  if (Hout * Wo > 128 && C > 64) return false;
  if ((int64_t)C * N >= 128 * 128) return false;
  WHaloGeom g;
  g.B = B; g.C = C; g.Hin = Hin; g.Win = Win; g.N = N; g.Hout = Hout; g.Wo = Wo;
  g.oh = oh; g.ow = ow;
  g.HP = Hout + KH - 1;
  g.WP = (Wo - 1) * SW + KW;
  const int hw = g.HP * g.WP;
  g.P = Hout * Wo;
  g.GST = g.P + ((2 - g.P % 32) + 32) % 32;
  if (g.WP < 2 || g.P >= (1 << 16)) return false;
  g.dv_hw = make_div16(hw);
  g.dv_wp = make_div16(g.WP);
  g.dv_gst = make_div16(g.GST);
  const int KK = KH * KW;
  int FN, CB;
  whalo_blocking(N, C, KK, &FN, &CB);
  g.PS = whalo_plane_stride(hw, KK, KW, g.WP, SW, CB);
  g.CB = CB;
  g.Kred = C * KK;
  g.kcols = kcols;
  const size_t fl = (size_t)FN * 16 * g.GST + (size_t)(CB + 1) * g.PS;
  if (fl * 4 > (size_t)HALO_LDS_MAX) return false;
  pl->nblk = (N + FN * 16 - 1) / (FN * 16);
  pl->cblk = (C + CB - 1) / CB;
  pl->S = whalo_splits(N, C, KK, B, pl->nblk, pl->cblk);
  g.ips = (B + pl->S - 1) / pl->S;
  pl->g = g;
  pl->FN = FN;
  pl->lds = fl * 4;
  return true;
}

template <int KH, int KW, int SW, bool REPL>
static void launch_wgrad_halo(const float* G, const float* in, float* slab, const WHaloPlan& pl,
                              hipStream_t st) {
  const dim3 grid(pl.S, pl.nblk, pl.cblk);
#define W_(FN_)                                                                              \
  hipLaunchKernelGGL((conv_wgrad_halo_kernel<KH, KW, SW, REPL, FN_>), grid, dim3(256), pl.lds, \
                     st, G, in, slab, pl.g)
  if (pl.FN == 1) W_(1); else if (pl.FN == 2) W_(2); else W_(4);
#undef W_
}

template <int KH, int KW, int SW, bool REPL>
static void launch_wgrad(const float* G, const float* in, float* slab, int splits, int pps,
                         const ConvGeom& g, int kcols, hipStream_t st) {
  if (g.N <= 16) {
    dim3 grid((kcols + 63) / 64, (g.N + 15) / 16, splits);
    hipLaunchKernelGGL((conv_wgrad_kernel<KH, KW, SW, REPL, 16, 64, 1, 4>), grid, dim3(256), 0, st,
                       G, in, slab, g, pps, kcols);
  } else {
    dim3 grid((kcols + 63) / 64, (g.N + 63) / 64, splits);
    hipLaunchKernelGGL((conv_wgrad_kernel<KH, KW, SW, REPL, 64, 64, 2, 2>), grid, dim3(256), 0, st,
                       G, in, slab, g, pps, kcols);
  }
}

static int wgrad_splits(const ConvGeom& g, int tiles, int* pps) {
  // aim for ~1024 blocks, each with >= 512 positions
  int splits = (1024 + tiles - 1) / tiles;
  const int maxs = (g.Mpos + 511) / 512;
  if (splits > maxs) splits = maxs;
  if (splits < 1) splits = 1;
  if (splits > 256) splits = 256;
  int per = (g.Mpos + splits - 1) / splits;
  per = (per + 15) / 16 * 16;
  splits = (g.Mpos + per - 1) / per;
  *pps = per;
  return splits;
}

// Deferred weight-gradient split sums (tvq_conv_wgrad_defer_*): inside a scope the
// slabs' reductions are recorded and run by a few batched launches at the flush instead
// of one launch per conv (the caller keeps the workspaces alive until then).  Each record
// carries the stream its producer ran on: the flush issues each stream's records as one
// batch on that stream (ordered after that stream's producers), so a backward spread over
// several streams (a branch's side stream) defers its reductions too.
struct RdRec {
  RrJob job;
  hipStream_t st;
};
static std::vector<RdRec> g_rd;
static bool g_rd_on = false, g_rd_paused = false;

static bool rd_records(int64_t rows) {
  return g_rd_on && !g_rd_paused && rows <= RR_ONE_ROWS;
}

static void wgrad_finish(float* slab, int splits, int64_t N, int64_t kcols, float* dw,
                         float* db, int accumulate, hipStream_t st) {
  // deterministic split sum; kcols = Kred+1 splits out the bias column.  The level-1
  // scratch follows the slab in the workspace.
  const int64_t L = kcols > 0 && db ? kcols : 0;
  if (rd_records(splits)) {  // the single-level case: batched at the flush
    g_rd.push_back({{slab, dw, db, splits, N * kcols, L, accumulate}, st});
    return;
  }
  reduce_rows(slab, splits, N * kcols, N * kcols, dw, db, L, accumulate,
              slab + (int64_t)splits * N * kcols, st);
}

// out[0..N) (+)= sum of the P contiguous rows of `in` (a parameter gradient only the
// optimizer reads): joins the open deferral scope's batch, else reduce_rows now
void param_rows_finish(const float* in, int64_t P, int64_t N, float* out, int accumulate,
                       float* scratch, hipStream_t st) {
  if (rd_records(P)) {
    g_rd.push_back({{in, out, nullptr, P, N, 0, accumulate}, st});
    return;
  }
  reduce_rows(in, P, N, N, out, nullptr, 0, accumulate, scratch, st);
}

void conv_wgrad_finish(float* slab, int splits, int64_t N, int64_t kcols, float* dw, float* db,
                       int accumulate, hipStream_t st) {
  wgrad_finish(slab, splits, N, kcols, dw, db, accumulate, st);
}

template <int W>
static void w8_launch_w(const W8Probs& pr, dim3 grid, int B, int C, int N, int kcols, int PS,
                        hipStream_t st) {
  static bool attr = false;  // > 64 KB of dynamic LDS must be opted into once per instance
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_wgrad_w8_kernel<W, 8>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
    attr = true;
  }
  hipLaunchKernelGGL((conv_wgrad_w8_kernel<W, 8>), grid, dim3(256), (w8_lds<W, 8>(PS)), st, pr, B,
                     C, N, kcols, PS);
}

// n <= 4 weight (+ bias) gradients of 3x3 stride-1 zero-padded C -> N convs of one shape on
// (B, C, 3, W) maps, W = 8 or 16, in one conv_wgrad_w8_kernel<W, 8> launch: problem i reduces
// dy[i] against x[i] into its S = B / W8_IMG slab rows ws[i], each summed in order into
// dw[i] / db[i] (bit for bit the sums of one launch per problem).  `note`: the caller's plan line.
template <typename... A>
static void w8_launch(int W, int n, const float* const* x, const float* const* dy, float* const* ws,
                      float* const* dw, float* const* db, int64_t B, int64_t C, int64_t N,
                      int kcols, int accumulate, hipStream_t st, const char* note, A... note_args) {
  const int S = (int)(B / W8_IMG);
  const int PS = whalo_plane_stride(5 * (W + 2), 9, 3, W + 2, 1, 8);
  const dim3 grid((unsigned)S, (unsigned)(n * (N / 32)), (unsigned)(C / 8));
  W8Probs pr = {};
  for (int i = 0; i < n; ++i) {
    pr.G[i] = dy[i];
    pr.X[i] = x[i];
    pr.slab[i] = ws[i];
  }
  TVQ_PLAN(note, note_args...);
  if (W == 8) w8_launch_w<8>(pr, grid, (int)B, (int)C, (int)N, kcols, PS, st);
  else w8_launch_w<16>(pr, grid, (int)B, (int)C, (int)N, kcols, PS, st);
  for (int i = 0; i < n; ++i) wgrad_finish(ws[i], S, N, kcols, dw[i], db[i], accumulate, st);
}

// the fused RB<32, 16> ResBlocks' conv1 / conv2 on (B, C, 3, 16) maps (tvq_resblock.hip)
int64_t conv_wgrad_w16_slab_floats(int64_t B, int64_t C, int64_t N) {
  return (B / W8_IMG) * N * (C * 9 + 1);
}
bool conv_wgrad_w16_fits(int64_t B, int64_t C, int64_t N) {
  return B % W8_IMG == 0 && C % 8 == 0 && N % 32 == 0 && B > 0;
}
void conv_wgrad_w16_multi(int n, const float* const* x, const float* const* dy, float* const* ws,
                          float* const* dw, float* const* db, int64_t B, int64_t C, int64_t N,
                          int accumulate, hipStream_t st) {
  w8_launch(16, n, x, dy, ws, dw, db, B, C, N, (int)(C * 9 + 1), accumulate, st,
            "conv_wgrad_w16 n=%d S=%d", n, (int)(B / W8_IMG));
}
// the LF ResBlock pair's four convs on (B, C, 3, 8) maps
bool conv_wgrad_w8_fits(int64_t B, int64_t C, int64_t N) {
  return w8_fits(B, C, 3, 8, N, 8, 3, 3, 1, 0);
}
void conv_wgrad_w8_multi(int n, const float* const* x, const float* const* dy, float* const* ws,
                         float* const* dw, float* const* db, int64_t B, int64_t C, int64_t N,
                         int accumulate, hipStream_t st) {
  w8_launch(8, n, x, dy, ws, dw, db, B, C, N, (int)(C * 9 + 1), accumulate, st,
            "conv_wgrad_w8 n=%d S=%d", n, (int)(B / W8_IMG));
}
// the fused LF ResBlock's conv1 and conv2 (tvq_resblock_w8.hip), each slab in its own workspace
bool conv_wgrad_w8_pair(const float* x0, const float* dy0, float* ws0, float* dw0, float* db0,
                        const float* x1, const float* dy1, float* ws1, float* dw1, float* db1,
                        int64_t B, int64_t C, int64_t N, int accumulate, hipStream_t st) {
  if (!w8_fits(B, C, 3, 8, N, 8, 3, 3, 1, 0)) return false;
  const float* const x[2] = {x0, x1};
  const float* const dy[2] = {dy0, dy1};
  float* const ws[2] = {ws0, ws1};
  float* const dw[2] = {dw0, dw1};
  float* const db[2] = {db0, db1};
  w8_launch(8, 2, x, dy, ws, dw, db, B, C, N, (int)(C * 9 + 1), accumulate, st,
            "conv_wgrad_w8 pair S=%d", (int)(B / W8_IMG));
  return true;
}

// Weight gradient workspace (floats): split slabs [splits][N][Kred+1].
static int64_t wgrad_ws(int64_t N, int64_t Kred, int64_t Mpos, int* splits_out, int* pps_out) {
  ConvGeom g;
  g.Mpos = (int)Mpos;
  const int64_t kc = Kred + 1;
  const int tiles = (int)(((kc + 63) / 64) * ((N + (N <= 16 ? 15 : 63)) / (N <= 16 ? 16 : 64)));
  int pps;
  const int splits = wgrad_splits(g, tiles, &pps);
  if (splits_out) *splits_out = splits;
  if (pps_out) *pps_out = pps;
  return (int64_t)splits * N * kc + reduce_rows_scratch(splits, N * kc);
}

static int64_t whalo_ws(int64_t N, int64_t C, int64_t KH, int64_t KW, int64_t B) {
  int FN, CB;
  const int KK = (int)(KH * KW);
  whalo_blocking(N, C, KK, &FN, &CB);
  const int nblk = (int)((N + FN * 16 - 1) / (FN * 16)), cblk = (int)((C + CB - 1) / CB);
  const int S = whalo_splits(N, C, KK, B, nblk, cblk);
  const int64_t kc = C * KK + 1;
  return (int64_t)S * N * kc + reduce_rows_scratch(S, N * kc);
}

int64_t conv_wgrad_ws(int64_t N, int64_t C, int64_t KH, int64_t KW, int64_t B, int64_t Hout,
                      int64_t Wo) {
  const int64_t a = wgrad_ws(N, C * KH * KW, B * Hout * Wo, nullptr, nullptr);
  const int64_t h = whalo_ws(N, C, KH, KW, B);
  const int64_t w = (KH == 3 && KW == 3 && B % W8_IMG == 0) ? w8_ws(B, N, C) : 0;
  const int64_t t = wt32_fits(B, C, Hout, Wo, N, Wo, KH, KW, 1, 0)
                        ? wt32_ws(B, C, Hout, Wo, N, KH * KW) : 0;
  // conv_wgrad_s2 (Wo: the width of G)
  const int64_t s2 = (KH == 3 && KW == 4 && C <= 16 && N <= 16) ? ws2_ws(B, C, Wo, N) : 0;
  return std::max(std::max(std::max(a, t), std::max(h, w)), s2);
}

}  // namespace tvq

using namespace tvq;

extern "C" int tvq_conv_wgrad_defer_begin(void) {
  TVQ_CHECK_ARG(!g_rd_on, "tvq_conv_wgrad_defer_begin: a scope is already open");
  g_rd.clear();
  g_rd_on = true;
  return TVQ_OK;
}

// kept for the ABI: every record now carries its own stream, so this is begin()
extern "C" int tvq_wgrad_defer_begin_stream(tvq_stream_t stream) {
  (void)stream;
  return tvq_conv_wgrad_defer_begin();
}

extern "C" int tvq_conv_wgrad_defer_pause(int64_t paused) {
  g_rd_paused = paused != 0;
  return TVQ_OK;
}

extern "C" int tvq_conv_wgrad_defer_flush(tvq_stream_t stream) {
  g_rd_on = false;
  g_rd_paused = false;
  // one batch per producing stream, in first-record order ((void)stream: kept for the ABI)
  (void)stream;
  std::vector<RrJob> jobs;
  while (!g_rd.empty()) {
    const hipStream_t st = g_rd.front().st;
    jobs.clear();
    std::vector<RdRec> rest;
    int64_t bytes = 0;
    for (const RdRec& r : g_rd) {
      if (r.st == st) {
        jobs.push_back(r.job);
        bytes += r.job.P * r.job.N * 4;
        TVQ_PLAN("wgrad_flush_job st=%p P=%lld N=%lld", (void*)st, (long long)r.job.P,
                 (long long)r.job.N);
      } else {
        rest.push_back(r);
      }
    }
    TVQ_PLAN("wgrad_flush st=%p jobs=%d MB=%.1f", (void*)st, (int)jobs.size(), bytes / 1e6);
    reduce_rows_batch(jobs.data(), (int)jobs.size(), st);
    g_rd.swap(rest);
  }
  return launch_status("tvq_conv_wgrad_defer_flush");
}

// Conv2d weight (+bias) gradient: dW[co,ci,kh,kw] (+)= sum dY[b,co,h,wo] X[b,ci,h+kh-PH, wo*SW+kw-PW],
// db[co] (+)= sum dY[b,co,h,wo] (db may be NULL)
extern "C" int tvq_conv2d_wgrad(const float* x, int64_t B, int64_t Ci, int64_t H, int64_t Wi,
                                const float* dy, int64_t Co, int64_t Wo, int64_t KH, int64_t KW,
                                int64_t SW, int64_t replicate, float* dw, float* db,
                                int64_t accumulate, float* workspace, tvq_stream_t stream) {
  TVQ_CHECK_ARG(x && dy && dw && workspace, "tvq_conv2d_wgrad: bad arguments");
  const int kind = kind_of((int)KH, (int)KW, (int)SW);
  TVQ_CHECK_ARG(kind >= 0, "tvq_conv2d_wgrad: unsupported kernel");
  ConvGeom g = make_geom((int)B, (int)Ci, (int)H, (int)Wi, (int)Co, (int)H, (int)Wo, (int)KH,
                         (int)KW, PH_OF(KH), PW_OF(KW), Ci * KH * KW, KH * KW);
  const int kcols = g.Kred + (db ? 1 : 0);
  hipStream_t st = (hipStream_t)stream;
  if (ws2_fits(Ci, H, Co, KH, KW, SW)) {
    const int S = ws2_launch(dy, x, workspace, (int)B, (int)Ci, (int)Co, (int)Wi, (int)Wo, kcols,
                             replicate != 0, st);
    wgrad_finish(workspace, S, Co, kcols, dw, db, (int)accumulate, st);
    return launch_status("tvq_conv2d_wgrad(s2)");
  }
  if (wt32_fits(B, Ci, H, Wi, Co, Wo, KH, KW, SW, replicate)) {
    WtGeom t;
    t.B = (int)B; t.C = (int)Ci; t.N = (int)Co; t.H = (int)H; t.W = (int)Wi;
    t.Kred = g.Kred; t.kcols = kcols; t.segs = (int)(Wi / 32);
    int S;
    wt32_plan(B, Ci, H, Wi, Co, KH * KW, &S, &t.spr);
    const int kt = (g.Kred + 127) / 128;
    t.ntiles = (int)((Co + 127) / 128);
    const dim3 grid(xcd_grid(S, kt * t.ntiles));
    TVQ_PLAN("conv_wgrad_t32 S=%d", S);
    if (KH == 3)
      hipLaunchKernelGGL((conv_wgrad_t32_kernel<3, 3>), grid, dim3(WT_T), 0, st, dy, x, workspace, t,
                         kt);
    else
      hipLaunchKernelGGL((conv_wgrad_t32_kernel<1, 3>), grid, dim3(WT_T), 0, st, dy, x, workspace, t,
                         kt);
    wgrad_finish(workspace, S, Co, kcols, dw, db, (int)accumulate, st);
    return launch_status("tvq_conv2d_wgrad(t32)");
  }
  if (w8_fits(B, Ci, H, Wi, Co, Wo, KH, KW, SW, replicate)) {
    w8_launch(8, 1, &x, &dy, &workspace, &dw, &db, B, Ci, Co, kcols, (int)accumulate, st,
              "conv_wgrad_w8 S=%d", (int)(B / W8_IMG));
    return launch_status("tvq_conv2d_wgrad(w8)");
  }
  WHaloPlan pl;
  if ((conv_config().halo & 2) && whalo_plan((int)B, (int)Ci, (int)H, (int)Wi, (int)Co, (int)H,
                                             (int)Wo, (int)KH, (int)KW, (int)SW, PH_OF(KH),
                                             PW_OF(KW), kcols, &pl)) {
    TVQ_PLAN("conv_wgrad_halo S=%d", pl.S);
#define M_(a, b_, c, d) launch_wgrad_halo<a, b_, c, d>(dy, x, workspace, pl, st);
    TVQ_DISPATCH_KIND(kind, replicate, M_)
#undef M_
    wgrad_finish(workspace, pl.S, Co, kcols, dw, db, (int)accumulate, st);
    return launch_status("tvq_conv2d_wgrad(halo)");
  }
  int splits, pps;
  wgrad_ws(Co, g.Kred, g.Mpos, &splits, &pps);
  TVQ_PLAN("conv_wgrad split=%d", splits);
#define M_(a, b_, c, d) launch_wgrad<a, b_, c, d>(dy, x, workspace, splits, pps, g, kcols, st);
  TVQ_DISPATCH_KIND(kind, replicate, M_)
#undef M_
  wgrad_finish(workspace, splits, Co, kcols, dw, db, (int)accumulate, st);
  return launch_status("tvq_conv2d_wgrad");
}

// ConvTranspose2d weight gradient: dW[ci,co,kh,kw] (+)= sum X[b,ci,h,wi] dY[b,co,h+kh-PH, wi*SW+kw-PW]
extern "C" int tvq_convT2d_wgrad(const float* x, int64_t B, int64_t Ci, int64_t H, int64_t Wi,
                                 const float* dy, int64_t Co, int64_t Wo, int64_t KH, int64_t KW,
                                 int64_t SW, float* dw, int64_t accumulate, float* workspace,
                                 tvq_stream_t stream) {
  TVQ_CHECK_ARG(x && dy && dw && workspace, "tvq_convT2d_wgrad: bad arguments");
  const int kind = kind_of((int)KH, (int)KW, (int)SW);
  TVQ_CHECK_ARG(kind >= 0, "tvq_convT2d_wgrad: unsupported kernel");
  // G = X (N = Ci channels at X's positions), In = dY gathered F-style (C = Co)
  ConvGeom g = make_geom((int)B, (int)Co, (int)H, (int)Wo, (int)Ci, (int)H, (int)Wi, (int)KH,
                         (int)KW, PH_OF(KH), PW_OF(KW), Co * KH * KW, KH * KW);
  hipStream_t st = (hipStream_t)stream;
  if (ws2_fits(Co, H, Ci, KH, KW, SW)) {
    const int S = ws2_launch(x, dy, workspace, (int)B, (int)Co, (int)Ci, (int)Wo, (int)Wi, g.Kred,
                             false, st);
    wgrad_finish(workspace, S, Ci, g.Kred, dw, nullptr, (int)accumulate, st);
    return launch_status("tvq_convT2d_wgrad(s2)");
  }
  WHaloPlan pl;
  if ((conv_config().halo & 2) && whalo_plan((int)B, (int)Co, (int)H, (int)Wo, (int)Ci, (int)H, (int)Wi,
                                      (int)KH, (int)KW, (int)SW, PH_OF(KH), PW_OF(KW), g.Kred,
                                      &pl)) {
    TVQ_PLAN("conv_wgrad_halo S=%d", pl.S);
#define M_(a, b_, c, d) launch_wgrad_halo<a, b_, c, false>(x, dy, workspace, pl, st);
    TVQ_DISPATCH_KIND(kind, 0, M_)
#undef M_
    wgrad_finish(workspace, pl.S, Ci, g.Kred, dw, nullptr, (int)accumulate, st);
    return launch_status("tvq_convT2d_wgrad(halo)");
  }
  int splits, pps;
  wgrad_ws(Ci, g.Kred, g.Mpos, &splits, &pps);
  TVQ_PLAN("conv_wgrad split=%d", splits);
#define M_(a, b_, c, d) launch_wgrad<a, b_, c, false>(x, dy, workspace, splits, pps, g, g.Kred, st);
  TVQ_DISPATCH_KIND(kind, 0, M_)
#undef M_
  wgrad_finish(workspace, splits, Ci, g.Kred, dw, nullptr, (int)accumulate, st);
  return launch_status("tvq_convT2d_wgrad");
}

extern "C" int64_t tvq_channel_sum_workspace(int64_t B, int64_t C, int64_t HW) {
  if (HW == 1) {
    const int64_t r = reduce_rows_scratch(B, C);
    return r > 0 ? r : 1;
  }
  int64_t chunks = (B * HW + 8191) / 8192;
  if (chunks > 64) chunks = 64;
  if (chunks < 1) chunks = 1;
  return C * chunks;
}

// out[c] (+)= sum_{b,p} x[b,c,p]   (bias gradients), deterministic
extern "C" int tvq_channel_sum(const float* x, int64_t B, int64_t C, int64_t HW, float* out,
                               int64_t accumulate, float* workspace, tvq_stream_t stream) {
  TVQ_CHECK_ARG(x && out && workspace && B > 0 && C > 0 && HW > 0, "tvq_channel_sum: bad args");
  if (HW == 1) {  // row-major (B, C): coalesced column sums
    reduce_rows(x, B, C, C, out, nullptr, 0, (int)accumulate, workspace, (hipStream_t)stream);
    return launch_status("tvq_channel_sum");
  }
  const int64_t chunks = tvq_channel_sum_workspace(B, C, HW) / C;
  hipStream_t st = (hipStream_t)stream;
  int* cnt = counters(C, FIN_REDUCE);
  // whole images per chunk (at most the workspace's `chunks`, which is <= 64)
  const int64_t ipc = (B + chunks - 1) / chunks;
  const int64_t nch = (B + ipc - 1) / ipc;
  TVQ_CHECK_ARG(ipc * HW < (1ll << 31), "tvq_channel_sum: bad geometry");
  const int vec = (HW & 3) == 0 && ((uintptr_t)x & 15) == 0;
  hipLaunchKernelGGL(chan_sum_partial_kernel, dim3((int)C, (int)nch), dim3(256), 0, st, x,
                     (int)B, (int)C, (int)HW, (int)ipc, (int)nch, vec, workspace, cnt, out,
                     (int)accumulate);
  if (!cnt)
    hipLaunchKernelGGL(chan_sum_final_kernel, dim3((int)((C + 127) / 128)), dim3(128), 0, st,
                       workspace, (int)C, (int)nch, out, (int)accumulate);
  return launch_status("tvq_channel_sum");
}
