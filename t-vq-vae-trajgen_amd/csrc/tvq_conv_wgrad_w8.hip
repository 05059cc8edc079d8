// conv_wgrad_w8_kernel: the image-batched 3x3 weight gradient on narrow (B, C, 3, W) maps,
// W = 8 or 16, its plan, and its launchers: one problem for tvq_conv2d_wgrad, up to four of
// one shape in a launch for the fused ResBlocks (conv_wgrad_w8_multi).
#include "tvq_conv_core.h"
#include "tvq_conv_internal.h"
#include "tvq_reduce.h"

namespace tvq {

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
// images (w8_splits), summed in order by the deferred slab sum.
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
  // a multi-problem launch (conv_wgrad_w8_multi) stacks the problems of
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

int w8_splits(int64_t B) { return B % W8_IMG == 0 ? (int)(B / W8_IMG) : 0; }

// the 3x3 stride-1 zero-padded C -> N convs on (B, C, 3, W) maps the kernel takes
bool conv_wgrad_w8_fits(int W, int64_t B, int64_t C, int64_t N) {
  return (W == 8 || W == 16) && w8_splits(B) > 0 && C % 8 == 0 && N % 32 == 0;
}

int64_t conv_wgrad_w8_slab_floats(int W, int64_t B, int64_t C, int64_t N) {
  (void)W;  // one row per image block at either width
  return wgrad_slab_floats(w8_splits(B), N, C, 9);
}

// n <= 4 problems of one shape in one conv_wgrad_w8_kernel<W, 8> launch: problem i reduces
// dy[i] against x[i] into the S = w8_splits(B) slab rows ws[i]
static void w8_launch(int W, int n, const float* const* x, const float* const* dy, float* const* ws,
                      int S, int B, int C, int N, int kcols, hipStream_t st) {
  const int PS = whalo_plane_stride(5 * (W + 2), 9, 3, W + 2, 1, 8);
  const dim3 grid((unsigned)S, (unsigned)(n * (N / 32)), (unsigned)(C / 8));
  W8Probs pr = {};
  for (int i = 0; i < n; ++i) {
    pr.G[i] = dy[i];
    pr.X[i] = x[i];
    pr.slab[i] = ws[i];
  }
  if (W == 8) w8_launch_w<8>(pr, grid, B, C, N, kcols, PS, st);
  else w8_launch_w<16>(pr, grid, B, C, N, kcols, PS, st);
}

int launch_wgrad_w8(const WgradArgs& a) {
  if (!(a.KH == 3 && a.KW == 3 && a.SW == 1 && !a.repl && a.Hin == 3 && a.Win == a.Wo &&
        a.Win == 8 && conv_wgrad_w8_fits(8, a.B, a.C, a.N)))
    return 0;
  const int S = w8_splits(a.B);
  TVQ_PLAN("conv_wgrad_w8 S=%d", S);
  w8_launch(8, 1, &a.in, &a.G, &a.slab, S, a.B, a.C, a.N, a.kcols, a.st);
  return S;
}

void conv_wgrad_w8_multi(int W, int n, const float* const* x, const float* const* dy,
                         float* const* ws, float* const* dw, float* const* db, int64_t B,
                         int64_t C, int64_t N, int accumulate, hipStream_t st) {
  const int S = w8_splits(B), kcols = (int)(C * 9 + 1);
  TVQ_PLAN(W == 8 ? "conv_wgrad_w8 n=%d S=%d" : "conv_wgrad_w16 n=%d S=%d", n, S);
  w8_launch(W, n, x, dy, ws, S, (int)B, (int)C, (int)N, kcols, st);
  for (int i = 0; i < n; ++i) conv_wgrad_finish(ws[i], S, N, kcols, dw[i], db[i], accumulate, st);
}

}  // namespace tvq
