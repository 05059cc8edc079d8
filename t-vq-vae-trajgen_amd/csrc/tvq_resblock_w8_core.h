// The one implementation of the fused ResBlocks on the LF band's (B, C, 3, 8) maps: the
// identity block 64 -> 64 (tvq_resblock_w8.hip) and the projection blocks 64 -> 128 /
// 128 -> 64 (tvq_resblock_w8p.hip) are one set of stage bodies templated on <CI, CO>, the
// projection steps compiled in when CI != CO, and one set of host-side builders (workspace
// layout, weight views, kernel arguments, weight gradients) at the end of this header.
//
// One 8-wave block per image.  Every conv runs on v_mfma_f32_32x32x2_f32 with the staged halo
// planes in LDS as the B operand and the weights, read from L2 (packed [tap][c][n] by the
// pack cache: one coalesced 128-B row per half-wave and step), as the A operand.  A conv of
// NCI -> NCO channels runs NCO / 32 output tiles x NCI / 16 input-channel chunks over the 8
// waves: wave w owns tile w % (NCO / 32) and a contiguous run of chunks, whose 72 weight
// values per chunk it requests a chunk ahead of their MFMAs (the first before the image is
// staged); the chunk-group partial tiles are summed in LDS in group order.  The 24 positions
// of an image fill 24 of a tile's 32 columns.
#pragma once
#include "tvq_bn.h"
#include "tvq_common.h"
#include "tvq_conv_internal.h"
#include "tvq_reduce.h"

namespace tvq {
namespace w8 {

constexpr int W = 8, P = 3 * W, NW = 8, T = 64 * NW;
constexpr int WP = W + 2;          // halo row stride
constexpr int PS = 80;             // halo plane stride (5 x 10 cells, padded; == 16 mod 32)
constexpr int RED = NW * 16 * 64;  // one partial 32 x 32 tile per wave

struct WView {  // element (row n, reduction channel c, tap t) at w[n*sn + c*sc + t*st]
  const float* w;
  int64_t sn, sc, st;
};

struct Args {
  const float *x, *h, *dy, *du_in;
  const float *a1, *b1, *a2, *b2, *bp;
  const float *bn_w, *bn_b, *rmean, *rvar;  // eval / BN backward
  const float* save;                         // mean | invstd | scale | shift
  const float* coef;                         // BN backward (sum du, sum du xhat) per channel
  WView w1, w2, wp;                          // forward views (eval / fwd) or data-gradient views
  float *h_out, *s_out, *y, *du, *dx, *g_out, *slabda;
  double* part;
  float eps, drop_p, drop_scale, invN;
  const int64_t* seed_ptr;
  uint64_t offset;
  int B;
};

// LDS of a <CI, CO> block: the halo planes of the wider side, then the partial tiles
template <int CI, int CO>
constexpr int planes_floats() { return (CI > CO ? CI : CO) * PS; }
template <int CI, int CO>
constexpr size_t lds_bytes() { return 4 * (size_t)(planes_floats<CI, CO>() + RED); }

__device__ __forceinline__ int wid_() { return __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); }

// halo cell of position p (the 3x3 window's centre)
__device__ __forceinline__ int cell(int c, int p) { return c * PS + WP + 1 + (p / W) * WP + p % W; }

// zero the border cells of NC halo planes
template <int NC>
__device__ __forceinline__ void border(float* __restrict__ S) {
  for (int i = threadIdx.x; i < NC * 26; i += T) {
    const int c = i / 26, r = i - 26 * c;
    int o;
    if (r < WP) o = r;
    else if (r < 2 * WP) o = 4 * WP + (r - WP);
    else {
      const int k = r - 2 * WP;
      o = (1 + (k >> 1)) * WP + ((k & 1) ? W + 1 : 0);
    }
    S[c * PS + o] = 0.f;
  }
}

// Elementwise layout of NC channels: wave w, iteration j < NC / 16 -> channel
// (NC / 8) w + 2 j + (lane >> 5), position lane & 31 (valid below 24); a channel's 24
// positions sit in one 32-lane half.
template <int NC>
__device__ __forceinline__ int el_c(int j) {
  return (NC / 8) * wid_() + 2 * j + ((threadIdx.x & 63) >> 5);
}
__device__ __forceinline__ int el_p() { return threadIdx.x & 31; }

// sum over the lane's 32-lane half (fixed xor tree)
__device__ __forceinline__ double half_sum_d(double v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Conv geometry of NCI -> NCO: NTO output tiles of 32 rows, NCG chunk groups of CPW chunks
// of 16 input channels; wave w owns tile w % NTO and chunks (w / NTO) * CPW + i.
template <int NCI, int NCO>
struct Geo {
  static constexpr int NTO = NCO / 32, NCG = NW / NTO, NCH = NCI / 16, CPW = NCH / NCG;
  static_assert(NCO % 32 == 0 && NW % NTO == 0 && NCI % 16 == 0 && NCH % NCG == 0 && CPW >= 1,
                "unsupported conv geometry");
  static __device__ __forceinline__ int tile() { return (unsigned)wid_() % NTO; }
  static __device__ __forceinline__ int chunk0() { return (unsigned)wid_() / NTO * CPW; }
};

// this lane's TAPS x 8 weights of chunk ch: W(row 32 nt + (l & 31), reduction channel
// 16 ch + (l >> 5) + 2u, tap t)
template <int NCI, int NCO, int TAPS>
__device__ __forceinline__ void load_chunk(const WView wv, int ch, float (&a)[TAPS][8]) {
  const int lane = threadIdx.x & 63;
  const float* wp = wv.w + (int64_t)(32 * Geo<NCI, NCO>::tile() + (lane & 31)) * wv.sn +
                    (int64_t)(16 * ch + (lane >> 5)) * wv.sc;
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int u = 0; u < 8; ++u) a[t][u] = wp[(int64_t)(2 * u) * wv.sc + (int64_t)t * wv.st];
}

// The wave's first chunk, issued ahead (at the kernel's start, before an epilogue: the
// weights do not depend on the staged image), so its L2 round trip overlaps the elementwise
// work; the scheduling barrier keeps the loads from sinking next to their MFMAs.
template <int NCI, int NCO, int TAPS>
__device__ __forceinline__ void preload(const WView wv, float (&a)[TAPS][8]) {
  load_chunk<NCI, NCO, TAPS>(wv, Geo<NCI, NCO>::chunk0(), a);
  __builtin_amdgcn_sched_barrier(0);
}

// one chunk's TAPS x 8 MFMA steps: weights a, the chunk's first plane at the lane's window sp
template <int TAPS, bool FLIP>
__device__ __forceinline__ floatx16 conv_chunk(const float (&a)[TAPS][8],
                                               const float* __restrict__ sp, floatx16 acc) {
#pragma unroll
  for (int t = 0; t < TAPS; ++t) {
    const int tt = FLIP ? TAPS - 1 - t : t, off = TAPS == 1 ? 0 : (tt / 3) * WP + tt % 3;
#pragma unroll
    for (int u = 0; u < 8; ++u)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t][u], sp[2 * u * PS + off], acc, 0, 0, 0);
  }
  return acc;
}

// The block's conv of the staged planes S (NCI of them) into red[w][16][64]; a0 holds the
// first chunk's weights (preload), the following chunks alternate between a0 and a second
// buffer.  FLIP: data gradient (taps mirrored).  TAPS = 1: the 1x1 conv (centre cells).
template <int NCI, int NCO, int TAPS, bool FLIP>
__device__ __forceinline__ void conv(const WView wv, float (&a0)[TAPS][8],
                                     const float* __restrict__ S, float* __restrict__ red) {
  using G = Geo<NCI, NCO>;
  const int lane = threadIdx.x & 63, wid = wid_();
  const int r32 = lane & 31, hl = lane >> 5;
  const int ch0 = G::chunk0();
  const int m = r32 < P ? r32 : 0;
  const float* sp = S + (16 * ch0 + hl) * PS + (m / W) * WP + (m % W) + (TAPS == 1 ? WP + 1 : 0);
  floatx16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  if constexpr (G::CPW == 1) {
    // one chunk: no second buffer, and no scheduling barriers around the MFMAs (they cost
    // the 64 -> 64 kernels registers, the pair kernels an occupancy step)
    acc = conv_chunk<TAPS, FLIP>(a0, sp, acc);
  } else {
    float a1[TAPS][8];
#pragma unroll
    for (int i = 0; i < G::CPW; ++i) {
      float(&cur)[TAPS][8] = (i & 1) ? a1 : a0;
      float(&nxt)[TAPS][8] = (i & 1) ? a0 : a1;
      if (i + 1 < G::CPW) load_chunk<NCI, NCO, TAPS>(wv, ch0 + i + 1, nxt);
      __builtin_amdgcn_sched_barrier(0);
      acc = conv_chunk<TAPS, FLIP>(cur, sp + 16 * i * PS, acc);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) red[(wid * 16 + r) * 64 + lane] = acc[r];
}

// conv result (row n, position p): the NCG chunk-group partials of tile n / 32, group order
template <int NCI, int NCO>
__device__ __forceinline__ float conv_at(const float* __restrict__ red, int n, int p) {
  using G = Geo<NCI, NCO>;
  const int nt = n >> 5, i = n & 31, h = (i >> 2) & 1, r = (i & 3) + 4 * (i >> 3);
  const int l = p + 32 * h;
  float s = red[(nt * 16 + r) * 64 + l];
#pragma unroll
  for (int g = 1; g < G::NCG; ++g) s += red[((nt + G::NTO * g) * 16 + r) * 64 + l];
  return s;
}

// ---------------------------------------------------------------- stage bodies
//   fwd1  s1 = Snake_a1(x) staged (and stored: the conv1 weight gradient's input) ->
//         h = conv1(s1) + b1 -> store h; per-image fp64 BN partial sums
//   fwd2  s2 = Snake_a2(BN(h)) staged (and stored) -> v = Dropout(conv2(s2) + b2);
//         y = x + v, or the raw x restaged -> y = (proj(x) + bp) + v
//   eval  both (three) convs in one launch, BN from the running statistics
//   bwd2  g2 = Dropout'(dy) staged (and stored) -> ds2 = conv2^T(g2) -> du = ds2 * Snake'(u)
//         (u = BN(h) recomputed) -> store du; per-image (sum du, sum du xhat, Snake a2 term)
//   bwd1  dh = BN'(du) staged (and stored) -> ds1 = conv1^T(dh) -> dx = ds1 * Snake'(x) + dy,
//         or dy restaged -> ... + proj^T(dy); the Snake a1 term (a slab row)
// The bodies take the block's LDS, the 3x3 weight registers and, for a fused pair of
// consecutive identity blocks (w8_fwd21 / w8_bwd12), the activation handed over in registers
// (every body has the same elementwise layout) with the next body's weights already loaded
// (`next`: issued right after this body's last 3x3 MFMA).
template <int CI, int CO>
__device__ __forceinline__ void fwd1_body(const Args& a, float* sm, float (&wa)[9][8],
                                          const float (*xin)[CI / 16]) {
  float* S = sm;
  float* red = sm + planes_floats<CI, CO>();
  constexpr int JI = CI / 16, JO = CO / 16;
  const int b = blockIdx.x, p = el_p(), pp = p < P ? p : 0;
  const int64_t i0 = (int64_t)b * CI * P, o0 = (int64_t)b * CO * P;
  float xv[JI], av[JI], bv[JO];
#pragma unroll
  for (int j = 0; j < JI; ++j) {
    xv[j] = xin ? (*xin)[j] : a.x[i0 + el_c<CI>(j) * P + pp];
    av[j] = a.a1[el_c<CI>(j)];
  }
#pragma unroll
  for (int j = 0; j < JO; ++j) bv[j] = a.b1[el_c<CO>(j)];
  // after the staging operands: their wait leaves the weights in flight (a pair's second
  // body has them already)
  if (!xin) preload<CI, CO, 9>(a.w1, wa);
  border<CI>(S);
#pragma unroll
  for (int j = 0; j < JI; ++j) {
    const int c = el_c<CI>(j);
    if (p >= P) continue;
    const float s = snake_f(xv[j], av[j], 1.0f / av[j]);
    S[cell(c, p)] = s;
    a.s_out[i0 + c * P + p] = s;
  }
  __syncthreads();
  conv<CI, CO, 9, false>(a.w1, wa, S, red);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < JO; ++j) {
    const int c = el_c<CO>(j);
    double s0 = 0.0, s1 = 0.0;
    if (p < P) {
      const float v = conv_at<CI, CO>(red, c, p) + bv[j];
      a.h_out[o0 + c * P + p] = v;
      s0 = (double)v;
      s1 = (double)v * (double)v;
    }
    s0 = half_sum_d(s0);
    s1 = half_sum_d(s1);
    if ((threadIdx.x & 31) == 0) {  // [c][image][2]: bn_stats_final_kernel's chunk layout
      a.part[((int64_t)c * a.B + b) * 2 + 0] = s0;
      a.part[((int64_t)c * a.B + b) * 2 + 1] = s1;
    }
  }
}

template <int CI, int CO>
__device__ __forceinline__ void fwd2_body(const Args& a, float* sm, float (&wa)[9][8],
                                          float (&yout)[CO / 16], const WView* next) {
  constexpr bool PROJ = CI != CO;
  float* S = sm;
  float* red = sm + planes_floats<CI, CO>();
  constexpr int JI = CI / 16, JO = CO / 16;
  const int b = blockIdx.x, p = el_p(), pp = p < P ? p : 0;
  const int64_t i0 = (int64_t)b * CI * P, o0 = (int64_t)b * CO * P;
  float hv[JO], xv[JI], av[JO], bv[JO];
  float sc[JO], sh[JO];  // the batch statistics' affine form (bn_stats_final_kernel's)
#pragma unroll
  for (int j = 0; j < JO; ++j) {
    const int c = el_c<CO>(j);
    hv[j] = a.h[o0 + c * P + pp];
    av[j] = a.a2[c];
    bv[j] = a.b2[c];
    sc[j] = a.save[2 * CO + c];
    sh[j] = a.save[3 * CO + c];
  }
#pragma unroll
  for (int j = 0; j < JI; ++j) xv[j] = a.x[i0 + el_c<CI>(j) * P + pp];
  float wq[1][8];
  preload<CO, CO, 9>(a.w2, wa);
  if constexpr (PROJ) preload<CI, CO, 1>(a.wp, wq);
  border<CO>(S);
#pragma unroll
  for (int j = 0; j < JO; ++j) {
    const int c = el_c<CO>(j);
    if (p >= P) continue;
    const float s = snake_f(fmaf(hv[j], sc[j], sh[j]), av[j], 1.0f / av[j]);
    S[cell(c, p)] = s;
    a.s_out[o0 + c * P + p] = s;
  }
  __syncthreads();
  conv<CO, CO, 9, false>(a.w2, wa, S, red);
  if (next) preload<CI, CO, 9>(*next, wa);
  __syncthreads();
  const uint64_t seed = a.drop_p > 0.f ? mix_seed(a.seed_ptr, a.offset) : 0ull;
#pragma unroll
  for (int j = 0; j < JO; ++j) {
    const int c = el_c<CO>(j);
    yout[j] = 0.f;
    if (p >= P) continue;
    const int64_t gi = o0 + c * P + p;
    float v = conv_at<CO, CO>(red, c, p) + bv[j];
    if (a.drop_p > 0.f) v = uniform01(seed, (uint64_t)gi) >= a.drop_p ? v * a.drop_scale : 0.f;
    if constexpr (PROJ) {
      yout[j] = v;  // the projection joins below
    } else {
      yout[j] = xv[j] + v;
      a.y[gi] = yout[j];
    }
  }
  if constexpr (PROJ) {
    __syncthreads();  // red and S read: the projection's input and partials reuse them
#pragma unroll
    for (int j = 0; j < JI; ++j)
      if (p < P) S[cell(el_c<CI>(j), p)] = xv[j];
    __syncthreads();
    conv<CI, CO, 1, false>(a.wp, wq, S, red);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < JO; ++j) {
      const int c = el_c<CO>(j);
      if (p >= P) continue;
      yout[j] = (conv_at<CI, CO>(red, c, p) + a.bp[c]) + yout[j];
      a.y[o0 + c * P + p] = yout[j];
    }
  }
}

template <int CI, int CO>
__device__ __forceinline__ void eval_body(const Args& a, float* sm) {
  constexpr bool PROJ = CI != CO;
  float* S = sm;
  float* red = sm + planes_floats<CI, CO>();
  constexpr int JI = CI / 16, JO = CO / 16;
  const int b = blockIdx.x, p = el_p(), pp = p < P ? p : 0;
  const int64_t i0 = (int64_t)b * CI * P, o0 = (int64_t)b * CO * P;
  float wa[9][8], wq[1][8], xv[JI];
#pragma unroll
  for (int j = 0; j < JI; ++j) xv[j] = a.x[i0 + el_c<CI>(j) * P + pp];
  preload<CI, CO, 9>(a.w1, wa);
  border<CI>(S);
#pragma unroll
  for (int j = 0; j < JI; ++j) {
    const int c = el_c<CI>(j);
    if (p >= P) continue;
    const float av = a.a1[c];
    S[cell(c, p)] = snake_f(xv[j], av, 1.0f / av);
  }
  __syncthreads();
  conv<CI, CO, 9, false>(a.w1, wa, S, red);
  preload<CO, CO, 9>(a.w2, wa);  // conv2's first weights in flight during conv1's epilogue
  __syncthreads();
  float s2[JO];
#pragma unroll
  for (int j = 0; j < JO; ++j) {  // BN from the running statistics (bn_eval's affine form)
    const int c = el_c<CO>(j);
    const float inv = 1.0f / sqrtf(a.rvar[c] + a.eps);
    const float scv = (a.bn_w ? a.bn_w[c] : 1.f) * inv;
    const float shv = (a.bn_b ? a.bn_b[c] : 0.f) - a.rmean[c] * scv;
    const float av = a.a2[c];
    s2[j] = snake_f(fmaf(conv_at<CI, CO>(red, c, pp) + a.b1[c], scv, shv), av, 1.0f / av);
  }
  __syncthreads();  // conv1's partials read; S free
  if constexpr (CO > CI) border<CO>(S);  // planes CI .. CO - 1 have no zero border yet
#pragma unroll
  for (int j = 0; j < JO; ++j)
    if (p < P) S[cell(el_c<CO>(j), p)] = s2[j];
  __syncthreads();
  conv<CO, CO, 9, false>(a.w2, wa, S, red);
  if constexpr (PROJ) preload<CI, CO, 1>(a.wp, wq);
  __syncthreads();
  if constexpr (!PROJ) {
#pragma unroll
    for (int j = 0; j < JO; ++j) {
      const int c = el_c<CO>(j);
      if (p < P) a.y[o0 + c * P + p] = xv[j] + (conv_at<CO, CO>(red, c, p) + a.b2[c]);
    }
  } else {
    float v2[JO];
#pragma unroll
    for (int j = 0; j < JO; ++j) v2[j] = conv_at<CO, CO>(red, el_c<CO>(j), pp) + a.b2[el_c<CO>(j)];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < JI; ++j)
      if (p < P) S[cell(el_c<CI>(j), p)] = xv[j];
    __syncthreads();
    conv<CI, CO, 1, false>(a.wp, wq, S, red);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < JO; ++j) {
      const int c = el_c<CO>(j);
      if (p < P) a.y[o0 + c * P + p] = (conv_at<CI, CO>(red, c, p) + a.bp[c]) + v2[j];
    }
  }
}

template <int CI, int CO>
__device__ __forceinline__ void bwd2_body(const Args& a, float* sm, float (&wa)[9][8],
                                          const float (*dyin)[CO / 16]) {
  float* G = sm;
  float* red = sm + planes_floats<CI, CO>();
  constexpr int JO = CO / 16;
  const int b = blockIdx.x, p = el_p(), pp = p < P ? p : 0;
  const int64_t o0 = (int64_t)b * CO * P;
  float gv[JO], hv[JO];
#pragma unroll
  for (int j = 0; j < JO; ++j) {
    const int64_t gi = o0 + el_c<CO>(j) * P + pp;
    gv[j] = dyin ? (*dyin)[j] : a.dy[gi];
    hv[j] = a.h[gi];
  }
  if (!dyin) preload<CO, CO, 9>(a.w2, wa);
  border<CO>(G);
  const uint64_t seed = a.drop_p > 0.f ? mix_seed(a.seed_ptr, a.offset) : 0ull;
#pragma unroll
  for (int j = 0; j < JO; ++j) {
    const int c = el_c<CO>(j);
    if (p >= P) continue;
    const int64_t gi = o0 + c * P + p;
    float d = gv[j];
    if (a.drop_p > 0.f) d = uniform01(seed, (uint64_t)gi) >= a.drop_p ? d * a.drop_scale : 0.f;
    G[cell(c, p)] = d;
    a.g_out[gi] = d;
  }
  __syncthreads();
  conv<CO, CO, 9, true>(a.w2, wa, G, red);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < JO; ++j) {
    const int c = el_c<CO>(j);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    if (p < P) {
      const float av = a.a2[c], inv_a = 1.0f / av;
      const float sc = a.save[2 * CO + c], sh = a.save[3 * CO + c];
      const float mu = a.save[c], is = a.save[CO + c];
      const float gs = conv_at<CO, CO>(red, c, p);  // d loss / d s2
      const float uu = fmaf(hv[j], sc, sh);
      float sn, cs;
      sincosf(av * uu, &sn, &cs);
      const float tt = 2.0f * sn * cs;
      const float d = gs + gs * inv_a * tt * av;  // d loss / d u (bn_bwd_partial_kernel)
      const float xhat = (hv[j] - mu) * is;
      a.du[o0 + c * P + p] = d;
      s0 = d;
      s1 = (double)d * xhat;
      s2 = (double)(gs * inv_a * tt * uu) - (double)(gs * (sn * sn) * inv_a * inv_a);
    }
    s0 = half_sum_d(s0);
    s1 = half_sum_d(s1);
    s2 = half_sum_d(s2);
    if ((threadIdx.x & 31) == 0) {  // [c][image][3]: bn_bwd_final_kernel's chunk layout
      double* q = a.part + ((int64_t)c * a.B + b) * 3;
      q[0] = s0;
      q[1] = s1;
      q[2] = s2;
    }
  }
}

// the data gradients run CO -> CI: conv1^T's (and proj^T's) rows are the input channels
template <int CI, int CO>
__device__ __forceinline__ void bwd1_body(const Args& a, float* sm, float (&wa)[9][8],
                                          float (&dxout)[CI / 16], const WView* next) {
  constexpr bool PROJ = CI != CO;
  float* G = sm;
  float* red = sm + planes_floats<CI, CO>();
  constexpr int JI = CI / 16, JO = CO / 16;
  const int b = blockIdx.x, p = el_p(), pp = p < P ? p : 0;
  const int64_t i0 = (int64_t)b * CI * P, o0 = (int64_t)b * CO * P;
  float dv[JO], hv[JO], yv[JO], xv[JI];
#pragma unroll
  for (int j = 0; j < JO; ++j) {
    const int64_t gi = o0 + el_c<CO>(j) * P + pp;
    dv[j] = a.du_in[gi];
    hv[j] = a.h[gi];
    yv[j] = a.dy[gi];  // the epilogue's operands, requested with the prologue's
  }
#pragma unroll
  for (int j = 0; j < JI; ++j) xv[j] = a.x[i0 + el_c<CI>(j) * P + pp];
  float md[JO], mx[JO];  // the BN backward coefficients (bn_bwd_final_kernel's sums)
#pragma unroll
  for (int j = 0; j < JO; ++j) {
    md[j] = a.coef[2 * el_c<CO>(j)] * a.invN;
    mx[j] = a.coef[2 * el_c<CO>(j) + 1] * a.invN;
  }
  float wq[1][8];
  preload<CO, CI, 9>(a.w1, wa);
  if constexpr (PROJ) preload<CO, CI, 1>(a.wp, wq);
  border<CO>(G);
  // dh = w * invstd * (du - mean(du) - xhat * mean(du * xhat))  (bn_bwd_apply_kernel)
#pragma unroll
  for (int j = 0; j < JO; ++j) {
    const int c = el_c<CO>(j);
    if (p >= P) continue;
    const float mu = a.save[c], is = a.save[CO + c], bw = a.bn_w ? a.bn_w[c] : 1.f;
    const float xhat = (hv[j] - mu) * is;
    const float g = bw * is * (dv[j] - md[j] - xhat * mx[j]);
    G[cell(c, p)] = g;
    a.g_out[o0 + c * P + p] = g;
  }
  __syncthreads();
  conv<CO, CI, 9, true>(a.w1, wa, G, red);
  if (next) preload<CO, CI, 9>(*next, wa);
  __syncthreads();
  float gs1[JI];  // d loss / d s1, read before the projection's partials replace conv1^T's
  if constexpr (PROJ) {
#pragma unroll
    for (int j = 0; j < JI; ++j) gs1[j] = conv_at<CO, CI>(red, el_c<CI>(j), pp);
    __syncthreads();  // red and G read: the projection's input and partials reuse them
#pragma unroll
    for (int j = 0; j < JO; ++j)
      if (p < P) G[cell(el_c<CO>(j), p)] = yv[j];
    __syncthreads();
    conv<CO, CI, 1, false>(a.wp, wq, G, red);
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < JI; ++j) {
    const int c = el_c<CI>(j);
    double s0 = 0.0;
    dxout[j] = 0.f;
    if (p < P) {
      const float av = a.a1[c], inv_a = 1.0f / av;
      float gs;
      if constexpr (PROJ) gs = gs1[j];
      else gs = conv_at<CO, CI>(red, c, p);
      float sn, cs;
      sincosf(av * xv[j], &sn, &cs);
      const float tt = 2.0f * sn * cs;
      // snake_bwd_kernel, plus the skip's gradient: dy, or the projection's input gradient
      // (one expression each: how it is written decides which products the compiler
      // contracts into FMAs, and with that the last bit of dx)
      if constexpr (PROJ) dxout[j] = (gs + gs * inv_a * tt * av) + conv_at<CO, CI>(red, c, p);
      else dxout[j] = (gs + gs * inv_a * tt * av) + yv[j];
      a.dx[i0 + c * P + p] = dxout[j];
      s0 = (double)(gs * inv_a * tt * xv[j]) - (double)(gs * (sn * sn) * inv_a * inv_a);
    }
    s0 = half_sum_d(s0);
    if ((threadIdx.x & 31) == 0) a.slabda[(int64_t)b * CI + c] = (float)s0;
  }
}

// ---------------------------------------------------------------- host side
// one block per image
template <int CI, int CO, typename... A>
static void launch(void (*k)(A...), int64_t B, hipStream_t st, A... a) {
  constexpr size_t lds = lds_bytes<CI, CO>();
  hipLaunchKernelGGL(k, dim3((unsigned)B), dim3(T), lds, st, a...);
}

static size_t al(size_t n) { return (n + 255) & ~(size_t)255; }

struct Ws {  // workspace layout (bytes); wgp is empty and the packs hold no wp when Ci == Co
  size_t part, slabda1, coef, g2, dh, du, wg1, wg2, wgp, pk, total;
  int64_t n1, n2, np;  // floats of a w1 / w2 / wp pack: forward views, then data-gradient views
};
static Ws ws_layout(int64_t B, int64_t Ci, int64_t Co) {
  Ws w;
  const bool proj = Ci != Co;
  const size_t img = (size_t)B * Co * P * 4;
  const size_t slabd = (size_t)(B * Ci + reduce_rows_scratch(B, Ci)) * 4;
  w.n1 = 9 * Ci * Co; w.n2 = 9 * Co * Co; w.np = proj ? Ci * Co : 0;
  w.part = 0;
  w.slabda1 = w.part + al((size_t)B * Co * 3 * 8);
  w.coef = w.slabda1 + al(slabd);
  w.g2 = w.coef + al((size_t)2 * Co * 4);
  w.dh = w.g2 + al(img);
  w.du = w.dh + al(img);
  w.wg1 = w.du + al(img);
  w.wg2 = w.wg1 + al((size_t)tvq_conv_workspace(4, B, Ci, 3, W, Co, 3, 3, 1, 0) * 4);
  w.wgp = w.wg2 + al((size_t)tvq_conv_workspace(4, B, Co, 3, W, Co, 3, 3, 1, 0) * 4);
  w.pk = w.wgp + (proj ? al((size_t)tvq_conv_workspace(4, B, Ci, 3, W, Co, 1, 1, 1, 0) * 4) : 0);
  w.total = w.pk + al((size_t)2 * (w.n1 + w.n2 + w.np) * 4);
  return w;
}

// forward: rows = the conv's output channels, reduction = its input channels; data
// gradient (transposed): rows = input channels, reduction = output channels
static WView view(const float* w, int64_t cin, int64_t cout, int KK, bool transposed, float* ws,
                  hipStream_t st) {
  WView v;
  if (transposed)
    v.w = conv_pack_view(w, (int)cin, (int)cout, KK, KK, cin * KK, ws, st, &v.sn, &v.sc, &v.st);
  else
    v.w = conv_pack_view(w, (int)cout, (int)cin, KK, cin * KK, KK, ws, st, &v.sn, &v.sc, &v.st);
  return v;
}

// the three weight views, packed into pk (null: the open pack-cache scope's packs, else the
// weights as they are)
static void set_views(Args& a, const Ws& L, int64_t Ci, int64_t Co, const float* w1,
                      const float* w2, const float* wp, bool transposed, float* pk,
                      hipStream_t st) {
  a.w1 = view(w1, Ci, Co, 9, transposed, pk, st);
  a.w2 = view(w2, Co, Co, 9, transposed, pk ? pk + L.n1 : nullptr, st);
  if (Ci != Co) a.wp = view(wp, Ci, Co, 1, transposed, pk ? pk + L.n1 + L.n2 : nullptr, st);
}

static void set_dropout(Args& a, float drop_p, const int64_t* seed_ptr, uint64_t offset) {
  a.drop_p = drop_p;
  a.drop_scale = drop_p > 0.f ? 1.0f / (1.0f - drop_p) : 1.0f;
  a.seed_ptr = seed_ptr; a.offset = offset;
}

// Parameter lists: p = {a1, w1, b1, bn_w, bn_b, a2, w2, b2, wp, bp}, rs = {running_mean,
// running_var}, q = {a1, w1, bn_w, save, a2, w2, wp}, g = {da1, dw1, db1, dbn_w, dbn_b, da2,
// dw2, db2, dwp, dbp}; the projection's entries are read when Ci != Co only.
struct Fwd {
  Args a;  // s_out: set per launch to s1 / s2
  BNFinal fin;
  float *s1, *s2;
};
static Fwd fwd_args(int64_t Ci, int64_t Co, const float* x, int64_t B, const float* const* p,
                    float* const* rs, int64_t* nbt, float momentum, float eps, float drop_p,
                    const int64_t* seed_ptr, uint64_t offset, float* saved, float* y, float* save,
                    void* workspace, hipStream_t st) {
  const Ws L = ws_layout(B, Ci, Co);
  char* ws = (char*)workspace;
  Fwd f = {};
  Args& a = f.a;
  a.x = x; a.a1 = p[0]; a.b1 = p[2]; a.a2 = p[5]; a.b2 = p[7];
  if (Ci != Co) a.bp = p[9];
  set_views(a, L, Ci, Co, p[1], p[6], Ci != Co ? p[8] : nullptr, false, (float*)(ws + L.pk), st);
  a.h_out = saved; a.h = saved; a.y = y; a.save = save;  // saved: h | s1 | s2
  f.s1 = saved + B * P * Co;
  f.s2 = saved + B * P * (Co + Ci);
  a.part = (double*)(ws + L.part);
  a.B = (int)B;
  set_dropout(a, drop_p, seed_ptr, offset);
  // the per-image partials -> save, running statistics
  f.fin = {(int)Co, (int)B, B * P, eps, momentum, p[3], p[4], rs[0], rs[1], nbt,
           save, save + Co, save + 2 * Co, save + 3 * Co};
  return f;
}

static Args eval_args(int64_t Ci, int64_t Co, const float* x, int64_t B, const float* const* p,
                      const float* running_mean, const float* running_var, float eps, float* y,
                      hipStream_t st) {
  Args a = {};
  a.x = x; a.a1 = p[0]; a.b1 = p[2]; a.a2 = p[5]; a.b2 = p[7];
  if (Ci != Co) a.bp = p[9];
  a.bn_w = p[3]; a.bn_b = p[4]; a.rmean = running_mean; a.rvar = running_var; a.eps = eps;
  // no workspace: the open pack-cache scope's packs, else the weights as they are
  set_views(a, Ws{}, Ci, Co, p[1], p[6], Ci != Co ? p[8] : nullptr, false, nullptr, st);
  a.y = y; a.B = (int)B;
  return a;
}

struct Bwd {
  Args a;  // g_out: set per launch to g2 / dh
  BNBwdFinal bfin;
  const float *s1, *s2;
  float *g2, *dh, *wg1, *wg2, *wgp;
};
static Bwd bwd_args(int64_t Ci, int64_t Co, const float* dy, const float* x, const float* saved,
                    int64_t B, const float* const* q, float drop_p, const int64_t* seed_ptr,
                    uint64_t offset, float* dx, float* const* g, int64_t accumulate,
                    void* workspace, hipStream_t st) {
  const Ws L = ws_layout(B, Ci, Co);
  char* ws = (char*)workspace;
  auto at = [&](size_t off) { return (float*)(ws + off); };
  Bwd b = {};
  Args& a = b.a;
  b.s1 = saved + B * P * Co; b.s2 = saved + B * P * (Co + Ci);
  b.g2 = at(L.g2); b.dh = at(L.dh);
  b.wg1 = at(L.wg1); b.wg2 = at(L.wg2); b.wgp = at(L.wgp);
  a.x = x; a.h = saved; a.dy = dy; a.du_in = at(L.du);
  a.a1 = q[0]; a.a2 = q[4]; a.bn_w = q[2]; a.save = q[3];
  set_views(a, L, Ci, Co, q[1], q[5], Ci != Co ? q[6] : nullptr, true,
            at(L.pk) + L.n1 + L.n2 + L.np, st);
  a.du = at(L.du); a.dx = dx; a.slabda = at(L.slabda1);
  a.part = (double*)(ws + L.part);
  a.B = (int)B;
  set_dropout(a, drop_p, seed_ptr, offset);
  a.invN = 1.0f / (float)(B * P);
  a.coef = at(L.coef);
  // per-image partials -> the BN backward coefficients, BN weight / bias and Snake a2 gradients
  b.bfin = {(int)Co, (int)B, at(L.coef), g[3], g[4], g[5], (int)accumulate};
  return b;
}

// The block's two 3x3 weight gradients, conv2 (s2, g2) and conv1 (s1, dh): one launch when
// both have conv_wgrad_w8's shape, else the conv engine's
static int wgrad_3x3(const Bwd& b, int64_t Ci, int64_t Co, float* const* g, int64_t accumulate,
                     hipStream_t st) {
  const int64_t B = b.a.B;
  if (Ci == Co && conv_wgrad_w8_fits(W, B, Ci, Co)) {
    const float* const x[2] = {b.s2, b.s1};
    const float* const dy[2] = {b.g2, b.dh};
    float* const ws[2] = {b.wg2, b.wg1};
    float* const dw[2] = {g[6], g[1]};
    float* const db[2] = {g[7], g[2]};
    conv_wgrad_w8_multi(W, 2, x, dy, ws, dw, db, B, Ci, Co, (int)accumulate, st);
    return TVQ_OK;
  }
  const int rc = tvq_conv2d_wgrad(b.s2, B, Co, 3, W, b.g2, Co, W, 3, 3, 1, 0, g[6], g[7],
                                  accumulate, b.wg2, st);
  if (rc) return rc;
  return tvq_conv2d_wgrad(b.s1, B, Ci, 3, W, b.dh, Co, W, 3, 3, 1, 0, g[1], g[2], accumulate,
                          b.wg1, st);
}

// the Snake a1 gradient out of bwd1's slab rows
static void da1_finish(const Bwd& b, int64_t Ci, float* da1, int64_t accumulate, hipStream_t st) {
  conv_wgrad_finish(b.a.slabda, b.a.B, Ci, 1, da1, nullptr, (int)accumulate, st);
}

}  // namespace w8
}  // namespace tvq
