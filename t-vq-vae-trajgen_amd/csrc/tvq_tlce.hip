// The priors' training loss head on the masked tokens only: tied logits, cross-entropy and its
// gradient with respect to the logits and to the head output
// (bidirectional_transformer.py:186-191 logits = h tok_emb[:K]^T + bias[pos]; maskgit.py:183-191
// loss = F.cross_entropy(logits[~keep], target[~keep])), for the backward pass that starts
// right at this loss (MaskGIT.forward_backward: the root gradient `gscale`, a device scalar,
// is known in the forward).  The loss reads only the masked tokens (about 37 % of them under
// the cosine schedule), so tvq_masked_rows first lists them: rows[r] = token id m = b n + pos,
// ordered by position, then by sample; pos_off[pos] = first list index of position pos,
// pos_off[n] = cnt.  Per listed token m = rows[r]:
//   l = h_m W^T + b_{m mod n}      lse = log sum_k exp(l_k)      loss_m = lse - l_target
//   D_r = (softmax(l) - onehot(target)) * gscale / cnt
//   dh_m = D_r W        Hc_r = h_m
// The logits never reach memory.  D and Hc are compact (row r; rows at or beyond cnt are never
// written or read): the tied-table gradient D^T Hc and the per-position bias gradient (the
// column sums of D over [pos_off[pos], pos_off[pos + 1])) run over cnt rows
// (tvq_tied_ce_grads).  dh is dense: zero-filled, then the masked rows are scattered into it.
// cnt stays on the device: the grid is the worst case ceil(M / 16) and a block whose first
// row is at or beyond cnt returns at once, so one captured graph serves every mask.
//
// Layout: one block per 16 listed tokens on v_mfma_f32_16x16x4_f32; its 4 waves split the K
// codes (wave w: the NT / 4 16-code tiles from tile w NT / 4).  Lane l = (i = l & 15, g = l >> 4).
//   logits tile c (16 codes): rows = codes, cols = tokens; k-slot g of step (q, e) is feature
//     16 q + 4 g + e, so a lane's B operands are h[token i][16 q + 4 g ..+3] (8 float4 loads)
//     and its A operands W[16 c + i][16 q + 4 g ..+3] (8 16-byte LDS reads); the lane ends
//     with codes 16 c + 4 g + r (r = 0..3: one float4 of D per tile) of token i.
//   softmax over the 4 waves: row maxima through LDS, then every wave sums expf(l - mx) with
//     the row's global max; the four sums (and the target logit) add in wave order 0+1+2+3.
//   dh: rows = features (8 tiles of 16; row i of tile ft = feature 64 (ft >> 2) + 4 i +
//     (ft & 3)), cols = tokens; step (c, r) takes k-slot g = code 16 c + 4 g + r, i.e. the
//     lane's own D register r of tile c as the B operand and A = W[that code][feature]: two
//     float4 loads per (c, r) feed the 8 feature tiles (a quarter-wave reads 256 contiguous
//     bytes).  Each wave's partial dh (its codes) goes to LDS; the four add in wave order.
// Every W element is read from L2 once per block and sweep, one tile ahead of its use, and no
// wave shares a W element with another: there is no block barrier inside a sweep.  The dh
// sweep loads its operands straight into registers.  The logits sweep's operands lie in one
// table row per lane, so its tiles are loaded as whole rows and turned through a wave-private
// LDS area (measured against direct row-strided loads: HF 41.9 vs 48.1 us, LF 19.2 vs 20.7 us);
// the same area then carries the wave's partial dh.
#include <math.h>

#include "tvq_gemm.h"

namespace tvq {

constexpr int TLCE_D = 128;

struct TlceArgs {
  const float* h;       // (M, 128)
  const float* W;       // (>= K, 128) tied table
  const float* bias;    // (n, ldb)
  int64_t ldb;
  const int64_t* target;
  const int* rows;      // masked token ids (tvq_masked_rows)
  const int* pos_off;   // (n + 1); pos_off[n] = cnt
  const float* gscale;
  float* D;             // (M, K), rows < cnt written
  float* Hc;            // (M, 128), rows < cnt written
  float* dh;            // (M, 128), zero-filled before the launch
  float* part;          // per-block loss sums (blocks < ceil(cnt / 16))
  int n;
};

// Block `pos` (of n + 1) counts the masked tokens at positions < pos (pos_off[pos]; block n:
// cnt) and its wave 0 lists position pos's masked tokens in sample order.  Integers only.
__global__ __launch_bounds__(1024) void masked_rows_kernel(const bool* __restrict__ keep, int B,
                                                           int n, int* __restrict__ rows,
                                                           int* __restrict__ pos_off) {
  __shared__ int red[16];
  const int pos = (int)blockIdx.x, M = B * n;
  int c = 0;
  for (int m = threadIdx.x; m < M; m += 1024) c += (!keep[m] && m % n < pos) ? 1 : 0;
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x >= 64) return;
  int base = 0;
  for (int w = 0; w < 16; ++w) base += red[w];
  if (threadIdx.x == 0) pos_off[pos] = base;
  if (pos == n) return;
  const int lane = threadIdx.x;
  for (int b0 = 0; b0 < B; b0 += 64) {
    const int b = b0 + lane;
    const bool masked = b < B && !keep[b * n + pos];
    const unsigned long long bal = __ballot(masked);
    if (masked) rows[base + __popcll(bal & ((1ull << lane) - 1ull))] = b * n + pos;
    base += __popcll(bal);
  }
}

// Row stride (floats) of a wave's LDS area: 16 rows of 128.  136 = 8 mod 64 keeps the logits
// sweep's 16-byte reads (row i, column 16 q + 4 g) on distinct banks in every 16-lane group.
constexpr int TLCE_RS = 136;

// one 16-code tile in flight = 512 float4, 8 per lane: load u is table rows 2 u and 2 u + 1 of
// the tile, 512 contiguous bytes per half-wave (named registers of the native vector type:
// neither an array to index nor a struct copy, which would go through private memory)
struct TlceStage {
  floatx4 r0, r1, r2, r3, r4, r5, r6, r7;
};
__device__ __forceinline__ void tlce_tile_load(const float* __restrict__ p, TlceStage& r) {
  r.r0 = *reinterpret_cast<const floatx4*>(p);
  r.r1 = *reinterpret_cast<const floatx4*>(p + 2 * TLCE_D);
  r.r2 = *reinterpret_cast<const floatx4*>(p + 4 * TLCE_D);
  r.r3 = *reinterpret_cast<const floatx4*>(p + 6 * TLCE_D);
  r.r4 = *reinterpret_cast<const floatx4*>(p + 8 * TLCE_D);
  r.r5 = *reinterpret_cast<const floatx4*>(p + 10 * TLCE_D);
  r.r6 = *reinterpret_cast<const floatx4*>(p + 12 * TLCE_D);
  r.r7 = *reinterpret_cast<const floatx4*>(p + 14 * TLCE_D);
}
__device__ __forceinline__ void tlce_tile_store(float* p, const TlceStage& r) {
  *reinterpret_cast<floatx4*>(p) = r.r0;
  *reinterpret_cast<floatx4*>(p + 2 * TLCE_RS) = r.r1;
  *reinterpret_cast<floatx4*>(p + 4 * TLCE_RS) = r.r2;
  *reinterpret_cast<floatx4*>(p + 6 * TLCE_RS) = r.r3;
  *reinterpret_cast<floatx4*>(p + 8 * TLCE_RS) = r.r4;
  *reinterpret_cast<floatx4*>(p + 10 * TLCE_RS) = r.r5;
  *reinterpret_cast<floatx4*>(p + 12 * TLCE_RS) = r.r6;
  *reinterpret_cast<floatx4*>(p + 14 * TLCE_RS) = r.r7;
}

template <int NT>
__global__ __launch_bounds__(256, 2) void tlce_kernel(TlceArgs a) {
  constexpr int NTW = NT / 4, K = NT * 16;
  const int cnt = a.pos_off[a.n];
  const int r0 = (int)blockIdx.x * 16;
  if (r0 >= cnt) return;  // before any barrier
  __shared__ float xs[3][4][16];            // row max | exp sum | target logit, per wave
  // per wave 16 x TLCE_RS floats: its W tile during the logits sweep, then its partial dh tile
  __shared__ __attribute__((aligned(16))) float ds[4 * 16 * TLCE_RS];
  const int lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4, w = threadIdx.x >> 6;
  // a ragged last group computes its missing rows on the last listed row and stores nothing
  const bool ok = r0 + i < cnt;
  const int r = ok ? r0 + i : cnt - 1;
  const int64_t m = a.rows[r];
  // B operands of the logits: h[m][16 q + 4 g + e]
  float xb[32];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const float4 v = *reinterpret_cast<const float4*>(a.h + m * TLCE_D + 16 * q + 4 * g);
    xb[4 * q] = v.x;
    xb[4 * q + 1] = v.y;
    xb[4 * q + 2] = v.z;
    xb[4 * q + 3] = v.w;
  }
  // the compact copy of h: wave w writes its quarter of the row (after every load of h: the
  // compiler cannot tell Hc from h, and would wait for each load before the next store)
  if (ok) {
    float* hc = a.Hc + (int64_t)r * TLCE_D + 32 * w + 4 * g;
#pragma unroll
    for (int q = 0; q < 8; ++q)
      if ((q >> 1) == w)
        *reinterpret_cast<float4*>(hc + 16 * (q & 1)) =
            make_float4(xb[4 * q], xb[4 * q + 1], xb[4 * q + 2], xb[4 * q + 3]);
  }
  const int c0 = w * NTW;  // this wave's first 16-code tile
  const float* brow = a.bias + (m % a.n) * a.ldb + 16 * c0 + 4 * g;
  // ---- logits sweep: the wave's NTW tiles in registers.  A lane's A operands lie in one table
  // row per lane (512 bytes apart), so each 16 x 128 tile is loaded as whole rows (2 rows per
  // load instruction) and turned through the wave's own LDS area; tile c + 1 is in flight in
  // registers while tile c computes.  The area is wave-private: no block barrier.
  floatx4 L[NTW];
  float* wt = ds + w * 16 * TLCE_RS;
  const float* wg = a.W + (int64_t)(16 * c0 + (lane >> 5)) * TLCE_D + 4 * (lane & 31);
  float* wst = wt + (lane >> 5) * TLCE_RS + 4 * (lane & 31);
  const float* wrd = wt + i * TLCE_RS + 4 * g;
  TlceStage st;
  tlce_tile_load(wg, st);
#pragma unroll
  for (int c = 0; c < NTW; ++c) {
    // tile c into the area (the wave's reads of tile c - 1 were issued before: LDS keeps a
    // wave's operations in order), then tile c + 1 loads while tile c computes
    __builtin_amdgcn_wave_barrier();
    tlce_tile_store(wst, st);
    __builtin_amdgcn_wave_barrier();
    if (c + 1 < NTW) tlce_tile_load(wg + (c + 1) * 16 * TLCE_D, st);
    // keep the whole next tile in flight behind this tile's MFMAs (the scheduler otherwise
    // sinks each load to just before its use)
    __builtin_amdgcn_sched_barrier(0);
    const float b0 = brow[16 * c], b1 = brow[16 * c + 1], b2 = brow[16 * c + 2],
                b3 = brow[16 * c + 3];  // bias rows are K + 1 long: not 16-byte aligned
    floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const float4 v = *reinterpret_cast<const float4*>(wrd + 16 * q);
      acc = mfma16x16x4(v.x, xb[4 * q], acc);
      acc = mfma16x16x4(v.y, xb[4 * q + 1], acc);
      acc = mfma16x16x4(v.z, xb[4 * q + 2], acc);
      acc = mfma16x16x4(v.w, xb[4 * q + 3], acc);
    }
    L[c][0] = acc[0] + b0;
    L[c][1] = acc[1] + b1;
    L[c][2] = acc[2] + b2;
    L[c][3] = acc[3] + b3;
  }
  // the dh sweep's first tile, loading while the softmax runs:
  // wd[r][hh] = W[16 (c0 + c) + 4 g + r][64 hh + 4 i ..+3]
  const float* wdp = a.W + (int64_t)(16 * c0 + 4 * g) * TLCE_D + 4 * i;
  float4 wd[2][4][2];
#pragma unroll
  for (int rr = 0; rr < 4; ++rr)
#pragma unroll
    for (int hh = 0; hh < 2; ++hh)
      wd[0][rr][hh] = *reinterpret_cast<const float4*>(wdp + rr * TLCE_D + 64 * hh);
  __builtin_amdgcn_sched_barrier(0);
  // ---- softmax statistics of token i: the wave's codes over the 4 lane groups (xor 16, xor
  // 32), then the 4 waves through LDS
  float mx = -INFINITY;
#pragma unroll
  for (int c = 0; c < NTW; ++c)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) mx = fmaxf(mx, L[c][rr]);
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  if (g == 0) xs[0][w][i] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(xs[0][0][i], xs[0][1][i]), fmaxf(xs[0][2][i], xs[0][3][i]));
  const int tgt = (int)a.target[m];
  float se = 0.f, lt = 0.f;
#pragma unroll
  for (int c = 0; c < NTW; ++c)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      se += expf(L[c][rr] - mx);
      lt += (16 * (c0 + c) + 4 * g + rr == tgt) ? L[c][rr] : 0.f;
    }
  se += __shfl_xor(se, 16, 64);
  se += __shfl_xor(se, 32, 64);
  lt += __shfl_xor(lt, 16, 64);
  lt += __shfl_xor(lt, 32, 64);
  if (g == 0) {
    xs[1][w][i] = se;
    xs[2][w][i] = lt;
  }
  __syncthreads();
  se = ((xs[1][0][i] + xs[1][1][i]) + xs[1][2][i]) + xs[1][3][i];
  lt = ((xs[2][0][i] + xs[2][1][i]) + xs[2][2][i]) + xs[2][3][i];
  const float lse = mx + logf(se);
  const float sc = a.gscale[0] / (float)cnt;
  // ---- D = (softmax - onehot) * gscale / cnt, one float4 per tile at compact row r
  float* drow = a.D + (int64_t)r * K + 16 * c0 + 4 * g;
#pragma unroll
  for (int c = 0; c < NTW; ++c) {
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const float p = expf(L[c][rr] - lse);
      L[c][rr] = (p - ((16 * (c0 + c) + 4 * g + rr == tgt) ? 1.0f : 0.0f)) * sc;
    }
    if (ok) *reinterpret_cast<float4*>(drow + 16 * c) = make_float4(L[c][0], L[c][1], L[c][2], L[c][3]);
  }
  // ---- dh sweep over the wave's codes: dh^T = W^T D^T; B = D register r of tile c
  floatx4 dacc[8];
#pragma unroll
  for (int ft = 0; ft < 8; ++ft) dacc[ft] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < NTW; ++c) {
    if (c + 1 < NTW) {
#pragma unroll
      for (int rr = 0; rr < 4; ++rr)
#pragma unroll
        for (int hh = 0; hh < 2; ++hh)
          wd[(c + 1) & 1][rr][hh] =
              *reinterpret_cast<const float4*>(wdp + ((c + 1) * 16 + rr) * TLCE_D + 64 * hh);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const float4 v = wd[c & 1][rr][hh];
        dacc[4 * hh] = mfma16x16x4(v.x, L[c][rr], dacc[4 * hh]);
        dacc[4 * hh + 1] = mfma16x16x4(v.y, L[c][rr], dacc[4 * hh + 1]);
        dacc[4 * hh + 2] = mfma16x16x4(v.z, L[c][rr], dacc[4 * hh + 2]);
        dacc[4 * hh + 3] = mfma16x16x4(v.w, L[c][rr], dacc[4 * hh + 3]);
      }
  }
  // the lane holds features 64 hh + 16 g + 4 rr + e (= dacc[4 hh + e][rr]) of token i
  float* dsw = ds + (w * 16 + i) * TLCE_RS + 16 * g;
#pragma unroll
  for (int hh = 0; hh < 2; ++hh)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
      *reinterpret_cast<float4*>(dsw + 64 * hh + 4 * rr) = make_float4(
          dacc[4 * hh][rr], dacc[4 * hh + 1][rr], dacc[4 * hh + 2][rr], dacc[4 * hh + 3][rr]);
  __syncthreads();
  {
    // thread t: token t >> 4, features 8 (t & 15) ..+7; wave partials in the order 0+1+2+3
    const int tk = threadIdx.x >> 4, f0 = 8 * (threadIdx.x & 15);
    if (r0 + tk < cnt) {
      float* hrow = a.dh + (int64_t)a.rows[r0 + tk] * TLCE_D + f0;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const float* p = ds + tk * TLCE_RS + f0 + 4 * u;
        const float4 p0 = *reinterpret_cast<const float4*>(p);
        const float4 p1 = *reinterpret_cast<const float4*>(p + 16 * TLCE_RS);
        const float4 p2 = *reinterpret_cast<const float4*>(p + 32 * TLCE_RS);
        const float4 p3 = *reinterpret_cast<const float4*>(p + 48 * TLCE_RS);
        *reinterpret_cast<float4*>(hrow + 4 * u) =
            make_float4(((p0.x + p1.x) + p2.x) + p3.x, ((p0.y + p1.y) + p2.y) + p3.y,
                        ((p0.z + p1.z) + p2.z) + p3.z, ((p0.w + p1.w) + p2.w) + p3.w);
      }
    }
  }
  // ---- the block's loss sum over its listed tokens (wave 0, lane group 0: one copy per token)
  if (w != 0) return;
  float ls = (ok && g == 0) ? lse - lt : 0.f;
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) ls += __shfl_xor(ls, o, 64);
  if (lane == 0) a.part[blockIdx.x] = ls;
}

// loss = sum of the block partials (fixed order) / cnt; out = {loss, cnt}
__global__ __launch_bounds__(256) void tlce_final_kernel(const float* __restrict__ part,
                                                         const int* __restrict__ pos_off, int n,
                                                         float* __restrict__ out) {
  __shared__ float red[4];
  const int cnt = pos_off[n], P = (cnt + 15) / 16;
  float s = 0.f;
  for (int i = threadIdx.x; i < P; i += 256) s += part[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) {
    out[0] = s / (float)cnt;
    out[1] = (float)cnt;
  }
}

// out[pos * ldo + d] (+)= sum of Dc[r][d] over r in [pos_off[pos], pos_off[pos + 1]): the
// bias gradient on the compact rows.  Block = 32 columns x 8 row parts as in
// batch_colsum8_kernel: part q sums its rows in order, the 8 partials add in part order.
__global__ __launch_bounds__(256) void seg_colsum8_kernel(const float* __restrict__ Dc,
                                                          const int* __restrict__ pos_off, int n,
                                                          int K, float* __restrict__ out,
                                                          int64_t ldo, int accumulate) {
  __shared__ float part[8][32];
  const int c = threadIdx.x & 31, q = threadIdx.x >> 5;
  const int e = (int)blockIdx.x * 32 + c;  // K is a multiple of 32: one position per block
  const int j = e / K, d = e - j * K;
  const int s0 = pos_off[j], s1 = pos_off[j + 1];
  const int per = (s1 - s0 + 7) / 8;
  const int b0 = s0 + q * per, b1 = min(s1, b0 + per);
  const float* p = Dc + d;
  float s = 0.f;
#pragma unroll 8
  for (int b = b0; b < b1; ++b) s += p[(int64_t)b * K];
  part[q][c] = s;
  __syncthreads();
  if (q != 0) return;
  float t = part[0][c];
#pragma unroll
  for (int k = 1; k < 8; ++k) t += part[k][c];
  float* o = out + j * ldo + d;
  *o = accumulate ? *o + t : t;
}

}  // namespace tvq

using namespace tvq;

static bool tlce_nt_ok(int64_t K) { return K == 64 || K == 128 || K == 256 || K == 512; }

extern "C" int tvq_masked_rows(const bool* keep, int64_t B, int64_t n, int32_t* rows,
                               int32_t* pos_off, tvq_stream_t stream) {
  TVQ_CHECK_ARG(keep && rows && pos_off && B > 0 && n > 0 && B * n < (int64_t)1 << 31,
                "tvq_masked_rows: bad arguments (B n < 2^31)");
  hipLaunchKernelGGL(masked_rows_kernel, dim3((unsigned)(n + 1)), dim3(1024), 0,
                     (hipStream_t)stream, keep, (int)B, (int)n, rows, pos_off);
  return launch_status("tvq_masked_rows");
}

extern "C" int64_t tvq_tied_logits_ce_workspace(int64_t M, int64_t K) {
  if (M < 1 || !tlce_nt_ok(K)) return -1;
  return (M + 15) / 16;  // block partials of the loss
}

extern "C" int tvq_tied_logits_ce(const float* h, int64_t M, int64_t D, const float* W, int64_t K,
                                  const float* bias, int64_t n, int64_t ldb, const int64_t* target,
                                  const int32_t* rows, const int32_t* pos_off, const float* gscale,
                                  float* dlogits, float* hc, float* dh, float* out,
                                  float* workspace, tvq_stream_t stream) {
  TVQ_CHECK_ARG(h && W && bias && target && rows && pos_off && gscale && dlogits && hc && dh &&
                    out && workspace && M > 0 && M < (int64_t)1 << 31 && n > 0 && ldb >= K &&
                    D == TLCE_D && tlce_nt_ok(K),
                "tvq_tied_logits_ce: bad arguments (D 128, K in {64, 128, 256, 512})");
  TVQ_CHECK_ARG(((uintptr_t)h & 15) == 0 && ((uintptr_t)W & 15) == 0 &&
                    ((uintptr_t)dlogits & 15) == 0 && ((uintptr_t)dh & 15) == 0 &&
                    ((uintptr_t)hc & 15) == 0,
                "tvq_tied_logits_ce: pointers must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  // the kept tokens' dh rows are zero; the kernel writes the listed rows only
  if (hipMemsetAsync(dh, 0, (size_t)M * TLCE_D * sizeof(float), st) != hipSuccess)
    return launch_status("tvq_tied_logits_ce(fill)");
  TlceArgs a;
  a.h = h; a.W = W; a.bias = bias; a.ldb = ldb; a.target = target; a.rows = rows;
  a.pos_off = pos_off; a.gscale = gscale; a.D = dlogits; a.Hc = hc; a.dh = dh;
  a.part = workspace; a.n = (int)n;
  const dim3 grid((unsigned)((M + 15) / 16));  // the worst case: every token masked
  TVQ_PLAN("tied_logits_ce M=%lld K=%lld", (long long)M, (long long)K);
  if (K == 512) hipLaunchKernelGGL(tlce_kernel<32>, grid, dim3(256), 0, st, a);
  else if (K == 256) hipLaunchKernelGGL(tlce_kernel<16>, grid, dim3(256), 0, st, a);
  else if (K == 128) hipLaunchKernelGGL(tlce_kernel<8>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(tlce_kernel<4>, grid, dim3(256), 0, st, a);
  hipLaunchKernelGGL(tlce_final_kernel, dim3(1), dim3(256), 0, st, workspace, pos_off, (int)n, out);
  return launch_status("tvq_tied_logits_ce");
}

extern "C" int64_t tvq_tied_ce_grads_workspace(int64_t M, int64_t K) {
  if (M < 1 || !tlce_nt_ok(K)) return -1;
  const int s = gemm_direct_splits(K, TLCE_D, M);
  return s > 1 ? (int64_t)s * K * TLCE_D : 0;
}

extern "C" int tvq_tied_ce_grads(const float* dlogits, const float* hc, const int32_t* pos_off,
                                 int64_t M, int64_t K, int64_t n, float* dW, int64_t dw_accumulate,
                                 float* dbias, int64_t ldb, int64_t db_accumulate,
                                 float* workspace, tvq_stream_t stream) {
  TVQ_CHECK_ARG(dlogits && hc && pos_off && M > 0 && M < (int64_t)1 << 31 && n > 0 &&
                    tlce_nt_ok(K) && (!dbias || ldb >= K),
                "tvq_tied_ce_grads: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  if (dW) {  // dW[:K] (+)= Dc^T Hc over the first cnt rows
    GemmArgs g;
    g.A = dlogits; g.B = hc; g.C = dW;
    g.M = (int)K; g.N = TLCE_D; g.K = (int)M;
    g.sam = 1; g.sak = K; g.sbk = TLCE_D; g.sbn = 1; g.ldc = TLCE_D;
    g.bias = nullptr; g.R = nullptr; g.ldr = 0; g.rmod = 0; g.pre = nullptr;
    g.act = 0; g.accumulate = (int)dw_accumulate; g.gate = nullptr;
    g.alpha = 1.0f;
    g.kper = (int)M;
    g.cnt = nullptr;
    g.slab = nullptr;
    g.kdev = pos_off + n;
    TVQ_CHECK_ARG(workspace || gemm_direct_splits(K, TLCE_D, M) <= 1,
                  "tvq_tied_ce_grads: workspace missing");
    if (!gemm_direct(g, workspace, st)) {
      set_error("tvq_tied_ce_grads: no kernel for the tied-table gradient");
      return TVQ_ERR_ARG;
    }
  }
  if (dbias)
    hipLaunchKernelGGL(seg_colsum8_kernel, dim3((unsigned)(n * K / 32)), dim3(256), 0, st, dlogits,
                       pos_off, (int)n, (int)K, dbias, ldb, (int)db_accumulate);
  return launch_status("tvq_tied_ce_grads");
}

__global__ void scalar_ratio_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                    float* __restrict__ out) {
  if (threadIdx.x == 0) out[0] = a[0] / b[0];
}

// out[0] = a[0] / b[0] (device scalars; _TiedLogitsCE's root-gradient rescale)
extern "C" int tvq_scalar_ratio(const float* a, const float* b, float* out, tvq_stream_t stream) {
  TVQ_CHECK_ARG(a && b && out, "tvq_scalar_ratio: null argument");
  hipLaunchKernelGGL(scalar_ratio_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a, b, out);
  return launch_status("tvq_scalar_ratio");
}
