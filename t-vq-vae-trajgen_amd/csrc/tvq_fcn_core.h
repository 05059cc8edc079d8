// The FCN's stride-1 conv1d as an implicit GEMM on the matrix cores: one core for the eval
// forward (tvq_fcn.hip) and for the training forward and the data gradient
// (tvq_fcn_train.hip).
//
//   fcn_conv_kernel<K, PADL, EP, WY, WG>.  A block of 4 waves owns a (64 output channels x 128
//     positions) tile of one sample: wave (wco, wpos) holds two 32x32 accumulators of
//     v_mfma_f32_32x32x2_f32, rows = channels 32 wco.., columns = positions 64 wpos + 32 p...
//     The reduction runs over chunks of FC_CC = 8 input channels (Ci padded with zeros), inside
//     a chunk over the flat index r = ci K + k in steps of 2: lane half h supplies r = 2 s + h.
//       A (weights)  read from the packed form of fcn_pack_kernel, one coalesced dword per
//                    lane and step, straight into registers; the next chunk's are in flight
//                    while this chunk multiplies.
//       B (input)    the chunk's rows with their K-1 halo (PADL of it on the left), zeros
//                    outside [0, L), staged through two LDS buffers (next chunk's global loads
//                    in registers during the MFMAs; one barrier per chunk).  A half-wave reads
//                    32 consecutive floats: no bank conflict.
//     Every output is one k-ordered fmaf chain over r ascending, so it does not depend on
//     the batch or the grid.  Epilogues:
//       FC_EP_EVAL   relu(fma(scale, acc, shift)).  WY: y is stored.  WG: the block walks all
//                    position tiles of its sample (gridDim.y == 1); a lane adds its column's
//                    values tile after tile, then the 32 columns are added by a fixed xor tree
//                    and the two position halves through LDS: an order that depends on L only.
//                    aux = gap (float).
//       FC_EP_TRAIN  u = acc + scale[co] (`scale` is the conv bias) is stored in y, and the
//                    block writes the fp64 sums of u and u^2 of its 128 positions per channel:
//                    aux = part (double) [2][Co][B][tiles], a lane's two columns first, then
//                    the 32 columns by the xor tree, then the two position halves.
//                    gridDim.y == tiles.
//       FC_EP_PLAIN  acc is stored in y (the data gradient: x = du, wp = the flipped transpose).
#pragma once
#include "tvq_common.h"

namespace tvq {
namespace {

constexpr int FC_T = 256;             // threads per block: 2 (channels) x 2 (positions) waves
constexpr int FC_CC = 8;               // input channels per chunk
constexpr int FC_TL = 128;             // positions per block tile
constexpr int FC_ROW = FC_TL + 8;      // LDS row: tile + halo of up to 7
constexpr int FC_COT = 64;             // output channels per block
constexpr int FC_MAXK = 8;
constexpr int FC_EP_EVAL = 0, FC_EP_TRAIN = 1, FC_EP_PLAIN = 2;

template <int K, int PADL, int EP, bool WY, bool WG>
__global__ __launch_bounds__(FC_T, 2) void fcn_conv_kernel(
    const float* __restrict__ x, const float* __restrict__ wp, const float* __restrict__ scale,
    const float* __restrict__ shift, float* __restrict__ y, void* __restrict__ aux, int Ci, int L,
    int Co, int nch) {
  constexpr int S = FC_CC * K / 2;       // MFMA steps per chunk
  constexpr int SPAN = FC_TL + K - 1;    // staged positions per row
  constexpr int NST = (FC_CC * SPAN + FC_T - 1) / FC_T;
  __shared__ float xs[2][FC_CC * FC_ROW];
  __shared__ float red[2][FC_COT];
  float* __restrict__ gap = (float*)aux;

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int j = lane & 31, h = lane >> 5, wco = wid & 1, wpos = wid >> 1;
  const int64_t b = blockIdx.x;
  const int cot = blockIdx.z * 2 + wco;  // this wave's 32-channel tile
  const bool active = cot * 32 < Co;     // wave-uniform
  const int ntiles = (L + FC_TL - 1) / FC_TL;
  const float* xb = x + b * (int64_t)Ci * L;
  const float* wt = wp + (int64_t)cot * nch * S * 64 + lane;

  // staging map: element e = tid + FC_T i of the chunk's (FC_CC x SPAN) image
  int st_row[NST], st_t[NST];
#pragma unroll
  for (int i = 0; i < NST; ++i) {
    const int e = tid + FC_T * i;
    st_row[i] = e / SPAN;
    st_t[i] = e - st_row[i] * SPAN;
  }

  float gsum[16];
#pragma unroll
  for (int g = 0; g < 16; ++g) gsum[g] = 0.f;

  for (int tile = blockIdx.y; tile < ntiles; tile += gridDim.y) {
    const int l0 = tile * FC_TL;
    floatx16 acc0, acc1;
#pragma unroll
    for (int g = 0; g < 16; ++g) acc0[g] = acc1[g] = 0.f;

    float st[NST], a[S], an[S];
    auto stage_load = [&](int c) {
#pragma unroll
      for (int i = 0; i < NST; ++i) {
        const int ci = c * FC_CC + st_row[i], pos = l0 + st_t[i] - PADL;
        const bool ok = st_row[i] < FC_CC && ci < Ci && pos >= 0 && pos < L;
        st[i] = ok ? xb[(int64_t)ci * L + pos] : 0.f;
      }
    };
    auto stage_write = [&](int buf) {
#pragma unroll
      for (int i = 0; i < NST; ++i)
        if (st_row[i] < FC_CC) xs[buf][st_row[i] * FC_ROW + st_t[i]] = st[i];
    };

    stage_load(0);
    if (active) {
#pragma unroll
      for (int s = 0; s < S; ++s) a[s] = wt[s * 64];
    }
    stage_write(0);
    __syncthreads();

    for (int c = 0; c < nch; ++c) {
      const bool more = c + 1 < nch;
      if (more) {
        stage_load(c + 1);
        if (active) {
#pragma unroll
          for (int s = 0; s < S; ++s) an[s] = wt[((int64_t)(c + 1) * S + s) * 64];
        }
      }
      if (active) {
        const float* xr = xs[c & 1] + wpos * 64 + j;
#pragma unroll
        for (int s = 0; s < S; ++s) {
          const int o0 = ((2 * s) / K) * FC_ROW + (2 * s) % K;
          const int o1 = ((2 * s + 1) / K) * FC_ROW + (2 * s + 1) % K;
          const int off = h ? o1 : o0;
          const float b0 = xr[off], b1 = xr[off + 32];
          acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b0, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b1, acc1, 0, 0, 0);
        }
      }
      if (more) {
        stage_write((c + 1) & 1);
        if (active) {
#pragma unroll
          for (int s = 0; s < S; ++s) a[s] = an[s];
        }
      }
      __syncthreads();  // buffer (c+1)&1 is complete; buffer c&1 is free for chunk c+2
    }

    if constexpr (EP == FC_EP_EVAL) {
      if (active) {
        const int la = l0 + wpos * 64 + j, lb = la + 32;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
          const int co = cot * 32 + (g & 3) + 8 * (g >> 2) + 4 * h;
          const float sc = scale[co], sh = shift[co];
          const float va = fmaxf(fmaf(sc, acc0[g], sh), 0.f);
          const float vb = fmaxf(fmaf(sc, acc1[g], sh), 0.f);
          if (WY) {
            float* yr = y + (b * Co + co) * (int64_t)L;
            if (la < L) yr[la] = va;
            if (lb < L) yr[lb] = vb;
          }
          if (WG) {
            gsum[g] += la < L ? va : 0.f;
            gsum[g] += lb < L ? vb : 0.f;
          }
        }
      }
    } else {
      __shared__ double redd[2][2][FC_COT];  // [position half][sum, sum of squares][channel]
      if (active) {
        const int la = l0 + wpos * 64 + j, lb = la + 32;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
          const int cl = (g & 3) + 8 * (g >> 2) + 4 * h, co = cot * 32 + cl;
          const float bias = EP == FC_EP_TRAIN ? scale[co] : 0.f;
          const float ua = acc0[g] + bias, ub = acc1[g] + bias;
          float* yr = y + (b * Co + co) * (int64_t)L;
          if (la < L) yr[la] = ua;
          if (lb < L) yr[lb] = ub;
          if constexpr (EP == FC_EP_TRAIN) {
            const double da = la < L ? (double)ua : 0.0, db = lb < L ? (double)ub : 0.0;
            double s1 = da + db, s2 = da * da + db * db;
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) {
              s1 += __shfl_xor(s1, o, 64);
              s2 += __shfl_xor(s2, o, 64);
            }
            if (j == 0) {
              redd[wpos][0][wco * 32 + cl] = s1;
              redd[wpos][1][wco * 32 + cl] = s2;
            }
          }
        }
      }
      if constexpr (EP == FC_EP_TRAIN) {
        __syncthreads();
        const int q = tid >> 6, cl = tid & 63, co = blockIdx.z * FC_COT + cl;
        if (q < 2 && co < Co) {
          double* part = (double*)aux;
          part[(((int64_t)q * Co + co) * gridDim.x + b) * ntiles + tile] =
              redd[0][q][cl] + redd[1][q][cl];
        }
        __syncthreads();
      }
    }
  }

  if (WG) {
    if (active) {
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        float v = gsum[g];
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);  // the 32 columns of a half
        if (j == 0) red[wpos][wco * 32 + (g & 3) + 8 * (g >> 2) + 4 * h] = v;
      }
    }
    __syncthreads();
    const int co = blockIdx.z * FC_COT + tid;
    if (tid < FC_COT && co < Co) gap[b * Co + co] = (red[0][tid] + red[1][tid]) / (float)L;
  }
}

}  // namespace
}  // namespace tvq
