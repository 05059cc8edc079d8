// Internal (non-ABI) entry points of the conv engine used by other kernel files.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tvq {
// A weight's (n, c, tap) view (element w[n*wsn + c*wsc + tap]) packed [tap][c][n] from the
// open pack-cache scope, else into ws (N*C*KK floats), else unpacked when ws is null; the
// returned pointer's strides (n, c, tap) go to *sn, *sc, *st.
const float* conv_pack_view(const float* w, int N, int C, int KK, int64_t wsn, int64_t wsc,
                            float* ws, hipStream_t st, int64_t* sn, int64_t* sc, int64_t* stp);
// n <= 4 weight (+ bias) gradients of 3x3 stride-1 zero-padded C -> N convs of one shape on
// (B, C, 3, W) maps, W = 8 or 16, in one conv_wgrad_w8_kernel launch (the fused ResBlocks'
// conv1 / conv2, tvq_resblock_w8.hip / tvq_resblock.hip): problem i reduces dy[i] against x[i]
// into ws[i] (conv_wgrad_w8_slab_floats floats, alive until the deferral scope's flush), summed
// in order into dw[i] / db[i] -- bit for bit the sums of one launch per problem.  Call only
// where conv_wgrad_w8_fits.
bool conv_wgrad_w8_fits(int W, int64_t B, int64_t C, int64_t N);
int64_t conv_wgrad_w8_slab_floats(int W, int64_t B, int64_t C, int64_t N);
void conv_wgrad_w8_multi(int W, int n, const float* const* x, const float* const* dy,
                         float* const* ws, float* const* dw, float* const* db, int64_t B,
                         int64_t C, int64_t N, int accumulate, hipStream_t st);
}  // namespace tvq
