// The LF band's 64-channel ResBlock on (B, 64, 3, 8) maps (tvq_resblock_w8.hip), as called
// by the tvq_resblock_* entry points (tvq_resblock.hip) for that shape.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tvq {
bool w8_supported(int64_t B, int64_t C, int64_t H, int64_t W);
int64_t w8_workspace(int64_t B);
int64_t w8_saved_floats(int64_t B);
int w8_train_fwd(const float* x, int64_t B, const float* a1, const float* w1, const float* b1,
                 const float* bn_w, const float* bn_b, float* running_mean, float* running_var,
                 int64_t* nbt, float momentum, float eps, const float* a2, const float* w2,
                 const float* b2, float drop_p, const int64_t* seed_ptr, uint64_t offset,
                 float* saved, float* y, float* save, void* workspace, hipStream_t st);
int w8_eval_fwd(const float* x, int64_t B, const float* a1, const float* w1, const float* b1,
                const float* bn_w, const float* bn_b, const float* running_mean,
                const float* running_var, float eps, const float* a2, const float* w2,
                const float* b2, float* y, hipStream_t st);
int w8_bwd(const float* dy, const float* x, const float* saved, int64_t B, const float* a1,
           const float* w1, const float* bn_w, const float* save, const float* a2,
           const float* w2, float drop_p, const int64_t* seed_ptr, uint64_t offset, float* dx,
           float* da1, float* dw1, float* db1, float* dbn_w, float* dbn_b, float* da2, float* dw2,
           float* db2, int64_t accumulate, void* workspace, hipStream_t st);
// Two consecutive blocks: p = {a1, w1, b1, bn_w, bn_b, a2, w2, b2}, rs = {running_mean,
// running_var}, q = {a1, w1, bn_w, save, a2, w2}, g = {da1, dw1, db1, dbn_w, dbn_b, da2, dw2,
// db2}
int w8_pair_train_fwd(const float* x, int64_t B, const float* const* p1, const float* const* p2,
                      float* const* rs1, float* const* rs2, int64_t* nbt1, int64_t* nbt2,
                      float momentum, float eps, float drop_p, const int64_t* seed_ptr,
                      uint64_t off1, uint64_t off2, float* saved1, float* y1, float* save1,
                      float* saved2, float* y2, float* save2, void* ws1, void* ws2,
                      hipStream_t st);
int w8_pair_bwd(const float* dy, const float* x, int64_t B, const float* const* q1,
                const float* const* q2, const float* saved1, const float* y1,
                const float* saved2, float drop_p, const int64_t* seed_ptr, uint64_t off1,
                uint64_t off2, float* dx, float* dy1, float* const* g1, float* const* g2,
                int64_t accumulate, void* ws1, void* ws2, hipStream_t st);
}  // namespace tvq
