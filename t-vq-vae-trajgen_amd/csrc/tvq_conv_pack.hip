// Weight packing for the conv engine and the per-step pack cache (tvq_conv_packcache_*).
#include "tvq_conv_core.h"
#include "tvq_conv_internal.h"

#include <map>
#include <vector>

namespace tvq {

// Repack a weight seen as (n, c, tap) with strides (wsn, wsc, 1) into [tap][c][n] so the
// A-operand loads of a K-step read TN consecutive floats (one or two cache lines) instead
// of TN rows a whole filter apart.
__global__ void conv_pack_weight_kernel(const float* __restrict__ w, int N, int C, int KK,
                                        int64_t wsn, int64_t wsc, float* __restrict__ out) {
  const int64_t total = (int64_t)N * C * KK;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int n = (int)(i % N);
    const int64_t r = i / N;
    const int c = (int)(r % C);
    const int tap = (int)(r / C);
    out[i] = w[n * wsn + c * wsc + tap];
  }
}

// Per-step weight-pack cache (tvq_conv_packcache_*).  Inside a scope, the first time a
// (weight, view) is packed it gets a slot in the caller's arena and is recorded; at the
// next scope's begin every recorded entry is repacked from the current weights by a few
// batched launches, and the convs of the scope read their slot without packing again.
// The scope must not contain weight updates (a trainer opens it around forward+backward,
// the optimizer step is outside).  Entries belong to one cache id (one arena); several ids
// keep their entries side by side, so two step segments captured as separate graphs (the
// DP trainer's stage1 and stage2) each repack only their own weights.  An id's entries are
// dropped by tvq_conv_packcache_release (its owner is freed) or when the id begins with
// another arena.
struct PackEntry {
  const float* src;
  int N, C, KK;
  int64_t wsn, wsc, off;
};
struct PackCacheState {
  std::vector<PackEntry> entries;
  float* arena = nullptr;
  int64_t cap = 0, used = 0;
};
static std::map<int64_t, PackCacheState> g_pcs;
static PackCacheState* g_pc_cur = nullptr;  // the open scope's cache (null: no scope)
static int64_t g_pc_last = -1;              // id of the last scope (entries query)

// one launch repacks a whole step's weights (a stage1 + stage2 step records ~70): 36 bytes
// per entry keep PACK_BATCH of them inside a 4 KB kernel-argument block
constexpr int PACK_BATCH = 96;
struct PackBatch {
  const float* src[PACK_BATCH];
  int64_t off[PACK_BATCH];
  int wsn[PACK_BATCH], wsc[PACK_BATCH];
  int N[PACK_BATCH], C[PACK_BATCH], KK[PACK_BATCH];
};
static_assert(sizeof(PackBatch) <= 3900, "pack batch kernel arguments");

// blockIdx.y = entry; blocks stride over the entry's N*C*KK elements ([tap][c][n] order)
__global__ void conv_pack_multi_kernel(PackBatch b, float* __restrict__ arena) {
  const int j = blockIdx.y;
  const int N = b.N[j], C = b.C[j];
  const int64_t total = (int64_t)N * C * b.KK[j];
  const float* w = b.src[j];
  float* out = arena + b.off[j];
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int n = (int)(i % N);
    const int64_t r = i / N;
    const int c = (int)(r % C);
    const int tap = (int)(r / C);
    out[i] = w[(int64_t)n * b.wsn[j] + (int64_t)c * b.wsc[j] + tap];
  }
}

static void pack_launch(const float* wt, int N, int C, int KK, int64_t wsn, int64_t wsc,
                        float* dst, hipStream_t st) {
  const int64_t total = (int64_t)N * C * KK;
  const int blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
  hipLaunchKernelGGL(conv_pack_weight_kernel, dim3(blocks), dim3(256), 0, st, wt, N, C, KK, wsn,
                     wsc, dst);
}

// The open scope's arena slot of (src, view), or null (no open scope, or a new entry and the
// arena is full).  *packed: the entry was recorded before, so this scope's begin repacked it;
// a new entry is recorded here and the caller packs it now.
static float* lookup_or_insert(const float* src, int N, int C, int KK, int64_t wsn, int64_t wsc,
                               bool* packed) {
  *packed = false;
  PackCacheState* pc = g_pc_cur;
  if (!pc) return nullptr;
  for (const PackEntry& p : pc->entries)
    if (p.src == src && p.N == N && p.C == C && p.KK == KK && p.wsn == wsn && p.wsc == wsc) {
      *packed = true;
      return pc->arena + p.off;
    }
  const int64_t slot = ((int64_t)N * C * KK + 63) / 64 * 64;
  if (pc->used + slot > pc->cap) return nullptr;
  pc->entries.push_back({src, N, C, KK, wsn, wsc, pc->used});
  pc->used += slot;
  return pc->arena + pc->used - slot;
}

// A (weight, view) packed [tap][c][n] for a kernel outside the conv engine (the fused LF
// ResBlock): from the open pack-cache scope (recorded and repacked at each scope's begin like
// the engine's own), else packed into `ws`, else (no slot, no ws) the unpacked weight.
// Returns the pointer and the view's strides (n, c, tap) in *sn / *sc / *st.
const float* conv_pack_view(const float* w, int N, int C, int KK, int64_t wsn, int64_t wsc,
                            float* ws, hipStream_t st, int64_t* sn, int64_t* sc, int64_t* stp) {
  bool packed;
  float* slot = lookup_or_insert(w, N, C, KK, wsn, wsc, &packed);
  float* dst = slot ? slot : ws;
  if (!dst) {
    *sn = wsn; *sc = wsc; *stp = 1;
    return w;
  }
  if (!packed) pack_launch(w, N, C, KK, wsn, wsc, dst, st);
  *sn = 1; *sc = N; *stp = (int64_t)N * C;
  return dst;
}

// Pack `wt` into `ws` (N*C*KK floats) when given -- or serve it from the open pack cache --
// and retarget the geometry's weight strides; a null `ws` leaves the weight unpacked and the
// cache untouched.
const float* pack_weight(const float* wt, ConvGeom& g, int KK, float* ws, hipStream_t st) {
  if (!ws) return wt;
  return conv_pack_view(wt, g.N, g.C, KK, g.wsn, g.wsc, ws, st, &g.wsn, &g.wsc, &g.wst);
}

}  // namespace tvq

using namespace tvq;

extern "C" int tvq_conv_packcache_begin(int64_t id, float* arena, int64_t cap_floats,
                                        tvq_stream_t stream) {
  TVQ_CHECK_ARG(id >= 0 && arena && cap_floats > 0, "tvq_conv_packcache_begin: bad arguments");
  TVQ_CHECK_ARG(!g_pc_cur, "tvq_conv_packcache_begin: a scope is already open");
  PackCacheState& pc = g_pcs[id];
  if (arena != pc.arena || cap_floats != pc.cap) {
    pc.entries.clear();
    pc.arena = arena;
    pc.cap = cap_floats;
    pc.used = 0;
  }
  hipStream_t st = (hipStream_t)stream;
  for (size_t i0 = 0; i0 < pc.entries.size(); i0 += PACK_BATCH) {
    PackBatch b;
    int n = 0;
    int64_t most = 0;
    for (size_t i = i0; i < pc.entries.size() && n < PACK_BATCH; ++i, ++n) {
      const PackEntry& p = pc.entries[i];
      b.src[n] = p.src; b.wsn[n] = (int)p.wsn; b.wsc[n] = (int)p.wsc; b.off[n] = p.off;
      b.N[n] = p.N; b.C[n] = p.C; b.KK[n] = p.KK;
      const int64_t t = (int64_t)p.N * p.C * p.KK;
      most = t > most ? t : most;
    }
    const int bx = (int)((most + 255) / 256 < 512 ? (most + 255) / 256 : 512);
    hipLaunchKernelGGL(conv_pack_multi_kernel, dim3(bx, n), dim3(256), 0, st, b, pc.arena);
  }
  g_pc_cur = &pc;
  g_pc_last = id;
  return launch_status("tvq_conv_packcache_begin");
}

extern "C" int tvq_conv_packcache_end(void) {
  g_pc_cur = nullptr;
  return TVQ_OK;
}

// pause(1): convs run without the open scope's cache (weights computed inside the scope,
// e.g. folded per call, must not be recorded: the cache repacks at the NEXT scope's begin,
// before such a weight is recomputed); pause(0) resumes it
static PackCacheState* g_pc_paused = nullptr;
extern "C" int tvq_conv_packcache_pause(int64_t on) {
  if (on) {
    TVQ_CHECK_ARG(!g_pc_paused, "tvq_conv_packcache_pause: already paused");
    g_pc_paused = g_pc_cur;
    g_pc_cur = nullptr;
  } else {
    g_pc_cur = g_pc_paused;
    g_pc_paused = nullptr;
  }
  return TVQ_OK;
}

extern "C" int tvq_conv_packcache_release(int64_t id) {
  auto it = g_pcs.find(id);
  if (it == g_pcs.end()) return TVQ_OK;
  TVQ_CHECK_ARG(g_pc_cur != &it->second, "tvq_conv_packcache_release: the cache's scope is open");
  g_pcs.erase(it);
  return TVQ_OK;
}

extern "C" int64_t tvq_conv_packcache_entries(void) {
  auto it = g_pcs.find(g_pc_last);
  return it == g_pcs.end() ? 0 : (int64_t)it->second.entries.size();
}

