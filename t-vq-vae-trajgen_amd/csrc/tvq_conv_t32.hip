// The conv engine's wide-channel tile: conv_t32_kernel.
#include "tvq_conv_core.h"

namespace tvq {

// Wide-channel implicit GEMM on v_mfma_f32_32x32x2_f32 for the N % 128 == 0 convs on a full
// grid (128->128 ResBlock convs at W 32, the Upscale Conv1d pair, the HF band's 16 -> 128
// forward and 128 -> 16 data gradient).  Block tile 128 channels x 96 positions, 12 waves:
// wave w owns the 32x32 tile (channels 32 (w % 4), positions 32 (w / 4)), one accumulator,
// three waves per SIMD so one wave's barrier / address work hides behind the others'
// MFMAs; one block per CU covers the 24,576-position maps in 256 blocks without split-K.
// K runs tap-major over BK-channel stages (BK = 64, or 32 / 16 where the channels do not
// divide 64; packed weights [tap][c][n], n contiguous -> dwordx4 loads).  The first 4
// waves stage the weights, the other 8 the input; the next stage is loaded into registers
// while the current one feeds BK / 2 MFMAs per wave from the other half of a
// double-buffered LDS tile (112 KB at BK = 64), one barrier per stage.  Loads are raw
// buffer loads: per-thread offsets are three position bases + compile-time row steps, and
// an invalid (padding) source gets an offset past the buffer end, which the hardware
// returns as 0.  Each output is the same k-ordered fma chain as conv_tap_kernel's unsplit
// path (tap-major, channel order within a stage), so the two kernels agree bit for bit.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* p, int64_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0,
                                           (int)(bytes < 0x7fffffff ? bytes : 0x7fffffff),
                                           0x00020000);
}

// The tile: T32_TN channels x T32_TM positions, T32_NW waves of one 32x32 tile each.
constexpr int T32_TN = 128, T32_TM = 96, T32_NW = 12;

template <int MODE, int KH, int KW, int SW, bool REPL, int BK, bool POST = false>
__global__ __launch_bounds__(T32_NW * 64) void conv_t32_kernel(const float* __restrict__ in,
                                                           const float* __restrict__ wt,
                                                           float* __restrict__ out, ConvGeom g,
                                                           Epi e) {
  constexpr int TM = T32_TM, TN = T32_TN, NWN = TN / 32;
  constexpr int ATH = 64 * NWN;             // threads loading A (the first NWN waves)
  constexpr int LB = 128 * NWN;             // threads loading B (the other 2 NWN waves)
  constexpr int ROWF4 = TN / 4;             // dwordx4 per A row (one k)
  constexpr int APASS = ATH / ROWF4;        // A rows per pass (8)
  constexpr int PSTEP = LB % 96;            // position step between a thread's B rows
  constexpr int KSTEP = 3 * LB / 96;        // k step per 3 B elements
  constexpr int A4 = BK / APASS;            // dwordx4 A loads per A-loading thread
  constexpr int BL = TM * BK / LB;          // dword B loads per B-loading thread
  static_assert(BK % APASS == 0, "A rows");
  constexpr int BAD = 0x40000000;        // offset past any buffer end -> loads 0
  extern __shared__ float smem[];
  float* As = smem;                      // [2][BK][TN]
  float* Bs = smem + 2 * BK * TN;        // [2][BK][TM]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  // this thread stages A | B (two compares: a single flag and its negation compile to
  // another prologue schedule than the one measured)
  const bool aload = tid < ATH, bload = tid >= ATH;
  const int bt = tid - ATH;  // index among the B-loading threads
  const int wch = wid % NWN, wpos = wid / NWN;
  const int n0 = blockIdx.y * TN, m0 = blockIdx.x * TM;
  const int csteps = g.C / BK;
  const int nsteps = KH * KW * csteps;
  const int plane = g.Hin * g.Win;
  const __amdgpu_buffer_rsrc_t rin = buf_rsrc(in, (int64_t)g.B * g.C * plane * 4);
  const __amdgpu_buffer_rsrc_t rwt = buf_rsrc(wt, (int64_t)KH * KW * g.C * g.N * 4);

  // B element i (< BL) of this thread: e = bt + LB i -> position (bt + PSTEP (i%3)) % 96,
  // row k = (bt + LB (i%3)) / 96 + KSTEP (i/3)
  static_assert(BK % 8 == 0 && (TM * BK) % (3 * LB) == 0, "stage rows");
  int pm_b[3], pm_h[3], pm_w[3], krow[3];
  bool pm_ok[3];
#pragma unroll
  for (int u = 0; u < 3; ++u) {
    const int m = m0 + (bt + PSTEP * u) % TM;
    krow[u] = (bt + LB * u) / TM;
    pm_ok[u] = m < g.Mpos;
    const int mc = pm_ok[u] ? m : 0;
    const uint32_t bh = fdiv((uint32_t)mc, g.fd_wo);
    pm_w[u] = mc - (int)bh * g.Wo;
    pm_b[u] = (int)fdiv((uint32_t)mc, g.fd_hwo);
    pm_h[u] = (int)bh - pm_b[u] * g.Hout;
  }
  const int a_k = tid / ROWF4, a_n = n0 + (tid % ROWF4) * 4;
  float4 ra[A4];
  float rb[BL];
  auto load = [&](int step) {
    const int tap = step / csteps;
    const int c0 = (step - tap * csteps) * BK;
    const int kh = tap / KW, kw = tap - kh * KW;
    if (aload) {
      const int abase = (((tap * g.C + c0 + a_k) * g.N) + a_n) * 4;
#pragma unroll
      for (int i = 0; i < A4; ++i)
        ra[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(
                                               rwt, abase, i * APASS * g.N * 4, 0));
    }
    if (!bload) return;
    int boff[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      int hi, wi;
      bool v = pm_ok[u];
      if (MODE == GATHER_F) {
        hi = pm_h[u] + kh - g.oph;
        wi = pm_w[u] * SW + kw - g.opw;
        if (REPL) {
          hi = hi < 0 ? 0 : (hi >= g.Hin ? g.Hin - 1 : hi);
          wi = wi < 0 ? 0 : (wi >= g.Win ? g.Win - 1 : wi);
        } else {
          v = v && hi >= 0 && hi < g.Hin && wi >= 0 && wi < g.Win;
        }
      } else {
        hi = pm_h[u] - kh + g.oph;
        const int wn = pm_w[u] - kw + g.opw;
        v = v && hi >= 0 && hi < g.Hin && wn >= 0 && (SW == 1 || (wn & 1) == 0);
        wi = wn / SW;
        v = v && wi < g.Win;
      }
      boff[u] = v ? (((pm_b[u] * g.C + c0 + krow[u]) * plane) + hi * g.Win + wi) * 4 : BAD;
    }
#pragma unroll
    for (int i = 0; i < BL; ++i)
      rb[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                            rin, boff[i % 3], (i / 3) * KSTEP * plane * 4, 0));
  };
  auto store = [&](int buf) {
    if (aload) {
      float* a = As + buf * BK * TN + a_k * TN + (tid % ROWF4) * 4;
#pragma unroll
      for (int i = 0; i < A4; ++i) *reinterpret_cast<float4*>(a + i * APASS * TN) = ra[i];
    }
    if (bload) {
      float* bb = Bs + buf * BK * TM;
#pragma unroll
      for (int i = 0; i < BL; ++i) {
        const int u = i % 3;
        bb[(krow[u] + KSTEP * (i / 3)) * TM + (bt + PSTEP * u) % TM] = rb[i];
      }
    }
  };

  floatx16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const int r32 = lane & 31, hl = lane >> 5;
  load(0);
  store(0);
  __syncthreads();
  for (int step = 0; step < nsteps; ++step) {
    const int buf = step & 1;
    if (step + 1 < nsteps) load(step + 1);
    const float* a = As + buf * BK * TN + hl * TN + wch * 32 + r32;
    const float* bb = Bs + buf * BK * TM + hl * TM + wpos * 32 + r32;
    // fragments of FG k-pairs are read one group ahead of the MFMAs that use them, so
    // the LDS latency hides behind FG MFMAs instead of stalling every one or two
    constexpr int FG = 4, NG = BK / 2 / FG;
    float fa[2][FG], fb[2][FG];
    auto fread = [&](int grp, int slot) {
#pragma unroll
      for (int u = 0; u < FG; ++u) {
        const int kp = grp * FG + u;
        fa[slot][u] = a[2 * kp * TN];
        fb[slot][u] = bb[2 * kp * TM];
      }
    };
    fread(0, 0);
#pragma unroll
    for (int grp = 0; grp < NG; ++grp) {
      if (grp + 1 < NG) fread(grp + 1, (grp + 1) & 1);
#pragma unroll
      for (int u = 0; u < FG; ++u)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[grp & 1][u], fb[grp & 1][u], acc, 0, 0, 0);
      // emit the next group's LDS reads ahead of this group's MFMAs (T19)
      __builtin_amdgcn_sched_group_barrier(0x100, 2 * FG, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, FG, 0);
    }
    if (step + 1 < nsteps) store(buf ^ 1);
    __syncthreads();
  }

  // epilogue: acc[reg] = (channel n0 + 32 wch + (reg & 3) + 8 (reg >> 2) + 4 hl,
  // position m0 + 32 wpos + lane % 32); bias, dropout, residual as epi_store
  const uint64_t seed = e.drop_p > 0.f ? mix_seed(e.seed_ptr, e.offset) : 0ull;
  const int64_t hw = (int64_t)g.Hout * g.Wo;
  PostCh pc[POST ? 16 : 1];  // POST: this lane's 16 channels' BN / Snake terms
  if constexpr (POST) {
#pragma unroll
    for (int r = 0; r < 16; ++r)
      pc[r] = epi_post_ch(e, min(n0 + wch * 32 + (r & 3) + 8 * (r >> 2) + 4 * hl, g.N - 1));
  }
  const int m = m0 + r32 + wpos * 32;
  const bool pv = m < g.Mpos;
  const int mc = pv ? m : 0;
  const uint32_t bh = fdiv((uint32_t)mc, g.fd_wo);
  const int w = mc - (int)bh * g.Wo;
  const int b = (int)fdiv((uint32_t)mc, g.fd_hwo);
  const int h = (int)bh - b * g.Hout;
  const int64_t ob = ((int64_t)b * g.N * g.Hout + h) * g.Wo + w;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int n = n0 + wch * 32 + (r & 3) + 8 * (r >> 2) + 4 * hl;
    if (!pv || n >= g.N) continue;
    const int64_t o = ob + (int64_t)n * hw;
    float v = acc[r] + (e.bias ? e.bias[n] : 0.f);
    if constexpr (POST) v = epi_post_apply(pc[r], v, e.gelu != 0);
    if (e.drop_p > 0.f) v = uniform01(seed, (uint64_t)o) >= e.drop_p ? v * e.drop_scale : 0.f;
    if (e.residual) v += e.residual[o];
    out[o] = v;
  }
}

// LDS per block: 2 stages x BK x (128 + 96) floats
static size_t t32_lds(int bk) { return (size_t)2 * bk * (T32_TN + T32_TM) * 4; }

// One launch of the <.., BK, POST> instance.  BK = 64 takes 112 KB of dynamic LDS, which
// must be opted into once per instance (> 64 KB); BK = 32 / 16 stay under it.
template <int MODE, int KH, int KW, int SW, bool REPL, int BK, bool POST>
static void t32_run(unsigned mt, const float* in, const float* wt, float* out, const ConvGeom& g,
                    const Epi& e, hipStream_t st) {
  auto* kern = &conv_t32_kernel<MODE, KH, KW, SW, REPL, BK, POST>;
  if constexpr (BK == 64) {
    static bool lds_set = false;
    if (!lds_set) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)t32_lds(BK));
      lds_set = true;
    }
  }
  hipLaunchKernelGGL(kern, dim3(mt, g.N / T32_TN), dim3(64 * T32_NW), t32_lds(BK), st, in, wt,
                     out, g, e);
}

// The shapes conv_t32_kernel takes and its launch; false: not its shape.  *post: the
// epilogue-fused instance ran (it applied e's eval BN / Snake).
template <int MODE, int KH, int KW, int SW, bool REPL>
static bool launch_t32_t(const float* in, const float* wt, float* out, const ConvGeom& g,
                         const Epi& e, hipStream_t st, bool* post) {
  // wide channels on a full grid: 32x32 MFMA tile, no split-K (needs packed weights)
  const unsigned mt = (unsigned)((g.Mpos + T32_TM - 1) / T32_TM);
  if (!(conv_config().t32 && g.wsn == 1 && g.wsc == g.N &&
        (int64_t)g.B * g.C * g.Hin * g.Win < (1ll << 29) &&
        (int64_t)KH * KW * g.C * g.N < (1ll << 29) && g.N % T32_TN == 0 &&
        (int64_t)mt * (g.N / T32_TN) >= 192))
    return false;
  // K stage: 64 where the channels divide it, else 32 / 16 (C = 16 / 48: the HF band's
  // 16 -> 128 3x3 forward and the 128 -> 16 conv's data gradient)
  const int bk = g.C % 64 == 0 ? 64 : (g.C % 32 == 0 ? 32 : 16);
#define TVQ_T32(POSTV)                                                                   \
  if (bk == 64) t32_run<MODE, KH, KW, SW, REPL, 64, POSTV>(mt, in, wt, out, g, e, st);      \
  else if (bk == 32) t32_run<MODE, KH, KW, SW, REPL, 32, POSTV>(mt, in, wt, out, g, e, st); \
  else t32_run<MODE, KH, KW, SW, REPL, 16, POSTV>(mt, in, wt, out, g, e, st)
  // eval conv -> BN (-> Snake / after GELU): the epilogue-fused instance (Upscale's
  // Conv1d, the 128-channel ResBlock convs, the HF encoder's 16 -> 128 conv)
  constexpr bool t32_post = MODE == GATHER_F && !REPL &&
                            ((KH == 1 && KW == 3) || (KH == 3 && KW == 3));
  if constexpr (t32_post) {
    if (e.bn_rv) {
      TVQ_PLAN("conv_t32 bk%d nw12 tn128 post", bk);
      TVQ_T32(true);
      *post = true;
      return true;
    }
  }
  TVQ_PLAN("conv_t32 bk%d nw12 tn128", bk);
  TVQ_T32(false);
#undef TVQ_T32
  return true;
}

bool launch_t32(int mode, int kind, bool repl, const float* in, const float* wt, float* out,
                const ConvGeom& g, const Epi& e, hipStream_t st, bool* post) {
  *post = false;
#define M_(m, a, b_, c, d) return launch_t32_t<m, a, b_, c, d>(in, wt, out, g, e, st, post);
  TVQ_DISPATCH_CONV(mode, kind, repl, M_)
#undef M_
  return false;
}

}  // namespace tvq
