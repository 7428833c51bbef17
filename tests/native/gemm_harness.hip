// Test-only harness of the prefill-sized GEMM kernels (tests/test_gemm_kernels_gpu.py, tests/test_gemm_harness_cpu.py).
// It includes the product headers and launches the product's own templates - gemm_glds_kernel instances one by one, the LDS-tiled and
// register-blocked fallbacks, the 128-row PRO_COPY strips on both entry points, and launch_gemm<WT, PRO_COPY, EPI> - on device pointers that
// the test allocates with torch. No kernel code of its own.
//
// Built by the tests with build()'s hipcc flags, once per (engine dtype, epilogue) part in parallel plus one common part:
//   -DGH_COMMON                                       weight packing, the list of gemm_glds_kernel instances, error plumbing
//   -DGH_WT=bf16_t|float -DGH_EPI=<EPI_*> -DGH_TAG=t0 entry points gh_<kind>_<tag> of that dtype and epilogue (t = bf16, f = fp32)
// Every entry returns a PTTS_* status (launch_gemm_glds: -1 = shape declined); the message is in gh_last_error().
#include "ptts_common.h"
#include "ptts_lm_kernels.h"
#include "ptts_gemm_launch.h"

#define GH_API extern "C" __attribute__((visibility("default")))

// the operands of one GEMM; the harness copies them into GemmArgs (consecutive activation rows: x_row_mul 1, x_row_off 0)
struct GhArgs {
  const void* W;          // packed weights (gh_pack), or null with kv_layers
  const void* x;          // activations in the engine dtype, [M][x_ld]
  void* out;              // [M][out_ld]: fp32 (EPI_STORE / EPI_RESID) or the engine dtype (_WT epilogues)
  void* kcache;           // EPI_KV / EPI_STORE with kv_col0: [b][head][kv_cap][64] in the engine dtype
  void* vcache;
  const void* kv_layers;  // EPI_KV: device array of KvLayer {W, k, v}, or null
  const float* rs_part;   // folded RMSNorm consumer fields (ptts_t5.hip)
  void* nx_out;
  const float* nx_gamma;
  float* ss_out;
  int M, N, K, x_ld, out_ld;
  int nheads, kv_rows_per_b, kv_cap, kv_col0, kv_nlayers;
  int rs_n;
  float rs_invD, rms_eps;
  int xcd_swz;
};

// every gemm_glds_kernel<EPI, BNS, BMT, WN, WM, NST, RP> that launch_gemm_glds can select for the epilogues the product runs on it
#define GH_GLDS_INSTANCES(X)                                                                                                      \
  X(EPI_STORE, 12, 8, 4, 2, 2, 1) X(EPI_STORE, 4, 4, 2, 2, 3, 0) X(EPI_STORE, 8, 8, 4, 2, 2, 1) X(EPI_STORE, 8, 4, 2, 2, 2, 1)  \
  X(EPI_RESID, 4, 4, 2, 2, 3, 0) X(EPI_RESID, 8, 8, 4, 2, 2, 1) X(EPI_RESID, 8, 4, 2, 2, 2, 1)                                 \
  X(EPI_KV, 4, 4, 2, 2, 3, 0) X(EPI_KV, 8, 8, 4, 2, 2, 1) X(EPI_KV, 8, 4, 2, 2, 2, 1)                                          \
  X(EPI_GELU_WT, 4, 4, 2, 2, 3, 0) X(EPI_GELU_WT, 8, 8, 4, 2, 2, 1) X(EPI_GELU_WT, 8, 4, 2, 2, 2, 1)                           \
  X(EPI_GATE_WT, 11, 16, 1, 8, 2, 1) X(EPI_GATE_WT, 4, 4, 2, 2, 3, 0) X(EPI_GATE_WT, 8, 8, 4, 2, 2, 1) X(EPI_GATE_WT, 8, 4, 2, 2, 2, 1)

static GemmArgs gh_gemm_args(const GhArgs& g) {
  GemmArgs a = {};
  a.W = g.W; a.x = reinterpret_cast<const float*>(g.x); a.out = reinterpret_cast<float*>(g.out);
  a.M = g.M; a.N = g.N; a.K = g.K; a.x_ld = g.x_ld; a.out_ld = g.out_ld; a.x_row_mul = 1; a.x_row_off = 0;
  a.kcache = g.kcache; a.vcache = g.vcache; a.nheads = g.nheads; a.kv_rows_per_b = g.kv_rows_per_b; a.kv_cap = g.kv_cap; a.kv_col0 = g.kv_col0;
  a.kv_layers = reinterpret_cast<const KvLayer*>(g.kv_layers); a.kv_nlayers = g.kv_nlayers;
  a.rs_part = g.rs_part; a.rs_n = g.rs_n; a.rs_invD = g.rs_invD; a.rms_eps = g.rms_eps; a.nx_out = g.nx_out; a.nx_gamma = g.nx_gamma; a.ss_out = g.ss_out;
  a.xcd_swz = g.xcd_swz;
  return a;
}

static int gh_launched(const char* what) {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? PTTS_OK : ptts_fail(PTTS_E_HIP, "%s launch failed: %s", what, hipGetErrorString(e));
}

#ifdef GH_COMMON

thread_local std::string g_ptts_err;
int ptts_fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_ptts_err = buf;
  return code;
}
// the e4m3 strips (ptts_lm_w8.hip) and the strips on fragment-order rows (x_fo, m_split) are tests/native/step_harness.hip's, which links the
// product's ptts_lm_w8.hip; here launch_gemm never gets to this stand-in without GemmArgs::W8
int ptts_strip_w8_launch(int, int, int, const GemmArgs&, dim3, dim3, size_t, hipStream_t) { return -1; }

GH_API const char* gh_last_error(void) { return g_ptts_err.c_str(); }
GH_API int gh_args_size(void) { return (int)sizeof(GhArgs); }

// the 7 template arguments of every instance in GH_GLDS_INSTANCES, row after row; returns the number of instances
GH_API int gh_glds_instances(int* out, int cap) {
  int n = 0;
#define GH_LIST(E, BNS, BMT, WN, WM, NST, RP)                                  \
  if (n < cap) {                                                                \
    const int t[7] = {E, BNS, BMT, WN, WM, NST, RP};                            \
    for (int i = 0; i < 7; ++i) out[7 * n + i] = t[i];                          \
  }                                                                             \
  ++n;
  GH_GLDS_INSTANCES(GH_LIST)
#undef GH_LIST
  return n;
}

// row-major fp32 W[N][K] -> A-fragment order of the engine dtype (bf16 = 1: bf16, else fp32), as the engines pack their weights
GH_API int gh_pack(int bf16, const float* src, void* dst, int N, int K, void* stream) {
  const int KT = bf16 ? Elem<bf16_t>::KT : Elem<float>::KT;
  if (N % 16 || K % KT || N <= 0 || K <= 0) return ptts_fail(PTTS_E_INVALID, "gh_pack: N=%d K=%d", N, K);
  const size_t total = (size_t)(N / 16) * (K / KT) * 64;
  const dim3 grid((unsigned)((total + 255) / 256));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (bf16) hipLaunchKernelGGL((pack_weight_kernel<bf16_t, float>), grid, dim3(256), 0, st, src, reinterpret_cast<bf16_t*>(dst), N, K, 0, K / KT);
  else hipLaunchKernelGGL((pack_weight_kernel<float, float>), grid, dim3(256), 0, st, src, reinterpret_cast<float*>(dst), N, K, 0, K / KT);
  return gh_launched("pack_weight_kernel");
}

#else  // one (engine dtype, epilogue) part

#define GH_CAT2(a, b) a##_##b
#define GH_CAT(a, b) GH_CAT2(a, b)
#define GH_NAME(kind) GH_CAT(kind, GH_TAG)
typedef GH_WT WT;
constexpr int EPI = GH_EPI;

// launch_gemm<WT, PRO_COPY, EPI>: the dispatcher the engines call (glds / tile / block above 256 rows, strips below)
GH_API int GH_NAME(gh_gemm)(const GhArgs* g, void* stream) {
  return launch_gemm<WT, PRO_COPY, EPI>(gh_gemm_args(*g), reinterpret_cast<hipStream_t>(stream));
}

// launch_gemm_tile<WT, EPI> directly (the dispatcher sets xcd_swz = 1; here it is the caller's)
GH_API int GH_NAME(gh_tile)(const GhArgs* g, void* stream) {
  return launch_gemm_tile<WT, EPI>(gh_gemm_args(*g), reinterpret_cast<hipStream_t>(stream));
}

// gemm_block_kernel<WT, EPI, NS> on launch_gemm's grid
GH_API int GH_NAME(gh_block)(int ns, const GhArgs* g, void* stream) {
  const GemmArgs a = gh_gemm_args(*g);
  const int nstrips = a.N / 16;
  if (a.N % 16 || a.K % Elem<WT>::KT || (ns != 2 && ns != 4) || nstrips % ns || a.M <= 0)
    return ptts_fail(PTTS_E_INVALID, "gh_block: N=%d K=%d NS=%d", a.N, a.K, ns);
  const dim3 grid(nstrips / ns, (a.M + 255) / 256), block(256);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (ns == 4) hipLaunchKernelGGL((gemm_block_kernel<WT, EPI, 4>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((gemm_block_kernel<WT, EPI, 2>), grid, block, 0, st, a);
  return gh_launched("gemm_block_kernel");
}

// the 128-row PRO_COPY strip instance gemm_strip_kernel<WT, PRO_COPY, EPI, 8, FULL> (64 < M: rows_per_pass = min(M, 128)) with launch_gemm's
// wave count, fragments per wave and LDS size, on the preloaded entry point (what launch_gemm runs) or by value (gemm_strip_kernel_bv)
template <bool FULL, bool BV>
static int gh_strip128(GemmArgs a, int W, hipStream_t st) {
  const void* fn = BV ? reinterpret_cast<const void*>(&gemm_strip_kernel_bv<WT, PRO_COPY, EPI, 8, FULL>)
                      : reinterpret_cast<const void*>(&gemm_strip_kernel<WT, PRO_COPY, EPI, 8, FULL>);
  static PttsPerDeviceOnce attr_once;
  const int attr_dev = PttsPerDeviceOnce::device();
  if (attr_once.need(attr_dev)) {
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return ptts_fail(PTTS_E_HIP, "hipFuncSetAttribute(max dynamic LDS) failed: %s", hipGetErrorString(e));
    attr_once.done(attr_dev);
  }
  const size_t sh = (size_t)W * 8 * 1024 + 256;
  const dim3 grid(a.N / 16, 1, (EPI == EPI_KV && a.kv_layers) ? a.kv_nlayers : 1), block(W * 64);
  if constexpr (BV) hipLaunchKernelGGL((gemm_strip_kernel_bv<WT, PRO_COPY, EPI, 8, FULL>), grid, block, sh, st, a);
  else ptts_klaunch(gemm_strip_kernel<WT, PRO_COPY, EPI, 8, FULL>, grid, block, sh, st, a);
  return gh_launched("gemm_strip_kernel");
}
GH_API int GH_NAME(gh_strip)(int by_value, const GhArgs* g, void* stream) {
  GemmArgs a = gh_gemm_args(*g);
  constexpr int KT = Elem<WT>::KT, wmax = GemmMaxThreads<PRO_COPY, 8>::value / 64;
  if (a.N % 16 || a.K % KT || a.M <= 64) return ptts_fail(PTTS_E_INVALID, "gh_strip: N=%d K=%d M=%d (the 128-row instance needs M > 64)", a.N, a.K, a.M);
  const int nfrag = a.K / KT;
  int W = 0;  // launch_gemm: FULL when every wave owns whole 8-fragment groups and K % 256 == 0
  if (a.K % 256 == 0)
    for (int w = wmax; w >= 2; --w)
      if (nfrag % (8 * w) == 0) { W = w; break; }
  const bool full = W > 0;
  if (!full) W = std::min(std::max((nfrag + 7) / 8, 2), wmax);
  a.frags_per_wave = nfrag / W;
  a.invK = 1.0f / (float)a.K;
  a.rows_per_pass = std::min(a.M, 128);
  a.m_split = 0;
  a.x_fo = 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (full) return by_value ? gh_strip128<true, true>(a, W, st) : gh_strip128<true, false>(a, W, st);
  return by_value ? gh_strip128<false, true>(a, W, st) : gh_strip128<false, false>(a, W, st);
}

#ifdef GH_BF16
// launch_gemm_glds<EPI>: the policy choice and the shape checks of the LDS-DMA GEMM (-1 = declined)
GH_API int GH_NAME(gh_glds_dispatch)(const GhArgs* g, void* stream) {
  GemmArgs a = gh_gemm_args(*g);
  return launch_gemm_glds<EPI>(a, reinterpret_cast<hipStream_t>(stream));
}

// one gemm_glds_kernel instance of GH_GLDS_INSTANCES directly (launch_gemm_glds_inst), whatever the policy would pick for the shape
// (a template, so that the instances of the other epilogues are discarded, not compiled into this part)
template <int E>
static int gh_glds_one(const int* t, const GemmArgs& a, hipStream_t st) {
#define GH_INST(E1, BNS, BMT, WN, WM, NST, RP)                                                                                   \
  if constexpr (E1 == E) {                                                                                                       \
    if (t[0] == E1 && t[1] == BNS && t[2] == BMT && t[3] == WN && t[4] == WM && t[5] == NST && t[6] == RP) {                     \
      if (a.K % 64 || a.K <= 0 || a.N % (16 * BNS) || a.N <= 0 || a.x_ld % 8 || a.M <= 0)                                        \
        return ptts_fail(PTTS_E_INVALID, "gh_glds: N=%d K=%d x_ld=%d M=%d on %d-column tiles", a.N, a.K, a.x_ld, a.M, 16 * BNS); \
      return launch_gemm_glds_inst<E1, BNS, BMT, WN, WM, NST, RP>(a, st);                                                       \
    }                                                                                                                            \
  }
  GH_GLDS_INSTANCES(GH_INST)
#undef GH_INST
  return ptts_fail(PTTS_E_INVALID, "gh_glds: no instance <%d, %d, %d, %d, %d, %d, %d>", t[0], t[1], t[2], t[3], t[4], t[5], t[6]);
}
GH_API int GH_NAME(gh_glds)(const int* t, const GhArgs* g, void* stream) {
  return gh_glds_one<EPI>(t, gh_gemm_args(*g), reinterpret_cast<hipStream_t>(stream));
}
#endif

#endif
