// Test-only harness of the teacher-forced scoring kernel (tests/test_score_kernel_gpu.py, tools/score_probe.py). It includes the product headers and
// launches the product's own templates on device pointers the test allocates with torch: pack_weight_kernel, score_launch (the function the engine
// calls, ptts_score_launch.h) and - as the comparison - the existing final-LayerNorm + heads projection the way ln_gemm<WT,
// EPI_STORE> (ptts_lm.hip) runs it: the fused prologue up to 8 rows, rows_prep + the PRO_COPY GEMM above. No kernel code of its own.
// Every entry returns a PTTS_* status; the message is in sh_last_error(). dtype: 0 = fp32 engine, 1 = bf16 engine.
#include "ptts_common.h"
#include "ptts_lm_kernels.h"
#include "ptts_gemm_launch.h"
#include "ptts_score_launch.h"

#define SH_API extern "C" __attribute__((visibility("default")))

struct ShArgs {
  const float* x;          // residual rows fp32 [B * Q][x_ld]
  const float* gamma;
  const float* beta;
  const void* W;           // packed heads (sh_pack)
  const long long* ids;    // [B * K][T]
  const long long* labels; // [B][T][K] or null
  float* nll;
  int* counted;
  float* logits;           // [B * K][Qs][V] or null
  void* xw;                // sh_project: engine-dtype scratch [M][H]
  float* out;              // sh_project: [M][K * V]
  int x_ld, H, K, V, B, Q, Qs, T, bos, eos, M;
};

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
// the e4m3 strips live in ptts_lm_w8.hip; launch_gemm never gets to this stand-in without GemmArgs::W8
int ptts_strip_w8_launch(int, int, int, const GemmArgs&, dim3, dim3, size_t, hipStream_t) { return -1; }

SH_API const char* sh_last_error(void) { return g_ptts_err.c_str(); }
SH_API int sh_args_size(void) { return (int)sizeof(ShArgs); }

template <typename WT>
static int sh_pack_t(const float* src, void* dst, int N, int K, hipStream_t st) {
  if (N % 16 || K % Elem<WT>::KT) return ptts_fail(PTTS_E_INVALID, "pack: N=%d K=%d", N, K);
  const int nfrag = K / Elem<WT>::KT;
  const size_t total = (size_t)(N / 16) * nfrag * 64;
  hipLaunchKernelGGL((pack_weight_kernel<WT, float>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, src, reinterpret_cast<WT*>(dst), N, K, 0, nfrag);
  return launch_status("pack");
}
SH_API int sh_pack(int dtype, const float* src, void* dst, int N, int K, void* stream) {
  return dtype ? sh_pack_t<bf16_t>(src, dst, N, K, (hipStream_t)stream) : sh_pack_t<float>(src, dst, N, K, (hipStream_t)stream);
}

SH_API int sh_score(int dtype, const ShArgs* g, void* stream) {
  ScoreArgs s = {};
  s.x = g->x; s.gamma = g->gamma; s.beta = g->beta; s.W = g->W; s.ids = g->ids; s.labels = g->labels; s.nll = g->nll; s.counted = g->counted;
  s.logits = g->logits; s.x_ld = g->x_ld; s.H = g->H; s.K = g->K; s.V = g->V; s.B = g->B; s.Q = g->Q; s.Qs = g->Qs; s.T = g->T; s.bos = g->bos; s.eos = g->eos;
  return dtype ? score_launch<bf16_t>(s, (hipStream_t)stream) : score_launch<float>(s, (hipStream_t)stream);
}

// out[m][n] = heads[n] . LayerNorm(x[m]) over M consecutive rows of x, as ln_gemm<WT, EPI_STORE> (ptts_lm.hip) computes the engine's logits
template <typename WT>
static int sh_project_t(const ShArgs* a, hipStream_t st) {
  GemmArgs g = {};
  g.W = a->W; g.x = a->x; g.x_ld = a->x_ld; g.x_row_mul = 1; g.x_row_off = 0; g.gamma = a->gamma; g.beta = a->beta;
  g.out = a->out; g.out_ld = a->K * a->V; g.M = a->M; g.N = a->K * a->V; g.K = a->H;
  if (g.M <= 8) return launch_gemm<WT, PRO_LN, EPI_STORE>(g, st);
  GemmArgs gp = g;
  gp.out_fo = 0;
  PTTS_TRY((launch_prep<WT, PRO_LN>(gp, a->xw, st)));
  g.x = reinterpret_cast<const float*>(a->xw);
  g.x_ld = g.K;
  return launch_gemm<WT, PRO_COPY, EPI_STORE>(g, st);
}
SH_API int sh_project(int dtype, const ShArgs* a, void* stream) {
  return dtype ? sh_project_t<bf16_t>(a, (hipStream_t)stream) : sh_project_t<float>(a, (hipStream_t)stream);
}
