// Test-only harness of the batched decode-step kernels (tests/test_step_kernels_gpu.py, tests/test_step_harness_cpu.py): the six kinds of node of
// ptts_lm.hip::strip_path above 8 rows, and its fused-prologue strips up to 8 rows.
// It includes the product headers and launches the product's own templates through the product's own launch functions - launch_gemm<WT, PRO, EPI>,
// launch_prep<WT, PRO>, launch_lnproj<WT, EPI>, launch_xattn_fused<WT> (ptts_gemm_launch.h), pack_weight_kernel / pack_w8_kernel as ptts_lm.hip
// launches them - on device pointers that the test allocates with torch. No kernel code of its own. The entry point of a strip instance (preloaded or
// by value) is whatever launch_strip / PTTS_STRIP_PRELOAD picks.
//
// Built by the tests with build()'s hipcc flags, in parts that compile in parallel (tests/step_harness.py: parts()):
//   -DSH_COMMON                                                    weight packing, instance lists, struct sizes, error plumbing
//   -DSH_GEMM -DSH_WT=bf16_t|float -DSH_PRO=<PRO_*> -DSH_EPI=<EPI_*> -DSH_TAG=<t|f><pro><epi>   sh_gemm_<tag>
//   -DSH_PREP / -DSH_LNPROJ / -DSH_XATTN -DSH_WT=... -DSH_TAG=<t|f>  sh_rows_prep_<tag> / sh_lnproj_<tag> / sh_xattn_<tag>
// and the product's ptts_lm_w8.hip as one more part, so that ptts_strip_w8_launch (the e4m3 strips) is the product's.
// Every entry returns a PTTS_* status; the message is in sh_last_error(). A shape the harness cannot address safely is PTTS_E_INVALID, not a launch.
#include "ptts_common.h"
#include "ptts_lm_kernels.h"
#include "ptts_gemm_launch.h"
#include "ptts_step_plan.h"

#define SH_API extern "C" __attribute__((visibility("default")))

// the operands of one strip GEMM or rows_prep launch: the GemmArgs fields the decode step sets
struct ShGemm {
  const void* W;          // packed weights (sh_pack)
  const void* W8;         // e4m3 strips (sh_pack_w8) or null
  const float* wscale;    // W8: [N]
  const void* x;          // PRO_PLAIN / PRO_LN / PRO_LNS: fp32 rows; PRO_COPY: engine-dtype rows, row-major or fragment order (x_fo)
  void* out;              // fp32 [M][out_ld], or the engine dtype (_WT epilogues: row-major or fragment order by out_fo)
  void* dst;              // sh_rows_prep: the prepared rows
  const float* gamma;
  const float* beta;
  const float* part;      // PRO_ATTN: [M][S][K]
  const float* stats;     // PRO_ATTN: [M][S][nheads][2]
  float* stats_out;       // EPI_RESID: [M][N/16][2] or null
  const float* lnstat;    // PRO_LNS: [M][K/16][2]
  int M, N, K, x_ld, out_ld, x_row_mul, x_row_off, x_fo, out_fo, decode, S, nheads;
};

// one lnproj_fused_kernel launch (LnProjArgs)
struct ShLnProj {
  const void* W;
  const float* x;
  const float* gamma;
  const float* beta;
  void* out;
  void* kcache;
  void* vcache;
  int M, N, K, x_ld, out_ld, out_fo, kv_Q, kv_cap, kv_heads, kv_H;
};

// one xattn_fused_kernel launch (XAttnArgs); DevDims lives in device memory, written by the test as raw bytes
struct ShXAttn {
  const void* W;
  const float* x;
  const float* gamma;
  const float* beta;
  void* kcache;
  void* vcache;
  const int* cur_len;
  const void* dims;
  const int* mask;
  const float* cos;
  const float* sin;
  void* out;
  int B, K, x_ld, x_row_mul, x_row_off, cap, mask_ld, nheads, kv_heads, n_rep, out_fo;
  float scale;
};

#if defined(SH_COMMON)

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

SH_API const char* sh_last_error(void) { return g_ptts_err.c_str(); }
// 0: ShGemm, 1: ShLnProj, 2: ShXAttn, 3: DevDims
SH_API int sh_args_size(int which) {
  return which == 0 ? (int)sizeof(ShGemm) : which == 1 ? (int)sizeof(ShLnProj) : which == 2 ? (int)sizeof(ShXAttn) : which == 3 ? (int)sizeof(DevDims) : -1;
}

// every template instance the harness reaches, five ints per instance (unused ones 0); returns the number of instances of `kind`
//   0 lnproj_fused_kernel (bf16, UW, NF4, G, EPI)   1 xattn_fused_kernel (bf16, UW, NF4, G)   2 rows_prep_kernel (bf16, PRO)
//   3 gemm_strip_kernel<bf16_t, PRO, EPI, MTP, FULL = true, W8 = true> (PRO, EPI, MTP): the list of ptts_lm_w8.hip
SH_API int sh_instances(int kind, int* out, int cap) {
  int n = 0;
  auto put = [&](int a, int b, int c, int d, int e) {
    if (n < cap) { out[5 * n] = a; out[5 * n + 1] = b; out[5 * n + 2] = c; out[5 * n + 3] = d; out[5 * n + 4] = e; }
    ++n;
  };
  static const int uwnf[3][2] = {{16, 4}, {8, 4}, {8, 6}};  // launch_lnproj / launch_xattn_fused: hidden 1024 (16- and 8-fragment groups), 1536
  if (kind == 0) {
    for (int bf = 0; bf < 2; ++bf)
      for (int epi : {EPI_STORE, EPI_GELU_WT})
        for (const auto& u : uwnf)
          for (int g : {16, 4, 8}) put(bf, u[0], u[1], g, epi);
  } else if (kind == 1) {
    for (int bf = 0; bf < 2; ++bf) {
      for (int g : {4, 2, 8}) { put(bf, 16, 4, g, 0); put(bf, 8, 6, g, 0); }
      put(bf, 8, 4, 8, 0);
      put(bf, 8, 2, 8, 0);
    }
  } else if (kind == 2) {
    for (int bf = 0; bf < 2; ++bf) { put(bf, PRO_LN, 0, 0, 0); put(bf, PRO_ATTN, 0, 0, 0); }
  } else if (kind == 3) {
    put(PRO_LN, EPI_STORE, 1, 0, 0); put(PRO_ATTN, EPI_RESID, 1, 0, 0); put(PRO_LN, EPI_GELU, 1, 0, 0); put(PRO_PLAIN, EPI_RESID, 1, 0, 0);
    for (int mtp : {1, 2, 4}) { put(PRO_COPY, EPI_STORE, mtp, 0, 0); put(PRO_COPY, EPI_RESID, mtp, 0, 0); }
    put(PRO_COPY, EPI_GELU_WT, 4, 0, 0);
    put(PRO_LNS, EPI_GELU_WT, 1, 0, 0); put(PRO_LNS, EPI_GELU_WT, 2, 0, 0);
  } else {
    return -1;
  }
  return n;
}

// ---- the product's plan of a strip-path forward (ptts_step_plan.h), host only: nothing is launched and no device is touched -------------------------------
// 0: StepSwitches, 1: StepConfig, 2: StripPlan
SH_API int sh_plan_size(int which) { return which == 0 ? (int)sizeof(StepSwitches) : which == 1 ? (int)sizeof(StepConfig) : which == 2 ? (int)sizeof(StripPlan) : -1; }
SH_API int sh_lns_fits(int M, int K, int bf16) { return pro_lns_fits(M, K, bf16 ? 2 : 4) ? 1 : 0; }
// strip_plan of a prefill over Q positions per utterance, or of a decode step (Q = 1), of B utterances; counts[0] = kernel launches of one layer,
// counts[1] = of the head projection. PTTS_E_INVALID for a config ptts_engine_create refuses, or a call that does not run the strip path
SH_API int sh_strip_plan(const ptts_config* c, const StepSwitches* sw, int prefill, int B, int Q, int prefill_attn_mode, StripPlan* out, int* counts) {
  if (!c || !sw || !out || !counts || c->hidden_size <= 0 || c->num_heads <= 0 || c->hidden_size != 64 * c->num_heads || (c->dtype != PTTS_F32 && c->dtype != PTTS_BF16) ||
      c->ffn_dim <= 0 || c->max_batch < 1 || c->max_ctx < 2 || c->max_enc < 1 || c->max_prompt < 1 || c->num_kv_heads < 0 || c->num_cross_kv_heads < 0 ||
      (c->kv_fp8 && (c->dtype != PTTS_BF16 || c->max_batch <= GV_MAX_ROWS)))
    return ptts_fail(PTTS_E_INVALID, "sh_strip_plan: null or invalid config");
  const StepConfig sc = step_config(*c);
  if (B < 1 || B > c->max_batch || Q < 1 || (prefill ? Q > c->max_prompt : Q != 1) || step_on_gemv(sc, prefill != 0, B))
    return ptts_fail(PTTS_E_INVALID, "sh_strip_plan: prefill=%d B=%d Q=%d is no strip-path forward of this engine", prefill, B, Q);
  *out = strip_plan(sc, *c, *sw, prefill != 0, B, Q, prefill_attn_mode);
  counts[0] = out->launches(); counts[1] = out->head_launches();
  return PTTS_OK;
}

// row-major fp32 W[N][K] -> A-fragment order of the engine dtype (bf16 = 1: bf16, else fp32), as the engines pack their weights
SH_API int sh_pack(int bf16, const float* src, void* dst, int N, int K, void* stream) {
  const int KT = bf16 ? Elem<bf16_t>::KT : Elem<float>::KT;
  if (!src || !dst || N % 16 || K % KT || N <= 0 || K <= 0) return ptts_fail(PTTS_E_INVALID, "sh_pack: N=%d K=%d", N, K);
  const size_t total = (size_t)(N / 16) * (K / KT) * 64;
  const dim3 grid((unsigned)((total + 255) / 256));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (bf16) hipLaunchKernelGGL((pack_weight_kernel<bf16_t, float>), grid, dim3(256), 0, st, src, reinterpret_cast<bf16_t*>(dst), N, K, 0, K / KT);
  else hipLaunchKernelGGL((pack_weight_kernel<float, float>), grid, dim3(256), 0, st, src, reinterpret_cast<float*>(dst), N, K, 0, K / KT);
  return launch_status("pack_weight_kernel");
}

// row-major e4m3 bytes W8[N][K] -> the e4m3 strips' fragment-pair order [N/16][K/64][64 lanes][16 B]
SH_API int sh_pack_w8(const void* src, void* dst, int N, int K, void* stream) {
  if (!src || !dst || N % 16 || K % 64 || N <= 0 || K <= 0) return ptts_fail(PTTS_E_INVALID, "sh_pack_w8: N=%d K=%d", N, K);
  const size_t total = (size_t)(N / 16) * (K / 64) * 64;
  hipLaunchKernelGGL(pack_w8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const uint8_t*>(src), reinterpret_cast<uint4*>(dst), N, K, 0, K / 64);
  return launch_status("pack_w8_kernel");
}

#else

#define SH_CAT2(a, b) a##_##b
#define SH_CAT(a, b) SH_CAT2(a, b)
#define SH_NAME(kind) SH_CAT(kind, SH_TAG)
typedef SH_WT WT;
[[maybe_unused]] constexpr int KTw = Elem<WT>::KT;

[[maybe_unused]] static GemmArgs sh_gemm_args(const ShGemm& g) {
  GemmArgs a = {};
  a.W = g.W; a.W8 = g.W8; a.wscale = g.wscale; a.x = reinterpret_cast<const float*>(g.x); a.out = reinterpret_cast<float*>(g.out);
  a.M = g.M; a.N = g.N; a.K = g.K; a.x_ld = g.x_ld; a.out_ld = g.out_ld; a.x_row_mul = g.x_row_mul; a.x_row_off = g.x_row_off;
  a.x_fo = g.x_fo; a.out_fo = g.out_fo; a.decode = g.decode; a.stats_out = g.stats_out; a.lnstat = g.lnstat;
  a.part = g.part; a.stats = g.stats; a.S = g.S; a.nheads = g.nheads; a.gamma = g.gamma; a.beta = g.beta;
  return a;
}

#if defined(SH_GEMM)
constexpr int PRO = SH_PRO, EPI = SH_EPI;

// launch_gemm<WT, PRO, EPI> on up to 256 rows (the strip kernels; above, launch_gemm leaves them: tests/native/gemm_harness.hip), with the row limits
// of the product's own choice (ptts_step_plan.h: pro_gemm): fused prologues up to 8 rows, PRO_LNS at 9..32 rows where all rows fit in LDS
SH_API int SH_NAME(sh_gemm)(const ShGemm* g, void* stream) {
  const bool wt_out = EPI == EPI_GELU_WT;
  if (!g->W || !g->out || g->M <= 0 || g->M > 256 || g->N <= 0 || g->N % 16 || g->K <= 0 || g->K % KTw || g->out_ld < g->N || g->out_ld % 4)
    return ptts_fail(PTTS_E_INVALID, "sh_gemm: M=%d N=%d K=%d out_ld=%d", g->M, g->N, g->K, g->out_ld);
  if ((g->out_fo && (!wt_out || g->out_ld != g->N || g->N % KTw)) || (g->stats_out && EPI != EPI_RESID))
    return ptts_fail(PTTS_E_INVALID, "sh_gemm: out_fo=%d stats_out=%p on epilogue %d (out_ld=%d N=%d)", g->out_fo, (void*)g->stats_out, EPI, g->out_ld, g->N);
  if (g->W8 && (sizeof(WT) != 2 || !g->wscale || g->K % 64)) return ptts_fail(PTTS_E_INVALID, "sh_gemm: e4m3 strips need the bf16 engine, wscale and K %% 64 == 0");
  if (PRO == PRO_ATTN) {
    if (!g->part || !g->stats || g->S <= 0 || g->nheads <= 0 || g->nheads * 64 != g->K)
      return ptts_fail(PTTS_E_INVALID, "sh_gemm: PRO_ATTN S=%d heads=%d K=%d", g->S, g->nheads, g->K);
  } else if (!g->x || (unsigned)g->x_row_mul > 0xffffu || (unsigned)g->x_row_off > 0xffffu || g->x_row_mul < 1) {
    return ptts_fail(PTTS_E_INVALID, "sh_gemm: x=%p rows %d * m + %d", g->x, g->x_row_mul, g->x_row_off);
  }
  if (PRO == PRO_COPY) {
    if (g->x_fo ? (g->x_row_mul != 1 || g->x_row_off != 0) : (g->x_ld < g->K || g->x_ld % (16 / (int)sizeof(WT))))
      return ptts_fail(PTTS_E_INVALID, "sh_gemm: PRO_COPY x_fo=%d x_ld=%d rows %d * m + %d", g->x_fo, g->x_ld, g->x_row_mul, g->x_row_off);
  } else {
    const int how = pro_gemm(g->M, g->K, sizeof(WT), PRO == PRO_LNS && g->lnstat);
    if (g->x_fo || (PRO != PRO_LNS && how != PG_FUSED) || (PRO == PRO_LNS && g->M > 32)) return ptts_fail(PTTS_E_INVALID, "sh_gemm: prologue %d on %d rows (x_fo=%d)", PRO, g->M, g->x_fo);
    if (PRO != PRO_ATTN && (g->x_ld < g->K || g->x_ld % 4)) return ptts_fail(PTTS_E_INVALID, "sh_gemm: x_ld=%d K=%d", g->x_ld, g->K);
    if ((PRO == PRO_LN || PRO == PRO_LNS) && (!g->gamma || !g->beta)) return ptts_fail(PTTS_E_INVALID, "sh_gemm: LayerNorm without gamma / beta");
    if (PRO == PRO_LNS && how != PG_LNS)
      return ptts_fail(PTTS_E_INVALID, "sh_gemm: PRO_LNS on M=%d K=%d lnstat=%p", g->M, g->K, (void*)g->lnstat);
  }
  return launch_gemm<WT, PRO, EPI>(sh_gemm_args(*g), reinterpret_cast<hipStream_t>(stream));
}

#elif defined(SH_PREP)

// launch_prep<WT, PRO_LN | PRO_ATTN>: rows_prep_kernel into g->dst, row-major or fragment order (out_fo)
SH_API int SH_NAME(sh_rows_prep)(int pro, const ShGemm* g, void* stream) {
  if (!g->dst || g->M <= 0 || g->K <= 0 || g->K % KTw || (pro != PRO_LN && pro != PRO_ATTN))
    return ptts_fail(PTTS_E_INVALID, "sh_rows_prep: pro=%d M=%d K=%d", pro, g->M, g->K);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int rc;
  if (pro == PRO_LN) {
    if (!g->x || !g->gamma || !g->beta || g->x_ld < g->K || g->x_ld % 4 || g->x_row_mul < 1)
      return ptts_fail(PTTS_E_INVALID, "sh_rows_prep: PRO_LN x_ld=%d K=%d rows %d * m + %d", g->x_ld, g->K, g->x_row_mul, g->x_row_off);
    rc = launch_prep<WT, PRO_LN>(sh_gemm_args(*g), g->dst, st);
  } else {
    if (!g->part || !g->stats || g->S <= 0 || g->nheads <= 0 || g->nheads * 64 != g->K)
      return ptts_fail(PTTS_E_INVALID, "sh_rows_prep: PRO_ATTN S=%d heads=%d K=%d", g->S, g->nheads, g->K);
    rc = launch_prep<WT, PRO_ATTN>(sh_gemm_args(*g), g->dst, st);
  }
  return rc != PTTS_OK ? rc : launch_status("rows_prep_kernel");
}

#elif defined(SH_LNPROJ)

// launch_lnproj<WT, EPI_STORE | EPI_GELU_WT> with g utterances per workgroup, under the plan's width rule for the node (lnproj_width_ok)
SH_API int SH_NAME(sh_lnproj)(int epi, int gsz, const ShLnProj* g, void* stream) {
  if (!g->W || !g->x || !g->gamma || !g->beta || !g->out || g->M <= 0 || g->N <= 0 || !lnproj_width_ok(g->K, KTw, g->N) ||
      g->x_ld < g->K || g->x_ld % 4 || g->out_ld < g->N || g->out_ld % 4 || (gsz != 4 && gsz != 8 && gsz != 16) || (epi != EPI_STORE && epi != EPI_GELU_WT))
    return ptts_fail(PTTS_E_INVALID, "sh_lnproj: M=%d N=%d K=%d x_ld=%d out_ld=%d g=%d epi=%d", g->M, g->N, g->K, g->x_ld, g->out_ld, gsz, epi);
  if (g->out_fo && (epi != EPI_GELU_WT || g->out_ld != g->N || g->N % KTw)) return ptts_fail(PTTS_E_INVALID, "sh_lnproj: out_fo on epilogue %d, out_ld=%d N=%d", epi, g->out_ld, g->N);
  if (g->kcache || g->vcache) {
    if (epi != EPI_STORE || !g->kcache || !g->vcache || g->kv_Q <= 0 || g->kv_Q > g->kv_cap || g->kv_heads <= 0 || g->kv_H <= 0 || g->kv_H % 64 ||
        g->kv_H + 2 * 64 * g->kv_heads != g->N)
      return ptts_fail(PTTS_E_INVALID, "sh_lnproj: cache append Q=%d cap=%d heads=%d H=%d N=%d", g->kv_Q, g->kv_cap, g->kv_heads, g->kv_H, g->N);
  }
  if ((size_t)std::min(g->M, gsz) * ((size_t)g->K * sizeof(WT) + 16) + 8 * 1024 > 160 * 1024) return ptts_fail(PTTS_E_INVALID, "sh_lnproj: rows do not fit in LDS");
  LnProjArgs p = {};
  p.W = g->W; p.x = g->x; p.x_ld = g->x_ld; p.gamma = g->gamma; p.beta = g->beta; p.K = g->K; p.out = g->out; p.out_ld = g->out_ld; p.out_fo = g->out_fo;
  p.M = g->M; p.N = g->N; p.kcache = g->kcache; p.vcache = g->vcache; p.kv_Q = g->kv_Q; p.kv_cap = g->kv_cap; p.kv_heads = g->kv_heads; p.kv_H = g->kv_H;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return epi == EPI_STORE ? launch_lnproj<WT, EPI_STORE>(nullptr, p, st, gsz) : launch_lnproj<WT, EPI_GELU_WT>(nullptr, p, st, gsz);
}

#elif defined(SH_XATTN)

// launch_xattn_fused<WT> with gsz utterances per workgroup, under the plan's width and group rules for the node (the lengths behind dims / cur_len are the
// test's to keep inside cap, mask_ld and the RoPE tables)
SH_API int SH_NAME(sh_xattn)(int gsz, const ShXAttn* g, void* stream) {
  if (!g->W || !g->x || !g->gamma || !g->beta || !g->kcache || !g->vcache || !g->dims || !g->out || g->B <= 0 || g->B > 256 ||
      !xattn_width_ok(g->K, KTw) || g->x_ld < g->K || g->x_ld % 4 || g->x_row_mul < 1 || g->x_row_off < 0 ||
      g->nheads * 64 != g->K || g->kv_heads <= 0 || g->n_rep <= 0 || g->kv_heads * g->n_rep != g->nheads || g->cap <= 0 || (g->mask && g->mask_ld <= 0) ||
      (!g->cos) != (!g->sin) || (g->cos && !g->cur_len))
    return ptts_fail(PTTS_E_INVALID, "sh_xattn: B=%d K=%d x_ld=%d heads=%d x %d / %d cap=%d mask_ld=%d", g->B, g->K, g->x_ld, g->kv_heads, g->n_rep, g->nheads, g->cap, g->mask_ld);
  // hidden 512 has the 8-utterance instance only (launch_xattn_fused would size the grid for gsz and run G = 8)
  if (!xattn_group_ok(g->K, gsz, g->B))
    return ptts_fail(PTTS_E_INVALID, "sh_xattn: %d utterances per workgroup at K=%d B=%d", gsz, g->K, g->B);
  XAttnArgs x = {};
  x.W = g->W; x.x = g->x; x.x_ld = g->x_ld; x.x_row_mul = g->x_row_mul; x.x_row_off = g->x_row_off; x.gamma = g->gamma; x.beta = g->beta; x.K = g->K;
  x.invK = 1.0f / (float)g->K; x.kcache = g->kcache; x.vcache = g->vcache; x.cap = g->cap; x.cur_len = g->cur_len; x.dims = reinterpret_cast<const DevDims*>(g->dims);
  x.mask = g->mask; x.mask_ld = g->mask_ld; x.cos = g->cos; x.sin = g->sin; x.out = g->out; x.B = g->B; x.nheads = g->nheads; x.kv_heads = g->kv_heads;
  x.n_rep = g->n_rep; x.scale = g->scale; x.out_fo = g->out_fo;
  launch_xattn_fused<WT>(x, gsz, reinterpret_cast<hipStream_t>(stream));
  return launch_status("xattn_fused_kernel");
}

#else
#error "step_harness.hip: one of SH_COMMON, SH_GEMM, SH_PREP, SH_LNPROJ, SH_XATTN"
#endif

#endif
