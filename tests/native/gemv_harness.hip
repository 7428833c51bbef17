// Test-only harness of the row-per-wave GEMV decode step (tests/test_gemv_kernels_gpu.py, tests/test_gemv_harness_cpu.py): gemv_kernel with every
// prologue / epilogue pair of ptts_lm.hip::gemv_step, qkv_attn_kernel, xfold_attn_kernel and xq_attn_kernel.
// It declares the product's interface (ptts_gemv.h) and calls the product's own launch functions - ptts_gemv_launch, ptts_qkvattn_launch,
// ptts_xfoldattn_launch, ptts_xqattn_launch and their *_ok / rows_per_split queries - on device pointers that the test allocates with torch. No kernel
// code of its own and no template instantiated here: the kernels come from the product's three translation units ptts_gemv_{bf16,f32,w8}.hip, linked
// in as the objects build() left beside the sources, or compiled as further parts with build()'s flags where those are missing or stale
// (tests/gemv_harness.py). A linker version script keeps everything but the gvh_* entry points local to the library.
//
// The caller describes every buffer by its size in elements (the n_* fields). A launch whose arguments let a kernel form an index outside a buffer
// so described, or a shape / batch / split combination the step does not have (the split cap is the product's: ptts_step_plan.h), is PTTS_E_INVALID
// with a message in gvh_last_error() and never reaches the device. The gvh_step_config / gvh_gemv_plan entry points launch nothing: they hand the
// product's own plan of a step (ptts_step_plan.h) to the tests. The bounds are read off the kernels (ptts_gemv_kernels.h); each check names the access it covers.
#include <stdarg.h>
#include <stdio.h>

#include <string>

#include "ptts_gemv.h"
#include "ptts_step_plan.h"

#define GVH_API extern "C" __attribute__((visibility("default")))
#define GVH_E_HIP PTTS_E_HIP                  // the launch function reported -2, or a device-to-host read of a length failed
#define GVH_E_UNSUPPORTED PTTS_E_UNSUPPORTED  // the launch function reported -1: no instance

// one gemv_kernel launch: the GemvArgs fields gemv_step sets, and the extent of every buffer in elements of its own type (W: bytes)
struct GvhGemv {
  const void* W;
  const float* wscale;
  const float* x;
  const void* xw;
  const float* resid;
  const float* part;
  const float* stats;
  const float* gamma;
  const float* beta;
  const int* mask;
  const int* n_valid;
  void* out;
  float* hsum;
  long long n_W, n_wscale, n_x, n_xw, n_resid, n_part, n_stats, n_gamma, n_mask, n_out, n_hsum;
  int mode, pro, epi, S, M, N, K, npart, nheads, ne, x_ld, xw_ld, out_ld, pad_;
};

// one qkv_attn_kernel launch (QkvAttnArgs)
struct GvhQkvAttn {
  const void* W;
  const float* wscale;
  const float* x;
  const float* gamma;
  const float* beta;
  void* kcache;
  void* vcache;
  const int* cur_len;
  const int* P;
  const int* mask;
  float* part;
  float* stats;
  long long n_W, n_wscale, n_x, n_gamma, n_cache, n_cur_len, n_mask, n_part, n_stats;
  int mode, S, M, H, nheads, kv_heads, x_ld, cap, kv_bound, mask_ld;
  float scale;
  int pad_;
};

// one xfold_attn_kernel launch (XfoldAttnArgs)
struct GvhXfold {
  const void* Mw;
  const void* Uw;
  const float* x;
  const float* gamma;
  const float* beta;
  const int* n_valid;
  const int* mask;
  float* xpart;
  long long n_Mw, n_Uw, n_x, n_gamma, n_mask, n_xpart;
  int mode, H, nheads, nur;
};

// one xq_attn_kernel launch (XqAttnArgs)
struct GvhXq {
  const void* W;
  const float* wscale;
  const float* x;
  const float* gamma;
  const float* beta;
  const void* kcache;
  const void* vcache;
  const int* mask;
  const int* n_valid;
  void* out;
  long long n_W, n_wscale, n_x, n_gamma, n_cache, n_mask, n_out;
  int mode, M, H, nheads, kv_heads, x_ld, out_ld, mask_ld, cap;
  float scale;
};

static thread_local std::string g_err;
static int gvh_fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
static int gvh_status(int rc, const char* what) {
  if (rc == 0) return PTTS_OK;
  return rc == -1 ? gvh_fail(GVH_E_UNSUPPORTED, "%s: no instance for this shape", what) : gvh_fail(GVH_E_HIP, "%s: launch error", what);
}
static bool mode_ok(int mode) { return mode == GV_F32 || mode == GV_BF16 || mode == GV_BF16_W8; }
static int esize(int mode) { return mode == GV_F32 ? 4 : 2; }
// the device-resident lengths are read back before the launch: the guards hold for the values the kernel will read
static bool read_ints(const int* dev, int n, int* host) { return hipMemcpy(host, dev, (size_t)n * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess; }

GVH_API const char* gvh_last_error(void) { return g_err.c_str(); }
// 0: GvhGemv, 1: GvhQkvAttn, 2: GvhXfold, 3: GvhXq
GVH_API int gvh_args_size(int which) {
  return which == 0 ? (int)sizeof(GvhGemv) : which == 1 ? (int)sizeof(GvhQkvAttn) : which == 2 ? (int)sizeof(GvhXfold) : which == 3 ? (int)sizeof(GvhXq) : -1;
}
// 0: GV_PMAX, 1: GV_MAX_ROWS
GVH_API int gvh_const(int which) { return which == 0 ? GV_PMAX : which == 1 ? GV_MAX_ROWS : -1; }
GVH_API int gvh_gemv_k_ok(int K, int mode) { return mode_ok(mode) && ptts_gemv_k_ok(K, mode) ? 1 : 0; }
GVH_API int gvh_qkvattn_ok(int H, int mode) { return mode_ok(mode) && ptts_qkvattn_ok(H, mode) ? 1 : 0; }
GVH_API int gvh_xfoldattn_ok(int H, int nheads, int mode) { return mode_ok(mode) && ptts_xfoldattn_ok(H, nheads, mode) ? 1 : 0; }
GVH_API int gvh_xqattn_ok(int H, int mode) { return mode_ok(mode) && ptts_xqattn_ok(H, mode) ? 1 : 0; }
GVH_API int gvh_qkvattn_rows_per_split(int mode) { return mode_ok(mode) ? ptts_qkvattn_rows_per_split(mode) : -1; }

// ---- the product's plan of a GEMV step (ptts_step_plan.h), host only: nothing is launched and no device is touched -------------------------------------
// what ptts_engine_create checks before it derives anything from a config
static bool config_ok(const ptts_config* c) {
  return c && c->hidden_size > 0 && c->num_heads > 0 && c->hidden_size == 64 * c->num_heads && (c->dtype == PTTS_F32 || c->dtype == PTTS_BF16) && c->ffn_dim > 0 &&
         c->num_layers >= 1 && c->num_codebooks >= 1 && c->vocab_size > 0 && c->max_batch >= 1 && c->max_ctx >= 2 && c->max_enc >= 1 && c->num_kv_heads >= 0 &&
         c->num_cross_kv_heads >= 0;
}
GVH_API int gvh_step_config(const ptts_config* c, StepConfig* out) {
  if (!config_ok(c) || !out) return gvh_fail(PTTS_E_INVALID, "gvh_step_config: null or invalid config");
  *out = step_config(*c);
  return PTTS_OK;
}
// the switches as an engine holds them with nothing set in the environment; returns sizeof(StepSwitches)
GVH_API int gvh_default_switches(StepSwitches* out) {
  if (out) *out = StepSwitches();
  return (int)sizeof(StepSwitches);
}
GVH_API int gvh_step_config_size(void) { return (int)sizeof(StepConfig); }
// gemv_plan for M utterances: the ptts_gemv_launch calls of one gemv_step in launch order, seven ints each (pro, epi, S, M, N, K, mode), into
// out[cap] (counted past cap); counts[0] = kernel launches of one layer, counts[1] = of the head projection, counts[2] = GemvCross, counts[3] = fuse_qa,
// counts[4] = S_f. Returns the number of ptts_gemv_launch calls, or PTTS_E_INVALID where the engine would not take the GEMV step
GVH_API int gvh_gemv_plan(const ptts_config* c, const StepSwitches* sw, int M, int kv_bound, int xfold_valid, int* out, int cap, int* counts) {
  if (!config_ok(c) || !sw || !counts || M < 1 || M > c->max_batch || kv_bound < 1 || kv_bound > c->max_ctx)
    return gvh_fail(PTTS_E_INVALID, "gvh_gemv_plan: config / M=%d / kv_bound=%d", M, kv_bound);
  const StepConfig sc = step_config(*c);
  if (!step_on_gemv(sc, false, M)) return gvh_fail(PTTS_E_INVALID, "gvh_gemv_plan: %d utterances of this engine do not run the GEMV step", M);
  const GemvPlan p = gemv_plan(sc, *c, *sw, M, kv_bound, xfold_valid != 0);
  int n = 0;
  auto put = [&](const GemvNode& g) {
    if (!g.on) return;
    if (n < cap) { int* o = out + 7 * n; o[0] = g.pro; o[1] = g.epi; o[2] = g.S; o[3] = p.M; o[4] = g.N; o[5] = g.K; o[6] = g.mode; }
    ++n;
  };
  for (int l = 0; l < c->num_layers; ++l)
    for (int i = 0; p.layer_nodes(i); ++i) put(*p.layer_nodes(i));
  put(p.heads);
  counts[0] = p.launches(); counts[1] = p.head_launches(); counts[2] = p.cross; counts[3] = p.fuse_qa; counts[4] = p.S_f;
  return n;
}

// the (prologue, epilogue, S, M) combinations of ptts_gemv_launch's dispatch (GV_FN in ptts_gemv_launch.inc); fp32 instances serve one utterance
static bool gemv_combo_ok(int mode, int pro, int epi, int S, int M) {
  if (M < 1 || M > GV_MAX_ROWS || (mode == GV_F32 && M != 1)) return false;
  if (pro == GV_LN) return (epi == GV_STORE || epi == GV_GELU_WT) && S == 1;
  if (pro == GV_COPY) return epi == GV_RESID && S == 1;
  if (pro == GV_SOFTMAX) return epi == GV_RESID && S == 1 && M == 1 && mode != GV_BF16_W8;  // the folded matrices are never e4m3
  if (pro == GV_ATTN) return epi == GV_RESID && (S == 2 || S == 4 || S == 8);
  if (pro == GV_LNP) return epi == GV_GELU_WT && S == 1 && M == 1;
  if (pro == GV_ATTN2) return epi == GV_RESID && (S == 1 || S == 2 || S == 4 || S == 8) && S <= qkvattn_split_cap(M);
  return false;
}

GVH_API int gvh_gemv(const GvhGemv* g, void* stream) {
  if (!g) return gvh_fail(PTTS_E_INVALID, "gvh_gemv: null arguments");
  const int M = g->M, N = g->N, K = g->K, S = g->S, pro = g->pro, epi = g->epi, mode = g->mode;
  if (!mode_ok(mode) || !gemv_combo_ok(mode, pro, epi, S, M))
    return gvh_fail(PTTS_E_INVALID, "gvh_gemv: mode=%d pro=%d epi=%d S=%d M=%d is not a combination of the dispatch", mode, pro, epi, S, M);
  const int es = esize(mode);
  if (N <= 0 || K <= 0 || !ptts_gemv_k_ok(K, mode) || (pro != GV_COPY && K > 2048))
    return gvh_fail(PTTS_E_INVALID, "gvh_gemv: N=%d K=%d (prologue %d)", N, K, pro);
  // weight rows 0 .. N - 1 (rows past N are clamped to N - 1), K elements each: engine dtype, or one e4m3 byte per element
  const long long wbytes = (long long)N * K * (mode == GV_BF16_W8 ? 1 : es);
  if (!g->W || g->n_W < wbytes) return gvh_fail(PTTS_E_INVALID, "gvh_gemv: W holds %lld bytes, rows [0, N) need %lld", g->n_W, wbytes);
  if (mode == GV_BF16_W8 && (!g->wscale || g->n_wscale < N)) return gvh_fail(PTTS_E_INVALID, "gvh_gemv: wscale holds %lld of N=%d", g->n_wscale, N);
  // out[em * out_ld + row], row < N, em < M; GV_RESID reads the same elements of resid (or of out)
  if (!g->out || g->out_ld < N || g->n_out < (long long)(M - 1) * g->out_ld + N)
    return gvh_fail(PTTS_E_INVALID, "gvh_gemv: out holds %lld, M=%d rows of out_ld=%d need %lld (N=%d)", g->n_out, M, g->out_ld, (long long)(M - 1) * g->out_ld + N, N);
  if (epi == GV_RESID && g->resid && g->n_resid < (long long)(M - 1) * g->out_ld + N)
    return gvh_fail(PTTS_E_INVALID, "gvh_gemv: resid holds %lld of %lld", g->n_resid, (long long)(M - 1) * g->out_ld + N);
  if (pro == GV_LN || pro == GV_LNP) {
    // x[m * x_ld + k], k < K as float4; gamma / beta [K]
    if (!g->x || !g->gamma || !g->beta || g->n_gamma < K || g->x_ld < K || g->x_ld % 4 || g->n_x < (long long)(M - 1) * g->x_ld + K)
      return gvh_fail(PTTS_E_INVALID, "gvh_gemv: LayerNorm operands x=%p (%lld) x_ld=%d gamma=%p beta=%p (%lld) K=%d", (const void*)g->x, g->n_x, g->x_ld,
                      (const void*)g->gamma, (const void*)g->beta, g->n_gamma, K);
  }
  if (pro == GV_LNP) {
    // part[i * K + k], i < npart <= GV_PMAX; hsum[k]
    if (!g->part || g->npart < 0 || g->npart > GV_PMAX || g->n_part < (long long)g->npart * K || (g->hsum && g->n_hsum < K))
      return gvh_fail(PTTS_E_INVALID, "gvh_gemv: GV_LNP npart=%d part %lld hsum %lld K=%d", g->npart, g->n_part, g->n_hsum, K);
  }
  if (pro == GV_COPY) {
    // xw[m * xw_ld + k], k < K, as 16-byte vectors
    if (!g->xw || g->xw_ld < K || (g->xw_ld * es) % 16 || g->n_xw < (long long)(M - 1) * g->xw_ld + K)
      return gvh_fail(PTTS_E_INVALID, "gvh_gemv: GV_COPY xw=%p (%lld) xw_ld=%d K=%d", g->xw, g->n_xw, g->xw_ld, K);
  }
  if (pro == GV_ATTN || pro == GV_ATTN2) {
    // part[(m * slots + sp) * K + k], stats[((m * slots + sp) * nheads + (k >> 6)) * 2 + {0, 1}], slots = S (+ 1: the new position)
    const int slots = S + (pro == GV_ATTN2 ? 1 : 0);
    if (!g->part || !g->stats || g->nheads <= 0 || g->nheads * 64 != K || g->n_part < (long long)M * slots * K || g->n_stats < (long long)M * slots * g->nheads * 2)
      return gvh_fail(PTTS_E_INVALID, "gvh_gemv: combine of %d slots x M=%d: part %lld stats %lld heads=%d K=%d", slots, M, g->n_part, g->n_stats, g->nheads, K);
  }
  if (pro == GV_SOFTMAX) {
    // x[k], k < K; mask[(k & (ne - 1)) .. + 3]; *n_valid
    if (!g->x || g->n_x < K || !g->n_valid || (g->ne != 32 && g->ne != 64) || K % g->ne || (g->mask && g->n_mask < g->ne))
      return gvh_fail(PTTS_E_INVALID, "gvh_gemv: GV_SOFTMAX x %lld ne=%d mask %lld K=%d", g->n_x, g->ne, g->n_mask, K);
  }
  GemvArgs a = {};
  a.W = g->W; a.wscale = g->wscale; a.x = g->x; a.xw = g->xw; a.resid = g->resid; a.part = g->part; a.stats = g->stats; a.gamma = g->gamma; a.beta = g->beta;
  a.mask = g->mask; a.n_valid = g->n_valid; a.out = reinterpret_cast<float*>(g->out); a.hsum = g->hsum;
  a.N = N; a.M = (unsigned char)M; a.npart = (unsigned char)g->npart; a.nheads = (unsigned short)g->nheads; a.ne = g->ne;
  a.x_ld = g->x_ld; a.xw_ld = g->xw_ld; a.out_ld = g->out_ld; a.K = K;
  return gvh_status(ptts_gemv_launch(mode, pro, epi, S, a, reinterpret_cast<hipStream_t>(stream)), "ptts_gemv_launch");
}

GVH_API int gvh_qkvattn(const GvhQkvAttn* g, void* stream) {
  if (!g) return gvh_fail(PTTS_E_INVALID, "gvh_qkvattn: null arguments");
  const int M = g->M, S = g->S, H = g->H, nh = g->nheads, nkv = g->kv_heads, mode = g->mode;
  // a power of two up to the product's cap for M utterances (ptts_step_plan.h: qkvattn_split_cap); the fp32 engine serves one utterance
  if (!mode_ok(mode) || !ptts_qkvattn_ok(H, mode) || M < 1 || M > GV_MAX_ROWS || (mode == GV_F32 && M != 1) || (S != 1 && S != 2 && S != 4 && S != 8) ||
      S > qkvattn_split_cap(M))
    return gvh_fail(PTTS_E_INVALID, "gvh_qkvattn: mode=%d H=%d S=%d M=%d", mode, H, S, M);
  if (nh <= 0 || nh * 64 != H || nkv <= 0 || nh % nkv) return gvh_fail(PTTS_E_INVALID, "gvh_qkvattn: heads=%d kv_heads=%d H=%d", nh, nkv, H);
  const long long rows = (long long)H + 2 * nkv * 64;
  // weight rows [0, H + 2 * kv_heads * 64) of H elements; wscale per row
  if (!g->W || g->n_W < rows * H * (mode == GV_BF16_W8 ? 1 : esize(mode)) || (mode == GV_BF16_W8 && (!g->wscale || g->n_wscale < rows)))
    return gvh_fail(PTTS_E_INVALID, "gvh_qkvattn: W holds %lld bytes, wscale %lld, for %lld rows", g->n_W, g->n_wscale, rows);
  // x[b * x_ld + k], k < H as float4; gamma / beta [H]
  if (!g->x || !g->gamma || !g->beta || g->n_gamma < H || g->x_ld < H || g->x_ld % 4 || g->n_x < (long long)(M - 1) * g->x_ld + H)
    return gvh_fail(PTTS_E_INVALID, "gvh_qkvattn: x %lld x_ld=%d gamma %lld H=%d", g->n_x, g->x_ld, g->n_gamma, H);
  // the first K/V batch fetches rows below kv_bound of [M][kv_heads][cap][64]; its mask reads stop at mask_ld
  if (!g->kcache || !g->vcache || g->cap <= 0 || g->kv_bound <= 0 || g->kv_bound > g->cap || g->n_cache < (long long)M * nkv * g->cap * 64)
    return gvh_fail(PTTS_E_INVALID, "gvh_qkvattn: cache %lld for M=%d kv_heads=%d cap=%d, kv_bound=%d", g->n_cache, M, nkv, g->cap, g->kv_bound);
  if (g->mask && (g->mask_ld <= 0 || g->n_mask < (long long)M * g->mask_ld)) return gvh_fail(PTTS_E_INVALID, "gvh_qkvattn: mask %lld for M=%d x mask_ld=%d", g->n_mask, M, g->mask_ld);
  // part[(b * (S + 1) + slot) * H + col], stats[((b * (S + 1) + slot) * nheads + h) * 2 + {0, 1}]
  if (!g->part || !g->stats || g->n_part < (long long)M * (S + 1) * H || g->n_stats < (long long)M * (S + 1) * nh * 2)
    return gvh_fail(PTTS_E_INVALID, "gvh_qkvattn: part %lld stats %lld for M=%d x (S + 1)=%d slots", g->n_part, g->n_stats, M, S + 1);
  if (!g->cur_len || !g->P || g->n_cur_len < M) return gvh_fail(PTTS_E_INVALID, "gvh_qkvattn: cur_len %lld for M=%d, P=%p", g->n_cur_len, M, (const void*)g->P);
  // the new position pos = P + cur_len[b] - 1: rows [0, pos) are read (below kv_bound in the first batch), row pos is written; later batches read mask[t], t < P
  int P = 0, cl[GV_MAX_ROWS];
  if (!read_ints(g->P, 1, &P) || !read_ints(g->cur_len, M, cl)) return gvh_fail(GVH_E_HIP, "gvh_qkvattn: P / cur_len could not be read");
  if (P < 0 || (g->mask && P > g->mask_ld)) return gvh_fail(PTTS_E_INVALID, "gvh_qkvattn: P=%d mask_ld=%d", P, g->mask_ld);
  for (int b = 0; b < M; ++b) {
    const int pos = P + cl[b] - 1;
    if (pos < 0 || pos >= g->kv_bound) return gvh_fail(PTTS_E_INVALID, "gvh_qkvattn: utterance %d at position %d, kv_bound=%d", b, pos, g->kv_bound);
  }
  QkvAttnArgs a = {};
  a.W = g->W; a.wscale = g->wscale; a.x = g->x; a.gamma = g->gamma; a.beta = g->beta; a.kcache = g->kcache; a.vcache = g->vcache; a.cur_len = g->cur_len; a.P = g->P;
  a.mask = g->mask; a.part = g->part; a.stats = g->stats; a.S = S; a.nheads = nh; a.H = H; a.kv_heads = nkv; a.x_ld = g->x_ld; a.M = M;
  a.cap = g->cap; a.kv_bound = g->kv_bound; a.mask_ld = g->mask_ld; a.scale = g->scale;
  return gvh_status(ptts_qkvattn_launch(mode, a, reinterpret_cast<hipStream_t>(stream)), "ptts_qkvattn_launch");
}

GVH_API int gvh_xfoldattn(const GvhXfold* g, void* stream) {
  if (!g) return gvh_fail(PTTS_E_INVALID, "gvh_xfoldattn: null arguments");
  const int H = g->H, nh = g->nheads, mode = g->mode;
  if (!mode_ok(mode) || mode == GV_BF16_W8 || nh <= 0 || nh * 64 != H || !ptts_xfoldattn_ok(H, nh, mode) || (g->nur != 2 && g->nur != 4))
    return gvh_fail(PTTS_E_INVALID, "gvh_xfoldattn: mode=%d H=%d heads=%d nur=%d", mode, H, nh, g->nur);
  // Mw rows [0, heads * 64) of H elements; Uw rows [0, H) of heads * 64 elements (grid.y * nur * rows per round = H); xpart[h * H + n]; mask[lane], lane < 64
  const long long mat = (long long)nh * 64 * H;
  if (!g->Mw || !g->Uw || g->n_Mw < mat || g->n_Uw < mat || !g->xpart || g->n_xpart < (long long)nh * H || (g->mask && g->n_mask < 64))
    return gvh_fail(PTTS_E_INVALID, "gvh_xfoldattn: Mw %lld Uw %lld of %lld elements, xpart %lld, mask %lld", g->n_Mw, g->n_Uw, mat, g->n_xpart, g->n_mask);
  if (!g->x || !g->gamma || !g->beta || !g->n_valid || g->n_x < H || g->n_gamma < H) return gvh_fail(PTTS_E_INVALID, "gvh_xfoldattn: x %lld gamma %lld H=%d", g->n_x, g->n_gamma, H);
  XfoldAttnArgs a = {};
  a.Mw = g->Mw; a.Uw = g->Uw; a.x = g->x; a.gamma = g->gamma; a.beta = g->beta; a.n_valid = g->n_valid; a.nheads = nh; a.H = H; a.mask = g->mask; a.xpart = g->xpart; a.nur = g->nur;
  return gvh_status(ptts_xfoldattn_launch(mode, a, reinterpret_cast<hipStream_t>(stream)), "ptts_xfoldattn_launch");
}

GVH_API int gvh_xqattn(const GvhXq* g, void* stream) {
  if (!g) return gvh_fail(PTTS_E_INVALID, "gvh_xqattn: null arguments");
  const int M = g->M, H = g->H, nh = g->nheads, nkv = g->kv_heads, mode = g->mode;
  if (!mode_ok(mode) || !ptts_xqattn_ok(H, mode) || M < 1 || M > GV_MAX_ROWS || (mode == GV_F32 && M != 1) || nh <= 0 || nh * 64 != H || nkv <= 0 || nh % nkv)
    return gvh_fail(PTTS_E_INVALID, "gvh_xqattn: mode=%d H=%d M=%d heads=%d kv_heads=%d", mode, H, M, nh, nkv);
  if (!g->W || g->n_W < (long long)H * H * (mode == GV_BF16_W8 ? 1 : esize(mode)) || (mode == GV_BF16_W8 && (!g->wscale || g->n_wscale < H)))
    return gvh_fail(PTTS_E_INVALID, "gvh_xqattn: W holds %lld bytes, wscale %lld, H=%d", g->n_W, g->n_wscale, H);
  if (!g->x || !g->gamma || !g->beta || g->n_gamma < H || g->x_ld < H || g->x_ld % 4 || g->n_x < (long long)(M - 1) * g->x_ld + H)
    return gvh_fail(PTTS_E_INVALID, "gvh_xqattn: x %lld x_ld=%d gamma %lld H=%d", g->n_x, g->x_ld, g->n_gamma, H);
  // the first K/V batch fetches rows below cap of [M][kv_heads][cap][64] and mask entries below mask_ld; out[b * out_ld + col], col < H
  if (!g->kcache || !g->vcache || g->cap <= 0 || g->n_cache < (long long)M * nkv * g->cap * 64 || (g->mask && (g->mask_ld <= 0 || g->n_mask < (long long)M * g->mask_ld)))
    return gvh_fail(PTTS_E_INVALID, "gvh_xqattn: cache %lld for M=%d kv_heads=%d cap=%d; mask %lld x mask_ld=%d", g->n_cache, M, nkv, g->cap, g->n_mask, g->mask_ld);
  if (!g->out || g->out_ld < H || g->n_out < (long long)(M - 1) * g->out_ld + H) return gvh_fail(PTTS_E_INVALID, "gvh_xqattn: out %lld out_ld=%d H=%d M=%d", g->n_out, g->out_ld, H, M);
  // later batches read K/V rows and mask entries below the description length
  int L = 0;
  if (!g->n_valid) return gvh_fail(PTTS_E_INVALID, "gvh_xqattn: n_valid is null");
  if (!read_ints(g->n_valid, 1, &L)) return gvh_fail(GVH_E_HIP, "gvh_xqattn: n_valid could not be read");
  if (L < 0 || L > g->cap || (g->mask && L > g->mask_ld)) return gvh_fail(PTTS_E_INVALID, "gvh_xqattn: description length %d, cap=%d mask_ld=%d", L, g->cap, g->mask_ld);
  XqAttnArgs a = {};
  a.W = g->W; a.wscale = g->wscale; a.x = g->x; a.gamma = g->gamma; a.beta = g->beta; a.kcache = g->kcache; a.vcache = g->vcache; a.mask = g->mask; a.n_valid = g->n_valid;
  a.out = g->out; a.x_ld = g->x_ld; a.out_ld = g->out_ld; a.mask_ld = g->mask_ld; a.cap = g->cap; a.nheads = nh; a.H = H; a.kv_heads = nkv; a.M = M; a.scale = g->scale;
  return gvh_status(ptts_xqattn_launch(mode, a, reinterpret_cast<hipStream_t>(stream)), "ptts_xqattn_launch");
}
