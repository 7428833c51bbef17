// Test-only harness of the sampler tail (tests/test_sampler_tail_gpu.py, tests/test_tail_harness_cpu.py).
// It includes the product headers and launches the product's own kernels - tail_kernel<NV, SESSION> through tail_launch (the function
// the engine calls), session_reset_rows_kernel and embed_kernel<WT, SESSION> - on device pointers that the test allocates with torch.
// No kernel code of its own. Built by the tests with build()'s hipcc flags as one translation unit.
// Every entry returns a PTTS_* status; the message is in th_last_error().
#include "ptts_common.h"
#include "ptts_lm_kernels.h"
#include "ptts_tail_launch.h"

#define TH_API extern "C" __attribute__((visibility("default")))

// the operands of one tail / embedding launch; DevGen and DevDims live in device memory, written by the test as raw bytes
struct ThArgs {
  const float* logits;    // [B][K][V]
  long long* ids;         // [B*K][ids_ld]
  int* cur_len;           // [B]
  int* unfinished;        // [B*K]
  int* has_eos;           // [B*K]
  int* first_unf;         // [B]
  const void* gen;        // DevGen
  const void* dims;       // DevDims
  const void* tables;     // [K][V+1][H] fp32 or bf16, or null: no embedding of the next column
  const float* pos_table; // [positions][H] or null
  float* h;               // [B][H]
  const int* row_maxlen;  // [B], session launches only
  int ids_ld, B, K, V, eos, pad, H, bos, bf16_tables;
  int session;            // 0: tail_kernel<NV, false> / embed_kernel<WT, false>; 1: the per-slot instances
  int row0, grid;         // th_tail: first slot and number of workgroups (static: row0 0)
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

static int th_launched(const char* what) {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? PTTS_OK : ptts_fail(PTTS_E_HIP, "%s launch failed: %s", what, hipGetErrorString(e));
}

TH_API const char* th_last_error(void) { return g_ptts_err.c_str(); }
// 0: ThArgs, 1: DevGen, 2: DevDims
TH_API int th_args_size(int which) { return which == 0 ? (int)sizeof(ThArgs) : which == 1 ? (int)sizeof(DevGen) : which == 2 ? (int)sizeof(DevDims) : -1; }

// (NV, SESSION) of every tail_kernel instance tail_launch can select, pair after pair; returns the number of instances
TH_API int th_tail_instances(int* out, int cap) {
  const int nv[3] = {8, 18, 32};
  int n = 0;
  for (int s = 0; s < 2; ++s)
    for (int i = 0; i < 3; ++i, ++n)
      if (n < cap) { out[2 * n] = nv[i]; out[2 * n + 1] = s; }
  return n;
}

static int th_check(const ThArgs& g, const char* who) {
  if (!g.gen || !g.dims || !g.ids || !g.cur_len || !g.unfinished || !g.has_eos || !g.first_unf) return ptts_fail(PTTS_E_INVALID, "%s: null state pointer", who);
  if (g.B <= 0 || g.K <= 0 || g.K > 32 || g.V <= 0 || g.V > PTTS_SORT_N || g.ids_ld <= 0 || (g.session && !g.row_maxlen) ||
      (g.tables && (g.H <= 0 || g.H % 4)))
    return ptts_fail(PTTS_E_INVALID, "%s: B=%d K=%d V=%d H=%d ids_ld=%d session=%d", who, g.B, g.K, g.V, g.H, g.ids_ld, g.session);
  return PTTS_OK;
}

// tail_launch: the engine's instance choice on the caller's grid - (B, row0 0) is a decode step, (1, slot) a session admission
TH_API int th_tail(const ThArgs* g, void* stream) {
  if (int rc = th_check(*g, "th_tail")) return rc;
  if (g->grid <= 0 || g->row0 < 0 || g->row0 + g->grid > g->B || (!g->session && g->row0))
    return ptts_fail(PTTS_E_INVALID, "th_tail: grid=%d row0=%d B=%d session=%d", g->grid, g->row0, g->B, g->session);
  TailArgs t = {};
  t.logits = g->logits; t.ids = g->ids; t.ids_ld = g->ids_ld; t.cur_len = g->cur_len; t.unfinished = g->unfinished;
  t.has_eos = g->has_eos; t.first_unf = g->first_unf; t.gen = reinterpret_cast<const DevGen*>(g->gen);
  t.B = g->B; t.K = g->K; t.V = g->V; t.eos = g->eos; t.pad = g->pad;
  t.dims = reinterpret_cast<const DevDims*>(g->dims);
  if (g->tables) { t.tables = g->tables; t.pos_table = g->pos_table; t.h = g->h; t.H = g->H; t.bos = g->bos; t.bf16_tables = g->bf16_tables; }
  tail_launch(t, g->session ? g->row_maxlen : nullptr, g->row0, dim3(g->grid), reinterpret_cast<hipStream_t>(stream));
  return th_launched("tail_kernel");
}

// session_reset_rows_kernel on slots [row0, row0 + nrows): live = 1 with the request's max_length admits, live = 0 retires
TH_API int th_reset_rows(const ThArgs* g, int* row_maxlen, int row0, int nrows, int live, int max_length, void* stream) {
  if (int rc = th_check(*g, "th_reset_rows")) return rc;
  if (nrows <= 0 || row0 < 0 || row0 + nrows > g->B) return ptts_fail(PTTS_E_INVALID, "th_reset_rows: row0=%d nrows=%d B=%d", row0, nrows, g->B);
  hipLaunchKernelGGL(session_reset_rows_kernel, dim3((nrows * g->K + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), g->ids,
                     g->ids_ld, g->cur_len, g->unfinished, g->has_eos, g->first_unf, row_maxlen, row0, nrows, g->K, g->bos, live, max_length);
  return th_launched("session_reset_rows_kernel");
}

// embed_kernel<float | bf16_t, SESSION> of the decode step: h[b] = embedding of column cur_len[b] - 1, for every b < B
TH_API int th_embed(const ThArgs* g, void* stream) {
  if (int rc = th_check(*g, "th_embed")) return rc;
  if (!g->tables || !g->h) return ptts_fail(PTTS_E_INVALID, "th_embed: no tables");
  EmbedArgs ea = {};
  ea.tables = g->tables; ea.pos_table = g->pos_table; ea.ids = g->ids; ea.ids_ld = g->ids_ld; ea.cur_len = g->cur_len;
  ea.dims = reinterpret_cast<const DevDims*>(g->dims); ea.h = g->h;
  ea.H = g->H; ea.K = g->K; ea.V1 = g->V + 1; ea.bos = g->bos; ea.pad = g->pad; ea.prefill = 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(1, g->B), block(256);
  if (g->session) {
    const EmbedSessionArgs es{ea, g->row_maxlen};
    if (g->bf16_tables) hipLaunchKernelGGL((embed_kernel<bf16_t, true>), grid, block, 0, st, es);
    else hipLaunchKernelGGL((embed_kernel<float, true>), grid, block, 0, st, es);
  } else {
    if (g->bf16_tables) hipLaunchKernelGGL((embed_kernel<bf16_t, false>), grid, block, 0, st, ea);
    else hipLaunchKernelGGL((embed_kernel<float, false>), grid, block, 0, st, ea);
  }
  return th_launched("embed_kernel");
}
