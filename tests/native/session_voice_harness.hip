// Test-only harness of the per-slot voice-prompt length of a continuous session (tests/test_session_voice_tail_gpu.py). Next to
// slot_gen_harness.hip, which keeps launching tail_launch with its six arguments: this one passes the seventh (the per-slot prefix lengths)
// and launches the product's kernels that a voice admission runs on the sampler state (admit_voice_slots_kernel with a list of
// one; fill_int_kernel). No kernel code of its own. Built by the tests with build()'s hipcc flags as one translation unit. Every entry returns a
// PTTS_* status; the message is in sv_last_error().
#include "ptts_common.h"
#include "ptts_lm_kernels.h"
#include "ptts_tail_launch.h"

#define SV_API extern "C" __attribute__((visibility("default")))

// struct ThArgs of tail_harness.hip, field for field (tests/tail_harness.py::ThArgs describes both)
struct ThArgs {
  const float* logits;
  long long* ids;
  int* cur_len;
  int* unfinished;
  int* has_eos;
  int* first_unf;
  const void* gen;
  const void* dims;
  const void* tables;
  const float* pos_table;
  float* h;
  const int* row_maxlen;
  int ids_ld, B, K, V, eos, pad, H, bos, bf16_tables;
  int session;
  int row0, grid;
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

static int sv_launched(const char* what) {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? PTTS_OK : ptts_fail(PTTS_E_HIP, "%s launch failed: %s", what, hipGetErrorString(e));
}

SV_API const char* sv_last_error(void) { return g_ptts_err.c_str(); }
// 0: ThArgs, 1: DevGen, 2: DevDims, 3: SlotGen (its 48 bytes are part of the contract), 4: TailSessionArgs, 5: EmbedSessionArgs
SV_API int sv_args_size(int which) {
  return which == 0 ? (int)sizeof(ThArgs) : which == 1 ? (int)sizeof(DevGen) : which == 2 ? (int)sizeof(DevDims) : which == 3 ? (int)sizeof(SlotGen)
       : which == 4 ? (int)sizeof(TailSessionArgs) : which == 5 ? (int)sizeof(EmbedSessionArgs) : -1;
}

// tail_launch on the session instances with the per-slot prefix lengths (slot_gen may be null): (B, row0 0) is a decode step, (1, slot) an admission
SV_API int sv_tail(const ThArgs* g, const void* slot_gen, const int* slot_tprefix, void* stream) {
  if (!g->gen || !g->dims || !g->ids || !g->cur_len || !g->unfinished || !g->has_eos || !g->first_unf || !g->row_maxlen)
    return ptts_fail(PTTS_E_INVALID, "sv_tail: null state pointer");
  if (!g->session || g->B <= 0 || g->K <= 0 || g->K > 32 || g->V <= 0 || g->V > PTTS_SORT_N || g->ids_ld <= 0 || (g->tables && (g->H <= 0 || g->H % 4)) ||
      g->grid <= 0 || g->row0 < 0 || g->row0 + g->grid > g->B)
    return ptts_fail(PTTS_E_INVALID, "sv_tail: B=%d K=%d V=%d H=%d ids_ld=%d session=%d grid=%d row0=%d", g->B, g->K, g->V, g->H, g->ids_ld, g->session,
                     g->grid, g->row0);
  TailArgs t = {};
  t.logits = g->logits; t.ids = g->ids; t.ids_ld = g->ids_ld; t.cur_len = g->cur_len; t.unfinished = g->unfinished;
  t.has_eos = g->has_eos; t.first_unf = g->first_unf; t.gen = reinterpret_cast<const DevGen*>(g->gen);
  t.B = g->B; t.K = g->K; t.V = g->V; t.eos = g->eos; t.pad = g->pad;
  t.dims = reinterpret_cast<const DevDims*>(g->dims);
  if (g->tables) { t.tables = g->tables; t.pos_table = g->pos_table; t.h = g->h; t.H = g->H; t.bos = g->bos; t.bf16_tables = g->bf16_tables; }
  tail_launch(t, g->row_maxlen, g->row0, dim3(g->grid), reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const SlotGen*>(slot_gen), slot_tprefix);
  return sv_launched("tail_kernel");
}

// embed_kernel<float, true> of every slot's last column with the per-slot prefix lengths (the manual path's embedding), into g->h
SV_API int sv_embed(const ThArgs* g, const int* slot_tprefix, void* stream) {
  if (!g->dims || !g->ids || !g->cur_len || !g->row_maxlen || !g->tables || !g->h || g->bf16_tables || g->B <= 0 || g->K <= 0 || g->K > 32 || g->H <= 0)
    return ptts_fail(PTTS_E_INVALID, "sv_embed: fp32 tables and the session state are required");
  EmbedArgs ea = {};
  ea.tables = g->tables; ea.pos_table = g->pos_table; ea.ids = g->ids; ea.ids_ld = g->ids_ld; ea.cur_len = g->cur_len;
  ea.dims = reinterpret_cast<const DevDims*>(g->dims); ea.h = g->h; ea.H = g->H; ea.K = g->K; ea.V1 = g->V + 1; ea.bos = g->bos; ea.pad = g->pad;
  hipLaunchKernelGGL((embed_kernel<float, true>), dim3(1, g->B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     EmbedSessionArgs{ea, g->row_maxlen, slot_tprefix});
  return sv_launched("embed_kernel");
}

// What a voice admission runs on the sampler state of slot `row` behind its session_reset_rows_kernel: the id columns 1..T from the slot's
// prefix rows (`prefix` [B*K][prefix_ld], already holding the codes), the slot's prefix length, and its clock at T + 1. T == 0 only writes the length
// (what ptts_retire_row and session begin do).
SV_API int sv_set_prefix(const ThArgs* g, const long long* prefix, int prefix_ld, int* slot_tprefix, int row, int T, int max_length, void* stream) {
  if (!g->ids || !g->cur_len || !slot_tprefix || row < 0 || row >= g->B || T < 0 || (T > 0 && (!prefix || T > prefix_ld || T + 1 >= g->ids_ld)))
    return ptts_fail(PTTS_E_INVALID, "sv_set_prefix: row=%d T=%d B=%d prefix_ld=%d ids_ld=%d", row, T, g->B, prefix_ld, g->ids_ld);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (T == 0) {
    hipLaunchKernelGGL(fill_int_kernel, dim3(1), dim3(64), 0, st, slot_tprefix + row, 0, (size_t)1);
    return sv_launched("fill_int_kernel");
  }
  static DevDims* row_dims = nullptr;  // the kernel also writes the DevDims of the admission's prefill pass: nobody reads them here
  if (!row_dims && hipMalloc(reinterpret_cast<void**>(&row_dims), sizeof(DevDims)) != hipSuccess) return ptts_fail(PTTS_E_HIP, "sv_set_prefix: hipMalloc failed");
  AdmitVoiceSlotsArgs a = {};
  a.ids = g->ids; a.prefix = prefix; a.slot_T = slot_tprefix; a.cur_len = g->cur_len; a.row_dims = row_dims;
  a.ids_ld = g->ids_ld; a.prefix_ld = prefix_ld; a.K = g->K; a.bos = g->bos; a.pad = g->pad;
  a.rows[0] = row; a.Ts[0] = T; a.Ls[0] = max_length;
  hipLaunchKernelGGL(admit_voice_slots_kernel, dim3((g->K * T + 255) / 256, 1), dim3(256), 0, st, a);
  return sv_launched("admit_voice_slots_kernel");
}
