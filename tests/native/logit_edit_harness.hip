// Test-only harness of the logit-edit node (tests/test_logit_edit_kernel_gpu.py, tests/test_logit_edit_abi_cpu.py).
// It includes the product headers and launches the product's own logit_edit_kernel through logit_edit_launch (the function the engine calls)
// and copy_logit_edit_kernel, on device pointers that the test allocates with torch. No kernel code of its own. Built by the tests with
// build()'s hipcc flags as one translation unit. Every entry returns a PTTS_* status; the message is in lh_last_error().
#include "ptts_common.h"
#include "ptts_logit_edit_launch.h"

#define LH_API extern "C" __attribute__((visibility("default")))

// the operands of one launch; the records live in device memory, written by the test in the layout of LogitEditRecs
struct LhArgs {
  float* logits;         // [B][K][V]
  const int* cur_len;    // [B]
  const int* t_prefix;   // [B] voice-prompt frames (stride 1), or one value for the batch (stride 0)
  void* hdr;             // LogitEditHeader [nrec]
  float* bias;           // [nrec][ld_v]
  float* decay;          // [nrec][ld_t]
  unsigned char* flags;  // [nrec][ld_v]
  int ld_v, ld_t, t_prefix_stride, B, K, V, eos;
  int row0, nb;          // utterances [row0, row0 + nb): (0, B) is a decode step, (slot, 1) a session admission
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

static int lh_launched(const char* what) {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? PTTS_OK : ptts_fail(PTTS_E_HIP, "%s launch failed: %s", what, hipGetErrorString(e));
}

static LogitEditRecs lh_recs(const LhArgs* g) {
  LogitEditRecs r = {};
  r.hdr = reinterpret_cast<LogitEditHeader*>(g->hdr); r.bias = g->bias; r.decay = g->decay; r.flags = g->flags; r.ld_v = g->ld_v; r.ld_t = g->ld_t;
  return r;
}

LH_API const char* lh_last_error(void) { return g_ptts_err.c_str(); }
// 0: LhArgs, 1: LogitEditHeader, 2: the widest vocabulary logit_edit_launch serves
LH_API int lh_args_size(int which) {
  return which == 0 ? (int)sizeof(LhArgs) : which == 1 ? (int)sizeof(LogitEditHeader) : which == 2 ? PTTS_LOGIT_EDIT_MAX_V : -1;
}

// copy_logit_edit_kernel: records [dst0, dst0 + n) = record src (the engine's "restore the default"); the caller's arrays hold > max(src, dst0 + n - 1) records
LH_API int lh_copy_records(const LhArgs* g, int src, int dst0, int n, void* stream) {
  if (!g->hdr || !g->bias || !g->decay || !g->flags || src < 0 || dst0 < 0 || n <= 0) return ptts_fail(PTTS_E_INVALID, "lh_copy_records: src=%d dst0=%d n=%d", src, dst0, n);
  hipLaunchKernelGGL(copy_logit_edit_kernel, dim3(4, n), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), lh_recs(g), src, dst0);
  return lh_launched("copy_logit_edit_kernel");
}

// logit_edit_launch on the caller's utterance range
LH_API int lh_logit_edit(const LhArgs* g, void* stream) {
  if (!g->logits || !g->cur_len || !g->t_prefix || !g->hdr || !g->bias || !g->decay || !g->flags) return ptts_fail(PTTS_E_INVALID, "lh_logit_edit: null pointer");
  if (g->B <= 0 || g->nb <= 0 || g->row0 < 0 || g->row0 + g->nb > g->B)
    return ptts_fail(PTTS_E_INVALID, "lh_logit_edit: row0=%d nb=%d B=%d", g->row0, g->nb, g->B);
  LogitEditArgs a = {};
  a.logits = g->logits; a.cur_len = g->cur_len; a.t_prefix = g->t_prefix; a.t_prefix_stride = g->t_prefix_stride; a.recs = lh_recs(g);
  a.K = g->K; a.V = g->V; a.eos = g->eos;
  if (!logit_edit_launch(a, g->row0, g->nb, reinterpret_cast<hipStream_t>(stream)))
    return ptts_fail(PTTS_E_UNSUPPORTED, "lh_logit_edit: no kernel for K=%d V=%d ld_v=%d ld_t=%d", g->K, g->V, g->ld_v, g->ld_t);
  return lh_launched("logit_edit_kernel");
}
