// Test-only harness of the history-penalty node (tests/test_history_penalty_kernel_gpu.py, tests/test_penalty_abi_cpu.py).
// It includes the product headers and launches the product's own history_penalty_kernel through penalty_launch (the function the engine
// calls) and set_penalty_kernel, on device pointers that the test allocates with torch. No kernel code of its own. Built by the tests with
// build()'s hipcc flags as one translation unit. Every entry returns a PTTS_* status; the message is in ph_last_error().
#include "ptts_common.h"
#include "ptts_penalty_launch.h"

#define PH_API extern "C" __attribute__((visibility("default")))

// the operands of one launch; the records live in device memory, written through ph_set_records
struct PhArgs {
  float* logits;         // [B][K][V]
  const long long* ids;  // [B*K][ids_ld]
  const int* cur_len;    // [B]
  void* pen;             // HistoryPenalty [B]
  int ids_ld, B, K, V;
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

static int ph_launched(const char* what) {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? PTTS_OK : ptts_fail(PTTS_E_HIP, "%s launch failed: %s", what, hipGetErrorString(e));
}

PH_API const char* ph_last_error(void) { return g_ptts_err.c_str(); }
// 0: PhArgs, 1: HistoryPenalty, 2: the widest vocabulary penalty_launch serves
PH_API int ph_args_size(int which) { return which == 0 ? (int)sizeof(PhArgs) : which == 1 ? (int)sizeof(HistoryPenalty) : which == 2 ? PTTS_PENALTY_MAX_V : -1; }

// set_penalty_kernel: records [row0, row0 + nrows) = (repetition_penalty, no_repeat_ngram)
PH_API int ph_set_records(void* pen, int row0, int nrows, float repetition_penalty, int no_repeat_ngram, void* stream) {
  if (!pen || row0 < 0 || nrows <= 0) return ptts_fail(PTTS_E_INVALID, "ph_set_records: row0=%d nrows=%d", row0, nrows);
  hipLaunchKernelGGL(set_penalty_kernel, dim3((nrows + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<HistoryPenalty*>(pen), row0, nrows, HistoryPenalty{repetition_penalty, no_repeat_ngram});
  return ph_launched("set_penalty_kernel");
}

// penalty_launch on the caller's utterance range
PH_API int ph_penalty(const PhArgs* g, void* stream) {
  if (!g->logits || !g->ids || !g->cur_len || !g->pen) return ptts_fail(PTTS_E_INVALID, "ph_penalty: null pointer");
  if (g->B <= 0 || g->nb <= 0 || g->row0 < 0 || g->row0 + g->nb > g->B)
    return ptts_fail(PTTS_E_INVALID, "ph_penalty: row0=%d nb=%d B=%d", g->row0, g->nb, g->B);
  PenaltyArgs p = {};
  p.logits = g->logits; p.ids = g->ids; p.cur_len = g->cur_len; p.pen = reinterpret_cast<const HistoryPenalty*>(g->pen);
  p.ids_ld = g->ids_ld; p.K = g->K; p.V = g->V;
  if (!penalty_launch(p, g->row0, g->nb, reinterpret_cast<hipStream_t>(stream)))
    return ptts_fail(PTTS_E_UNSUPPORTED, "ph_penalty: no kernel for K=%d V=%d ids_ld=%d", g->K, g->V, g->ids_ld);
  return ph_launched("history_penalty_kernel");
}
