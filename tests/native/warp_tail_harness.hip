// Test-only harness of the WARP instances of the sampler tail (tests/test_warp_tail_gpu.py): tail_warp_kernel<NV, SESSION> through tail_launch,
// the function the engine calls, with the per-utterance warper records (DevWarp) and, in a session, the per-slot sampler records (SlotGen).
// A null `warp` launches tail_kernel<NV, SESSION> on the same operands. No kernel code of its own: the records are written by the product's
// set_warp_kernel / set_slot_gen_kernel. Built by the tests with build()'s hipcc flags as one translation unit.
// Every entry returns a PTTS_* status; the message is in wh_last_error().
#include "ptts_common.h"
#include "ptts_lm_kernels.h"
#include "ptts_tail_launch.h"

#define WH_API extern "C" __attribute__((visibility("default")))

struct WhArgs {
  const float* logits;    // [B][K][V]
  long long* ids;         // [B*K][ids_ld]
  int* cur_len;           // [B]
  int* unfinished;        // [B*K]
  int* has_eos;           // [B*K]
  int* first_unf;         // [B]
  const void* gen;        // DevGen
  const void* dims;       // DevDims
  const int* row_maxlen;  // [B], session launches only
  const void* slot_gen;   // [B] SlotGen, session launches only, or null
  const void* warp;       // [B] DevWarp, or null: the instances without the feature
  int ids_ld, B, K, V, eos, pad;
  int session, row0, grid;
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

static int wh_launched(const char* what) {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? PTTS_OK : ptts_fail(PTTS_E_HIP, "%s launch failed: %s", what, hipGetErrorString(e));
}

WH_API const char* wh_last_error(void) { return g_ptts_err.c_str(); }
// 0: WhArgs, 1: DevGen, 2: DevDims, 3: SlotGen, 4: DevWarp
WH_API int wh_args_size(int which) {
  const int sz[5] = {(int)sizeof(WhArgs), (int)sizeof(DevGen), (int)sizeof(DevDims), (int)sizeof(SlotGen), (int)sizeof(DevWarp)};
  return which >= 0 && which < 5 ? sz[which] : -1;
}

WH_API int wh_tail(const WhArgs* g, void* stream) {
  if (!g->logits || !g->gen || !g->dims || !g->ids || !g->cur_len || !g->unfinished || !g->has_eos || !g->first_unf)
    return ptts_fail(PTTS_E_INVALID, "wh_tail: null pointer");
  if (g->B <= 0 || g->K <= 0 || g->K > 32 || g->V <= 0 || g->V > PTTS_SORT_N || g->ids_ld <= 0 || (g->session && !g->row_maxlen) || g->grid <= 0 ||
      g->row0 < 0 || g->row0 + g->grid > g->B || (!g->session && g->row0))
    return ptts_fail(PTTS_E_INVALID, "wh_tail: B=%d K=%d V=%d ids_ld=%d session=%d grid=%d row0=%d", g->B, g->K, g->V, g->ids_ld, g->session, g->grid, g->row0);
  TailArgs t = {};
  t.logits = g->logits; t.ids = g->ids; t.ids_ld = g->ids_ld; t.cur_len = g->cur_len; t.unfinished = g->unfinished;
  t.has_eos = g->has_eos; t.first_unf = g->first_unf; t.gen = reinterpret_cast<const DevGen*>(g->gen);
  t.B = g->B; t.K = g->K; t.V = g->V; t.eos = g->eos; t.pad = g->pad;
  t.dims = reinterpret_cast<const DevDims*>(g->dims);  // no tables: no embedding of the next column
  tail_launch(t, g->session ? g->row_maxlen : nullptr, g->row0, dim3(g->grid), reinterpret_cast<hipStream_t>(stream),
              g->session ? reinterpret_cast<const SlotGen*>(g->slot_gen) : nullptr, nullptr, reinterpret_cast<const DevWarp*>(g->warp));
  return wh_launched("tail_kernel");
}

// set_warp_kernel: the records of [row0, row0 + nrows)
WH_API int wh_set_warp(void* recs, int row0, int nrows, float min_p, float typical_p, float epsilon_cutoff, float eta_cutoff, void* stream) {
  if (!recs || row0 < 0 || nrows <= 0) return ptts_fail(PTTS_E_INVALID, "wh_set_warp: row0=%d nrows=%d", row0, nrows);
  hipLaunchKernelGGL(set_warp_kernel, dim3((nrows + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<DevWarp*>(recs), row0,
                     nrows, DevWarp{min_p, typical_p, epsilon_cutoff, eta_cutoff});
  return wh_launched("set_warp_kernel");
}

// set_slot_gen_kernel: the sampler record of one slot (gen: a host DevGen; own = 1) or, gen == null, no record of its own
WH_API int wh_set_slot_gen(void* recs, int row, const void* gen, int row_base, void* stream) {
  if (!recs || row < 0) return ptts_fail(PTTS_E_INVALID, "wh_set_slot_gen: row=%d", row);
  SlotGen rec = {};
  if (gen) { rec.g = *reinterpret_cast<const DevGen*>(gen); rec.own = 1; rec.row_base = row_base; }
  hipLaunchKernelGGL(set_slot_gen_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<SlotGen*>(recs), row, 1, rec);
  return wh_launched("set_slot_gen_kernel");
}
