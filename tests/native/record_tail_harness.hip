// Test-only harness of the step records (tests/test_record_tail_gpu.py): the RECORD instances of the sampler tail (tail_record_kernel /
// tail_warp_record_kernel<NV, SESSION>) through tail_launch, and the raw-logits node (step_logits_record_kernel) through
// step_logits_record_launch - the two functions the engine calls. A null `rec` launches the instances without the feature on the same operands.
// No kernel code of its own: the records are written by the product's set_step_record_kernel / set_warp_kernel / set_slot_gen_kernel.
// Built by the tests with build()'s hipcc flags as one translation unit. Every entry returns a PTTS_* status; the message is in rh_last_error().
#include "ptts_common.h"
#include "ptts_lm_kernels.h"
#include "ptts_tail_launch.h"
#include "ptts_step_record_launch.h"

#define RH_API extern "C" __attribute__((visibility("default")))

struct RhArgs {
  const float* logits;      // [B][K][V]
  long long* ids;           // [B*K][ids_ld]
  int* cur_len;             // [B]
  int* unfinished;          // [B*K]
  int* has_eos;             // [B*K]
  int* first_unf;           // [B]
  const void* gen;          // DevGen
  const void* dims;         // DevDims
  const int* row_maxlen;    // [B], session launches only
  const void* slot_gen;     // [B] SlotGen, session launches only, or null
  const int* slot_tprefix;  // [B] voice-prompt frames per slot, session launches only, or null
  const void* warp;         // [B] DevWarp, or null: the instances without the warpers
  const void* rec;          // [B] StepRecord, or null: the instances without the records
  const float* tables;      // [K][V+1][H] fp32, or null: no embedding of the next column
  const float* pos_table;   // or null
  float* h;                 // [B][H]
  int ids_ld, B, K, V, eos, pad, H, bos;
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

static int rh_launched(const char* what) {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? PTTS_OK : ptts_fail(PTTS_E_HIP, "%s launch failed: %s", what, hipGetErrorString(e));
}

static int rh_check(const RhArgs* g, const char* what) {
  if (!g->logits || !g->dims || !g->cur_len || !g->unfinished) return ptts_fail(PTTS_E_INVALID, "%s: null pointer", what);
  if (g->B <= 0 || g->K <= 0 || g->K > 32 || g->V <= 0 || g->V > PTTS_SORT_N || (g->session && !g->row_maxlen) || g->grid <= 0 || g->row0 < 0 ||
      g->row0 + g->grid > g->B || (!g->session && (g->row0 || g->grid != g->B)))
    return ptts_fail(PTTS_E_INVALID, "%s: B=%d K=%d V=%d session=%d grid=%d row0=%d", what, g->B, g->K, g->V, g->session, g->grid, g->row0);
  return PTTS_OK;
}

RH_API const char* rh_last_error(void) { return g_ptts_err.c_str(); }
// 0: RhArgs, 1: DevGen, 2: DevDims, 3: SlotGen, 4: DevWarp, 5: StepRecord
RH_API int rh_args_size(int which) {
  const int sz[6] = {(int)sizeof(RhArgs), (int)sizeof(DevGen), (int)sizeof(DevDims), (int)sizeof(SlotGen), (int)sizeof(DevWarp), (int)sizeof(StepRecord)};
  return which >= 0 && which < 6 ? sz[which] : -1;
}

RH_API int rh_tail(const RhArgs* g, void* stream) {
  if (int rc = rh_check(g, "rh_tail")) return rc;
  if (!g->gen || !g->ids || !g->has_eos || !g->first_unf || g->ids_ld <= 0) return ptts_fail(PTTS_E_INVALID, "rh_tail: null pointer");
  if (g->tables && (!g->h || g->H <= 0 || g->H % 4)) return ptts_fail(PTTS_E_INVALID, "rh_tail: tables without h, or H=%d", g->H);
  TailArgs t = {};
  t.logits = g->logits; t.ids = g->ids; t.ids_ld = g->ids_ld; t.cur_len = g->cur_len; t.unfinished = g->unfinished;
  t.has_eos = g->has_eos; t.first_unf = g->first_unf; t.gen = reinterpret_cast<const DevGen*>(g->gen);
  t.B = g->B; t.K = g->K; t.V = g->V; t.eos = g->eos; t.pad = g->pad;
  t.dims = reinterpret_cast<const DevDims*>(g->dims);
  t.tables = g->tables; t.pos_table = g->pos_table; t.h = g->h; t.H = g->H; t.bos = g->bos; t.bf16_tables = 0;
  tail_launch(t, g->session ? g->row_maxlen : nullptr, g->row0, dim3(g->grid), reinterpret_cast<hipStream_t>(stream),
              g->session ? reinterpret_cast<const SlotGen*>(g->slot_gen) : nullptr, g->session ? g->slot_tprefix : nullptr,
              reinterpret_cast<const DevWarp*>(g->warp), reinterpret_cast<const StepRecord*>(g->rec));
  return rh_launched("tail");
}

// the raw-logits node over the same operands, with the engine's choice of the voice-prompt source (a slot's own frames in a session, DevDims::T_prefix otherwise)
RH_API int rh_logits_record(const RhArgs* g, void* stream) {
  if (int rc = rh_check(g, "rh_logits_record")) return rc;
  if (!g->rec || (g->session && !g->slot_tprefix)) return ptts_fail(PTTS_E_INVALID, "rh_logits_record: null records or slot prefixes");
  LogitsRecordArgs r = {};
  r.logits = g->logits; r.cur_len = g->cur_len; r.unfinished = g->unfinished; r.rec = reinterpret_cast<const StepRecord*>(g->rec);
  r.t_prefix = g->session ? g->slot_tprefix : &reinterpret_cast<const DevDims*>(g->dims)->T_prefix; r.t_prefix_stride = g->session ? 1 : 0;
  r.B = g->B; r.K = g->K; r.V = g->V; r.session = g->session;
  if (!step_logits_record_launch(r, g->row0, g->grid, reinterpret_cast<hipStream_t>(stream))) return ptts_fail(PTTS_E_INVALID, "rh_logits_record: refused");
  return rh_launched("step_logits_record_kernel");
}

// set_step_record_kernel: records [row0, row0 + nrows), entry i = {scores + i per_row, logits + i per_row, cap_steps, step_stride} (null stays null)
RH_API int rh_set_step_record(void* recs, int row0, int nrows, float* scores, float* logits, int cap_steps, long long step_stride, long long per_row,
                              void* stream) {
  if (!recs || row0 < 0 || nrows <= 0) return ptts_fail(PTTS_E_INVALID, "rh_set_step_record: row0=%d nrows=%d", row0, nrows);
  hipLaunchKernelGGL(set_step_record_kernel, dim3((nrows + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<StepRecord*>(recs), row0, nrows, StepRecord{scores, logits, cap_steps, 0, step_stride}, per_row);
  return rh_launched("set_step_record_kernel");
}

RH_API int rh_set_warp(void* recs, int row0, int nrows, float min_p, float typical_p, float epsilon_cutoff, float eta_cutoff, void* stream) {
  if (!recs || row0 < 0 || nrows <= 0) return ptts_fail(PTTS_E_INVALID, "rh_set_warp: row0=%d nrows=%d", row0, nrows);
  hipLaunchKernelGGL(set_warp_kernel, dim3((nrows + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<DevWarp*>(recs), row0,
                     nrows, DevWarp{min_p, typical_p, epsilon_cutoff, eta_cutoff});
  return rh_launched("set_warp_kernel");
}

RH_API int rh_set_slot_gen(void* recs, int row, const void* gen, int row_base, void* stream) {
  if (!recs || row < 0) return ptts_fail(PTTS_E_INVALID, "rh_set_slot_gen: row=%d", row);
  SlotGen rec = {};
  if (gen) { rec.g = *reinterpret_cast<const DevGen*>(gen); rec.own = 1; rec.row_base = row_base; }
  hipLaunchKernelGGL(set_slot_gen_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<SlotGen*>(recs), row, 1, rec);
  return rh_launched("set_slot_gen_kernel");
}
