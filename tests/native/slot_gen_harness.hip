// Test-only harness of the per-slot sampler records of a continuous session (tests/test_slot_gen_tail_gpu.py, tests/test_slot_gen_cpu.py).
// Next to tail_harness.hip, which keeps launching tail_launch with its five arguments: this one passes the record pointer (the sixth) and
// launches the product's record-writing kernel, set_slot_gen_kernel. No kernel code of its own. Built by the tests with build()'s hipcc flags
// as one translation unit. Every entry returns a PTTS_* status; the message is in sg_last_error().
#include "ptts_common.h"
#include "ptts_lm_kernels.h"
#include "ptts_tail_launch.h"

#define SG_API extern "C" __attribute__((visibility("default")))

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

static int sg_launched(const char* what) {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? PTTS_OK : ptts_fail(PTTS_E_HIP, "%s launch failed: %s", what, hipGetErrorString(e));
}

SG_API const char* sg_last_error(void) { return g_ptts_err.c_str(); }
// 0: ThArgs, 1: DevGen, 2: SlotGen
SG_API int sg_args_size(int which) { return which == 0 ? (int)sizeof(ThArgs) : which == 1 ? (int)sizeof(DevGen) : which == 2 ? (int)sizeof(SlotGen) : -1; }

// tail_launch on the session instances with the per-slot records: (B, row0 0) is a decode step, (1, slot) an admission
SG_API int sg_tail(const ThArgs* g, const void* slot_gen, void* stream) {
  if (!g->gen || !g->dims || !g->ids || !g->cur_len || !g->unfinished || !g->has_eos || !g->first_unf || !g->row_maxlen || !slot_gen)
    return ptts_fail(PTTS_E_INVALID, "sg_tail: null state pointer");
  if (!g->session || g->B <= 0 || g->K <= 0 || g->K > 32 || g->V <= 0 || g->V > PTTS_SORT_N || g->ids_ld <= 0 || (g->tables && (g->H <= 0 || g->H % 4)) ||
      g->grid <= 0 || g->row0 < 0 || g->row0 + g->grid > g->B)
    return ptts_fail(PTTS_E_INVALID, "sg_tail: B=%d K=%d V=%d H=%d ids_ld=%d session=%d grid=%d row0=%d", g->B, g->K, g->V, g->H, g->ids_ld, g->session,
                     g->grid, g->row0);
  TailArgs t = {};
  t.logits = g->logits; t.ids = g->ids; t.ids_ld = g->ids_ld; t.cur_len = g->cur_len; t.unfinished = g->unfinished;
  t.has_eos = g->has_eos; t.first_unf = g->first_unf; t.gen = reinterpret_cast<const DevGen*>(g->gen);
  t.B = g->B; t.K = g->K; t.V = g->V; t.eos = g->eos; t.pad = g->pad;
  t.dims = reinterpret_cast<const DevDims*>(g->dims);
  if (g->tables) { t.tables = g->tables; t.pos_table = g->pos_table; t.h = g->h; t.H = g->H; t.bos = g->bos; t.bf16_tables = g->bf16_tables; }
  tail_launch(t, g->row_maxlen, g->row0, dim3(g->grid), reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const SlotGen*>(slot_gen));
  return sg_launched("tail_kernel");
}

// set_slot_gen_kernel on slots [row0, row0 + nrows) of the B records at `slot_gen`: gen (a HOST DevGen) with own = 1 and row_base 0 is what
// ptts_admit_row_gen writes for one slot; gen == NULL writes the cleared record (session begin, ptts_retire_row)
SG_API int sg_set_slots(void* slot_gen, int B, int row0, int nrows, const void* gen, void* stream) {
  if (!slot_gen || nrows <= 0 || row0 < 0 || row0 + nrows > B) return ptts_fail(PTTS_E_INVALID, "sg_set_slots: row0=%d nrows=%d B=%d", row0, nrows, B);
  SlotGen rec = {};
  if (gen) { rec.g = *reinterpret_cast<const DevGen*>(gen); rec.own = 1; rec.row_base = 0; }
  hipLaunchKernelGGL(set_slot_gen_kernel, dim3((nrows + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<SlotGen*>(slot_gen), row0, nrows, rec);
  return sg_launched("set_slot_gen_kernel");
}
