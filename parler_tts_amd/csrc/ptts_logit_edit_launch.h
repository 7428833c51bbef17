// Host-side launch of the logit-edit node (logit_edit_kernel, ptts_logit_edit_kernels.h). Shared by the engine (launch_tail, ptts_lm.hip) and
// the test harness (tests/native/logit_edit_harness.hip), so that a test of the kernel runs the grid and the argument struct the product would run
// for the same (K, V).
#pragma once
#include "ptts_logit_edit_kernels.h"

// Utterances [row0, row0 + nb) of the arrays in `a` (a.row0 is overwritten): nb = B with row0 0 for a prefill tail or a decode step, nb = 1 with
// row0 = the slot for a session admission. One workgroup per codebook row. Returns false, launching nothing, for a shape the kernel does not
// serve (a vocabulary wider than its threads' share, or wider than a record's rows).
static inline bool logit_edit_launch(LogitEditArgs a, int row0, int nb, hipStream_t st) {
  if (a.V < 1 || a.V > PTTS_LOGIT_EDIT_MAX_V || a.V > a.recs.ld_v || a.K < 1 || nb < 1 || row0 < 0 || a.recs.ld_t < 1 || a.t_prefix_stride < 0) return false;
  a.row0 = row0;
  hipLaunchKernelGGL(logit_edit_kernel, dim3(a.K, nb), dim3(PTTS_LOGIT_EDIT_THREADS), 0, st, a);
  return true;
}
