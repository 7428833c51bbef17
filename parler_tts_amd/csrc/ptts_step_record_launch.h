// Host-side launch of the raw-logits record node (step_logits_record_kernel, ptts_step_record_kernels.h). Shared by the engine (launch_tail,
// ptts_lm.hip) and the test harness (tests/native/record_tail_harness.hip), so that a test of the kernel runs the grid and the argument struct the
// product would run for the same (B, K, V).
#pragma once
#include "ptts_step_record_kernels.h"

// Utterances [row0, row0 + nb) of the arrays in `a` (a.row0 is overwritten): nb = B with row0 0 for a prefill tail or a decode step, nb = 1 with
// row0 = the slot for a session admission. One workgroup per utterance. Returns false, launching nothing, for arguments no call of the product makes.
static inline bool step_logits_record_launch(LogitsRecordArgs a, int row0, int nb, hipStream_t st) {
  if (!a.logits || !a.cur_len || !a.unfinished || !a.t_prefix || !a.rec || a.V < 1 || a.K < 1 || a.K > 32 || a.B < 1 || nb < 1 || row0 < 0 ||
      row0 + nb > a.B || a.t_prefix_stride < 0 || (!a.session && row0 != 0))
    return false;
  a.row0 = row0;
  hipLaunchKernelGGL(step_logits_record_kernel, dim3(nb), dim3(PTTS_STEP_RECORD_THREADS), 0, st, a);
  return true;
}
