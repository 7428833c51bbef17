// Host-side launch of the history-penalty node (history_penalty_kernel, ptts_penalty_kernels.h). Shared by the engine (launch_tail,
// ptts_lm.hip) and the test harness (tests/native/penalty_harness.hip), so that a test of the kernel runs the grid and the argument struct
// the product would run for the same (K, V).
#pragma once
#include "ptts_penalty_kernels.h"

// Utterances [row0, row0 + nb) of the arrays in `a` (a.row0 is overwritten): nb = B with row0 0 for a prefill tail or a decode step, nb = 1 with
// row0 = the slot for a session admission. One workgroup per codebook row. Returns false, launching nothing, for a shape the kernel does not
// serve (a vocabulary wider than its LDS bitmaps).
static inline bool penalty_launch(PenaltyArgs a, int row0, int nb, hipStream_t st) {
  if (a.V < 1 || a.V > PTTS_PENALTY_MAX_V || a.K < 1 || nb < 1 || row0 < 0 || a.ids_ld < 1) return false;
  a.row0 = row0;
  hipLaunchKernelGGL(history_penalty_kernel, dim3(a.K, nb), dim3(PTTS_PENALTY_THREADS), 0, st, a);
  return true;
}
