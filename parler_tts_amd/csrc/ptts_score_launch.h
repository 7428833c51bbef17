// Host side of ptts_score_kernels.h, shared by ptts_lm.hip and tests/native/score_harness.hip: instance choice and launch of the final LayerNorm +
// LM heads + cross-entropy kernel. The optional logits output is the STORE instance of the SAME kernel (not a second projection in front of a
// loss kernel): one code path to test, and the no-store instance computes its loss from bit-identical logits.
#pragma once
#include "ptts_score_kernels.h"
#include "ptts_gemm_launch.h"

inline size_t score_lds_bytes(int H, size_t esize, int MT) { return (size_t)16 * MT * ((size_t)H * esize + 16) + (size_t)SCORE_WAVES * MT * 64 * 3 * sizeof(float) + (size_t)16 * MT * sizeof(int); }

template <typename WT, int MT, bool STORE>
int score_launch_inst(const ScoreArgs& a, size_t sh, hipStream_t st) {
  static PttsPerDeviceOnce attr_once;  // > 64 KiB of dynamic LDS needs an explicit opt-in, once per instantiation
  const int attr_dev = PttsPerDeviceOnce::device();
  if (attr_once.need(attr_dev)) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&score_heads_kernel<WT, MT, STORE>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return ptts_fail(PTTS_E_HIP, "hipFuncSetAttribute(max dynamic LDS) failed: %s", hipGetErrorString(e));
    attr_once.done(attr_dev);
  }
  const int M = a.B * a.Qs;
  hipLaunchKernelGGL((score_heads_kernel<WT, MT, STORE>), dim3((M + 16 * MT - 1) / (16 * MT), a.K), dim3(SCORE_WAVES * 64), sh, st, a);
  return launch_status("score heads");
}

// Rows per workgroup: the most 16-row tiles (4, 2, 1) whose LayerNorm output fits in LDS beside the merge buffer - every tile more halves how often
// the codebook's weights are streamed again - and no more tiles than there are rows.
template <typename WT>
int score_launch(ScoreArgs a, hipStream_t st) {
  if (a.H < Elem<WT>::KT || a.H % Elem<WT>::KT != 0 || a.H > LN_MAX_F4 * 256 || a.V % 16 != 0 || a.x_ld % 4 != 0)
    return ptts_fail(PTTS_E_UNSUPPORTED, "score: hidden size %d / vocabulary %d outside the kernel's range (H %% %d == 0, H <= %d, V %% 16 == 0)", a.H, a.V,
                     Elem<WT>::KT, LN_MAX_F4 * 256);
  if (a.B < 1 || a.T < 1 || a.Qs < a.T || a.Q < a.Qs || (a.logits == nullptr && a.labels == nullptr) || (a.labels && !(a.ids && a.nll && a.counted)))
    return ptts_fail(PTTS_E_INVALID, "score: inconsistent rows or outputs");
  a.invH = 1.0f / (float)a.H;
  const int M = a.B * a.Qs;
  const size_t cap = 159 * 1024;
  int MT = 4;
  while (MT > 1 && (score_lds_bytes(a.H, sizeof(WT), MT) > cap || 16 * (MT / 2) >= M)) MT /= 2;
  const size_t sh = score_lds_bytes(a.H, sizeof(WT), MT);
  if (sh > cap) return ptts_fail(PTTS_E_UNSUPPORTED, "score: %zu bytes of LDS for one row tile at hidden size %d", sh, a.H);
  const bool store = a.logits != nullptr;
  if (MT == 4) return store ? score_launch_inst<WT, 4, true>(a, sh, st) : score_launch_inst<WT, 4, false>(a, sh, st);
  if (MT == 2) return store ? score_launch_inst<WT, 2, true>(a, sh, st) : score_launch_inst<WT, 2, false>(a, sh, st);
  return store ? score_launch_inst<WT, 1, true>(a, sh, st) : score_launch_inst<WT, 1, false>(a, sh, st);
}
