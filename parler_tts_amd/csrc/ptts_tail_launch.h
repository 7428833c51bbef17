// Host-side launch of the sampler tail (tail_kernel<NV, SESSION> / tail_warp_kernel<NV, SESSION> and their step-record twins, ptts_lm_kernels.h): the one
// place that picks the instance.
// Shared by the engine (launch_tail, ptts_lm.hip) and the test harnesses (tests/native/tail_harness.hip, ...), so that a test of the
// kernel runs the instance, the wave count and the argument struct the product would run for the same (V, K).
#pragma once
#include <algorithm>
#include <type_traits>

#include "ptts_lm_kernels.h"

// row_maxlen null: the static instances (every utterance on the shared clock, stop on DevGen::max_length; row0 unused).
// row_maxlen set: the session instances, slot b = row0 + blockIdx.x under its own max_length - grid (B) with row0 0 for a
// decode step, grid (1) with row0 = the slot for an admission. slot_gen (session only): the per-slot sampler records, or null.
// slot_tprefix (session only): the per-slot voice-prompt lengths, or null: no slot has a prefix.
// NV = logits per lane: 8 up to vocab 512, 18 up to 1152, 32 up to PTTS_SORT_N. One wave per codebook row (greedy arg-max or the
// sort-free sampler), at least 4 waves for the embedding of the next column, at most 16 (more codebooks loop).
// warp (null: off) picks the WARP instances (tail_warp_kernel): the per-utterance warper records (DevWarp, [B] indexed like cur_len) ride behind the arguments.
// rec (null: off) picks the RECORD instances (tail_record_kernel / tail_warp_record_kernel): the per-utterance step records (StepRecord, [B] indexed
// like cur_len) ride behind everything else. Null launches exactly what this function launched before it had the argument.
static inline void tail_launch(const TailArgs& t, const int* row_maxlen, int row0, dim3 grid, hipStream_t st, const SlotGen* slot_gen = nullptr,
                               const int* slot_tprefix = nullptr, const DevWarp* warp = nullptr, const StepRecord* rec = nullptr) {
  const int nw = std::min(std::max(t.K, 4), 16);
  auto launch = [&](auto session, auto warped, const auto& args) {  // one NV dispatch for every instance
    constexpr bool S = decltype(session)::value, W = decltype(warped)::value;
    if constexpr (W) {
      if (t.V <= 512) hipLaunchKernelGGL((tail_warp_kernel<8, S>), grid, dim3(nw * 64), 0, st, args);
      else if (t.V <= 1152) hipLaunchKernelGGL((tail_warp_kernel<18, S>), grid, dim3(nw * 64), 0, st, args);
      else hipLaunchKernelGGL((tail_warp_kernel<32, S>), grid, dim3(nw * 64), 0, st, args);
    } else {
      if (t.V <= 512) hipLaunchKernelGGL((tail_kernel<8, S>), grid, dim3(nw * 64), 0, st, args);
      else if (t.V <= 1152) hipLaunchKernelGGL((tail_kernel<18, S>), grid, dim3(nw * 64), 0, st, args);
      else hipLaunchKernelGGL((tail_kernel<32, S>), grid, dim3(nw * 64), 0, st, args);
    }
  };
  auto launch_record = [&](auto session, auto warped, const auto& args) {  // the same dispatch over the RECORD instances
    constexpr bool S = decltype(session)::value, W = decltype(warped)::value;
    if constexpr (W) {
      if (t.V <= 512) hipLaunchKernelGGL((tail_warp_record_kernel<8, S>), grid, dim3(nw * 64), 0, st, args);
      else if (t.V <= 1152) hipLaunchKernelGGL((tail_warp_record_kernel<18, S>), grid, dim3(nw * 64), 0, st, args);
      else hipLaunchKernelGGL((tail_warp_record_kernel<32, S>), grid, dim3(nw * 64), 0, st, args);
    } else {
      if (t.V <= 512) hipLaunchKernelGGL((tail_record_kernel<8, S>), grid, dim3(nw * 64), 0, st, args);
      else if (t.V <= 1152) hipLaunchKernelGGL((tail_record_kernel<18, S>), grid, dim3(nw * 64), 0, st, args);
      else hipLaunchKernelGGL((tail_record_kernel<32, S>), grid, dim3(nw * 64), 0, st, args);
    }
  };
  if (row_maxlen) {  // per-slot clocks
    const TailSessionArgs s{t, row_maxlen, row0, slot_gen, slot_tprefix};
    if (rec && warp) launch_record(std::true_type{}, std::true_type{}, TailSessionWarpRecordArgs{TailSessionWarpArgs{s, warp}, rec});
    else if (rec) launch_record(std::true_type{}, std::false_type{}, TailSessionRecordArgs{s, rec});
    else if (warp) launch(std::true_type{}, std::true_type{}, TailSessionWarpArgs{s, warp});
    else launch(std::true_type{}, std::false_type{}, s);
  } else if (rec) {
    if (warp) launch_record(std::false_type{}, std::true_type{}, TailWarpRecordArgs{TailWarpArgs{t, warp}, rec});
    else launch_record(std::false_type{}, std::false_type{}, TailRecordArgs{t, rec});
  } else if (warp) {
    launch(std::false_type{}, std::true_type{}, TailWarpArgs{t, warp});
  } else {
    launch(std::false_type{}, std::false_type{}, t);
  }
}
