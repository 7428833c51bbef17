// Step records (include/ptts_step_record.h): what transformers' _sample hands out as `scores` and `logits` under return_dict_in_generate, written
// step by step on the device into arenas the caller owns. Two kinds, two places:
//   raw logits        step_logits_record_kernel, a node of its own IN FRONT of the history-penalty and logit-edit nodes (they rewrite the logits
//                     buffer in place; output_logits is what the heads produced)
//   processed scores  the RECORD instances of the sampler tail (tail_record_kernel / tail_warp_record_kernel, ptts_lm_kernels.h), which hold each
//                     row's processed scores in registers before they draw
// Both find their destination in ONE table of per-utterance records (StepRecord, [max_batch], indexed like cur_len) whose address the step graphs
// hold: pointing a record somewhere else captures nothing again. Nothing here touches tail_kernel, tail_warp_kernel or their argument structs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PTTS_STEP_RECORD_THREADS 256

// The record of one utterance / slot. Step idx = cur_len - given (given = 1 + the utterance's voice-prompt frames) of codebook row k goes to
// base + idx * step_stride + k * V. Static call: every entry points into one arena [cap_steps][B][K][V] at its own utterance (step_stride = B K V);
// session: the slot's own [cap_steps][K][V] (step_stride = K V). A null pointer: that kind is not recorded for this utterance.
struct StepRecord {
  float* scores;
  float* logits;
  int cap_steps;  // nothing is written at or beyond this step
  int reserved;
  long long step_stride;  // floats
};

struct LogitsRecordArgs {
  const float* logits;    // [B][K][V], as the LM heads wrote them
  const int* cur_len;     // [B]
  const int* unfinished;  // [B*K], the tail's flags
  const int* t_prefix;    // voice-prompt frames: utterance b's at t_prefix[b * t_prefix_stride] (stride 0: one value for the whole batch)
  const StepRecord* rec;  // [B]
  int t_prefix_stride, row0, B, K, V, session;  // utterance of workgroup x = row0 + x
};

// One workgroup per utterance: a bit copy of its K * V logits into step idx of its record. It skips exactly when the tail that follows it skips
// (ptts_tail_body.inc): a static step after every row had finished before it (the reference loop has exited), a session slot that is not live.
// Nothing is written for a null record or a step at or beyond cap_steps. 16-byte loads and stores where both the utterance's logits and its
// destination are 16-byte aligned (K * V a multiple of 4 keeps every utterance of a static arena so), one float per thread otherwise.
static __global__ __launch_bounds__(PTTS_STEP_RECORD_THREADS) void step_logits_record_kernel(LogitsRecordArgs a) {
  const int b = a.row0 + blockIdx.x, tid = threadIdx.x;
  const int t = a.cur_len[b];
  const StepRecord r = a.rec[b];
  const int idx = t - 1 - a.t_prefix[(size_t)b * a.t_prefix_stride];
  int any_local = 0;
  if (a.session) {
    any_local = tid < a.K ? (a.unfinished[b * a.K + tid] > 0) : 0;
  } else {
    for (int i = tid; i < a.B * a.K; i += PTTS_STEP_RECORD_THREADS) {
      const int v = a.unfinished[i];
      any_local |= (v > 0) | (v <= -(t + 1));
    }
  }
  if (!__syncthreads_or(any_local)) return;
  if (!r.logits || idx < 0 || idx >= r.cap_steps) return;
  const size_t n = (size_t)a.K * a.V;
  const float* src = a.logits + (size_t)b * n;
  float* dst = r.logits + (size_t)idx * (size_t)r.step_stride;
  if ((((uintptr_t)src | (uintptr_t)dst) & 15u) == 0) {
    const size_t n4 = n >> 2;
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* d4 = reinterpret_cast<float4*>(dst);
    for (size_t i = tid; i < n4; i += PTTS_STEP_RECORD_THREADS) d4[i] = s4[i];
    for (size_t i = (n4 << 2) + tid; i < n; i += PTTS_STEP_RECORD_THREADS) dst[i] = src[i];
  } else {
    for (size_t i = tid; i < n; i += PTTS_STEP_RECORD_THREADS) dst[i] = src[i];
  }
}

// Records [row0, row0 + nrows): entry row0 + i = rec with both non-null pointers advanced by i * per_row floats (a static call lays its B
// utterances out inside one step of the arena; one slot, or a clear: per_row unused). The record travels by value, as SlotGen and DevWarp do.
static __global__ void set_step_record_kernel(StepRecord* recs, int row0, int nrows, StepRecord rec, long long per_row) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nrows) return;
  if (rec.scores) rec.scores += (size_t)i * per_row;
  if (rec.logits) rec.logits += (size_t)i * per_row;
  recs[row0 + i] = rec;
}
