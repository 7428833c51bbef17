// History penalties of the sampler on the device: transformers' RepetitionPenaltyLogitsProcessor and NoRepeatNGramLogitsProcessor as ONE node
// between the LM heads and the sampler tail. Both are pure functions of the step's logits and of the slot's row of ids.
// Nothing here touches tail_kernel, TailArgs or SlotGen: the node rewrites the logits in place and the tail reads them as it always did.
#pragma once
#include <hip/hip_runtime.h>

#define PTTS_PENALTY_THREADS 256
#define PTTS_PENALTY_MAX_V 2048  // = PTTS_SORT_N, the widest vocabulary the tail samples from: two bitmaps of V bits in LDS

// the record of one utterance (static call: every record holds the engine-wide values; session: the request in the slot)
struct HistoryPenalty {
  float repetition_penalty;  // 1.0f: none
  int no_repeat_ngram;       // 0: none
};

struct PenaltyArgs {
  float* logits;            // [B][K][V], updated in place
  const long long* ids;     // [B*K][ids_ld]; row r = b*K + k, columns [0, cur_len[b]) are its history
  const int* cur_len;       // [B]
  const HistoryPenalty* pen;  // [B]
  int ids_ld, row0, K, V;   // utterance of workgroup (k, y) = row0 + y
};

// One workgroup per codebook row. Phase 1 only sets bits: `seen` for every history token, `banned` for the last token of every window whose
// first n - 1 tokens equal the history's last n - 1. Phase 2, behind one barrier, gives every vocabulary entry to exactly ONE thread, which
// reads the logit once, applies the penalty once (however often the token occurred: a bit cannot compound) and the ban after it, and stores
// once. No two threads ever touch the same logit, so there is no read-modify-write to race on.
// A window's first token is the load the `seen` pass makes anyway; the remaining n - 2 comparisons stop at the first mismatch and read the row
// through the cache (the whole row is at most a few tens of KB), so the history needs no LDS copy and its length has no bound but ids_ld.
static __global__ __launch_bounds__(PTTS_PENALTY_THREADS) void history_penalty_kernel(PenaltyArgs a) {
  const int b = a.row0 + blockIdx.y, k = blockIdx.x, V = a.V;
  const HistoryPenalty rec = a.pen[b];
  const float p = rec.repetition_penalty;
  const int n = rec.no_repeat_ngram;
  if (p == 1.0f && n <= 0) return;  // neutral record (uniform over the workgroup): no store, the row keeps its bits
  __shared__ unsigned seen[PTTS_PENALTY_MAX_V / 32], banned[PTTS_PENALTY_MAX_V / 32];
  const int tid = threadIdx.x;
  for (int i = tid; i < PTTS_PENALTY_MAX_V / 32; i += PTTS_PENALTY_THREADS) { seen[i] = 0u; banned[i] = 0u; }
  __syncthreads();
  const int t = min(max(a.cur_len[b], 0), a.ids_ld);  // never a column at or past t, never past the row
  const long long* row = a.ids + (size_t)(b * a.K + k) * a.ids_ld;
  const bool rep = p != 1.0f;
  const int last_start = n >= 1 ? t - n : -1;  // windows start in [0, t - n]; t < n: none
  const int s0 = t - n + 1;                    // the history's last n - 1 tokens start here (read only when a window exists: s0 >= 1)
  for (int j = tid; j < t; j += PTTS_PENALTY_THREADS) {
    const long long tok = row[j];
    if (rep && tok >= 0 && tok < V) atomicOr(&seen[tok >> 5], 1u << (tok & 31));
    if (j <= last_start) {
      bool match = true;
      for (int i = 0; i < n - 1 && match; ++i) match = row[j + i] == row[s0 + i];  // j + i <= t - 2, s0 + i <= t - 1
      if (match) {
        const long long last = row[j + n - 1];  // j + n - 1 <= t - 1
        if (last >= 0 && last < V) atomicOr(&banned[last >> 5], 1u << (last & 31));
      }
    }
  }
  __syncthreads();
  float* lg = a.logits + (size_t)(b * a.K + k) * V;
  const float ninf = -__builtin_huge_valf();
  for (int v = tid; v < V; v += PTTS_PENALTY_THREADS) {
    const unsigned bit = 1u << (v & 31);
    const bool s = seen[v >> 5] & bit, x = banned[v >> 5] & bit;
    if (!(s || x)) continue;
    float l = lg[v];
    if (s) l = l < 0.0f ? l * p : __fdiv_rn(l, p);  // IEEE fp32 both ways: -inf stays -inf, +-0 keep their sign, NaN stays NaN
    if (x) l = ninf;                                // the ban comes after the penalty
    lg[v] = l;
  }
}

// the records of slots [row0, row0 + nrows) from kernel arguments (set_slot_gen_kernel's pattern: no staging buffer, no copy to wait on)
static __global__ void set_penalty_kernel(HistoryPenalty* recs, int row0, int nrows, HistoryPenalty rec) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nrows) recs[row0 + i] = rec;
}
