// Position and token edits of the logits on the device: transformers' SequenceBiasLogitsProcessor and NoBadWordsLogitsProcessor (single-token
// keys), ExponentialDecayLengthPenalty, SuppressTokensLogitsProcessor and SuppressTokensAtBeginLogitsProcessor as ONE node between the
// history-penalty node and the sampler tail. All five are pure functions of the step's logits, of the utterance's clock
// and of fixed token lists, so the node reads no id column. Nothing here touches tail_kernel, TailArgs or SlotGen: the node rewrites the logits in
// place and the tail reads them as it always did.
#pragma once
#include <hip/hip_runtime.h>

#define PTTS_LOGIT_EDIT_THREADS 256
#define PTTS_LOGIT_EDIT_MAX_V 2048  // = PTTS_SORT_N, the widest vocabulary the tail samples from
#define PTTS_LOGIT_EDIT_NV (PTTS_LOGIT_EDIT_MAX_V / PTTS_LOGIT_EDIT_THREADS)  // logits per thread

// stages of a record (LogitEditHeader::mask), in the order they run
#define PTTS_LE_BIAS 1      // sequence_bias: the whole row + bias[v]
#define PTTS_LE_BAD 2       // bad_words_ids: the whole row + (-inf at the listed tokens, 0 elsewhere)
#define PTTS_LE_DECAY 4     // exponential_decay_length_penalty
#define PTTS_LE_SUPPRESS 8  // suppress_tokens: -inf at the listed tokens, the others keep their bits
#define PTTS_LE_BEGIN 16    // begin_suppress_tokens: the same in the first generated column
// classes of a token (one byte per vocabulary entry)
#define PTTS_LEF_BAD 1
#define PTTS_LEF_SUPPRESS 2
#define PTTS_LEF_BEGIN 4

// the header of one utterance's record (static call: every record holds the engine-wide values; session: the request in the slot)
struct LogitEditHeader {
  int mask;         // PTTS_LE_* of the stages present; 0: the neutral record
  int decay_start;  // exponential_decay_length_penalty[0]
  int table_len;    // entries of the utterance's decay table (>= 2 while PTTS_LE_DECAY is set)
  int reserved;
};

// the records of the utterances, struct of arrays, every array indexed by utterance like cur_len
struct LogitEditRecs {
  LogitEditHeader* hdr;  // [B]
  float* bias;           // [B][ld_v]  bias[v], 0.0f where no key names v
  float* decay;          // [B][ld_t]  decay[idx] = (float)(pow((double)factor, idx) - 1.0), computed on the host
  unsigned char* flags;  // [B][ld_v]  PTTS_LEF_* of token v
  int ld_v, ld_t;
};

struct LogitEditArgs {
  float* logits;         // [B][K][V], updated in place
  const int* cur_len;    // [B] the clock t of each utterance = the id columns transformers' processors see
  const int* t_prefix;   // voice-prompt frames: utterance b's at t_prefix[b * t_prefix_stride] (stride 0: one value for the whole batch)
  LogitEditRecs recs;
  int t_prefix_stride, row0, K, V, eos;  // utterance of workgroup (k, y) = row0 + y
};

// One workgroup per codebook row; every logit belongs to exactly ONE thread, which loads it once, applies the active stages in transformers' order
// and stores it once. Which stages are active is uniform over the workgroup (the record and the clock), so a workgroup with nothing to do - the
// neutral record, or a decay / begin stage outside its columns with no other stage present - returns before any store and the row keeps its bits.
// The sums are IEEE fp32 adds over the WHOLE row, as torch's `scores + bias` is: -0.0 becomes +0.0 there. The decay's product and sum are two
// separately rounded operations (no FMA), as torch computes them.
static __global__ __launch_bounds__(PTTS_LOGIT_EDIT_THREADS) void logit_edit_kernel(LogitEditArgs a) {
#pragma clang fp contract(off)
  const int b = a.row0 + blockIdx.y, k = blockIdx.x, V = a.V, tid = threadIdx.x;
  const LogitEditHeader h = a.recs.hdr[b];
  const int mask = h.mask;
  if (mask == 0) return;
  const int t = a.cur_len[b], given = 1 + a.t_prefix[(size_t)b * a.t_prefix_stride];
  const int idx = t - h.decay_start - given;  // > 0: the decay is active (cur_len > regulation_start)
  const bool decay = (mask & PTTS_LE_DECAY) && idx > 0 && h.table_len > 0;
  const bool begin = (mask & PTTS_LE_BEGIN) && t == given;
  const bool bias_on = mask & PTTS_LE_BIAS, bad_on = mask & PTTS_LE_BAD, sup_on = mask & PTTS_LE_SUPPRESS;
  if (!(bias_on || bad_on || sup_on || decay || begin)) return;
  const float m = decay ? a.recs.decay[(size_t)b * a.recs.ld_t + min(idx, h.table_len - 1)] : 0.0f;  // never past the table
  const bool need_flags = bad_on || sup_on || begin;
  float* lg = a.logits + (size_t)(b * a.K + k) * V;
  const float* bias = a.recs.bias + (size_t)b * a.recs.ld_v;
  const unsigned char* flags = a.recs.flags + (size_t)b * a.recs.ld_v;
  const float ninf = -__builtin_huge_valf();
  // every load of the thread's entries goes in flight before the first use. Each array is read only under its stage's mask bit: a setter uploads
  // only the arrays of the stages present, so the others may hold an earlier request's values (upload_logit_edit, ptts_lm.hip)
  float l[PTTS_LOGIT_EDIT_NV], bv[PTTS_LOGIT_EDIT_NV];
  unsigned f[PTTS_LOGIT_EDIT_NV];
#pragma unroll
  for (int i = 0; i < PTTS_LOGIT_EDIT_NV; ++i) {
    const int v = tid + i * PTTS_LOGIT_EDIT_THREADS;
    const bool in = v < V;
    l[i] = in ? lg[v] : 0.0f;
    bv[i] = (in && bias_on) ? bias[v] : 0.0f;
    f[i] = (in && need_flags) ? flags[v] : 0u;
  }
#pragma unroll
  for (int i = 0; i < PTTS_LOGIT_EDIT_NV; ++i) {
    const int v = tid + i * PTTS_LOGIT_EDIT_THREADS;
    if (v >= V) break;
    float x = l[i];
    if (bias_on) x = __fadd_rn(x, bv[i]);
    if (bad_on) x = __fadd_rn(x, (f[i] & PTTS_LEF_BAD) ? ninf : 0.0f);
    if (decay) x = __fadd_rn(x, v == a.eos ? __fmul_rn(fabsf(x), m) : 0.0f);
    if (sup_on && (f[i] & PTTS_LEF_SUPPRESS)) x = ninf;
    if (begin && (f[i] & PTTS_LEF_BEGIN)) x = ninf;
    lg[v] = x;
  }
}

// Records [dst0, dst0 + n) = record `src` of the same arrays (the engine keeps the session's default in a record of its own behind the slots').
// grid (chunks, n): every element of a record is copied by one thread.
static __global__ void copy_logit_edit_kernel(LogitEditRecs r, int src, int dst0) {
  const int dst = dst0 + blockIdx.y;
  if (dst == src) return;
  const int i0 = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
  if (i0 == 0) r.hdr[dst] = r.hdr[src];
  for (int i = i0; i < r.ld_v; i += step) {
    r.bias[(size_t)dst * r.ld_v + i] = r.bias[(size_t)src * r.ld_v + i];
    r.flags[(size_t)dst * r.ld_v + i] = r.flags[(size_t)src * r.ld_v + i];
  }
  for (int i = i0; i < r.ld_t; i += step) r.decay[(size_t)dst * r.ld_t + i] = r.decay[(size_t)src * r.ld_t + i];
}
