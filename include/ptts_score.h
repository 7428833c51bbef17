/*
 * ptts_score.h - additive to the ABI v8 set of ptts.h (which does not include this header: include it beside ptts.h):
 * one teacher-forced decoder forward over given code columns - ParlerTTSForCausalLM.forward with labels - ending in a fused
 * final LayerNorm + LM heads + cross-entropy kernel that writes per-token negative log-likelihoods and never the logits.
 * Same conventions as ptts.h.
 */
#ifndef PTTS_SCORE_H_
#define PTTS_SCORE_H_

#include "ptts.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Device pointers. V = vocab_size, K = num_codebooks of the engine. */
typedef struct {
  const int64_t* input_ids;  /* [B*K, T] decoder_input_ids exactly as the model is to see them (no delay pattern is applied); ids in [0, V] */
  const int64_t* labels;     /* [B, T, K], or NULL: no loss */
  float* nll;                /* out [B, T, K]; NULL iff labels is NULL */
  int32_t* counted;          /* out [B, T, K]; NULL iff labels is NULL */
  float* logits;             /* out [B*K, P + T, V] fp32, or NULL: never materialised */
} ptts_score_io;

/*
 * One forward over Q = P + T positions per utterance: cross K/V from enc (masked by enc_mask), the P prompt rows prepended, the T given columns
 * embedded as they are (sum of the K codebook embeddings + position P + j), causal self-attention under [prompt_mask | ones] - the pass
 * ptts_prefill runs, over raw columns. Then, for every codebook k and each of the last T positions t of utterance b:
 *   nll[b, t, k]     = logsumexp(logits[b, k, t, :]) - logits[b, k, t, labels[b, t, k]]   where the position counts, 0.f elsewhere
 *   counted[b, t, k] = labels[b, t, k] != -100  &&  labels[b, t, k] != bos_token_id  &&  input_ids[b*K + k, t] != eos_token_id
 * (a label outside [0, V) that passes the three tests is not counted). With io->logits the same kernel also stores its fp32 logits for all
 * P + T positions, [B*K, P + T, V]; without it no buffer of that size is allocated or touched. At least one of labels / logits is required.
 *
 * Asynchronous on `stream`; not captured in a graph; no host synchronise inside. weights_fp8 engines score on the exact bf16 dequantisation,
 * as their prefill does; a single-utterance engine does not fold its cross block for this call.
 *
 * Capacity (PTTS_E_CAPACITY): P + T <= max_prompt, P + T <= max_ctx, B <= max_batch, N <= max_enc, P + T <= max_positions unless RoPE.
 * PTTS_E_INVALID: T < 1, a null or inconsistent io, P > 0 without prompt_dev; a continuous session in which a slot holds a request (the pass
 *   overwrites arena rows). PTTS_E_UNSUPPORTED: a kv_fp8 engine (the loss of a checkpoint is not to depend on an opt-in cache format); a pending
 *   voice prompt (ptts_set_audio_prefix). A refused call changes nothing.
 *
 * After the call the engine is in the state of one that was never prefilled: ptts_decode_steps is refused until the next ptts_prefill /
 * ptts_session_begin*. Generation parameters, penalty and warper switches, captured step graphs and packed weights are untouched.
 */
int ptts_score(ptts_engine* e, const float* enc_dev, const int32_t* enc_mask_dev, const float* prompt_dev, const int32_t* prompt_mask_dev,
               int32_t B, int32_t N, int32_t P, int32_t T, const ptts_score_io* io, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PTTS_SCORE_H_ */
