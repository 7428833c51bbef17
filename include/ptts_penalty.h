/*
 * ptts_penalty.h - additive to the ABI v8 set of ptts.h (which does not include this header: include it beside ptts.h):
 * transformers' repetition_penalty and no_repeat_ngram_size applied on the device, as one kernel node in front of the sampler tail,
 * for static calls (ptts_prefill + ptts_decode_steps) and per request inside a continuous session. Same conventions as ptts.h.
 */
#ifndef PTTS_PENALTY_H_
#define PTTS_PENALTY_H_

#include "ptts.h"

#ifdef __cplusplus
extern "C" {
#endif

/* repetition_penalty: finite and > 0; 1.0 = none. no_repeat_ngram_size: >= 0; 0 = none. (1.0, 0) is the neutral record: logits keep their bits. */
typedef struct {
  float repetition_penalty;
  int32_t no_repeat_ngram_size;
} ptts_history_penalty;

/*
 * What the node computes, for codebook row r of utterance b with t = the utterance's clock, over the t id columns ptts_ids exposes (BOS or
 * voice-prompt columns + the raw sampled ids: the input_ids transformers' processors receive), bit for bit what
 * RepetitionPenaltyLogitsProcessor followed by NoRepeatNGramLogitsProcessor give on the CPU:
 *   every logit l of a token that occurs in the history becomes l < 0 ? l * p : l / p (fp32, IEEE rounding, once per distinct token);
 *   then, with n = no_repeat_ngram_size >= 1 and t >= n, every window of n history tokens whose first n - 1 equal the history's last n - 1
 *   sets the logit of its last token to -inf. History ids outside [0, vocab_size) are ignored.
 * The node runs wherever the engine samples: the first token of ptts_prefill (sample != 0), every step of ptts_decode_steps (captured in the
 * step graph: one node more, ptts_debug_graph_nodes), the first token of every admission. ptts_step_forward / ptts_logits hand out raw logits.
 *
 * ptts_set_history_penalty: hp == NULL switches the feature off (the state of a new engine): no node is launched, step graphs and launches are
 *   exactly those of an engine that never heard of it. hp != NULL switches it on with *hp as the record of every utterance; neutral values are
 *   allowed (how a session is opened when only some requests will bring penalties). Call it before ptts_prefill / ptts_session_begin*.
 *   Inside a running session - one in which a slot holds a request - PTTS_E_INVALID: the node set of a session is fixed at its begin
 *   (retire its requests first; a session whose slots are all idle may be reconfigured, e.g. in front of the next ptts_session_begin*).
 *   Values out of range: PTTS_E_INVALID; a vocabulary above 2048: PTTS_E_UNSUPPORTED. A refused call changes nothing.
 */
int ptts_set_history_penalty(ptts_engine* e, const ptts_history_penalty* hp, void* stream);

/*
 * ptts_set_slot_history_penalty: the record the NEXT admission into slot `row` runs under, its own first-token tail included (any entry point:
 *   ptts_admit_row, _gen, _voice, ptts_admit_rows). hp == NULL restores the session's default (the values of ptts_set_history_penalty), as
 *   ptts_retire_row does. Refusals: no session, or a session begun with the feature off; row outside the session; a busy slot; values out of
 *   range: PTTS_E_INVALID. A refused call changes nothing.
 */
int ptts_set_slot_history_penalty(ptts_engine* e, int32_t row, const ptts_history_penalty* hp, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PTTS_PENALTY_H_ */
