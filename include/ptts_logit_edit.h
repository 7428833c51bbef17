/*
 * ptts_logit_edit.h - additive to the ABI v8 set of ptts.h (which does not include this header: include it beside ptts.h):
 * transformers' sequence_bias and bad_words_ids (single-token keys), exponential_decay_length_penalty, suppress_tokens and
 * begin_suppress_tokens applied on the device, as one kernel node between the history-penalty node and the sampler tail, for
 * static calls (ptts_prefill + ptts_decode_steps) and per request inside a continuous session. Same conventions as ptts.h.
 */
#ifndef PTTS_LOGIT_EDIT_H_
#define PTTS_LOGIT_EDIT_H_

#include "ptts.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The five options as host arrays (read during the call, never kept). A count of 0 (its pointer may be NULL) leaves that option out; a record
 * with every count 0 and decay_on == 0 is the neutral record: logits keep their bits.
 *   bias_tokens / bias_values [n_bias]   sequence_bias, one single-token key per entry: tokens in [0, vocab_size), values finite; of two entries
 *                                        that name the same token the later one holds
 *   bad_tokens [n_bad]                   bad_words_ids, one single-token entry each: tokens in [0, vocab_size). An entry equal to the EOS token is
 *                                        dropped, as NoBadWordsLogitsProcessor drops it (a list of nothing else still adds 0.0f to the row)
 *   suppress_tokens [n_suppress]         suppress_tokens; tokens outside [0, vocab_size) are ignored, as torch.isin ignores them
 *   begin_suppress_tokens [n_begin_suppress]   begin_suppress_tokens, likewise
 *   decay_on != 0                        exponential_decay_length_penalty = (decay_start >= 0, decay_factor finite and > 0)
 */
typedef struct {
  const int32_t* bias_tokens;
  const float* bias_values;
  const int32_t* bad_tokens;
  const int32_t* suppress_tokens;
  const int32_t* begin_suppress_tokens;
  int32_t n_bias;
  int32_t n_bad;
  int32_t n_suppress;
  int32_t n_begin_suppress;
  int32_t decay_on;
  int32_t decay_start;
  double decay_factor;
} ptts_logit_edits;

/*
 * What the node computes, for codebook row r of utterance b with t = the utterance's clock (its id columns: the input_ids.shape[-1] transformers'
 * processors see) and given = 1 + the utterance's voice-prompt frames (the count the tail's min_new_tokens test uses), bit for bit what
 * SequenceBiasLogitsProcessor, NoBadWordsLogitsProcessor, ExponentialDecayLengthPenalty, SuppressTokensLogitsProcessor and
 * SuppressTokensAtBeginLogitsProcessor give on the CPU, in that order, each skipped when its option is absent:
 *   1. sequence_bias: every logit l becomes l + bias[v] (0.0f where no key names v): an add over the whole row, -0.0 becomes +0.0;
 *   2. bad_words_ids: every logit becomes l + (-inf at the listed tokens, 0.0f elsewhere);
 *   3. exponential_decay_length_penalty, only while t > decay_start + given: with idx = t - decay_start - given and
 *      m = (float)(pow(decay_factor, idx) - 1.0) (the C library's pow, on the host, in a table uploaded with the record), the EOS logit becomes
 *      l + |l| * m - product and sum rounded separately, no FMA - and every other logit l + 0.0f;
 *   4. suppress_tokens: the listed tokens become -inf, every other logit keeps its bits;
 *   5. begin_suppress_tokens: the same, only while t == given (the first generated column).
 * A record none of whose stages is active at t stores nothing.
 *
 * Order. The node runs behind the history penalties and in front of the tail (min_new_tokens, EOS gate, temperature, top-k / top-p, warpers).
 * That is transformers' order but for two cases, which the caller must keep out (the engine cannot see them all; the Python layer enforces both):
 *   - sequence_bias precedes RepetitionPenaltyLogitsProcessor in transformers and does not commute with it: do not combine sequence_bias with
 *     a non-neutral history penalty (a neutral penalty record beside it is fine);
 *   - in transformers the decay runs behind MinNewTokensLength and turns the -inf it finds at EOS into NaN; here the tail blocks EOS behind the
 *     node. Keep min_new_tokens <= decay_start + 1: then the decay is never active while min_new_tokens still blocks EOS.
 * The node runs wherever the engine samples: the first token of ptts_prefill (sample != 0), every step of ptts_decode_steps (captured in the
 * step graph: one node more, ptts_debug_graph_nodes), the first token of every admission. ptts_step_forward / ptts_logits hand out raw logits.
 *
 * ptts_set_logit_edits: le == NULL switches the feature off (the state of a new engine): no node is launched, step graphs and launches are
 *   exactly those of an engine that never heard of it. le != NULL switches it on with *le as the record of every utterance; the neutral record
 *   is allowed (how a session is opened when only some requests will bring edits). Call it before ptts_prefill / ptts_session_begin*; the
 *   upload is ordered on `stream`. Inside a running session - one in which a slot holds a request - PTTS_E_INVALID: the node set of a session
 *   is fixed at its begin. A bias or bad-word token outside [0, vocab_size), a non-finite bias, decay_factor <= 0 or non-finite,
 *   decay_start < 0, a negative count or a NULL array with a positive count: PTTS_E_INVALID; a vocabulary above 2048: PTTS_E_UNSUPPORTED.
 *   A refused call changes nothing.
 */
int ptts_set_logit_edits(ptts_engine* e, const ptts_logit_edits* le, void* stream);

/*
 * ptts_set_slot_logit_edits: the record the NEXT admission into slot `row` runs under, its own first-token tail included (any entry point:
 *   ptts_admit_row, _gen, _voice, ptts_admit_rows, ptts_admit_rows_voice); given counts the slot's own voice-prompt frames. le == NULL restores
 *   the session's default (the record of ptts_set_logit_edits), as ptts_retire_row does. Refusals: no session, or a session begun with the
 *   feature off; row outside the session; a busy slot; values out of range as above: PTTS_E_INVALID. A refused call changes nothing.
 */
int ptts_set_slot_logit_edits(ptts_engine* e, int32_t row, const ptts_logit_edits* le, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PTTS_LOGIT_EDIT_H_ */
