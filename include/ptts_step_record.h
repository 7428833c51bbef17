/*
 * ptts_step_record.h - additive to the ABI v8 set of ptts.h (which does not include this header: include it beside ptts.h):
 * step records, i.e. what transformers' generate() returns as `scores` and `logits` under return_dict_in_generate, written on the device, step
 * by step, into arenas the caller owns - for static calls (ptts_prefill + ptts_decode_steps, inside the captured step graph) and per request
 * inside a continuous session. ("Step records", not "scores": that name belongs to the teacher-forced loss.) Same conventions as ptts.h.
 */
#ifndef PTTS_STEP_RECORD_H_
#define PTTS_STEP_RECORD_H_

#include "ptts.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Device arenas of fp32. Either pointer may be NULL: that kind is then not recorded.
 *   static call (ptts_set_step_records, for a batch of B):  [cap_steps][B][K][V] each - step i, utterance b, codebook row k at
 *                                                           ((i * B + b) * K + k) * V, i.e. step i is the [B*K, V] matrix transformers appends
 *   session slot (ptts_set_slot_step_records):              [cap_steps][K][V] each
 * K = num_codebooks, V = vocab_size. The caller owns the buffers and keeps them alive until the call / the slot's request is done.
 */
typedef struct {
  float* scores_dev;
  float* logits_dev;
  int32_t cap_steps;
} ptts_step_records;

/*
 * What is recorded. Step index i = t - given, with t = the utterance's clock before the step (its id columns: the input_ids.shape[-1] that
 * transformers' processors see) and given = 1 + the utterance's voice-prompt frames (the count the tail's min_new_tokens test uses). Step 0 is
 * the first sampled token: the tail of ptts_prefill (sample != 0), or an admission's own first-token tail.
 *
 *   logits[i]  the fp32 logits the LM heads produced for the step, bit for bit (what ptts_logits shows after the same ptts_step_forward) -
 *              `raw_logits += (next_token_logits,)` of transformers' GenerationMixin._sample (generation/utils.py:2904 in 5.15). Written by a
 *              small kernel node of its own in front of the history-penalty and logit-edit nodes, which rewrite the logits in place.
 *   scores[i]  the vector `scores += (next_token_scores,)` appends (generation/utils.py:2897-2902; parler_tts/modeling_parler_tts.py:3540-3566
 *              builds the processor list it comes from and hands it to _sample): the logits after the penalty and edit nodes, then
 *                greedy (do_sample == 0): -inf at the EOS entry while min_new_tokens (MinNewTokensLengthLogitsProcessor) or the Parler EOS gate
 *                  (ParlerTTSLogitsProcessor, logits_processors.py:44-53) blocks it; every other entry keeps its bits;
 *                sampling: l / temperature - the division the sampler itself performs, so the bits are its own - and -inf at the blocked EOS and at
 *                  every entry that top-k, top-p or an active warper stage (min_p, typical_p, epsilon_cutoff, eta_cutoff) removed.
 *              Which entries are removed is taken from each stage's own threshold test, never from "the softmax numerator is 0": with
 *              top_p == 1 an entry more than ~104 below the row maximum (its numerator underflows in fp32) is still kept by transformers and keeps
 *              a finite score. Ties and rounding bands are the sampler's: top-k keeps ties at the k-th value, top-p keeps
 *              every entry tied with its boundary value, and a mass within the rounding band of a threshold may fall on either side.
 *              Written by the RECORD instances of the sampler tail (tail_record_kernel / tail_warp_record_kernel): no extra node. Tokens, flags,
 *              clocks and the next column's embedding are bit-identical to those of the instances without the feature.
 *
 * A step is recorded exactly when the tail runs it: in a static batch the rows of an utterance that finished earlier are recorded for as long as
 * any utterance of the batch still runs (as transformers does), a no-op step after every utterance has finished writes nothing; an idle or finished
 * session slot records nothing. The engine never writes at or beyond cap_steps records; entries past the steps actually made are unspecified.
 * ptts_step_forward / ptts_logits are unchanged.
 *
 * ptts_set_step_records: r == NULL switches the feature off (the state of a new engine): no node is launched and no RECORD instance runs - step
 *   graphs and launches are exactly those of an engine that never heard of it. r != NULL switches it on for the next ptts_prefill, which lays
 *   the arenas out for its own batch size; with logits_dev == NULL the logits node is not launched (ptts_debug_graph_nodes: +0), with
 *   scores_dev == NULL the plain tail instances run (+1 node for the logits alone). For a session call it before ptts_session_begin* with
 *   both pointers NULL and cap_steps == 0 - "on, no slot records yet": the node set of a session is fixed at its begin, and such a session
 *   carries the logits node and the RECORD tail; slots without a record store nothing. Inside a running session - one in which a slot holds a
 *   request - PTTS_E_INVALID. A vocabulary above 2048 (PTTS_SORT_N): PTTS_E_UNSUPPORTED. cap_steps < 0, or a pointer with cap_steps == 0:
 *   PTTS_E_INVALID. A refused call changes nothing.
 */
int ptts_set_step_records(ptts_engine* e, const ptts_step_records* r, void* stream);

/*
 * ptts_set_slot_step_records: the record of the NEXT admission into slot `row`, whose own first-token tail is step 0 (any entry point:
 *   ptts_admit_row, _gen, _voice, ptts_admit_rows, ptts_admit_rows_voice; given counts the slot's own voice-prompt frames). r == NULL clears it,
 *   as ptts_retire_row does. Refusals: no session, or a session begun with the feature off; row outside the session; a busy slot; cap_steps < 0
 *   or a pointer with cap_steps == 0: PTTS_E_INVALID. A refused call changes nothing.
 */
int ptts_set_slot_step_records(ptts_engine* e, int32_t row, const ptts_step_records* r, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PTTS_STEP_RECORD_H_ */
