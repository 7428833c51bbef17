/*
 * ptts_session_voice.h - additive to the ABI v8 set of ptts.h and ptts_session.h (neither includes this header: include it beside ptts.h):
 * a request that continues a voice prompt (an audio prefix) inside a continuous session. Same conventions as ptts.h.
 */
#ifndef PTTS_SESSION_VOICE_H_
#define PTTS_SESSION_VOICE_H_

#include "ptts.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ptts_admit_row_voice: ptts_admit_row_gen for a request whose decoder continues T frames of given audio codes (generate()'s
 *   decoder_input_ids / input_values; what ptts_set_audio_prefix + ptts_prefill do for a static batch, for ONE slot of a session).
 *     codes_dev [K, T] int64 un-delayed codes, consumed on the stream (may be NULL iff T == 0); every other argument as ptts_admit_row_gen's
 *   T == 0: exactly ptts_admit_row_gen, launch for launch.
 *   T > 0: the slot is admitted with 1 + T given columns. Its id columns 1..T take the delay pattern of (BOS + prefix, the request's own
 *   max_length): BOS for j <= k, PAD for j - k >= max_length - K + 1, prefix[k][j - k - 1] otherwise, and the prefix un-shifted when
 *   max_length < 2K - 1 (no pattern). P + 1 + T positions run in ONE prefill pass on the slot's own arena rows (the kernels ptts_prefill runs
 *   for one utterance of that many rows): self K/V rows [0, P + 1 + T) - e4m3 bytes and scales on a kv_fp8 session -, cross K/V, and the
 *   step-0 logits, which equal those of ptts_set_audio_prefix + ptts_prefill of the same request at batch 1 bit for bit. The slot's clock
 *   (ptts_row_state) starts at T + 1; with `sample` != 0 its first token lands in column T + 1. From there on the slot decodes like any other:
 *   the ids the steps write are the raw sampled tokens (ptts_ids of the slot = the reference's raw sequence), the model is fed the shifted
 *   prompt codes where the pattern still holds one, and min_new_tokens counts from the 1 + T given columns.
 *   max_length counts ALL columns (BOS + T + generated), as ptts_set_audio_prefix's does; 0 = the session's.
 *   The slot's prefix length lives on the device beside its max_length and is cleared by ptts_retire_row and ptts_session_begin*; the step
 *   graphs do not change (no capture, same node count).
 *   Refusals: everything ptts_admit_row_gen refuses (a pending ptts_set_audio_prefix stays refused: this call is how a session takes a voice
 *   prompt); T < 0, or NULL codes with T > 0: PTTS_E_INVALID; P + 1 + T above the engine's max_prompt: PTTS_E_CAPACITY; T + 2 > max_length
 *   (no room for a generated token): PTTS_E_INVALID. All checks run before the first launch: a refused call changes nothing. */
int ptts_admit_row_voice(ptts_engine* e, int32_t row, const float* enc_dev, const int32_t* enc_mask_dev, const float* prompt_dev,
                         const int32_t* prompt_mask_dev, const int64_t* codes_dev, int32_t T, int32_t max_length, int32_t sample,
                         const ptts_gen_params* gp, void* stream);

/*
 * ptts_debug_slot_voice: the voice-prompt length of every slot of the session as the device holds it (frames_host: host array of the session's
 *   B entries; 0 = the slot continues no prefix). Synchronises the stream. For tests. */
int ptts_debug_slot_voice(ptts_engine* e, int32_t* frames_host, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PTTS_SESSION_VOICE_H_ */
