/*
 * ptts_session_voice_rows.h - additive to the ABI v8 set of ptts.h, ptts_session.h and ptts_session_voice.h (none of them includes this header:
 * include it beside ptts.h): a GROUP of requests that continue voice prompts, admitted into a continuous session with one prefill pass.
 * Same conventions as ptts.h.
 */
#ifndef PTTS_SESSION_VOICE_ROWS_H_
#define PTTS_SESSION_VOICE_ROWS_H_

#include "ptts.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ptts_admit_rows_voice: ptts_admit_rows for requests that continue voice prompts of ragged lengths (ptts_admit_row_voice, for n slots at once).
 *     rows, enc_dev [n, N, H], enc_mask_dev, prompt_dev [n, P, H], prompt_mask_dev, max_lengths, gps: as ptts_admit_rows'
 *     codes_dev   host array of n device pointers, entry j: [K, Ts[j]] int64 un-delayed codes, consumed on the stream; NULL iff Ts[j] == 0
 *                 (the array itself may be NULL when every Ts[j] == 0)
 *     Ts          host array of n: frames per request, ragged, 0 allowed
 *   Afterwards slot rows[j] is what ptts_admit_row_voice(rows[j], request j, Ts[j], max_lengths[j], ...) makes of it: self K/V rows
 *   [0, P + 1 + Ts[j]) - e4m3 bytes and scales on a kv_fp8 session -, cross K/V, both mask rows, id columns 1..Ts[j] under the delay pattern of
 *   the request's own max_length, the slot's prefix length and prefix rows, its clock at Ts[j] + 1, the step-0 logits, the request's own record,
 *   and with `sample` != 0 its first token in column Ts[j] + 1. Slots not listed are untouched; so are a listed slot's self K/V rows at and
 *   beyond P + 1 + Ts[j]. The step graphs do not change (no capture, same node count).
 *   ONE prefill pass runs on the spare arena rows B .. B + n - 1 over P + 1 + Tmax positions per row, Tmax = max Ts[j]. A shorter request is
 *   right-padded: its columns Ts[j] + 1 .. Tmax embed PAD (never an id the spare row happens to hold), causal attention keeps them from the
 *   request's own positions, and what is computed there is thrown away; its logits come from position P + Ts[j].
 *   n == 1: exactly ptts_admit_row_voice, launch for launch. Every Ts[j] == 0: exactly ptts_admit_rows, launch for launch. Every Ts[j] == T:
 *   the step-0 logits and id columns of slot rows[j] - on kv_fp8 the cache bytes and scales too - equal those of ptts_set_audio_prefix +
 *   ptts_prefill of the group at batch n bit for bit. In a ragged group a request's result depends on n and Tmax, which select the kernels, and
 *   not on the other requests' contents or lengths; against the same request admitted alone it differs by the rounding of those kernels, as
 *   ptts_admit_rows documents.
 *   Refusals: everything ptts_admit_rows and ptts_admit_row_voice refuse, for every entry: Ts[j] < 0, or NULL codes with Ts[j] > 0:
 *   PTTS_E_INVALID; P + 1 + Tmax above the engine's max_prompt: PTTS_E_CAPACITY; Ts[j] + 2 > max_length of request j: PTTS_E_INVALID; more
 *   requests than spare rows: PTTS_E_CAPACITY. All checks run before the first launch: a refused call changes nothing. */
int ptts_admit_rows_voice(ptts_engine* e, int32_t n, const int32_t* rows, const float* enc_dev, const int32_t* enc_mask_dev,
                          const float* prompt_dev, const int32_t* prompt_mask_dev, const int64_t* const* codes_dev, const int32_t* Ts,
                          const int32_t* max_lengths, int32_t sample, const ptts_gen_params* const* gps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PTTS_SESSION_VOICE_ROWS_H_ */
