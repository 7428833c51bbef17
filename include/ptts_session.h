/*
 * ptts_session.h - additive to the ABI v8 set of ptts.h (which includes this header; include ptts.h, not this file): admitting several
 * requests into a continuous session with one prefill pass. Same conventions as ptts.h.
 */
#ifndef PTTS_SESSION_H_
#define PTTS_SESSION_H_

#include "ptts.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ptts_admit_rows: n >= 1 requests into n distinct idle slots with ONE prefill pass. Request j goes into slot rows[j] (host array, any order); afterwards
 *   every listed slot is exactly what ptts_admit_row_gen(rows[j], request j, max_lengths[j], sample, gps ? gps[j] : NULL) makes of it: cross K/V, self
 *   K/V rows 0..P, step-0 logits, sampler state reset, its own record if gps[j] is given, and with `sample` != 0 its first token and the next column's
 *   embedding. The pass runs the launches ptts_prefill runs for a batch of n (chosen by n * (P + 1) rows), on the spare arena rows behind the
 *   session's slots, and one kernel then moves each spare row to its slot: so the step-0 logits of slot rows[j] equal row j of that static prefill
 *   bit for bit, n == 1 equals ptts_admit_row bit for bit, and a request admitted in a group differs from the same request admitted alone by the
 *   rounding of the projection kernels the row count selects (both are within the engine's tolerance of the reference). Other slots are untouched.
 *     enc_dev [n, N, H] float32, enc_mask_dev [n, N] int32 or NULL, prompt_dev [n, P, H] float32 (NULL iff P == 0), prompt_mask_dev [n, P] int32 or NULL
 *     max_lengths: host array of n, each as ptts_admit_row's max_length; gps: NULL, or a host array of n entries, each NULL or a record
 *   Every check of ptts_admit_row_gen applies to every entry; besides, n < 1 or a slot listed twice is PTTS_E_INVALID, and n above the engine's spare
 *   rows (max_batch - the session's B; ptts_session_begin reserves nothing: create the engine with slots + the largest group) is PTTS_E_CAPACITY.
 *   All checks run before the first launch: a refused call admits nothing and leaves every slot and record as it was. */
int ptts_admit_rows(ptts_engine* e, int32_t n, const int32_t* rows, const float* enc_dev, const int32_t* enc_mask_dev, const float* prompt_dev,
                    const int32_t* prompt_mask_dev, const int32_t* max_lengths, int32_t sample, const ptts_gen_params* const* gps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PTTS_SESSION_H_ */
