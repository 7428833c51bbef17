/*
 * ptts_warp.h - additive to the ABI v8 set of ptts.h (which does not include this header: include it beside ptts.h):
 * transformers' min_p, typical_p, epsilon_cutoff and eta_cutoff applied on the device, inside the sampler tail behind top-p, for static
 * calls (ptts_prefill + ptts_decode_steps) and per request inside a continuous session. Same conventions as ptts.h.
 */
#ifndef PTTS_WARP_H_
#define PTTS_WARP_H_

#include "ptts.h"

#ifdef __cplusplus
extern "C" {
#endif

/* min_p in [0, 1], 0 = none. typical_p in (0, 1], 1 = none. epsilon_cutoff, eta_cutoff in [0, 1), 0 = none. (0, 1, 0, 0) is the neutral
 * record: the tail draws the token it draws without the feature. */
typedef struct {
  float min_p;
  float typical_p;
  float epsilon_cutoff;
  float eta_cutoff;
} ptts_sample_warp;

/*
 * What the tail computes for a sampled row (do_sample != 0; a greedy row ignores the record), behind temperature, top-k and top-p, in
 * transformers' order MinP -> Typical -> Epsilon -> Eta, each stage on the distribution renormalised over the survivors of the one before
 * (p_i over the survivors, H = -sum p ln p), a stage at its neutral value skipped:
 *   min_p:          drop i iff p_i < min_p * p_max;
 *   typical_p:      s_i = |-ln p_i - H|; keep i iff the mass of {j : s_j < s_i} is < typical_p (ties at the boundary stay, the smallest s stays);
 *   epsilon_cutoff: drop i iff p_i < epsilon_cutoff and its score is below the largest surviving score;
 *   eta_cutoff:     the same with eta = min(eta_cutoff, sqrt(eta_cutoff) * exp(-H)).
 * The tail is the same kernel node as without the feature (another instance of it): ptts_debug_graph_nodes does not change.
 *
 * ptts_set_sample_warp: w == NULL switches the feature off (the state of a new engine): every tail launch and every step graph is exactly
 *   that of an engine that never heard of it. w != NULL switches it on with *w as the record of every utterance; neutral values are allowed
 *   (how a session is opened when only some requests will bring warpers). Call it before ptts_prefill / ptts_session_begin*.
 *   Inside a running session - one in which a slot holds a request - PTTS_E_INVALID: the tail instance of a session is fixed at its begin
 *   (retire its requests first; a session whose slots are all idle may be reconfigured, e.g. in front of the next ptts_session_begin*).
 *   Values out of range or not finite: PTTS_E_INVALID. A refused call changes nothing. Works together with ptts_set_history_penalty.
 */
int ptts_set_sample_warp(ptts_engine* e, const ptts_sample_warp* w, void* stream);

/*
 * ptts_set_slot_sample_warp: the record the NEXT admission into slot `row` runs under, its own first-token tail included (any entry point:
 *   ptts_admit_row, _gen, _voice, ptts_admit_rows). w == NULL restores the session's default (the values of ptts_set_sample_warp), as
 *   session begin and ptts_retire_row do. Refusals: no session, or a session begun with the feature off; row outside the session; a busy
 *   slot; values out of range: PTTS_E_INVALID. A refused call changes nothing.
 */
int ptts_set_slot_sample_warp(ptts_engine* e, int32_t row, const ptts_sample_warp* w, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PTTS_WARP_H_ */
