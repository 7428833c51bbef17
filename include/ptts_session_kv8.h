/*
 * ptts_session_kv8.h - additive to the ABI v8 set of ptts.h and ptts_session.h (neither includes this header: include it beside ptts.h):
 * continuous sessions on the e4m3 self-attention cache (ptts_config::kv_fp8), and a view of the self K/V arena. Same conventions as ptts.h.
 */
#ifndef PTTS_SESSION_KV8_H_
#define PTTS_SESSION_KV8_H_

#include "ptts.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ptts_session_begin_kv8: ptts_session_begin for an engine created with kv_fp8 (which ptts_session_begin refuses with PTTS_E_UNSUPPORTED): the
 *   same checks, the same state afterwards, the same refusal of a pending voice prompt. On an engine WITHOUT kv_fp8 it returns PTTS_E_INVALID
 *   (that engine's entry point is ptts_session_begin). Besides what ptts_session_begin resets, the e4m3 bytes and the scales of positions
 *   [0, P + 1) of every slot, and its cross K/V rows [0, N), are zeroed on the stream, so that an idle slot's discarded step computes on
 *   defined, finite values.
 *   The session it opens is an ordinary one: ptts_admit_row, ptts_admit_row_gen, ptts_admit_rows (which moves 64-byte self rows and the
 *   P + 1 K and V scales per layer and head), ptts_retire_row, ptts_row_state, ptts_decode_steps, ptts_step_forward, ptts_push_tokens,
 *   ptts_logits and ptts_ids behave as documented in ptts.h / ptts_session.h; ptts_prefill ends it. */
int ptts_session_begin_kv8(ptts_engine* e, int32_t B, int32_t N, int32_t P, void* stream);

/*
 * ptts_debug_self_kv: pointers INTO the self-attention K/V arena of one layer (no copies; the ptts_debug_hidden pattern), on any engine, session
 *   or static. *k_dev / *v_dev: [max_batch][kv_heads][cap][row_bytes] bytes, row_bytes = 64 on a kv_fp8 engine (e4m3), else 64 * sizeof(engine
 *   dtype). *kscale_dev / *vscale_dev: [max_batch][kv_heads][cap] float32, one power-of-two scale per cache row; NULL on engines without kv_fp8.
 *   cap = the engine's max_ctx. layer outside [0, num_layers) or a null argument is PTTS_E_INVALID. */
int ptts_debug_self_kv(ptts_engine* e, int32_t layer, void** k_dev, void** v_dev, float** kscale_dev, float** vscale_dev, int32_t* row_bytes,
                       int32_t* kv_heads, int32_t* cap);

#ifdef __cplusplus
}
#endif
#endif /* PTTS_SESSION_KV8_H_ */
