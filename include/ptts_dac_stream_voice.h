/*
 * ptts_dac_stream_voice.h - additive to the ABI v8 set of ptts.h (which does not include this header: include it beside ptts.h):
 * streaming a request that continues a voice prompt out of a continuous session. Same conventions as ptts.h; read its section
 * "streaming out of a continuous session" first.
 *
 * Behind a voice prompt of T frames the decoder's raw id buffer does not hold the request's frames: codebook k's columns T+1 .. T+k are raw
 * sampled tokens where the delay pattern (built over BOS + prefix) holds the prompt's codes, so for every frame f < T the true value of
 * codebook k is prefix[k][f], whatever the buffer holds. And a prompt is ready all at once, hundreds of frames, where the codec engine is
 * sized for about one chunk. Hence: the stream table keeps each slot's prefix, absorb reads from two sources, and a pass's emit is capped.
 */
#ifndef PTTS_DAC_STREAM_VOICE_H_
#define PTTS_DAC_STREAM_VOICE_H_

#include "ptts.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ptts_dac_stream_open_voice: ptts_dac_stream_open + per-slot prefix storage [slots][K][max_voice_frames] on the device. The only call of
 *   this header that allocates. max_voice_frames == 0: exactly ptts_dac_stream_open (which in turn drops a prefix storage opened earlier).
 *
 * ptts_dac_stream_reset_voice: ptts_dac_stream_reset, then the request's voice prompt enters the slot (all enqueued):
 *     codes_dev [K, T] int64 un-delayed codes, consumed on the stream (may be NULL iff T == 0)
 *     emit_prompt != 0: the prompt's frames are emitted like any others; 0: they are left context only (see below)
 *   T == 0: exactly ptts_dac_stream_reset. A plain ptts_dac_stream_reset of the slot clears the prefix length: the next request there does
 *   not see the old prefix.
 *   PTTS_E_INVALID with a message, before anything is enqueued: a table opened without prefix storage (T > 0), T < 0, T > max_voice_frames,
 *   NULL codes with T > 0, and what ptts_dac_stream_reset refuses.
 *
 * ptts_dac_stream_decode_capped: ptts_dac_stream_decode with
 *   1. absorb: raw frame f of codebook k is prefix[slot][k][f] for f < T_slot and the ids_dev cell of ptts_dac_stream_decode otherwise. The
 *      filter is the same and applies to prompt frames too (as compact_codes does on the whole utterance), WHEN they are absorbed: a request
 *      that ends with `complete` < T has only that many prompt frames. With emit_prompt == 0 the kept frames with f < T_slot count as emitted
 *      the moment they are absorbed; they stay in the table as left context, and the first sample the slot emits is the first sample of its
 *      first kept generated frame.
 *   2. plan: emit = min(ptts_dac_stream_decode's emit, max_emit).
 *   3. decode: the window is the kept frames [max(0, emitted - halo), min(kept, emitted + emit + halo)): a capped chunk has `halo` real frames
 *      of right context, so its samples are those of the whole-utterance decode, as any non-final chunk's.
 *   A `final` row with more than max_emit frames ready emits max_emit and is NOT flushed: list it again with final = 1 and the same
 *   `complete` until emitted == kept (out_dev gives (emit, kept) per pass; the emits add up to kept, less the kept prompt frames of a slot
 *   whose prompt is not emitted).
 *   Host bounds: ready's bound grows by complete - absorbed (by the part of it at or behind frame T for a slot whose prompt is not emitted)
 *   and after the pass is max(ptts_dac_stream_decode's rule, bound - max_emit). The launch is sized by the largest
 *   min(halo + bound, complete, 2 * halo + max_emit), which must fit max_frames; wave_ld must hold hop * min(bound of emit, max_emit).
 *   ptts_dac_stream_decode is this call without a cap; on a table without prefix storage it runs the kernel instance it always ran.
 *   PTTS_E_INVALID: max_emit < 1, and everything ptts_dac_stream_decode refuses. All checks run before the first launch: a refused call
 *   changes nothing.
 */
int ptts_dac_stream_open_voice(ptts_dac* d, int32_t slots, int32_t cap_frames, int32_t max_voice_frames, void* stream);
int ptts_dac_stream_reset_voice(ptts_dac* d, int32_t slot, const int64_t* codes_dev, int32_t T, int32_t emit_prompt, void* stream);
int ptts_dac_stream_decode_capped(ptts_dac* d, const int64_t* ids_dev, int64_t ids_ld, int32_t col0, int32_t delay,
                                  const ptts_dac_stream_row* rows_host, int32_t R, int32_t halo, float* wave_dev, int64_t wave_ld,
                                  int32_t* out_dev, void* stream, int32_t max_emit);

#ifdef __cplusplus
}
#endif
#endif /* PTTS_DAC_STREAM_VOICE_H_ */
