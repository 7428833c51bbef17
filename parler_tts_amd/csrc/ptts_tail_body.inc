// The body of the sampler tail, included into tail_kernel<NV, SESSION>, tail_warp_kernel<NV, SESSION> and their step-record twins
// tail_record_kernel / tail_warp_record_kernel<NV, SESSION> (ptts_lm_kernels.h), which define NV, SESSION, the constants WARP and RECORD and the
// argument struct `p` (TailK<SESSION, WARP>::T; RECORD: TailRK<SESSION, WARP>::T). Not a header: no include guard, no declarations.
// RECORD: the processed scores of every codebook row of this step go to the utterance's record (p.rec[b], ptts_step_record_kernels.h) at step
// cur_len - given. Everything it adds sits behind `if constexpr (RECORD)`: the other instances keep their instructions
// (profiles/device_step_records_isa_compare.txt).
  const TailArgs& a = p;
  __shared__ int s_tok[32];
  int b = blockIdx.x;
  if constexpr (SESSION) b += p.row0;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  // ---- t = 0: every load that does not depend on another load goes in flight together (the step's critical path ends
  // here: lengths / flags / parameters / this wave's logits row are ONE round trip, the embedding rows a second one)
  DevGen g = *a.gen;
  int hrow0 = b * a.K;  // first row index of this utterance in the draw hash
  const int t = a.cur_len[b];  // column the new token is written to; t-1 new tokens generated so far
  // static: "has the reference loop already exited?" = every row finished BEFORE this step. Rows that finish during this very launch
  // (other workgroups, stamp -(t + 1)) still count as active here, so the answer does not depend on workgroup timing.
  // session: is this slot live (read by all before any wave of this workgroup writes a flag)
  int any_local = 0;
  if constexpr (SESSION) {
    any_local = tid < a.K ? (a.unfinished[b * a.K + tid] > 0) : 0;
  } else {
    for (int i = tid; i < a.B * a.K; i += blockDim.x) {
      const int v = a.unfinished[i];
      any_local |= (v > 0) | (v <= -(t + 1));
    }
  }
  const int fu0 = a.first_unf[b];
  DevWarp wp = {0.f, 1.f, 0.f, 0.f};
  if constexpr (WARP) wp = p.warp[b];  // one more load of this batch: its address needs the kernel arguments and b alone
  [[maybe_unused]] float* rs = nullptr;  // RECORD: where this step's K rows of scores go, or null (no record, or a step at or beyond cap_steps)
  [[maybe_unused]] int rcap = 0;
  [[maybe_unused]] long long rstride = 0;
  if constexpr (RECORD) {  // likewise one load of this batch
    const StepRecord sr = p.rec[b];
    rs = sr.scores; rcap = sr.cap_steps; rstride = sr.step_stride;
  }
  DevDims dd = *a.dims;  // the embedding of the next column needs P / max_length / the voice-prompt prefix: fetched now, not after the argmax
  if constexpr (SESSION) {
    dd.max_length = p.row_maxlen[b];  // the pad triangle (and whether there is a pattern at all) follows the request's own length
  }
  if constexpr (SESSION) {
    // the slot's own record rides in the same batch of loads as *gen: both addresses come from kernel arguments alone (without records they
    // fall back on *gen, read twice), and the choice between the two sets of values is made in registers - no flag is waited for first
    // (written BEHIND the other loads of this prologue on purpose: in front of them the compiler ran out of SGPRs for the group and issued
    // row_maxlen[b] behind a wait of its own, profiles/per_request_sampling_isa_compare.txt)
    const bool recs = p.slot_gen != nullptr;
    const DevGen* sgp = recs ? &p.slot_gen[b].g : a.gen;
    const int* sfp = recs ? &p.slot_gen[b].own : &a.gen->max_length;  // {own, row_base}
    const DevGen sg = *sgp;
    const int sown = sfp[0], sbase = sfp[1];
    const bool own = recs && sown != 0;
    g.min_new_tokens = own ? sg.min_new_tokens : g.min_new_tokens; g.do_sample = own ? sg.do_sample : g.do_sample;
    g.top_k = own ? sg.top_k : g.top_k; g.use_eos_gate = own ? sg.use_eos_gate : g.use_eos_gate;
    g.temperature = own ? sg.temperature : g.temperature; g.top_p = own ? sg.top_p : g.top_p;
    g.seed = own ? sg.seed : g.seed;
    hrow0 = own ? sbase : hrow0;
    // the slot's voice-prompt length, the same way: a load of this batch whose address needs the kernel arguments alone (without the array
    // one more read of *gen), the zero of "no prefix" chosen in a register. What follows it: the min_new_tokens count and what the model is
    // fed for the next column (s_tok below); the ids written stay the raw sampled tokens
    const bool pres = p.slot_tprefix != nullptr;
    const int* tpp = pres ? &p.slot_tprefix[b] : &a.gen->max_length;
    const int stp = *tpp;
    dd.T_prefix = pres ? stp : 0;
  }
  const int t_prefix = dd.T_prefix;
  const int he = lane < a.K ? a.has_eos[b * a.K + lane] : 0;  // every wave: the K EOS flags of this utterance
  float lg[NV];
  const int k0 = w;  // greedy: wave w starts with codebook row w
  if (k0 < a.K) {
    const float* sc0 = a.logits + (size_t)(b * a.K + k0) * a.V;
#pragma unroll
    for (int i = 0; i < NV; ++i) lg[i] = (lane + 64 * i < a.V) ? sc0[lane + 64 * i] : -INFINITY;
  }
  const int unf0 = k0 < a.K ? (a.unfinished[b * a.K + k0] > 0) : 0;
  // static: every row of every utterance finished, the reference loop has exited (no-op step); session: idle or finished slot
  if (!__syncthreads_or(any_local)) return;

  int fu = fu0;
  if (__shfl(he, fu0) > 0 && fu0 < a.K - 1) fu += 1;  // logits_processors.py:48 (advance <= 1 per step)
  if (tid == 0) a.first_unf[b] = fu;
  const bool block_eos_all = (t - 1 - t_prefix) < g.min_new_tokens;  // new tokens = columns after the (1 + T_prefix) given ones
  if constexpr (RECORD) {  // step index = cur_len - given; the engine never writes at or beyond cap_steps records
    const int ridx = t - 1 - t_prefix;
    rs = (rs && ridx >= 0 && ridx < rcap) ? rs + (size_t)ridx * (size_t)rstride : nullptr;
  }

  // one wave per codebook row, no workgroup barrier until every row has its token. greedy: torch.argmax semantics (first
  // index on ties); do_sample: the warpers + multinomial on the same wave (wave_sample_row)
  for (int k = w; k < a.K; k += (int)(blockDim.x >> 6)) {
    const int row = b * a.K + k;
    if (k != k0) {
      const float* sc = a.logits + (size_t)row * a.V;
#pragma unroll
      for (int i = 0; i < NV; ++i) lg[i] = (lane + 64 * i < a.V) ? sc[lane + 64 * i] : -INFINITY;
    }
    const bool eos_blocked = block_eos_all || (g.use_eos_gate && k > fu);
    int widx;
    if (!g.do_sample) {
      float best = -INFINITY;
      int bi = 0x7fffffff;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int v = lane + 64 * i;
        float x = lg[i];
        if (eos_blocked && v == a.eos) x = -INFINITY;
        if constexpr (RECORD) {  // greedy: the logits as read, -inf at the blocked EOS, every other entry with its bits
          if (rs && v < a.V) rs[(size_t)k * a.V + v] = x;
        }
        if (v < a.V && (x > best || (x == best && v < bi))) { best = x; bi = v; }
      }
      const float wbest = wave_max(best);
      const float cand = (best == wbest) ? (float)bi : 3.0e9f;  // vocabulary indices are exact in fp32
      widx = (int)(-wave_max(-cand));
    } else {
      const int hrow = SESSION ? hrow0 + k : row;  // a slot with its own record: the codebook index inside the slot
      const unsigned long long hsh = splitmix64(g.seed ^ splitmix64(((unsigned long long)t << 32) ^ (unsigned long long)hrow));
      const float u = (float)((hsh >> 40) + 0.5) * (1.0f / 16777216.0f);  // [2^-25, 1], DESIGN.md 4.6
      if constexpr (RECORD) widx = wave_sample_row<NV, WARP, true>(lg, a.V, lane, g, eos_blocked, a.eos, u, wp, rs ? rs + (size_t)k * a.V : nullptr);
      else if constexpr (WARP) widx = wave_sample_row<NV, true>(lg, a.V, lane, g, eos_blocked, a.eos, u, wp);
      else widx = wave_sample_row<NV>(lg, a.V, lane, g, eos_blocked, a.eos, u);
    }
    if (lane == 0) {
      const int unf = k == k0 ? unf0 : (a.unfinished[row] > 0);
      const int nxt = unf ? widx : a.pad;  // next_tokens * unfinished + pad * (1 - unfinished)
      a.ids[(size_t)row * a.ids_ld + t] = nxt;
      s_tok[k] = nxt;
      if constexpr (SESSION) {
        // behind a voice prompt the model is FED the shifted prompt code while the pattern holds one for this codebook (the first K - 1 steps of
        // such a slot; BOS / PAD still win in tail_embed_rows); what is stored stays the raw token. Resolved here, by the one lane that owns the
        // codebook and only for such a slot, so that the embedding below keeps its one batch of table-row loads (see there)
        // (the pointer and the stride are read HERE, through volatile, not taken from the prologue's copy of *dims: kept live from there through
        // the token loop they cost the prologue its load groups - profiles/session_voice_isa_compare.txt)
        if (t - k - 1 < t_prefix && t > k && dd.max_length >= 2 * a.K - 1) {
          const long long* pf = *reinterpret_cast<const long long* const volatile*>(&a.dims->prefix);
          const int pld = *reinterpret_cast<const volatile int*>(&a.dims->prefix_ld);
          s_tok[k] = (int)pf[(size_t)row * pld + (t - k - 1)];
        }
      }
      if (nxt == a.eos) a.has_eos[row] = 1;
      // EosTokenCriteria | MaxLengthCriteria (the slot's own length in a session)
      if (unf && ((nxt == a.eos) || (t + 1 >= (SESSION ? dd.max_length : g.max_length)))) a.unfinished[row] = -(t + 1);
    }
  }
  __syncthreads();
  if (tid == 0) a.cur_len[b] = t + 1;
  if constexpr (SESSION) dd.T_prefix = 0;  // s_tok already holds the prompt codes: no load of them between the table rows' loads
  tail_embed_next(a, dd, b, t, s_tok, tid);
