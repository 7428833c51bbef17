// Decoder-LM engine behind the C ABI of include/ptts.h: packed weights, static KV arena, device-resident
// sampler state, one captured hipGraph per batch size. Replaces ParlerTTSForCausalLM.forward + the
// transformers `_sample` loop of the reference (modeling_parler_tts.py:1865, :3564).
#include <array>
#include <map>
#include <set>
#include <string>
#include <type_traits>
#include <vector>

#include "ptts_common.h"
#include "../../include/ptts_session_kv8.h"
#include "../../include/ptts_session_voice.h"
#include "../../include/ptts_session_voice_rows.h"
#include "../../include/ptts_penalty.h"
#include "../../include/ptts_warp.h"
#include "../../include/ptts_logit_edit.h"
#include "../../include/ptts_score.h"
#include "../../include/ptts_step_record.h"
#include "ptts_lm_kernels.h"
#include "ptts_gemv.h"
#include "ptts_step_plan.h"
#include "ptts_strip_w8.h"
#include "ptts_gemm_launch.h"
#include "ptts_tail_launch.h"
#include "ptts_penalty_launch.h"
#include "ptts_logit_edit_launch.h"
#include "ptts_step_record_launch.h"
#include "ptts_score_launch.h"

thread_local std::string g_ptts_err;
int ptts_fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_ptts_err = buf;
  return code;
}
extern "C" const char* ptts_last_error(void) { return g_ptts_err.c_str(); }
extern "C" int ptts_abi_version(void) { return PTTS_ABI_VERSION; }

namespace {

struct LayerW {
  void *qkv = nullptr, *o = nullptr, *cq = nullptr, *ckv = nullptr, *co = nullptr, *fc1 = nullptr, *fc2 = nullptr;
  float *ln1_g = nullptr, *ln1_b = nullptr, *ln2_g = nullptr, *ln2_b = nullptr, *ln3_g = nullptr, *ln3_b = nullptr;
  void *k_self = nullptr, *v_self = nullptr, *k_cross = nullptr, *v_cross = nullptr;
  float *ks_self = nullptr, *vs_self = nullptr;  // kv_fp8 engines: one power-of-two scale per (utterance, K/V head, position) of the e4m3 self cache
  // row-major [N][K] copies in the engine dtype for the single-utterance GEMV step (ptts_gemv_kernels.h); null = path off
  void *qkv_rm = nullptr, *o_rm = nullptr, *cq_rm = nullptr, *co_rm = nullptr, *fc1_rm = nullptr, *fc2_rm = nullptr;
  // weights_fp8: the row-major copies hold OCP e4m3 bytes, one power-of-two scale per output row
  float *qkv_sc = nullptr, *o_sc = nullptr, *cq_sc = nullptr, *co_sc = nullptr, *fc1_sc = nullptr, *fc2_sc = nullptr;
  // weights_fp8, engines that decode on the MFMA strips (max_batch > GV_MAX_ROWS): e4m3 strips [N/16][K/64][64][16 B] (same scales).
  // The cross q projection stays bf16: it lives inside the fused cross-block kernel.
  void *qkv_p8 = nullptr, *o_p8 = nullptr, *co_p8 = nullptr, *fc1_p8 = nullptr, *fc2_p8 = nullptr;
  void *xM = nullptr, *xU = nullptr;  // folded cross-attention of the current single utterance: M [heads*NE][H], U [H][heads*NE] (engine dtype)
};

}  // namespace

struct ptts_engine {
  ptts_config cfg;
  int max_prompt = 0;  // P + 1 rows capacity per utterance
  size_t esize = 4;
  hipStream_t own_stream = nullptr;
  hipEvent_t ev_first = nullptr;                  // first token of the last prefill materialised (recorded right after the sampler tail)
  hipEvent_t ev_tail0 = nullptr;                  // recorded right before that sampler tail (ptts_first_token_times)
  hipEvent_t ev_pre0 = nullptr;                   // recorded when the stream reaches the last ptts_prefill's first piece of work
  bool first_recorded = false;
  std::vector<void*> allocs;
  std::vector<LayerW> L;
  void* embed = nullptr;       // [K][V+1][H]
  float* pos_table = nullptr;  // [max_pos][H]
  float *rope_cos = nullptr, *rope_sin = nullptr;
  float *lnf_g = nullptr, *lnf_b = nullptr;
  void* heads = nullptr;  // [K*V][H] packed
  void* heads_rm = nullptr;  // [K*V][H] row-major (GEMV step)
  void* heads_p8 = nullptr;  // [K*V][H] e4m3 strips (weights_fp8, MFMA decode)
  float* heads_sc = nullptr;
  StepSwitches sw;           // the environment switches, read once at create (read_env_switches)
  StepConfig sc = {};        // what create derives once from cfg (step_config): which step kernels this engine runs, split factors, K/V heads
  KvLayer* kv_layers = nullptr;      // [layers] operands of the batched cross K/V projection (device memory, written once at create)
  FoldLayer* fold_layers = nullptr;  // [layers] operand pointers of the fold kernels (device memory, written once at create)
  bool xfold_valid = false;  // the folded matrices of the CURRENT call are in place (single utterance)
  std::set<std::string> loaded_fp8, required_fp8;
  std::set<std::string> loaded, required;
  // scratch
  float *h = nullptr, *qkv = nullptr, *qc = nullptr, *part = nullptr, *stats = nullptr, *ffn = nullptr, *logits = nullptr;
  float* sort_buf = nullptr;
  void *xw = nullptr, *xw2 = nullptr;  // engine-dtype activation rows for the M > 8 path: [rows][H], [rows][F]
  long long* prefix = nullptr;         // voice-prompt codes [max_batch*K][max_ctx], valid for the next prefill when pending_T > 0
  int pending_T = 0;
  float* lnstat = nullptr;             // strip statistics of the residual rows (EPI_RESID -> PRO_LNS), [max_batch][H/16][2]
  // state
  long long* ids = nullptr;
  int ids_ld = 0;
  int *cur_len = nullptr, *unfinished = nullptr, *has_eos = nullptr, *first_unf = nullptr;
  int *enc_mask = nullptr, *prompt_mask = nullptr;
  DevDims* dims = nullptr;
  DevGen* gen = nullptr;
  ptts_gen_params gp;
  // per-call
  int B = 0, N = 0, P = 0;
  bool prefilled = false;
  bool h_ready = false;  // residual-stream input of the next decode step already embedded by the last tail
  int last_graph_nodes = 0;   // kernel nodes of the step graph captured last (ptts_debug_graph_nodes)
  float* xpart = nullptr;     // [nheads][H] per-head partial rows of the fused cross block
  float* h2 = nullptr;        // [H] residual row after the cross block (x + partial rows), written by the LN3 + fc1 node
  int kv_ub = 0;         // host-side upper bound of the self-KV positions written so far (prefill + one per decode forward)
  int kv_bound = 0;      // attention fetch bound of the next decode forward: kv_ub + 1 rounded up to 64, <= max_ctx
  std::map<long long, hipGraphExec_t> graphs;  // key: 2 * batch size + folded-cross-block flag + context bucket + session / penalty / warper bits (get_graph)
  int* host_pinned = nullptr;
  // continuous session (ptts_session_begin): every slot of the batch has its own clock, end and fetch bound
  bool session = false;
  int session_max_length = 0;            // max_length of the generation parameters the session was opened with
  int* row_maxlen = nullptr;             // [max_batch] device: max_length of the request in each slot
  SlotGen* slot_gen = nullptr;           // [max_batch] device: sampler record of the request in each slot (ptts_admit_row_gen); own = 0: the session's
  int* slot_T = nullptr;                 // [max_batch] device: voice-prompt frames of the request in each slot (ptts_admit_row_voice); 0: none
  DevDims* dims_adm = nullptr;           // [max_batch] device: per arena row, the DevDims a voice admission's prefill embedding reads for the request that runs on it
                                         // (its max_length, T, prefix rows; FwdView::row_dims): the slot itself in place, entries B .. B + n - 1 for a group on the spare rows
  float* h_adm = nullptr;                // [max_prompt][H] residual rows of a row prefill: the step input h[B][H] of the other slots is live between steps
  KvLayer* kv_layers_rows = nullptr;     // [max_batch][layers] operands of the batched cross K/V projection with each slot's arena rows as base
  float* h_adm_rows = nullptr;           // [(max_batch - 1) * max_prompt][H] residual rows of a group prefill (ptts_admit_rows), allocated at its first use
  AdmitMoveLayer* move_layers = nullptr; // [layers] arena bases of admit_move_rows_kernel, written with h_adm_rows
  AdmitScaleLayer* move_scales = nullptr; // [layers] kv_fp8 engines: scale arrays of admit_move_scales_kernel, written with h_adm_rows
  std::vector<char> slot_busy;           // host: admitted and not yet retired
  std::vector<int> slot_ub, slot_maxlen; // host: upper bound of the slot's self-KV positions (P + 1 + steps since admission), its max_length
  // history penalties (ptts_penalty.h): one node in front of every sampler tail while pen_on
  HistoryPenalty* pen = nullptr;         // [max_batch] device: the record of each utterance / slot; allocated at the first switch-on, the step graphs hold the pointer
  bool pen_on = false;                   // the node is part of every tail (and of the step graph: its own key bit)
  HistoryPenalty pen_default = {1.0f, 0}; // the values of ptts_set_history_penalty: every utterance of a static call, a slot without a request's own
  // sampling warpers (ptts_warp.h): every tail launch is the WARP instance while warp_on
  DevWarp* warp = nullptr;               // [max_batch] device: the record of each utterance / slot; allocated at the first switch-on, the step graphs hold the pointer
  bool warp_on = false;                  // the tail of every launch (and of the step graph: its own key bit) is tail_warp_kernel<NV, SESSION>
  DevWarp warp_default = {0.f, 1.f, 0.f, 0.f};  // the values of ptts_set_sample_warp
  // logit edits (ptts_logit_edit.h): one node between the penalty node and every sampler tail while le_on
  LogitEditRecs le = {};                 // device: max_batch + 1 records - each utterance's / slot's, then (index max_batch) the values of ptts_set_logit_edits;
                                         // allocated at the first switch-on, the step graphs hold the pointers
  bool le_on = false;                    // the node is part of every tail (and of the step graph: its own key bit)
  bool le_ready = false;                 // every array of `le` is allocated and zeroed (ensure_logit_edit_records)
  unsigned char* le_stage = nullptr;     // pinned host: one staging area per record, what its last upload copies from
  size_t le_stage_stride = 0;
  std::vector<hipEvent_t> le_ev;         // per record: the end of that upload (waited for before the area is written again)
  // step records (ptts_step_record.h): the raw-logits node in front of the penalty node while rec_node, the RECORD tail instances while rec_tail
  StepRecord* rec = nullptr;             // [max_batch] device: the record of each utterance / slot; allocated at the first switch-on, the step graphs hold the pointer
  bool rec_on = false;                   // ptts_set_step_records(non-null) holds
  bool rec_node = false, rec_tail = false;  // what every tail launch (and the step graph: a key bit each) carries: both in a session, by the arenas given in a static call
  ptts_step_records rec_call = {};       // the arenas of ptts_set_step_records: laid out over the batch at the next ptts_prefill
#ifdef PTTS_TIMING
  long long* dbg_stamps = nullptr;  // measurement build: [layers + 1][5 or 7 nodes][3 workgroups][16] wall-clock stamps of the decode step (ptts_debug_stamps)
#endif

  template <typename T> int alloc(T** p, size_t n) {
    void* v = nullptr;
    hipError_t e = hipMalloc(&v, n * sizeof(T) > 0 ? n * sizeof(T) : 16);
    if (e != hipSuccess) return ptts_fail(PTTS_E_HIP, "hipMalloc(%zu bytes) failed: %s", n * sizeof(T), hipGetErrorString(e));
    allocs.push_back(v);
    *p = reinterpret_cast<T*>(v);
    return PTTS_OK;
  }
  int alloc_bytes(void** p, size_t bytes) {
    char* c = nullptr;
    PTTS_TRY(alloc(&c, bytes));
    *p = c;
    return PTTS_OK;
  }
};

namespace {

// What one forward pass addresses: the whole engine (whole_view) or a few arena rows of it (rows_view). A caller that wants a pass somewhere
// else builds another view; the engine itself is never edited to aim one.
struct FwdView {
  int B, N, P;
  int T;                         // voice-prompt columns folded into this prefill pass (batched multi-column prefill)
  int kv_bound;                  // attention fetch bound of a decode forward
  bool session, xfold_valid;
  float *h, *logits;             // residual rows [B * Q][H]; logits [B][K * V]
  long long* ids;
  int *cur_len, *unfinished, *has_eos, *first_unf, *enc_mask, *prompt_mask;
  const KvLayer* kv_layers;      // [layers] operands of the batched cross K/V projection
  const DevDims* row_dims;       // [B] or null. A voice admission (one request or a group): every row of the prefill pass under its own request -
                                 // its delay pattern, its T <= v.T columns (the rest of the row is padding), and the position its logits come from
  size_t self_off, cross_off;    // bytes from a layer's self / cross K/V arena to utterance 0 of this view
  size_t scale_off;              // kv_fp8 engines: floats from a layer's K / V scale array (LayerW::ks_self, vs_self) to utterance 0 of this view
};

// the whole engine, now
FwdView whole_view(const ptts_engine* e) {
  FwdView v = {};
  v.B = e->B; v.N = e->N; v.P = e->P; v.kv_bound = e->kv_bound; v.session = e->session; v.xfold_valid = e->xfold_valid;
  v.h = e->h; v.logits = e->logits; v.ids = e->ids; v.cur_len = e->cur_len; v.unfinished = e->unfinished; v.has_eos = e->has_eos;
  v.first_unf = e->first_unf; v.enc_mask = e->enc_mask; v.prompt_mask = e->prompt_mask; v.kv_layers = e->kv_layers;
  return v;
}

// Rows [row, row + n) of a session's engine as an n-utterance engine: the prefill kernels address utterance 0 of what they are given. The
// residual rows go to `h` (h_adm, h_adm_rows), because e->h[B][H] holds the other slots' next step input.
FwdView rows_view(const ptts_engine* e, int row, int n, float* h) {
  const ptts_config& c = e->cfg;
  const size_t r = (size_t)row, K = (size_t)c.num_codebooks;
  FwdView v = whole_view(e);
  v.B = n; v.h = h; v.kv_layers = e->kv_layers_rows + r * c.num_layers;
  v.ids += r * K * e->ids_ld; v.cur_len += r; v.first_unf += r; v.unfinished += r * K; v.has_eos += r * K;
  v.logits += r * K * c.vocab_size; v.enc_mask += r * c.max_enc; v.prompt_mask += r * e->max_prompt;
  // an e4m3 self row is 64 bytes with one scale beside it; the cross arena stays in the engine dtype
  v.self_off = r * e->sc.nkv * c.max_ctx * 64 * (c.kv_fp8 ? 1 : e->esize); v.cross_off = r * e->sc.nkc * c.max_enc * 64 * e->esize;
  v.scale_off = r * e->sc.nkv * c.max_ctx;
  return v;
}

inline void* at(void* p, size_t off) { return static_cast<char*>(p) + off; }
inline float* scale_at(float* p, size_t off) { return p ? p + off : nullptr; }  // null = engine-dtype cache: stays null

#ifdef PTTS_TIMING  // measurement build: node number `node_` of the decode step stamps into its own 48 slots of e->dbg_stamps
#define PTTS_DBG_STAMP(args, on_, node_) (args).dbg = (e->dbg_stamps && (on_)) ? e->dbg_stamps + (node_) * 48 : nullptr
#else
#define PTTS_DBG_STAMP(args, on_, node_) do { } while (0)
#endif

// (launch_status, launch_lnproj and launch_xattn_fused: ptts_gemm_launch.h, shared with tests/native/step_harness.hip)

// rows_prep node (LayerNorm, or the split-KV combine) into e->xw, then the GEMM with copy staging
template <typename WT, int PRO, int EPI>
int prep_copy_gemm(const ptts_engine* e, GemmArgs g, hipStream_t st) {
  GemmArgs gp = g;
  gp.out_fo = g.x_fo;  // the prep kernel writes the rows in the order the consumer reads them (x_fo set by the caller: decode, batch > 8)
  PTTS_TRY((launch_prep<WT, PRO>(gp, e->xw, st)));
  g.x = reinterpret_cast<const float*>(e->xw);
  g.x_ld = g.K; g.x_row_mul = 1; g.x_row_off = 0;
  return launch_gemm<WT, PRO_COPY, EPI>(g, st);
}

// LayerNorm -> GEMM as the plan chose it (ptts_step_plan.h: pro_gemm)
template <typename WT, int EPI>
int ln_gemm(const ptts_engine* e, const GemmArgs& g, int how, hipStream_t st) {
  switch (how) {
    case PG_FUSED: return launch_gemm<WT, PRO_LN, EPI>(g, st);
    case PG_LNS: return launch_gemm<WT, PRO_LNS, EPI>(g, st);
    default: return prep_copy_gemm<WT, PRO_LN, EPI>(e, g, st);
  }
}

// Causal self-attention of layer `w` over the view's rows of the KV arena, Q positions per utterance from the QKV rows in e->qkv, RoPE fused: a
// decode pass appends the new position and splits the context S_self ways; a prefill reads the rows written before it and never splits (S: the plan's)
AttnArgs self_attn_args(const ptts_engine* e, const FwdView& v, const LayerW& w, int Q, bool prefill, int fo, int S) {
  const ptts_config& c = e->cfg;
  const int H = c.hidden_size, nh = c.num_heads, nkv = e->sc.nkv, Hkv = nkv * 64, QKV = H + 2 * Hkv;
  AttnArgs a = {};
  a.q = e->qkv; a.q_ld = QKV; a.knew = e->qkv + H; a.vnew = e->qkv + H + Hkv; a.kv_ld = QKV; a.kv_heads = nkv; a.n_rep = nh / nkv;
  a.kcache = at(w.k_self, v.self_off); a.vcache = at(w.v_self, v.self_off); a.cap = c.max_ctx; a.kv_bound = prefill ? c.max_ctx : v.kv_bound;
  a.cur_len = prefill ? nullptr : v.cur_len; a.dims = e->dims;
  a.mask = v.prompt_mask; a.mask_ld = e->max_prompt;
  a.cos = c.rope ? e->rope_cos : nullptr; a.sin = c.rope ? e->rope_sin : nullptr;
  a.part = e->part; a.stats = e->stats; a.S = S; a.Q = Q; a.nheads = nh; a.H = H; a.cross = 0;
  a.fused_append = prefill ? 0 : 1; a.scale = 1.0f / sqrtf((float)(H / nh)); a.kscale = scale_at(w.ks_self, v.scale_off); a.vscale = scale_at(w.vs_self, v.scale_off);
  a.direct_out = S == 1 ? e->xw : nullptr; a.out_fo = fo;
  return a;
}

// Cross-attention of layer `w` against the static description K/V, queries in e->qc. The description is short: never split, softmax finished
// in the attention kernel.
AttnArgs cross_attn_args(const ptts_engine* e, const FwdView& v, const LayerW& w, int Q, bool prefill, int fo) {
  const ptts_config& c = e->cfg;
  const int H = c.hidden_size, nh = c.num_heads, nkc = e->sc.nkc;
  AttnArgs a = {};
  a.q = e->qc; a.q_ld = H; a.kcache = at(w.k_cross, v.cross_off); a.vcache = at(w.v_cross, v.cross_off); a.cap = c.max_enc; a.kv_bound = c.max_enc;
  a.cur_len = prefill ? nullptr : v.cur_len; a.dims = e->dims; a.mask = v.enc_mask; a.mask_ld = c.max_enc;
  a.cos = c.rope ? e->rope_cos : nullptr; a.sin = c.rope ? e->rope_sin : nullptr;  // quirk: q rotated, keys not (:858 vs :880)
  a.part = e->part; a.stats = e->stats; a.S = 1; a.Q = Q; a.nheads = nh; a.H = H; a.cross = 1; a.kv_heads = nkc; a.n_rep = nh / nkc;
  a.fused_append = 0; a.scale = 1.0f / sqrtf((float)(H / nh)); a.direct_out = e->xw; a.out_fo = fo;
  return a;
}

// cross-attention K/V of the description, once per prefill (:877-878 then reused :872-875)
template <typename WT>
int project_cross_kv(const ptts_engine* e, FwdView v, hipStream_t st) {
  const ptts_config& c = e->cfg;
  const int H = c.hidden_size, nkc = e->sc.nkc, B = v.B;
  // encoder states were staged into qc by stage_inputs (fp32 row-major [B*N][H]); convert once to the engine dtype
  const size_t n = (size_t)B * v.N * H;
  hipLaunchKernelGGL((convert_kernel<WT, float>), dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, st, e->qc,
                     reinterpret_cast<WT*>(e->xw2), n);
  // every layer's K/V projection in ONE launch (blockIdx.z = layer): the strip kernel up to 256 rows, the bf16 engine's LDS-DMA GEMM above (round 6:
  // 24 launches of ~17 us at 32 descriptions x 64 tokens were one tenth of that prefill; a shape the GEMM declines falls back to the strips)
  const bool one_launch = (B * v.N <= 256 || (sizeof(WT) == 2 && H % 64 == 0 && (2 * nkc * 64) % 64 == 0));
  for (int l = 0; l < (one_launch ? 1 : c.num_layers); ++l) {
    GemmArgs g = {};
    g.W = e->L[l].ckv; g.M = B * v.N; g.N = 2 * nkc * 64; g.K = H;
    g.x = reinterpret_cast<const float*>(e->xw2); g.x_ld = H; g.x_row_mul = 1; g.x_row_off = 0;
    g.kcache = at(e->L[l].k_cross, v.cross_off); g.vcache = at(e->L[l].v_cross, v.cross_off); g.kv_rows_per_b = v.N; g.kv_cap = c.max_enc; g.nheads = nkc;
    if (one_launch) { g.kv_layers = v.kv_layers; g.kv_nlayers = c.num_layers; }
    PTTS_TRY((launch_gemm<WT, PRO_COPY, EPI_KV>(g, st)));
  }
  return PTTS_OK;
}

// the residual-stream input: Q positions per utterance at prefill (prompt rows staged in ffn + the BOS / voice-prompt columns), the last column at decode
template <typename WT>
void launch_embed(const ptts_engine* e, FwdView v, bool prefill, int Q, hipStream_t st) {
  const ptts_config& c = e->cfg;
  EmbedArgs ea = {};
  ea.tables = e->embed; ea.pos_table = c.rope ? nullptr : e->pos_table; ea.prompt = prefill ? e->ffn : nullptr;
  ea.ids = v.ids; ea.ids_ld = e->ids_ld; ea.cur_len = v.cur_len; ea.dims = e->dims; ea.h = v.h;
  ea.H = c.hidden_size; ea.K = c.num_codebooks; ea.V1 = c.vocab_size + 1; ea.bos = c.bos_token_id; ea.pad = c.pad_token_id;
  ea.prefill = prefill ? 1 : 0;
  if (prefill && v.row_dims)  // every row of the pass under its own request's delay pattern and prefix length
    hipLaunchKernelGGL((embed_rows_kernel<WT>), dim3(Q, v.B), dim3(256), 0, st, ea, v.row_dims);
  else if (v.session && !prefill)  // every slot under its own request's delay pattern
    hipLaunchKernelGGL((embed_kernel<WT, true>), dim3(1, v.B), dim3(256), 0, st, EmbedSessionArgs{ea, e->row_maxlen, e->slot_T});
  else
    hipLaunchKernelGGL((embed_kernel<WT, false>), dim3(Q, v.B), dim3(256), 0, st, ea);
}

// Decode step of 1..gemv_rows utterances up to the logits: row-per-wave GEMV / attention nodes, every weight matrix spread over all CUs and read
// once. Which nodes: the plan (ptts_step_plan.h: gemv_plan); this walker fills their arguments and launches them.
template <typename WT>
int gemv_step(const ptts_engine* e, FwdView v, const GemvPlan& p, hipStream_t st) {
  const ptts_config& c = e->cfg;
  const int H = c.hidden_size, F = c.ffn_dim, nh = c.num_heads, M = p.M;
  const int nkv = e->sc.nkv, nkc = e->sc.nkc, QKV = H + 2 * nkv * 64;  // grouped-query attention: fewer K/V heads
  const float scale = 1.0f / sqrtf((float)(H / nh));
  auto gv = [&](const GemvNode& n, GemvArgs g, const char* what) -> int {
    g.M = M; g.N = n.N; g.K = n.K;
    const int rc_ = ptts_gemv_launch(n.mode, n.pro, n.epi, n.S, g, st);
    if (rc_ == -1) return ptts_fail(PTTS_E_UNSUPPORTED, "gemv: no instance for %s (N=%d K=%d M=%d)", what, g.N, g.K, M);
    if (rc_ != 0) return ptts_fail(PTTS_E_HIP, "gemv launch failed (%s)", what);
    return PTTS_OK;
  };
#define PTTS_DBG_NODE(args, l_, k_) PTTS_DBG_STAMP(args, M == 1, (size_t)(l_) * 5 + (k_))
  for (int l = 0; l < c.num_layers; ++l) {
    const LayerW& w = e->L[l];
    if (p.fuse_qa) {  // LN1 + the head's q / k / v rows + split-KV self-attention + append in ONE node (qkv_attn_kernel), then combine + out_proj
      QkvAttnArgs q = {};
      q.W = w.qkv_rm; q.wscale = w.qkv_sc; q.x = v.h; q.gamma = w.ln1_g; q.beta = w.ln1_b;
      q.kcache = at(w.k_self, v.self_off); q.vcache = at(w.v_self, v.self_off); q.cur_len = v.cur_len; q.P = &e->dims->P; q.mask = v.prompt_mask;
      q.part = e->part; q.stats = e->stats; q.cap = c.max_ctx; q.kv_bound = v.kv_bound; q.mask_ld = e->max_prompt;
      q.S = p.S_f; q.nheads = nh; q.H = H; q.kv_heads = nkv; q.scale = scale; q.M = M; q.x_ld = H;
      PTTS_DBG_NODE(q, l, 0);
      if (ptts_qkvattn_launch(p.mode, q, st) != 0) return ptts_fail(PTTS_E_HIP, "qkv_attn launch failed");
    } else {
      GemvArgs g = {};  // LN1 + fused QKV projection (:1020-1021, :848-850)
      g.W = w.qkv_rm; g.wscale = w.qkv_sc; g.x = v.h; g.x_ld = H; g.gamma = w.ln1_g; g.beta = w.ln1_b; g.out = e->qkv; g.out_ld = QKV;
      PTTS_TRY(gv(p.qkv, g, "LN1+QKV"));
      // causal self-attention over the KV arena, fused RoPE + append
      PTTS_TRY((launch_attn<WT>(self_attn_args(e, v, w, 1, false, 0, p.S_self), M, st)));
    }
    {  // [combine splits] + out_proj + residual (:1034): the activation rows of an unsplit attention, or the partials of the node before
      GemvArgs g = {};
      g.W = w.o_rm; g.wscale = w.o_sc; g.out = v.h; g.out_ld = H;
      if (p.out_proj.pro == GV_COPY) { g.xw = e->xw; g.xw_ld = H; }
      else { g.part = e->part; g.stats = e->stats; g.nheads = nh; }
      PTTS_DBG_NODE(g, l, 1);
      PTTS_TRY(gv(p.out_proj, g, "[combine+]out_proj"));
    }
    switch (p.cross) {
      case XFOLD_ONE_NODE: {  // folded cross block as ONE node: LN2 + the head's rows of M + softmax + the head's columns of U -> xpart[h][:]
        XfoldAttnArgs x = {};
        x.Mw = w.xM; x.Uw = w.xU; x.x = v.h; x.gamma = w.ln2_g; x.beta = w.ln2_b; x.mask = v.enc_mask; x.n_valid = &e->dims->N;
        x.xpart = e->xpart; x.nheads = nh; x.H = H; x.nur = p.fuse_x_nur;
        PTTS_DBG_NODE(x, l, 2);
        if (ptts_xfoldattn_launch(p.fold_mode, x, st) != 0) return ptts_fail(PTTS_E_HIP, "xfold_attn launch failed");
        break;
      }
      case XFOLD_TWO_NODES: {  // folded cross block (xfold_*_kernel at prefill): LN2 + (K Wq) x -> base-2 scores; per-head softmax + (Wo V^T) p + residual
        GemvArgs g = {};
        g.W = w.xM; g.x = v.h; g.x_ld = H; g.gamma = w.ln2_g; g.beta = w.ln2_b; g.out = e->qc; g.out_ld = p.xscores.N;
        PTTS_TRY(gv(p.xscores, g, "LN2 + folded scores"));
        GemvArgs g2 = {};
        g2.W = w.xU; g2.x = e->qc; g2.mask = v.enc_mask; g2.n_valid = &e->dims->N; g2.ne = p.xfold_ne; g2.out = v.h; g2.out_ld = H;
        PTTS_TRY(gv(p.xsoftmax, g2, "softmax + folded out_proj"));
        break;
      }
      case XQ_FUSED: {  // LN2 + the head's cross-q rows + cross-attention of one (head, utterance) as ONE node (xq_attn_kernel): no static fold
        XqAttnArgs x = {};
        x.W = w.cq_rm; x.wscale = w.cq_sc; x.x = v.h; x.x_ld = H; x.gamma = w.ln2_g; x.beta = w.ln2_b;
        x.kcache = at(w.k_cross, v.cross_off); x.vcache = at(w.v_cross, v.cross_off); x.mask = v.enc_mask; x.mask_ld = c.max_enc; x.cap = c.max_enc; x.n_valid = &e->dims->N;
        x.out = e->xw; x.out_ld = H; x.nheads = nh; x.H = H; x.kv_heads = nkc; x.M = M; x.scale = scale;
        if (ptts_xqattn_launch(p.mode, x, st) != 0) return ptts_fail(PTTS_E_HIP, "xq_attn launch failed");
        break;
      }
      default: {  // PLAIN: LN2 + cross q projection (:1040, :855), then cross-attention against the static description K/V, softmax finished in the kernel
        GemvArgs g = {};
        g.W = w.cq_rm; g.wscale = w.cq_sc; g.x = v.h; g.x_ld = H; g.gamma = w.ln2_g; g.beta = w.ln2_b; g.out = e->qc; g.out_ld = H;
        PTTS_TRY(gv(p.cq, g, "LN2+cross q"));
        PTTS_TRY((launch_attn<WT>(cross_attn_args(e, v, w, 1, false, 0), M, st, p.cross_waves)));
      }
    }
    if (p.co.on) {  // cross out_proj + residual (:1052)
      GemvArgs g = {};
      g.W = w.co_rm; g.wscale = w.co_sc; g.xw = e->xw; g.xw_ld = H; g.out = v.h; g.out_ld = H;
      PTTS_TRY(gv(p.co, g, "cross out_proj"));
    }
    {  // LN3 + fc1 + GELU (engine dtype), fc2 + residual (:1059-1064)
      GemvArgs g = {};
      g.W = w.fc1_rm; g.wscale = w.fc1_sc; g.x = v.h; g.x_ld = H; g.gamma = w.ln3_g; g.beta = w.ln3_b;
      g.out = reinterpret_cast<float*>(e->xw2); g.out_ld = F;
      if (p.x_fused) { g.part = e->xpart; g.npart = nh; g.hsum = e->h2; }  // GV_LNP sums the cross block's partial rows
      PTTS_DBG_NODE(g, l, 3);
      PTTS_TRY(gv(p.fc1, g, "[partial rows+]LN3+fc1"));
      GemvArgs g2 = {};
      g2.W = w.fc2_rm; g2.wscale = w.fc2_sc; g2.xw = e->xw2; g2.xw_ld = F; g2.out = v.h; g2.out_ld = H;
      if (p.x_fused) g2.resid = e->h2;  // h = (x + partial rows) + fc2(...)
      PTTS_DBG_NODE(g2, l, 4);
      PTTS_TRY(gv(p.fc2, g2, "fc2"));
    }
  }
  GemvArgs g = {};  // final LayerNorm + all K LM heads (:1632, :1917-1960)
  g.W = e->heads_rm; g.wscale = e->heads_sc; g.x = v.h; g.x_ld = H; g.gamma = e->lnf_g; g.beta = e->lnf_b; g.out = v.logits; g.out_ld = p.heads.N;
  PTTS_DBG_NODE(g, c.num_layers, 0);
  PTTS_TRY(gv(p.heads, g, "final LN + LM heads"));
  return launch_status("forward");
}

// The MFMA strip path up to the logits: every prefill (Q positions per utterance), and the decode step above gemv_rows utterances
// (heads = false: the layers only, the residual rows stay in v.h - ptts_score runs its own heads + loss kernel over them).
// Which nodes: the plan (ptts_step_plan.h: strip_plan); this walker fills their arguments and launches them.
template <typename WT>
int strip_path(const ptts_engine* e, FwdView v, const StripPlan& p, hipStream_t st, bool heads = true) {
  static_assert(Elem<WT>::KT == step_kt(sizeof(WT) == 2), "ptts_step_plan.h: step_kt");
  const ptts_config& c = e->cfg;
  const int H = c.hidden_size, F = c.ffn_dim, nh = c.num_heads, B = p.B, Q = p.Q, M = p.M, fo = p.fo;
  const bool prefill = p.prefill != 0;
  const int nkv = e->sc.nkv, nkc = e->sc.nkc, Hkv = nkv * 64, QKV = H + 2 * Hkv;  // grouped-query attention: fewer K/V heads
  const float scale = 1.0f / sqrtf((float)(H / nh));
  auto attn = [&](AttnArgs a, int waves) -> int {  // self- or cross-attention node
    a.hostP = v.P; a.hostN = v.N;  // the prefill kernels' preloaded head (PrefillAttnHead::pack)
    return p.attn == ATTN_PREFILL ? launch_prefill_attn<WT>(a, B, st, p.prefill_attn_mode) : launch_attn<WT>(a, B, st, waves);
  };
#define PTTS_DBG_BIG(args, l_, k_) PTTS_DBG_STAMP(args, !prefill && M > 8, (size_t)(l_) * 7 + (k_))
  for (int l = 0; l < c.num_layers; ++l) {
    const LayerW& w = e->L[l];
    void *const k_self = at(w.k_self, v.self_off), *const v_self = at(w.v_self, v.self_off);
    switch (p.qkv) {
      case QKV_LNPROJ: case QKV_LNPROJ_KV: {  // LN1 + fused QKV projection in one node
        LnProjArgs a = {};
        PTTS_DBG_BIG(a, l, 0);
        a.W = w.qkv; a.x = v.h; a.x_ld = H; a.gamma = w.ln1_g; a.beta = w.ln1_b; a.K = H; a.out = e->qkv; a.out_ld = QKV; a.M = M; a.N = QKV;
        if (p.qkv == QKV_LNPROJ_KV) { a.kcache = k_self; a.vcache = v_self; a.kv_Q = Q; a.kv_cap = c.max_ctx; a.kv_heads = nkv; a.kv_H = H; }
        PTTS_TRY((launch_lnproj<WT, EPI_STORE>(e, a, st, p.lnproj_g)));
        break;
      }
      default: {  // QKV_GEMM, QKV_GEMM_KV: LN1 + fused QKV projection
        GemmArgs g = {}; g.decode = p.dec;
        g.W = w.qkv; g.W8 = w.qkv_p8; g.wscale = w.qkv_sc; g.x = v.h; g.x_ld = H; g.x_row_mul = 1; g.gamma = w.ln1_g; g.beta = w.ln1_b;
        g.out = e->qkv; g.out_ld = QKV; g.M = M; g.N = QKV; g.K = H; g.x_fo = fo;
        if (p.qkv == QKV_GEMM_KV) { g.kcache = k_self; g.vcache = v_self; g.kv_rows_per_b = Q; g.kv_cap = c.max_ctx; g.nheads = nkv; g.kv_col0 = H; }
        PTTS_TRY((ln_gemm<WT, EPI_STORE>(e, g, p.qkv_how, st)));
      }
    }
    if (p.kv_append == KVA_E4M3) {
      if constexpr (sizeof(WT) == 2)
        hipLaunchKernelGGL((kv_append_kernel<WT, true>), dim3(Q, nkv, B), dim3(64), 0, st, e->qkv + H, e->qkv + H + Hkv, QKV, k_self, v_self, c.max_ctx,
                           Q, nkv, c.rope ? e->rope_cos : nullptr, c.rope ? e->rope_sin : nullptr, scale_at(w.ks_self, v.scale_off), scale_at(w.vs_self, v.scale_off));
    } else if (p.kv_append == KVA_ENGINE) {
      hipLaunchKernelGGL((kv_append_kernel<WT>), dim3(Q, nkv, B), dim3(64), 0, st, e->qkv + H, e->qkv + H + Hkv, QKV, k_self,
                         v_self, c.max_ctx, Q, nkv, c.rope ? e->rope_cos : nullptr, c.rope ? e->rope_sin : nullptr);
    }
    {  // causal self-attention over the KV arena
      AttnArgs a = self_attn_args(e, v, w, Q, prefill, fo, p.S_used);
      PTTS_DBG_BIG(a, l, 1);
      PTTS_TRY(attn(a, 4));
    }
    {  // [combine splits] + out_proj + residual
      GemmArgs g = {}; g.decode = p.dec;
      g.W = w.o; g.W8 = w.o_p8; g.wscale = w.o_sc; g.part = e->part; g.stats = e->stats; g.S = p.S_used; g.nheads = nh;
      g.out = v.h; g.out_ld = H; g.M = M; g.N = H; g.K = H; g.x_fo = fo;
      if (p.lns) g.stats_out = e->lnstat;  // strip statistics of the new residual rows for LN2 (PRO_LNS)
      PTTS_DBG_BIG(g, l, 2);
      switch (p.out_proj) {
        case OUT_COPY:
          g.x = reinterpret_cast<const float*>(e->xw); g.x_ld = H; g.x_row_mul = 1;
          PTTS_TRY((launch_gemm<WT, PRO_COPY, EPI_RESID>(g, st)));
          break;
        case OUT_COMBINE_FUSED: PTTS_TRY((launch_gemm<WT, PRO_ATTN, EPI_RESID>(g, st))); break;
        default: PTTS_TRY((prep_copy_gemm<WT, PRO_ATTN, EPI_RESID>(e, g, st)));
      }
    }
    switch (p.cross) {
      case CROSS_XATTN_FUSED: {  // decode: LN2 + cross q projection + cross-attention fused, one workgroup per (head, p.xattn_g utterances)
        XAttnArgs x = {};
        x.W = w.cq; x.x = v.h; x.x_ld = H; x.x_row_mul = 1; x.x_row_off = 0; x.gamma = w.ln2_g; x.beta = w.ln2_b; x.K = H;
        x.invK = 1.0f / (float)H; x.kcache = at(w.k_cross, v.cross_off); x.vcache = at(w.v_cross, v.cross_off); x.cap = c.max_enc; x.cur_len = v.cur_len; x.dims = e->dims;
        x.mask = v.enc_mask; x.mask_ld = c.max_enc; x.cos = c.rope ? e->rope_cos : nullptr; x.sin = c.rope ? e->rope_sin : nullptr;
        x.out = e->xw; x.B = M; x.nheads = nh; x.kv_heads = nkc; x.n_rep = nh / nkc; x.scale = scale; x.out_fo = fo;
        PTTS_DBG_BIG(x, l, 3);
        launch_xattn_fused<WT>(x, p.xattn_g, st);
        break;
      }
      case CROSS_LNPROJ_ATTN: {  // LN2 + cross q projection as one node, then cross-attention against the static description K/V
        LnProjArgs a = {};
        a.W = w.cq; a.x = v.h; a.x_ld = H; a.gamma = w.ln2_g; a.beta = w.ln2_b; a.K = H; a.out = e->qc; a.out_ld = H; a.M = M; a.N = H;
        PTTS_TRY((launch_lnproj<WT, EPI_STORE>(e, a, st, p.lnproj_g)));
        PTTS_TRY(attn(cross_attn_args(e, v, w, Q, prefill, fo), p.cross_waves));
        break;
      }
      default: {  // CROSS_GEMM_ATTN: LN2 + cross q projection, then cross-attention
        GemmArgs g = {}; g.decode = p.dec;
        g.W = w.cq; g.x = v.h; g.x_ld = H; g.x_row_mul = 1; g.gamma = w.ln2_g; g.beta = w.ln2_b;
        g.out = e->qc; g.out_ld = H; g.M = M; g.N = H; g.K = H; g.x_fo = fo;
        if (p.lns) g.lnstat = e->lnstat;
        PTTS_TRY((ln_gemm<WT, EPI_STORE>(e, g, p.cq_how, st)));
        PTTS_TRY(attn(cross_attn_args(e, v, w, Q, prefill, fo), p.cross_waves));
      }
    }
    {  // cross out_proj + residual, activations read straight from the attention output
      GemmArgs g = {}; g.decode = p.dec;
      g.W = w.co; g.W8 = w.co_p8; g.wscale = w.co_sc; g.x = reinterpret_cast<const float*>(e->xw); g.x_ld = H; g.x_row_mul = 1; g.x_fo = fo;
      g.out = v.h; g.out_ld = H; g.M = M; g.N = H; g.K = H;
      if (p.lns) g.stats_out = e->lnstat;  // for LN3
      PTTS_DBG_BIG(g, l, 4);
      PTTS_TRY((launch_gemm<WT, PRO_COPY, EPI_RESID>(g, st)));
    }
    {  // LN3 + fc1 + GELU, then fc2 + residual. Above 8 rows the GELU output is written in the engine dtype so fc2
       // stages it with plain copies too.
      GemmArgs g = {}; g.decode = p.dec;
      g.W = w.fc1; g.W8 = w.fc1_p8; g.wscale = w.fc1_sc; g.x = v.h; g.x_ld = H; g.x_row_mul = 1; g.gamma = w.ln3_g; g.beta = w.ln3_b;
      g.out_ld = F; g.M = M; g.N = F; g.K = H;
      GemmArgs g2 = {}; g2.decode = p.dec;
      g2.W = w.fc2; g2.W8 = w.fc2_p8; g2.wscale = w.fc2_sc; g2.x_ld = F; g2.x_row_mul = 1; g2.out = v.h; g2.out_ld = H; g2.M = M; g2.N = H; g2.K = F;
      if (p.fc == FC_SMALL) {
        g.out = e->ffn;
        PTTS_TRY((launch_gemm<WT, PRO_LN, EPI_GELU>(g, st)));
        g2.x = e->ffn;
        PTTS_TRY((launch_gemm<WT, PRO_PLAIN, EPI_RESID>(g2, st)));
      } else {
        if (p.fc == FC_LNPROJ) {  // LN3 + fc1 + GELU in one node
          LnProjArgs a = {};
          a.W = w.fc1; a.x = v.h; a.x_ld = H; a.gamma = w.ln3_g; a.beta = w.ln3_b; a.K = H; a.out = e->xw2; a.out_ld = F; a.out_fo = fo; a.M = M; a.N = F;
          PTTS_DBG_BIG(a, l, 5);
          PTTS_TRY((launch_lnproj<WT, EPI_GELU_WT>(e, a, st, p.lnproj_g)));
        } else {
          g.out = reinterpret_cast<float*>(e->xw2); g.x_fo = fo; g.out_fo = fo;
          if (p.lns) g.lnstat = e->lnstat;
          PTTS_TRY((ln_gemm<WT, EPI_GELU_WT>(e, g, p.fc1_how, st)));
        }
        g2.x = reinterpret_cast<const float*>(e->xw2); g2.x_fo = fo;
        PTTS_DBG_BIG(g2, l, 6);
        // fc2 runs un-split at every batch size (round 6, profiles/r06_experiments.txt calls 15-16: the split-K partials of round 2 cost the next LN1 node
        // +1.0 us and the out_proj epilogue +1.2 us per layer - un-split: -2 % at 32, -3.3 % at 40, -7 % at Large-v1 x 32, equal at 12..16; only the
        // e4m3-weight Mini engine loses 1.4-3 %; the split path and its folds are gone)
        PTTS_TRY((launch_gemm<WT, PRO_COPY, EPI_RESID>(g2, st)));
      }
    }
  }
  if (heads) {  // final LayerNorm + all K LM heads as one [K*V, H] projection, last position of each utterance only
    if (prefill && v.row_dims) hipLaunchKernelGGL(gather_last_rows_kernel, dim3(B), dim3(256), 0, st, v.h, H, Q, v.row_dims);  // ... of a ragged group: the last GIVEN one
    GemmArgs g = {}; g.decode = p.dec;
    g.W = e->heads; g.W8 = e->heads_p8; g.wscale = e->heads_sc; g.x = v.h; g.x_ld = H; g.x_row_mul = Q; g.x_row_off = Q - 1; g.gamma = e->lnf_g; g.beta = e->lnf_b;
    g.out = v.logits; g.out_ld = c.num_codebooks * c.vocab_size; g.M = B; g.N = c.num_codebooks * c.vocab_size; g.K = H;
    g.x_fo = p.heads_x_fo;
    PTTS_TRY((ln_gemm<WT, EPI_STORE>(e, g, p.heads_how, st)));
  }
  return launch_status("forward");
}

// The plan of a strip-path forward. PTTS_PREFILL_ATTN is the one switch read per forward, not at create: 0: one workgroup per
// query row, 1: tiled VALU kernel, 2: f32-MFMA kernel, 3 (default): by batch
StripPlan strip_plan_now(const ptts_engine* e, const FwdView& v, bool prefill, int Q) {
  const int prefill_attn_mode = getenv("PTTS_PREFILL_ATTN") ? atoi(getenv("PTTS_PREFILL_ATTN")) : 3;
  return strip_plan(e->sc, e->cfg, e->sw, prefill, v.B, Q, prefill_attn_mode);
}

// One decoder forward over Q positions per utterance (Q = P+1 at prefill, 1 at decode) up to the logits: one plan, then its walker.
template <typename WT>
int forward(const ptts_engine* e, FwdView v, bool prefill, hipStream_t st, bool with_embed = true) {
  const int Q = prefill ? v.P + 1 + v.T : 1;  // prompt positions + BOS column [+ the voice-prompt columns, run in the same pass]
  if (prefill) PTTS_TRY(project_cross_kv<WT>(e, v, st));
  if (with_embed) launch_embed<WT>(e, v, prefill, Q, st);
  if (step_on_gemv(e->sc, prefill, v.B)) return gemv_step<WT>(e, v, gemv_plan(e->sc, e->cfg, e->sw, v.B, v.kv_bound, v.xfold_valid), st);  // batch 1..8 (fp32: 1)
  return strip_path<WT>(e, v, strip_plan_now(e, v, prefill, Q), st);
}

// the sampler tail over the view's utterances; row >= 0 (sessions only): the tail of that one slot (ptts_admit_row)
int launch_tail(const ptts_engine* e, FwdView v, hipStream_t st, bool embed_next, int row = -1) {
  TailArgs t = {};
  if (embed_next) {
    t.tables = e->embed; t.pos_table = e->cfg.rope ? nullptr : e->pos_table; t.dims = e->dims; t.h = v.h;
    t.H = e->cfg.hidden_size; t.bos = e->cfg.bos_token_id; t.bf16_tables = e->cfg.dtype == PTTS_BF16;
  }
  t.logits = v.logits; t.ids = v.ids; t.ids_ld = e->ids_ld; t.cur_len = v.cur_len; t.unfinished = v.unfinished;
  t.has_eos = v.has_eos; t.first_unf = v.first_unf; t.gen = e->gen; t.sort_buf = e->sort_buf;
  t.B = v.B; t.K = e->cfg.num_codebooks; t.V = e->cfg.vocab_size; t.eos = e->cfg.eos_token_id; t.pad = e->cfg.pad_token_id;
  const StepRecord* rec = e->rec_on ? e->rec + (v.cur_len - e->cur_len) : nullptr;  // indexed like cur_len
  if (rec && e->rec_node) {  // the logits as the heads wrote them: in front of the nodes that rewrite them in place
    LogitsRecordArgs r = {};
    r.logits = v.logits; r.cur_len = v.cur_len; r.unfinished = v.unfinished; r.rec = rec;
    r.t_prefix = v.session ? e->slot_T + (v.cur_len - e->cur_len) : &e->dims->T_prefix; r.t_prefix_stride = v.session ? 1 : 0;  // as the logit-edit node
    r.B = v.B; r.K = e->cfg.num_codebooks; r.V = e->cfg.vocab_size; r.session = v.session ? 1 : 0;
    if (!step_logits_record_launch(r, row < 0 ? 0 : row, row < 0 ? v.B : 1, st)) return ptts_fail(PTTS_E_INVALID, "step records: bad launch arguments");
  }
  if (e->pen_on) {  // history penalties rewrite the logits the tail is about to read; the records are indexed like cur_len
    PenaltyArgs p = {};
    p.logits = v.logits; p.ids = v.ids; p.cur_len = v.cur_len; p.pen = e->pen + (v.cur_len - e->cur_len);
    p.ids_ld = e->ids_ld; p.K = e->cfg.num_codebooks; p.V = e->cfg.vocab_size;
    if (!penalty_launch(p, row < 0 ? 0 : row, row < 0 ? v.B : 1, st)) return ptts_fail(PTTS_E_UNSUPPORTED, "history penalty: no kernel for vocab_size %d", p.V);
  }
  if (e->le_on) {  // position and token edits, behind the penalties as in transformers' chain; records and voice-prompt lengths indexed like cur_len
    const size_t off = (size_t)(v.cur_len - e->cur_len);
    LogitEditArgs a = {};
    a.logits = v.logits; a.cur_len = v.cur_len; a.recs = e->le;
    a.recs.hdr += off; a.recs.bias += off * e->le.ld_v; a.recs.decay += off * e->le.ld_t; a.recs.flags += off * e->le.ld_v;
    // given columns = 1 + T: a slot's own frames in a session, the call's (DevDims::T_prefix, what the tail reads) otherwise
    a.t_prefix = v.session ? e->slot_T + off : &e->dims->T_prefix; a.t_prefix_stride = v.session ? 1 : 0;
    a.K = e->cfg.num_codebooks; a.V = e->cfg.vocab_size; a.eos = e->cfg.eos_token_id;
    if (!logit_edit_launch(a, row < 0 ? 0 : row, row < 0 ? v.B : 1, st)) return ptts_fail(PTTS_E_UNSUPPORTED, "logit edits: no kernel for vocab_size %d", a.V);
  }
  // the instance (NV by vocabulary, static or per-slot clocks) and the wave count are chosen in tail_launch, shared with the test harness
  // warpers on: the WARP instances, with the records indexed like cur_len (null picks the instances of an engine without the feature)
  const DevWarp* warp = e->warp_on ? e->warp + (v.cur_len - e->cur_len) : nullptr;
  // step records on: the RECORD instances, likewise
  const StepRecord* trec = e->rec_tail ? rec : nullptr;
  if (v.session) tail_launch(t, e->row_maxlen, row < 0 ? 0 : row, dim3(row < 0 ? v.B : 1), st, e->slot_gen, e->slot_T, warp, trec);
  else tail_launch(t, nullptr, 0, dim3(v.B), st, nullptr, nullptr, warp, trec);
  return launch_status("tail");
}

// static cross-attention folding for the utterance just prefilled (xfold_*_kernel): 2 launches covering every layer
template <typename WT, bool W8>
int fold_cross(ptts_engine* e, hipStream_t st) {
  const ptts_config& c = e->cfg;
  const int H = c.hidden_size, nh = c.num_heads, NE = e->sc.xfold_ne, n_rep = nh / e->sc.nkc, L = c.num_layers;
  const float qscale = 1.44269504088896340736f / sqrtf((float)(H / nh));
  // tiled kernels (round 5; bit-identical to the row kernels, which serve the widths the tiles do not)
  if (H % 64 == 0 && NE <= 64) {
    hipLaunchKernelGGL((xfold_tile_kernel<WT, W8, false>), dim3(H / 64, nh, L), dim3(256), 0, st, e->fold_layers, nh, H, NE, c.max_enc, n_rep, e->dims, qscale);
    hipLaunchKernelGGL((xfold_tile_kernel<WT, W8, true>), dim3(H / 64, nh, L), dim3(256), 0, st, e->fold_layers, nh, H, NE, c.max_enc, n_rep, e->dims, qscale);
  } else {
    hipLaunchKernelGGL((xfold_m_kernel<WT, W8>), dim3((H / 8 + 63) / 64, NE, L * nh), dim3(64), 0, st, e->fold_layers, nh, H, NE, c.max_enc, n_rep,
                       e->dims, qscale);
    hipLaunchKernelGGL((xfold_u_kernel<WT, W8>), dim3((nh * NE + 63) / 64, H, L), dim3(64), 0, st, e->fold_layers, H, NE, nh, c.max_enc, n_rep, e->dims);
  }
  return launch_status("cross-attention fold");
}

int forward_dispatch(const ptts_engine* e, FwdView v, bool prefill, hipStream_t st, bool with_embed = true) {
  return e->cfg.dtype == PTTS_BF16 ? forward<bf16_t>(e, v, prefill, st, with_embed) : forward<float>(e, v, prefill, st, with_embed);
}

// attention fetch bound of a decode forward behind `ub` written self-KV positions: ub + 1 rounded up to 64, <= max_ctx
static int kv_bound_of(const ptts_engine* e, int ub) { return std::min(e->cfg.max_ctx, (ub + 1 + 63) / 64 * 64); }

// every decode forward appends one self-KV position: advance the host's bound before launching it (eagerly or as a graph)
// (session: one bound per busy slot, capped by the end of its request; the step's bound is their maximum, so it falls when a long request retires)
static void advance_kv(ptts_engine* e) {
  if (e->session) {
    int ub = e->P + 1;
    for (int b = 0; b < e->B; ++b)
      if (e->slot_busy[b]) {
        e->slot_ub[b] = std::min(e->slot_ub[b] + 1, e->P + e->slot_maxlen[b]);
        ub = std::max(ub, e->slot_ub[b]);
      }
    e->kv_ub = ub;
  } else {
    e->kv_ub += 1;
  }
  e->kv_bound = kv_bound_of(e, e->kv_ub);
}

// copy/convert a plain tensor into engine storage
template <typename DT>
int convert_into(DT* dst, const void* src, int src_dtype, size_t n, hipStream_t st) {
  const int blocks = (int)std::min<size_t>((n + 255) / 256, 4096);
  if (src_dtype == PTTS_F32) hipLaunchKernelGGL((convert_kernel<DT, float>), dim3(blocks), dim3(256), 0, st, (const float*)src, dst, n);
  else hipLaunchKernelGGL((convert_kernel<DT, bf16_t>), dim3(blocks), dim3(256), 0, st, (const bf16_t*)src, dst, n);
  return PTTS_OK;
}

template <typename WT>
int pack_into(void* dst, const void* src, int src_dtype, int N, int K, int row0, hipStream_t st) {
  constexpr int KT = Elem<WT>::KT;
  if (N % 16 || K % KT || row0 % 16) return ptts_fail(PTTS_E_INVALID, "weight [%d,%d] (row offset %d) not a multiple of the 16x%d MFMA tile", N, K, row0, KT);
  const size_t total = (size_t)(N / 16) * (K / KT) * 64;
  const int blocks = (int)((total + 255) / 256);
  if (src_dtype == PTTS_F32)
    hipLaunchKernelGGL((pack_weight_kernel<WT, float>), dim3(blocks), dim3(256), 0, st, (const float*)src, (WT*)dst, N, K, row0 / 16, K / KT);
  else
    hipLaunchKernelGGL((pack_weight_kernel<WT, bf16_t>), dim3(blocks), dim3(256), 0, st, (const bf16_t*)src, (WT*)dst, N, K, row0 / 16, K / KT);
  return PTTS_OK;
}

int pack_dispatch(ptts_engine* e, void* dst, const void* src, int src_dtype, int N, int K, int row0, hipStream_t st) {
  return e->cfg.dtype == PTTS_BF16 ? pack_into<bf16_t>(dst, src, src_dtype, N, K, row0, st) : pack_into<float>(dst, src, src_dtype, N, K, row0, st);
}

// row-major copy (rows [row0, row0 + N) of a [*, K] matrix) in the engine dtype for the GEMV step
int rowmajor_dispatch(ptts_engine* e, void* dst, const void* src, int src_dtype, int N, int K, int row0, hipStream_t st) {
  const size_t off = (size_t)row0 * K, n = (size_t)N * K;
  if (e->cfg.dtype == PTTS_BF16) return convert_into<bf16_t>(reinterpret_cast<bf16_t*>(dst) + off, src, src_dtype, n, st);
  return convert_into<float>(reinterpret_cast<float*>(dst) + off, src, src_dtype, n, st);
}

// The tensors of a decoder layer by name suffix. A projection matrix is rows [row0, row0 + N) of its packed destination, of the row-major copy
// (GEMV step), of the e4m3 strip copy and of the row scales (weights_fp8) - null where this engine holds none; K = -1: an fp32 vector of N
struct LayerTensor { const char* name; void *dst, *rm, *p8; float* sc; int N, K, row0; };
std::array<LayerTensor, 16> layer_tensors(const ptts_engine* e, const LayerW& w) {
  const int H = e->cfg.hidden_size, F = e->cfg.ffn_dim, kv = e->sc.nkv * 64, kc = e->sc.nkc * 64;
  return {{{"self_attn.q_proj.weight", w.qkv, w.qkv_rm, w.qkv_p8, w.qkv_sc, H, H, 0},
           {"self_attn.k_proj.weight", w.qkv, w.qkv_rm, w.qkv_p8, w.qkv_sc, kv, H, H},
           {"self_attn.v_proj.weight", w.qkv, w.qkv_rm, w.qkv_p8, w.qkv_sc, kv, H, H + kv},
           {"self_attn.out_proj.weight", w.o, w.o_rm, w.o_p8, w.o_sc, H, H, 0},
           {"encoder_attn.q_proj.weight", w.cq, w.cq_rm, nullptr, w.cq_sc, H, H, 0},
           {"encoder_attn.k_proj.weight", w.ckv, nullptr, nullptr, nullptr, kc, H, 0},
           {"encoder_attn.v_proj.weight", w.ckv, nullptr, nullptr, nullptr, kc, H, kc},
           {"encoder_attn.out_proj.weight", w.co, w.co_rm, w.co_p8, w.co_sc, H, H, 0},
           {"fc1.weight", w.fc1, w.fc1_rm, w.fc1_p8, w.fc1_sc, F, H, 0},
           {"fc2.weight", w.fc2, w.fc2_rm, w.fc2_p8, w.fc2_sc, H, F, 0},
           {"self_attn_layer_norm.weight", w.ln1_g, nullptr, nullptr, nullptr, H, -1, 0}, {"self_attn_layer_norm.bias", w.ln1_b, nullptr, nullptr, nullptr, H, -1, 0},
           {"encoder_attn_layer_norm.weight", w.ln2_g, nullptr, nullptr, nullptr, H, -1, 0}, {"encoder_attn_layer_norm.bias", w.ln2_b, nullptr, nullptr, nullptr, H, -1, 0},
           {"final_layer_norm.weight", w.ln3_g, nullptr, nullptr, nullptr, H, -1, 0}, {"final_layer_norm.bias", w.ln3_b, nullptr, nullptr, nullptr, H, -1, 0}}};
}

// The engine's environment switches, read once when it is created. PTTS_PREFILL_ATTN alone is read per forward (strip_plan_now).
void read_env_switches(StepSwitches* sw) {
  if (const char* ev = getenv("PTTS_FUSE_X")) sw->fuse_x = atoi(ev) ? 1 : 0;
  if (const char* ev = getenv("PTTS_FUSE_X_NUR")) { const int v = atoi(ev); if (v == 2 || v == 4) sw->fuse_x_nur = v; }
  sw->fuse_qa = !(getenv("PTTS_NO_FUSE_QA") && atoi(getenv("PTTS_NO_FUSE_QA")));
  if (const char* ev = getenv("PTTS_FUSE_QA_MAX")) sw->fuse_qa_max = std::max(1, std::min(GV_MAX_ROWS, atoi(ev)));
  sw->fuse_xq = !(getenv("PTTS_NO_FUSE_XQ") && atoi(getenv("PTTS_NO_FUSE_XQ")));
  if (const char* ev = getenv("PTTS_LNPROJ")) sw->lnproj = std::max(0, std::min(3, atoi(ev)));
  if (const char* ev = getenv("PTTS_LNPROJ_G")) sw->lnproj_g = atoi(ev) == 4 ? 4 : (atoi(ev) == 16 ? 16 : (atoi(ev) == 8 ? 8 : 0));
  if (const char* ev = getenv("PTTS_XATTN_G")) { const int g = atoi(ev); if (g == 2 || g == 4 || g == 8) sw->xattn_g = g; }  // (a width without the g < 8 instances runs 8: xattn_group_size)
  sw->xattn_groups = !(getenv("PTTS_NO_XATTN_GROUPS") && atoi(getenv("PTTS_NO_XATTN_GROUPS")));
}

// NULL is the legacy default stream (what torch.cuda.current_stream() is on ROCm unless the caller switched): pass through.
hipStream_t pick_stream(ptts_engine*, void* s) { return reinterpret_cast<hipStream_t>(s); }

}  // namespace

extern "C" int ptts_engine_create(const ptts_config* cfg, ptts_engine** out) {
  PTTS_CHECK(cfg && out, PTTS_E_INVALID, "null argument");
  const ptts_config& c = *cfg;
  PTTS_CHECK(c.hidden_size > 0 && c.num_heads > 0 && c.hidden_size % c.num_heads == 0, PTTS_E_INVALID, "hidden_size %d not divisible by num_heads %d", c.hidden_size, c.num_heads);
  PTTS_CHECK(c.hidden_size / c.num_heads == 64, PTTS_E_UNSUPPORTED, "head_dim must be 64 (Mini/Large v1), got %d", c.hidden_size / c.num_heads);
  PTTS_CHECK(c.dtype == PTTS_F32 || c.dtype == PTTS_BF16, PTTS_E_INVALID, "dtype must be PTTS_F32 or PTTS_BF16");
  PTTS_CHECK(c.hidden_size % 32 == 0 && c.ffn_dim % 32 == 0 && c.vocab_size % 16 == 0, PTTS_E_UNSUPPORTED,
             "hidden_size/ffn_dim must be multiples of 32 and vocab_size of 16");
  PTTS_CHECK(c.hidden_size <= 64 * 4 * LN_MAX_F4, PTTS_E_UNSUPPORTED, "hidden_size > %d unsupported", 64 * 4 * LN_MAX_F4);
  PTTS_CHECK(c.num_codebooks >= 1 && c.num_codebooks <= 32, PTTS_E_INVALID, "num_codebooks out of range");
  PTTS_CHECK(c.vocab_size <= PTTS_SORT_N, PTTS_E_UNSUPPORTED, "vocab_size > %d unsupported by the sampler", PTTS_SORT_N);
  PTTS_CHECK(c.max_batch >= 1 && c.max_ctx >= 2 && c.max_enc >= 1 && c.max_prompt >= 1 && c.max_prompt <= c.max_ctx, PTTS_E_INVALID, "bad capacities");
  const StepConfig sc = step_config(c);  // which step kernels this engine runs: it sizes the weight copies and the scratch below
  const int nkv_ = sc.nkv, nkc_ = sc.nkc;
  PTTS_CHECK(c.num_heads % nkv_ == 0 && c.num_heads % nkc_ == 0, PTTS_E_INVALID, "num_heads %d not divisible by the K/V head counts %d / %d", c.num_heads, nkv_, nkc_);
  // the bit-packed fields of the preloaded kernel heads: P and the prompt / description mask strides (PrefillAttnHead), the LM heads' row selection
  // Q, Q - 1 (RowsPrepHead) in 16 bits; the prefill GEMMs' tile grid over B x max_prompt rows and B x max_enc description rows (GemmGldsHead)
  PTTS_CHECK(c.max_prompt <= 0xffff && c.max_enc <= 0xffff, PTTS_E_UNSUPPORTED, "max_prompt %d / max_enc %d above 65535 (16-bit fields of the prefill kernels)",
             c.max_prompt, c.max_enc);
  const long long widest = std::max({(long long)c.hidden_size + 2LL * nkv_ * 64, (long long)c.ffn_dim, 2LL * nkc_ * 64,
                                    (long long)c.num_codebooks * c.vocab_size});
  PTTS_CHECK(GemmGldsHead::fits(widest, (long long)c.max_batch * std::max(c.max_prompt, c.max_enc)), PTTS_E_UNSUPPORTED,
             "max_batch %d x max_prompt %d / max_enc %d rows over widths up to %lld: the prefill GEMM's tile grid exceeds its 20- / 11-bit extents",
             c.max_batch, c.max_prompt, c.max_enc, widest);
  PTTS_DEVICE(c.device);
  ptts_engine* e = new ptts_engine();
  e->cfg = c;
  e->sc = sc;
  read_env_switches(&e->sw);
  e->esize = c.dtype == PTTS_BF16 ? 2 : 4;
  e->max_prompt = c.max_prompt;
  int rc = PTTS_OK;
  auto fail = [&](int r) { ptts_engine_destroy(e); return r; };
  if (hipStreamCreateWithFlags(&e->own_stream, hipStreamNonBlocking) != hipSuccess) return fail(ptts_fail(PTTS_E_HIP, "hipStreamCreate failed"));
  if (hipEventCreate(&e->ev_first) != hipSuccess || hipEventCreate(&e->ev_tail0) != hipSuccess || hipEventCreate(&e->ev_pre0) != hipSuccess)
    return fail(ptts_fail(PTTS_E_HIP, "hipEventCreate failed"));
  const int H = c.hidden_size, F = c.ffn_dim, K = c.num_codebooks, V = c.vocab_size, nh = c.num_heads;
  const size_t es = e->esize;
  e->L.resize(c.num_layers);
  if (c.kv_fp8 && (c.dtype != PTTS_BF16 || c.max_batch <= GV_MAX_ROWS))  // by capacity, not by path (a width without GEMV instances runs strips at 1..8 too)
    return fail(ptts_fail(PTTS_E_UNSUPPORTED, "kv_fp8 (e4m3 self-attention cache) needs the bf16 engine created for more than %d utterances (the MFMA strip step)", GV_MAX_ROWS));
  if (e->sc.w8 && (c.dtype != PTTS_BF16 || H % 512 || F % 512 || H > 2048))
    return fail(ptts_fail(PTTS_E_UNSUPPORTED, "weights_fp8 needs the bf16 engine and hidden / ffn sizes that are multiples of 512 (hidden <= 2048)"));
#define A(expr) if ((rc = (expr)) != PTTS_OK) return fail(rc)
  for (int l = 0; l < c.num_layers; ++l) {
    LayerW& w = e->L[l];
    const int nq = H + 2 * e->sc.nkv * 64;
    A(e->alloc_bytes(&w.qkv, (size_t)nq * H * es));
    A(e->alloc_bytes(&w.o, (size_t)H * H * es));
    A(e->alloc_bytes(&w.cq, (size_t)H * H * es));
    A(e->alloc_bytes(&w.ckv, (size_t)2 * e->sc.nkc * 64 * H * es));
    A(e->alloc_bytes(&w.co, (size_t)H * H * es));
    A(e->alloc_bytes(&w.fc1, (size_t)F * H * es));
    A(e->alloc_bytes(&w.fc2, (size_t)F * H * es));
    if (e->sc.use_gemv) {
      const size_t res = e->sc.w8 ? 1 : es;  // row-major element size: e4m3 bytes or the engine dtype
      A(e->alloc_bytes(&w.qkv_rm, (size_t)nq * H * res)); A(e->alloc_bytes(&w.o_rm, (size_t)H * H * res));
      A(e->alloc_bytes(&w.cq_rm, (size_t)H * H * res)); A(e->alloc_bytes(&w.co_rm, (size_t)H * H * res));
      A(e->alloc_bytes(&w.fc1_rm, (size_t)F * H * res)); A(e->alloc_bytes(&w.fc2_rm, (size_t)F * H * res));
      if (e->sc.xfold_ne) {
        A(e->alloc_bytes(&w.xM, (size_t)nh * e->sc.xfold_ne * H * es)); A(e->alloc_bytes(&w.xU, (size_t)nh * e->sc.xfold_ne * H * es));
      }
    }
    if (e->sc.w8) {  // row scales serve both e4m3 layouts (row-major for the GEMV step, strips for the MFMA step)
      A(e->alloc(&w.qkv_sc, nq)); A(e->alloc(&w.o_sc, H)); A(e->alloc(&w.cq_sc, H)); A(e->alloc(&w.co_sc, H));
      A(e->alloc(&w.fc1_sc, F)); A(e->alloc(&w.fc2_sc, H));
      if (e->sc.w8_strips) {
        A(e->alloc_bytes(&w.qkv_p8, (size_t)nq * H)); A(e->alloc_bytes(&w.o_p8, (size_t)H * H)); A(e->alloc_bytes(&w.co_p8, (size_t)H * H));
        A(e->alloc_bytes(&w.fc1_p8, (size_t)F * H)); A(e->alloc_bytes(&w.fc2_p8, (size_t)F * H));
      }
    }
    A(e->alloc(&w.ln1_g, H)); A(e->alloc(&w.ln1_b, H)); A(e->alloc(&w.ln2_g, H)); A(e->alloc(&w.ln2_b, H));
    A(e->alloc(&w.ln3_g, H)); A(e->alloc(&w.ln3_b, H));
    const size_t kvs = (size_t)c.max_batch * e->sc.nkv * c.max_ctx * 64 * (c.kv_fp8 ? 1 : es), kvc = (size_t)c.max_batch * e->sc.nkc * c.max_enc * 64 * es;
    A(e->alloc_bytes(&w.k_self, kvs)); A(e->alloc_bytes(&w.v_self, kvs));
    if (c.kv_fp8) { A(e->alloc(&w.ks_self, (size_t)c.max_batch * e->sc.nkv * c.max_ctx)); A(e->alloc(&w.vs_self, (size_t)c.max_batch * e->sc.nkv * c.max_ctx)); }
    A(e->alloc_bytes(&w.k_cross, kvc)); A(e->alloc_bytes(&w.v_cross, kvc));
    char nm[160];
    for (const LayerTensor& m : layer_tensors(e, w)) {
      snprintf(nm, sizeof nm, "model.decoder.layers.%d.%s", l, m.name); e->required.insert(nm);
      if (m.sc) e->required_fp8.insert(nm);  // weights_fp8: a matrix with row scales has an e4m3 copy to load
    }
  }
  {
    std::vector<KvLayer> kl(c.num_layers);
    for (int l = 0; l < c.num_layers; ++l) kl[l] = KvLayer{e->L[l].ckv, e->L[l].k_cross, e->L[l].v_cross};
    A(e->alloc(&e->kv_layers, (size_t)c.num_layers));
    if (hipMemcpy(e->kv_layers, kl.data(), kl.size() * sizeof(KvLayer), hipMemcpyHostToDevice) != hipSuccess)
      return fail(ptts_fail(PTTS_E_HIP, "hipMemcpy(cross K/V operand table) failed"));
  }
  if (e->sc.xfold_ne) {
    std::vector<FoldLayer> fl(c.num_layers);
    for (int l = 0; l < c.num_layers; ++l) {
      const LayerW& w = e->L[l];
      fl[l] = FoldLayer{w.cq_rm, w.cq_sc, w.k_cross, w.xM, w.co_rm, w.co_sc, w.v_cross, w.xU};
    }
    A(e->alloc(&e->fold_layers, (size_t)c.num_layers));
    if (hipMemcpy(e->fold_layers, fl.data(), fl.size() * sizeof(FoldLayer), hipMemcpyHostToDevice) != hipSuccess)
      return fail(ptts_fail(PTTS_E_HIP, "hipMemcpy(fold operand table) failed"));
  }
  A(e->alloc_bytes(&e->embed, (size_t)K * (V + 1) * H * es));
  A(e->alloc_bytes(&e->heads, (size_t)K * V * H * es));
  if (e->sc.use_gemv) A(e->alloc_bytes(&e->heads_rm, (size_t)K * V * H * (e->sc.w8 ? 1 : es)));
  if (e->sc.w8_strips) A(e->alloc_bytes(&e->heads_p8, (size_t)K * V * H));
  if (e->sc.w8) {
    A(e->alloc(&e->heads_sc, (size_t)K * V));
    for (int k = 0; k < K; ++k) { char nm[96]; snprintf(nm, sizeof nm, "lm_heads.%d.weight", k); e->required_fp8.insert(nm); }
  }
  A(e->alloc(&e->lnf_g, H)); A(e->alloc(&e->lnf_b, H));
  e->required.insert("model.decoder.layer_norm.weight");
  e->required.insert("model.decoder.layer_norm.bias");
  for (int k = 0; k < K; ++k) {
    char nm[96];
    snprintf(nm, sizeof nm, "model.decoder.embed_tokens.%d.weight", k); e->required.insert(nm);
    snprintf(nm, sizeof nm, "lm_heads.%d.weight", k); e->required.insert(nm);
  }
  if (c.rope) {
    // RoPE is computed for any position in the reference (:373-406): tables cover the whole KV capacity, not max_positions
    const size_t rope_rows = (size_t)std::max(c.max_positions, c.max_ctx);
    A(e->alloc(&e->rope_cos, rope_rows * 64)); A(e->alloc(&e->rope_sin, rope_rows * 64));
    e->required.insert("rope_cos"); e->required.insert("rope_sin");
  } else {
    A(e->alloc(&e->pos_table, (size_t)c.max_positions * H));
    e->required.insert("model.decoder.embed_positions.weights");
  }
  const size_t rows = (size_t)c.max_batch * e->max_prompt;
  const size_t enc_rows = (size_t)c.max_batch * c.max_enc;
  A(e->alloc(&e->h, rows * H));
  A(e->alloc(&e->qkv, rows * 3 * H));
  A(e->alloc(&e->qc, std::max(rows, enc_rows) * H));
  // qkv_attn_kernel: up to 8 splits + the new position's own slot for one utterance, up to 4 + 1 for each of 2..8
  const size_t part_rows = std::max(rows * (size_t)e->sc.S_self, (size_t)c.max_batch * 5) + 9;
  A(e->alloc(&e->part, part_rows * H));
  A(e->alloc(&e->stats, part_rows * nh * 2));
  A(e->alloc(&e->xpart, (size_t)nh * H));
  A(e->alloc(&e->h2, (size_t)H));
  A(e->alloc(&e->ffn, std::max(rows * F, rows * (size_t)H)));
  A(e->alloc(&e->logits, (size_t)c.max_batch * K * V));
  A(e->alloc(&e->sort_buf, 16));
  A(e->alloc_bytes(&e->xw, (rows + 16) * H * es));  // + 16 rows: fragment order addresses whole 16-row tiles
  A(e->alloc_bytes(&e->xw2, std::max((rows + 16) * F, enc_rows * (size_t)H) * es));
  A(e->alloc(&e->lnstat, (size_t)c.max_batch * (H / 16) * 2 + 16));
  A(e->alloc(&e->prefix, (size_t)c.max_batch * K * c.max_ctx));
  e->ids_ld = c.max_ctx + 8;
  A(e->alloc(&e->ids, (size_t)c.max_batch * K * e->ids_ld));
  A(e->alloc(&e->cur_len, c.max_batch)); A(e->alloc(&e->unfinished, (size_t)c.max_batch * K));
  A(e->alloc(&e->has_eos, (size_t)c.max_batch * K)); A(e->alloc(&e->first_unf, c.max_batch));
  A(e->alloc(&e->enc_mask, enc_rows + 64));  // + 64: the folded cross block reads the mask in int4 groups up to position 63 whatever max_enc is
  A(e->alloc(&e->prompt_mask, rows));
  A(e->alloc(&e->dims, 1)); A(e->alloc(&e->gen, 1));
#undef A
  if (hipHostMalloc((void**)&e->host_pinned, ((size_t)c.max_batch * (K + 1) + 16) * 4) != hipSuccess) return fail(ptts_fail(PTTS_E_HIP, "hipHostMalloc failed"));
#ifdef PTTS_TIMING
  {
    const size_t n = (size_t)(c.num_layers + 1) * 7 * 48;  // 5 nodes per layer of the GEMV step, 7 of the batch > 8 step
    rc = e->alloc(&e->dbg_stamps, n);
    if (rc != PTTS_OK) return fail(rc);
    hipMemset(e->dbg_stamps, 0, n * sizeof(long long));
  }
#endif
  ptts_gen_params gp = {};
  gp.max_length = c.max_ctx; gp.temperature = 1.f; gp.top_p = 1.f; gp.use_eos_gate = 1;
  e->gp = gp;
  *out = e;
  return PTTS_OK;
}

extern "C" void ptts_engine_destroy(ptts_engine* e) {
  if (!e) return;
  PttsDeviceGuard _dg(e->cfg.device);
  hipDeviceSynchronize();
  for (auto& kv : e->graphs) hipGraphExecDestroy(kv.second);
  for (void* p : e->allocs) hipFree(p);
  if (e->host_pinned) hipHostFree(e->host_pinned);
  if (e->le_stage) hipHostFree(e->le_stage);
  for (hipEvent_t ev : e->le_ev) if (ev) hipEventDestroy(ev);
  if (e->own_stream) hipStreamDestroy(e->own_stream);
  if (e->ev_first) hipEventDestroy(e->ev_first);
  if (e->ev_tail0) hipEventDestroy(e->ev_tail0);
  if (e->ev_pre0) hipEventDestroy(e->ev_pre0);
  delete e;
}

extern "C" int ptts_load_weight(ptts_engine* e, const char* name_c, const void* dev_ptr, int32_t src_dtype, const int64_t* shape,
                                int32_t ndim, void* stream) {
  PTTS_CHECK(e && name_c && dev_ptr && shape, PTTS_E_INVALID, "null argument");
  PTTS_CHECK(src_dtype == PTTS_F32 || src_dtype == PTTS_BF16, PTTS_E_INVALID, "src_dtype must be f32 or bf16");
  PTTS_DEVICE(e->cfg.device);
  hipStream_t st = pick_stream(e, stream);
  const ptts_config& c = e->cfg;
  const int H = c.hidden_size, K = c.num_codebooks, V = c.vocab_size;
  const std::string name(name_c);
  auto want = [&](int64_t a, int64_t b) -> int {
    if (b < 0) { if (ndim != 1 || shape[0] != a) return ptts_fail(PTTS_E_INVALID, "%s: expected shape [%lld]", name_c, (long long)a); }
    else if (ndim != 2 || shape[0] != a || shape[1] != b) return ptts_fail(PTTS_E_INVALID, "%s: expected shape [%lld, %lld]", name_c, (long long)a, (long long)b);
    return PTTS_OK;
  };
  int l = -1, k = -1;
  char tail[128] = {0};
  if (sscanf(name_c, "model.decoder.layers.%d.%127s", &l, tail) == 2) {
    PTTS_CHECK(l >= 0 && l < c.num_layers, PTTS_E_INVALID, "%s: layer index out of range", name_c);
    const std::string t(tail);
    for (const LayerTensor& m : layer_tensors(e, e->L[l]))
      if (t == m.name) {
        PTTS_TRY(want(m.N, m.K));
        if (m.K < 0) PTTS_TRY(convert_into<float>((float*)m.dst, dev_ptr, src_dtype, m.N, st));
        else PTTS_TRY(pack_dispatch(e, m.dst, dev_ptr, src_dtype, m.N, m.K, m.row0, st));
        if (m.rm && !e->sc.w8) PTTS_TRY(rowmajor_dispatch(e, m.rm, dev_ptr, src_dtype, m.N, m.K, m.row0, st));
        e->loaded.insert(name);
        return PTTS_OK;
      }
    return ptts_fail(PTTS_E_INVALID, "unknown tensor name %s", name_c);
  }
  if (sscanf(name_c, "model.decoder.embed_tokens.%d.weight", &k) == 1) {
    PTTS_CHECK(k >= 0 && k < K, PTTS_E_INVALID, "%s: codebook index out of range", name_c);
    PTTS_TRY(want(V + 1, H));
    char* dst = (char*)e->embed + (size_t)k * (V + 1) * H * e->esize;
    if (c.dtype == PTTS_BF16) PTTS_TRY(convert_into<bf16_t>((bf16_t*)dst, dev_ptr, src_dtype, (size_t)(V + 1) * H, st));
    else PTTS_TRY(convert_into<float>((float*)dst, dev_ptr, src_dtype, (size_t)(V + 1) * H, st));
    e->loaded.insert(name);
    return PTTS_OK;
  }
  if (sscanf(name_c, "lm_heads.%d.weight", &k) == 1) {
    PTTS_CHECK(k >= 0 && k < K, PTTS_E_INVALID, "%s: codebook index out of range", name_c);
    PTTS_TRY(want(V, H));
    PTTS_TRY(pack_dispatch(e, e->heads, dev_ptr, src_dtype, V, H, k * V, st));
    if (e->heads_rm && !e->sc.w8) PTTS_TRY(rowmajor_dispatch(e, e->heads_rm, dev_ptr, src_dtype, V, H, k * V, st));
    e->loaded.insert(name);
    return PTTS_OK;
  }
  if (name == "lm_heads.weight") {  // use_fused_lm_heads :1834-1840
    PTTS_TRY(want((int64_t)K * V, H));
    PTTS_TRY(pack_dispatch(e, e->heads, dev_ptr, src_dtype, K * V, H, 0, st));
    if (e->heads_rm && !e->sc.w8) PTTS_TRY(rowmajor_dispatch(e, e->heads_rm, dev_ptr, src_dtype, K * V, H, 0, st));
    for (int i = 0; i < K; ++i) { char nm[64]; snprintf(nm, sizeof nm, "lm_heads.%d.weight", i); e->loaded.insert(nm); }
    return PTTS_OK;
  }
  if (name == "model.decoder.layer_norm.weight" || name == "model.decoder.layer_norm.bias") {
    PTTS_TRY(want(H, -1));
    PTTS_TRY(convert_into<float>(name == "model.decoder.layer_norm.weight" ? e->lnf_g : e->lnf_b, dev_ptr, src_dtype, H, st));
    e->loaded.insert(name);
    return PTTS_OK;
  }
  if (name == "model.decoder.embed_positions.weights") {
    PTTS_CHECK(!c.rope, PTTS_E_INVALID, "%s given but rope_embeddings is set", name_c);
    PTTS_CHECK(ndim == 2 && shape[1] == H && shape[0] >= 1 && shape[0] <= c.max_positions, PTTS_E_INVALID, "%s: expected [<=%d, %d]", name_c, c.max_positions, H);
    PTTS_TRY(convert_into<float>(e->pos_table, dev_ptr, src_dtype, (size_t)shape[0] * H, st));
    e->loaded.insert(name);
    return PTTS_OK;
  }
  if (name == "rope_cos" || name == "rope_sin") {  // fp32 tables as ParlerTTSRotaryEmbedding.forward computes them (:373-406)
    PTTS_CHECK(c.rope, PTTS_E_INVALID, "%s given but rope_embeddings is off", name_c);
    const int rope_rows = std::max(c.max_positions, c.max_ctx);
    PTTS_CHECK(ndim == 2 && shape[1] == 64 && shape[0] >= c.max_ctx && shape[0] <= rope_rows, PTTS_E_INVALID, "%s: expected [%d..%d, 64] (one row per KV position)", name_c, c.max_ctx, rope_rows);
    PTTS_TRY(convert_into<float>(name == "rope_cos" ? e->rope_cos : e->rope_sin, dev_ptr, src_dtype, (size_t)shape[0] * 64, st));
    e->loaded.insert(name);
    return PTTS_OK;
  }
  return ptts_fail(PTTS_E_INVALID, "unknown tensor name %s", name_c);
}

extern "C" int ptts_weights_ready(ptts_engine* e) {
  PTTS_CHECK(e, PTTS_E_INVALID, "null engine");
  std::string missing;
  int n = 0;
  for (const auto& r : e->required)
    if (!e->loaded.count(r)) { if (n++ < 8) missing += (missing.empty() ? "" : ", ") + r; }
  if (n) return ptts_fail(PTTS_E_MISSING, "%d tensors not loaded: %s%s", n, missing.c_str(), n > 8 ? ", ..." : "");
  for (const auto& r : e->required_fp8)
    if (!e->loaded_fp8.count(r)) { if (n++ < 8) missing += (missing.empty() ? "" : ", ") + r; }
  if (n) return ptts_fail(PTTS_E_MISSING, "%d e4m3 weight copies not loaded (ptts_load_weight_fp8): %s%s", n, missing.c_str(), n > 8 ? ", ..." : "");
  return PTTS_OK;
}

// weights_fp8 engines: the OCP e4m3 bytes + per-row power-of-two scales of one projection matrix, quantised by the caller
// (parler_tts_amd/quant.py) from the SAME tensor whose exact bf16 dequantisation went through ptts_load_weight.
extern "C" int ptts_load_weight_fp8(ptts_engine* e, const char* name_c, const uint8_t* q_dev, const float* scale_dev, const int64_t* shape,
                                    int32_t ndim, void* stream) {
  PTTS_CHECK(e && name_c && q_dev && scale_dev && shape, PTTS_E_INVALID, "null argument");
  PTTS_CHECK(e->sc.w8, PTTS_E_INVALID, "ptts_load_weight_fp8 on an engine created without weights_fp8");
  PTTS_CHECK(ndim == 2, PTTS_E_INVALID, "%s: expected a matrix", name_c);
  PTTS_DEVICE(e->cfg.device);
  hipStream_t st = pick_stream(e, stream);
  const ptts_config& c = e->cfg;
  const int H = c.hidden_size, K = c.num_codebooks, V = c.vocab_size;
  LayerTensor m = {};  // the matrix named: rows of the row-major / strip copies and of the scales (no name: none found)
  int l = -1, k = -1;
  char tail[128] = {0};
  if (sscanf(name_c, "model.decoder.layers.%d.%127s", &l, tail) == 2) {
    PTTS_CHECK(l >= 0 && l < c.num_layers, PTTS_E_INVALID, "%s: layer index out of range", name_c);
    const std::string t(tail);
    for (const LayerTensor& x : layer_tensors(e, e->L[l]))  // (the cross K/V projections and the vectors have no scales: refused below)
      if (t == x.name) m = x;
  } else if (sscanf(name_c, "lm_heads.%d.weight", &k) == 1) {
    PTTS_CHECK(k >= 0 && k < K, PTTS_E_INVALID, "%s: codebook index out of range", name_c);
    m = LayerTensor{name_c, e->heads, e->heads_rm, e->heads_p8, e->heads_sc, V, H, k * V};
  }
  const int N = m.N, Kd = m.K, row0 = m.row0;
  PTTS_CHECK(m.name && m.sc, PTTS_E_INVALID, "%s has no e4m3 copy (only the decode-step projection matrices do)", name_c);
  PTTS_CHECK(shape[0] == N && shape[1] == Kd, PTTS_E_INVALID, "%s: expected shape [%d, %d]", name_c, N, Kd);
  // row-major bytes for the GEMV step (engines of <= GV_MAX_ROWS utterances), strip order for the MFMA step (wider engines)
  if (m.rm) PTTS_HIP(hipMemcpyAsync((uint8_t*)m.rm + (size_t)row0 * Kd, q_dev, (size_t)N * Kd, hipMemcpyDeviceToDevice, st));
  if (m.p8) {
    PTTS_CHECK(N % 16 == 0 && Kd % 64 == 0 && row0 % 16 == 0, PTTS_E_INVALID, "%s: [%d, %d] at row %d is not a whole number of 16 x 64 e4m3 strips", name_c, N, Kd, row0);
    const size_t total = (size_t)(N / 16) * (Kd / 64) * 64;
    hipLaunchKernelGGL(pack_w8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, q_dev, reinterpret_cast<uint4*>(m.p8), N, Kd, row0 / 16, Kd / 64);
  }
  PTTS_HIP(hipMemcpyAsync(m.sc + row0, scale_dev, (size_t)N * 4, hipMemcpyDeviceToDevice, st));
  e->loaded_fp8.insert(name_c);
  return PTTS_OK;
}

// the sampler fields of ptts_set_gen_params (the session's) and of ptts_admit_row_gen (one request's: the record reaches the device as it is,
// so its temperature is checked whether or not the request samples, and its min_new_tokens too)
static int check_sampler_params(const ptts_gen_params* gp, bool per_request) {
  if (per_request) PTTS_CHECK(std::isfinite(gp->temperature) && gp->temperature > 0.f, PTTS_E_INVALID, "temperature must be finite and > 0");
  else PTTS_CHECK(!gp->do_sample || gp->temperature > 0.f, PTTS_E_INVALID, "temperature must be > 0");
  PTTS_CHECK(gp->top_p > 0.f && gp->top_p <= 1.f, PTTS_E_INVALID, "top_p must be in (0, 1]");
  PTTS_CHECK(gp->top_k >= 0, PTTS_E_INVALID, "top_k must be >= 0");
  if (per_request) PTTS_CHECK(gp->min_new_tokens >= 0, PTTS_E_INVALID, "min_new_tokens must be >= 0");
  return PTTS_OK;
}

static DevGen dev_gen_of(const ptts_gen_params& gp, int max_length) {
  DevGen hg; hg.max_length = max_length; hg.min_new_tokens = gp.min_new_tokens; hg.do_sample = gp.do_sample;
  hg.top_k = gp.top_k; hg.use_eos_gate = gp.use_eos_gate; hg.temperature = gp.temperature; hg.top_p = gp.top_p;
  hg.seed = gp.seed;
  return hg;
}

extern "C" int ptts_set_gen_params(ptts_engine* e, const ptts_gen_params* gp) {
  PTTS_CHECK(e && gp, PTTS_E_INVALID, "null argument");
  PTTS_CHECK(gp->max_length >= 2, PTTS_E_INVALID, "max_length must be >= 2 (BOS column + 1 token)");
  PTTS_CHECK(gp->max_length <= e->cfg.max_ctx, PTTS_E_CAPACITY, "max_length %d exceeds engine max_ctx %d", gp->max_length, e->cfg.max_ctx);
  PTTS_TRY(check_sampler_params(gp, false));
  e->gp = *gp;
  return PTTS_OK;
}

extern "C" int ptts_set_audio_prefix(ptts_engine* e, const int64_t* codes_dev, int32_t B, int32_t T, void* stream) {
  PTTS_CHECK(e, PTTS_E_INVALID, "null engine");
  const ptts_config& c = e->cfg;
  PTTS_CHECK(T >= 0 && (T == 0 || codes_dev), PTTS_E_INVALID, "bad audio prefix");
  PTTS_CHECK(B >= 1 && B <= c.max_batch, PTTS_E_CAPACITY, "batch %d exceeds engine max_batch %d", B, c.max_batch);
  PTTS_CHECK(T + 2 <= c.max_ctx, PTTS_E_CAPACITY, "voice prompt of %d frames exceeds engine max_ctx %d", T, c.max_ctx);
  PTTS_DEVICE(c.device);
  if (T > 0)
    PTTS_HIP(hipMemcpy2DAsync(e->prefix, (size_t)c.max_ctx * 8, codes_dev, (size_t)T * 8, (size_t)T * 8, (size_t)B * c.num_codebooks,
                              hipMemcpyDeviceToDevice, pick_stream(e, stream)));
  e->pending_T = T;
  return PTTS_OK;
}

static int precapture_graphs(ptts_engine* e, int max_buckets);

// shape checks shared by ptts_prefill and ptts_session_begin (a session speaks of slots and of the widths every request is padded to)
static int check_call_shape(const ptts_engine* e, int B, int N, int P, bool session) {
  const ptts_config& c = e->cfg;
  PTTS_CHECK(B >= 1 && B <= c.max_batch, PTTS_E_CAPACITY, session ? "%d slots exceed engine max_batch %d" : "batch %d exceeds engine max_batch %d", B, c.max_batch);
  PTTS_CHECK(N >= 1 && N <= c.max_enc, PTTS_E_CAPACITY, session ? "encoder width %d exceeds engine max_enc %d" : "encoder length %d exceeds engine max_enc %d", N, c.max_enc);
  PTTS_CHECK(P >= 0 && P + 1 <= e->max_prompt, PTTS_E_CAPACITY, session ? "prompt width %d exceeds engine capacity %d" : "prompt length %d exceeds engine capacity %d", P, e->max_prompt - 1);
  PTTS_CHECK(P + e->gp.max_length <= c.max_ctx, PTTS_E_CAPACITY, "P + max_length = %d exceeds engine max_ctx %d", P + e->gp.max_length, c.max_ctx);
  PTTS_CHECK(P + e->gp.max_length <= c.max_positions || c.rope, PTTS_E_CAPACITY, "P + max_length = %d exceeds max_position_embeddings %d", P + e->gp.max_length, c.max_positions);
  return PTTS_OK;
}

// per-call device params travel as kernel arguments (no host staging buffer to keep alive); e->B / N / P are set by the caller
static void launch_set_params(ptts_engine* e, int T_prefix, hipStream_t st) {
  DevDims hd; hd.P = e->P; hd.N = e->N; hd.max_length = e->gp.max_length;
  hd.T_prefix = T_prefix; hd.prefix = e->prefix; hd.prefix_ld = e->cfg.max_ctx;
  hipLaunchKernelGGL(set_params_kernel, dim3(1), dim3(1), 0, st, e->dims, e->gen, hd, dev_gen_of(e->gp, e->gp.max_length));
}

// Inputs of a prefill over arena rows [row0, row0 + n). Masks: all-ones when absent, so that the captured graph never changes shape - the N / P
// given entries of each row, or the whole row (AdmitMoveArgs::enc_n / prompt_n move exactly that). Encoder states -> qc (consumed by the cross
// K/V projection), prompt embeddings -> ffn: both are scratch of a forward, dead between the steps of a session.
static int stage_inputs(const ptts_engine* e, int row0, int n, const float* enc_dev, const int32_t* enc_mask_dev, const float* prompt_dev,
                        const int32_t* prompt_mask_dev, hipStream_t st) {
  const ptts_config& c = e->cfg;
  const size_t N = e->N, P = e->P, H = c.hidden_size, enc_ld = c.max_enc, prompt_ld = e->max_prompt;
  int* em = e->enc_mask + row0 * enc_ld;
  int* pm = e->prompt_mask + row0 * prompt_ld;
  if (enc_mask_dev) PTTS_HIP(hipMemcpy2DAsync(em, enc_ld * 4, enc_mask_dev, N * 4, N * 4, n, hipMemcpyDeviceToDevice, st));
  else hipLaunchKernelGGL(fill_int_kernel, dim3(64), dim3(256), 0, st, em, 1, n * enc_ld);
  if (prompt_mask_dev && P > 0) PTTS_HIP(hipMemcpy2DAsync(pm, prompt_ld * 4, prompt_mask_dev, P * 4, P * 4, n, hipMemcpyDeviceToDevice, st));
  else hipLaunchKernelGGL(fill_int_kernel, dim3(64), dim3(256), 0, st, pm, 1, n * prompt_ld);
  PTTS_HIP(hipMemcpyAsync(e->qc, enc_dev, n * N * H * 4, hipMemcpyDeviceToDevice, st));
  if (P > 0) PTTS_HIP(hipMemcpyAsync(e->ffn, prompt_dev, n * P * H * 4, hipMemcpyDeviceToDevice, st));
  return PTTS_OK;
}

extern "C" int ptts_prefill(ptts_engine* e, const float* enc_dev, const int32_t* enc_mask_dev, const float* prompt_dev,
                            const int32_t* prompt_mask_dev, int32_t B, int32_t N, int32_t P, int32_t sample, void* stream) {
  PTTS_CHECK(e && enc_dev, PTTS_E_INVALID, "null argument");
  PTTS_TRY(ptts_weights_ready(e));
  const ptts_config& c = e->cfg;
  PTTS_TRY(check_call_shape(e, B, N, P, false));
  PTTS_CHECK(P == 0 || prompt_dev, PTTS_E_INVALID, "prompt_dev is null but P > 0");
  PTTS_CHECK(e->pending_T + 2 <= e->gp.max_length, PTTS_E_INVALID, "voice prompt of %d frames leaves no room below max_length %d", e->pending_T, e->gp.max_length);
  PTTS_DEVICE(c.device);
  hipStream_t st = pick_stream(e, stream);
  const int K = c.num_codebooks;
  e->B = B; e->N = N; e->P = P;
  e->session = false;  // a static batch ends a continuous session
  if (e->rec_on) {  // step records: the arenas of ptts_set_step_records laid out over this call's B utterances ([cap_steps][B][K][V])
    const long long kv = (long long)K * c.vocab_size;
    e->rec_node = e->rec_call.logits_dev != nullptr; e->rec_tail = e->rec_call.scores_dev != nullptr;
    hipLaunchKernelGGL(set_step_record_kernel, dim3((B + 255) / 256), dim3(256), 0, st, e->rec, 0, B,
                       StepRecord{e->rec_call.scores_dev, e->rec_call.logits_dev, e->rec_call.cap_steps, 0, (long long)B * kv}, kv);
  }
  if (sample) PTTS_HIP(hipEventRecord(e->ev_pre0, st));
  launch_set_params(e, e->pending_T, st);
  hipLaunchKernelGGL(session_reset_rows_kernel, dim3((B * K + 255) / 256), dim3(256), 0, st, e->ids, e->ids_ld, e->cur_len, e->unfinished,
                     e->has_eos, e->first_unf, (int*)nullptr, 0, B, K, c.bos_token_id, 1, 0);  // every row live; no per-row end
  PTTS_TRY(stage_inputs(e, 0, B, enc_dev, enc_mask_dev, prompt_dev, prompt_mask_dev, st));
  // voice prompt (ptts_set_audio_prefix): the reference runs BOS + the T given code columns in ONE multi-column forward
  // (:3136-3194, causal attention); so does this prefill whenever the row capacity (max_prompt) holds P + 1 + T positions
  // per utterance. Otherwise the T columns are teacher-forced one position at a time through the decode path (same numbers:
  // causal attention over the same cache).
  const int T = e->pending_T;
  e->pending_T = 0;
  const bool batched = T > 0 && P + 1 + T <= e->max_prompt;
  if (batched) hipLaunchKernelGGL(push_prefix_all_kernel, dim3((B * K * T + 255) / 256), dim3(256), 0, st, e->ids, e->ids_ld, e->dims, T, B, K, c.bos_token_id);
  e->xfold_valid = false;  // the prefill itself (and anything before the fold below) runs the un-folded cross-attention
  FwdView v = whole_view(e);
  v.T = batched ? T : 0;
  PTTS_TRY(forward_dispatch(e, v, true, st));
  e->kv_ub = P + 1 + (batched ? T : 0);  // self-KV positions written by this pass
  if (batched) hipLaunchKernelGGL(set_len_kernel, dim3((B + 255) / 256), dim3(256), 0, st, e->cur_len, B, T + 1);
  for (int j = 1; j <= (batched ? 0 : T); ++j) {  // (un-folded cross block: the fold below has not run yet)
    hipLaunchKernelGGL(push_prefix_col_kernel, dim3((B * K + 255) / 256), dim3(256), 0, st, e->ids, e->ids_ld, e->dims, j, B, K, c.bos_token_id);
    hipLaunchKernelGGL(set_len_kernel, dim3((B + 255) / 256), dim3(256), 0, st, e->cur_len, B, j + 1);
    advance_kv(e);
    PTTS_TRY(forward_dispatch(e, whole_view(e), false, st, true));
  }
  if (sample) { PTTS_HIP(hipEventRecord(e->ev_tail0, st)); PTTS_TRY(launch_tail(e, whole_view(e), st, true)); }  // also embeds the sampled column for the first decode step
  e->first_recorded = false;
  if (sample) { PTTS_HIP(hipEventRecord(e->ev_first, st)); e->first_recorded = true; }
  if (e->sc.xfold_ne && B == 1) {
    // The fold only needs the cross K/V cache. It is enqueued AFTER the sampler tail, so the first token is materialised before the
    // fold's two launches run (time-to-first-token does not pay for it); every decode step that follows on `st` sees the folded
    // matrices by stream order. (Round 2 ran 48 per-layer launches BEFORE the tail: +0.8 ms of time-to-first-token. Running it on a
    // second stream beside the prefill was measured and lost: 8.98 vs 8.44 ms to the first token, and the first streamed chunk 23 ms
    // later, the decode steps waiting on the second hardware queue.)
    if (c.dtype == PTTS_F32) PTTS_TRY((fold_cross<float, false>(e, st)));
    else if (e->sc.w8) PTTS_TRY((fold_cross<bf16_t, true>(e, st)));
    else PTTS_TRY((fold_cross<bf16_t, false>(e, st)));
    e->xfold_valid = true;
  }
  e->h_ready = sample != 0;
  e->prefilled = true;
  if (sample) PTTS_TRY(precapture_graphs(e, 3));  // device loop ahead: the step graphs of the next three 64-position buckets (the rest: ptts_decode_steps, ahead of the GPU)
  return PTTS_OK;
}

// The decode step (170 kernel nodes for Mini-v1 at batch <= 8) is captured ONCE per batch size on the engine's private stream
// (capture records, it does not execute; the legacy NULL stream cannot be captured) and replayed into the caller's.
static int get_graph(ptts_engine* e, int kv_bound, hipGraphExec_t* out) {
  // The node set of the step is its plan (ptts_step_plan.h), and gemv_plan / strip_plan take no engine: beside the engine's fixed cfg, sc and sw they
  // see the batch size, the folded-cross-block flag and the 64-position bucket `kv_bound` (also a kernel argument: the attention fetch bound) -
  // all three in the key. The tail adds session, pen_on, warp_on, le_on and the two step-record bits: the key's upper bits. (Several steps of one bucket per
  // graph launch - round 4's PTTS_GRAPH_STEPS - measured 0.3-0.7 %, profiles/r04_experiments.txt call 19: removed in round 6.)
  const long long key = e->B * 2 + (e->xfold_valid ? 1 : 0) + 4096LL * (kv_bound / 64) + (e->session ? 1LL << 40 : 0)  // session steps end in their own tail
                        + (e->pen_on ? 1LL << 41 : 0)                                                                            // the history-penalty node is present
                        + (e->warp_on ? 1LL << 42 : 0)                                                                           // the tail is the WARP instance
                        + (e->le_on ? 1LL << 43 : 0)                                                                             // the logit-edit node is present
                        + (e->rec_on && e->rec_node ? 1LL << 44 : 0)                                                             // the raw-logits record node is present
                        + (e->rec_on && e->rec_tail ? 1LL << 45 : 0);                                                            // the tail is the RECORD instance
  auto it = e->graphs.find(key);
  if (it != e->graphs.end()) { if (out) *out = it->second; return PTTS_OK; }
  hipGraph_t g = nullptr;
  hipStream_t st = e->own_stream;
  PTTS_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
  // decode step = layers + heads + tail; the tail embeds the column it just sampled for the NEXT replay (no embed node)
  FwdView v = whole_view(e);
  v.kv_bound = kv_bound;
  int rc = forward_dispatch(e, v, false, st, false);
  if (rc == PTTS_OK) rc = launch_tail(e, v, st, true);
  hipError_t ce = hipStreamEndCapture(st, &g);
  if (rc != PTTS_OK) { if (g) hipGraphDestroy(g); return rc; }
  if (ce != hipSuccess) return ptts_fail(PTTS_E_HIP, "hipStreamEndCapture failed: %s", hipGetErrorString(ce));
  hipGraphExec_t ex = nullptr;
  size_t nn = 0;
  if (hipGraphGetNodes(g, nullptr, &nn) == hipSuccess) e->last_graph_nodes = (int)nn;
  hipError_t ie = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
  hipGraphDestroy(g);
  if (ie != hipSuccess) return ptts_fail(PTTS_E_HIP, "hipGraphInstantiate failed: %s", hipGetErrorString(ie));
  e->graphs[key] = ex;
  if (out) *out = ex;
  return PTTS_OK;
}

// The step graphs of the next `max_buckets` 64-position buckets this call can still reach are captured AHEAD of the GPU: at prefill
// (host work that overlaps the prefill kernels already enqueued) and again at the end of every ptts_decode_steps (behind the launches it
// has just enqueued), never in the middle of a run of launches: a first long utterance or stream would otherwise stall for a capture +
// instantiate of ~170-270 nodes every 64 frames, on the latency-critical streaming path. Bounded: the stock generation
// config (max_length 2580) is ~41 buckets, three times what a call that stops on EOS needs, and all of them sat between the prefill and
// the first decode_steps of the first call of every batch size. Graphs are cached for the engine's life, so only the first call of a
// (batch, fold, bucket) pays.
static int precapture_graphs(ptts_engine* e, int max_buckets) {
  const int last_ub = std::min(e->cfg.max_ctx - 1, e->P + (e->session ? e->session_max_length : e->gp.max_length));  // positions the longest run of this call writes
  int rc = PTTS_OK, done = 0;
  for (int ub = e->kv_ub + 1; ub <= last_ub && rc == PTTS_OK && done < max_buckets; ++done) {
    const int bound = kv_bound_of(e, ub);
    rc = get_graph(e, bound, nullptr);
    ub = bound;  // first upper bound of the next bucket: kv_bound_of(ub) > bound
  }
  return rc;
}

extern "C" int ptts_decode_steps(ptts_engine* e, int32_t n_steps, void* stream) {
  PTTS_CHECK(e, PTTS_E_INVALID, "null engine");
  PTTS_CHECK(e->prefilled, PTTS_E_INVALID, "ptts_decode_steps called before ptts_prefill");
  PTTS_CHECK(n_steps >= 0, PTTS_E_INVALID, "n_steps < 0");
  PTTS_DEVICE(e->cfg.device);
  hipStream_t st = pick_stream(e, stream);
  if (n_steps > 0 && !e->h_ready) {  // previous column came from ptts_push_tokens / an un-sampled prefill: embed it once, eagerly
    advance_kv(e);
    PTTS_TRY(forward_dispatch(e, whole_view(e), false, st, true));
    PTTS_TRY(launch_tail(e, whole_view(e), st, true));
    e->h_ready = true;
    --n_steps;
  }
  for (int i = 0; i < n_steps; ++i) {
    hipGraphExec_t ex = nullptr;
    advance_kv(e);
    PTTS_TRY(get_graph(e, e->kv_bound, &ex));  // cached per (batch, fold, 64-position bucket)
    PTTS_HIP(hipGraphLaunch(ex, st));
  }
  if (n_steps > 0) PTTS_TRY(precapture_graphs(e, 2));  // the current bucket and the next one, while the GPU works through what was just enqueued
  return PTTS_OK;
}

// ---- teacher-forced scoring (include/ptts_score.h) ------------------------------------------------------------------------------------
template <typename WT>
static int score_forward(const ptts_engine* e, FwdView v, int T, const ptts_score_io* io, hipStream_t st) {
  const ptts_config& c = e->cfg;
  const int Q = v.P + T;
  PTTS_TRY(project_cross_kv<WT>(e, v, st));
  EmbedRawArgs ea = {};
  ea.tables = e->embed; ea.pos_table = c.rope ? nullptr : e->pos_table; ea.prompt = e->ffn; ea.ids = reinterpret_cast<const long long*>(io->input_ids); ea.h = v.h;
  ea.H = c.hidden_size; ea.K = c.num_codebooks; ea.V1 = c.vocab_size + 1; ea.P = v.P; ea.T = T;
  hipLaunchKernelGGL((embed_raw_kernel<WT>), dim3(Q, v.B), dim3(256), 0, st, ea);
  PTTS_TRY((strip_path<WT>(e, v, strip_plan_now(e, v, true, Q), st, false)));
  ScoreArgs s = {};
  s.x = v.h; s.x_ld = c.hidden_size; s.gamma = e->lnf_g; s.beta = e->lnf_b; s.W = e->heads;
  s.ids = reinterpret_cast<const long long*>(io->input_ids); s.labels = reinterpret_cast<const long long*>(io->labels);
  s.nll = io->nll; s.counted = io->counted; s.logits = io->logits;
  s.H = c.hidden_size; s.K = c.num_codebooks; s.V = c.vocab_size; s.B = v.B; s.Q = Q; s.Qs = io->logits ? Q : T; s.T = T;
  s.bos = c.bos_token_id; s.eos = c.eos_token_id;
  return score_launch<WT>(s, st);
}

extern "C" int ptts_score(ptts_engine* e, const float* enc_dev, const int32_t* enc_mask_dev, const float* prompt_dev, const int32_t* prompt_mask_dev,
                          int32_t B, int32_t N, int32_t P, int32_t T, const ptts_score_io* io, void* stream) {
  PTTS_CHECK(e && enc_dev && io, PTTS_E_INVALID, "null argument");
  PTTS_TRY(ptts_weights_ready(e));
  const ptts_config& c = e->cfg;
  PTTS_CHECK(T >= 1, PTTS_E_INVALID, "T = %d: at least one decoder column", T);
  PTTS_CHECK(io->input_ids && (io->labels || io->logits), PTTS_E_INVALID, "ptts_score_io: input_ids and at least one of labels / logits are required");
  PTTS_CHECK(io->labels ? (io->nll && io->counted) : (!io->nll && !io->counted), PTTS_E_INVALID, "ptts_score_io: nll and counted are given exactly when labels is");
  PTTS_CHECK(P >= 0 && (P == 0 || prompt_dev), PTTS_E_INVALID, "prompt length %d with prompt_dev %s", P, prompt_dev ? "given" : "null");
  PTTS_CHECK(c.hidden_size <= LN_MAX_F4 * 256 && c.hidden_size % 32 == 0, PTTS_E_UNSUPPORTED, "ptts_score: hidden size %d outside the loss kernel's range", c.hidden_size);
  PTTS_CHECK(!c.kv_fp8, PTTS_E_UNSUPPORTED, "ptts_score on a kv_fp8 engine: the loss of a checkpoint is not to depend on an opt-in cache format");
  PTTS_CHECK(e->pending_T == 0, PTTS_E_UNSUPPORTED, "ptts_score with a pending voice prompt of %d frames (ptts_set_audio_prefix)", e->pending_T);
  if (e->session)
    for (int b = 0; b < e->B; ++b) PTTS_CHECK(!e->slot_busy[b], PTTS_E_INVALID, "ptts_score inside a session whose slot %d holds a request: the pass overwrites arena rows", b);
  PTTS_CHECK(B >= 1 && B <= c.max_batch, PTTS_E_CAPACITY, "batch %d exceeds engine max_batch %d", B, c.max_batch);
  PTTS_CHECK(N >= 1 && N <= c.max_enc, PTTS_E_CAPACITY, "encoder length %d exceeds engine max_enc %d", N, c.max_enc);
  PTTS_CHECK((long long)P + T <= e->max_prompt, PTTS_E_CAPACITY, "P + T = %lld positions exceed the engine's prefill capacity %d (max_prompt)", (long long)P + T, e->max_prompt);
  PTTS_CHECK(P + T <= c.max_ctx, PTTS_E_CAPACITY, "P + T = %d exceeds engine max_ctx %d", P + T, c.max_ctx);
  PTTS_CHECK(P + T <= c.max_positions || c.rope, PTTS_E_CAPACITY, "P + T = %d exceeds max_position_embeddings %d", P + T, c.max_positions);
  PTTS_DEVICE(c.device);
  hipStream_t st = pick_stream(e, stream);
  e->B = B; e->N = N; e->P = P;
  e->session = false;      // (an idle session ends here, as at ptts_prefill)
  e->prefilled = false;    // the arena rows hold this pass, not a generation: ptts_decode_steps waits for the next prefill
  e->h_ready = false; e->first_recorded = false;
  e->xfold_valid = false;  // the un-folded cross block; nothing is folded for this call
  e->kv_ub = 0; e->kv_bound = 0;
  launch_set_params(e, 0, st);
  PTTS_TRY(stage_inputs(e, 0, B, enc_dev, enc_mask_dev, prompt_dev, prompt_mask_dev, st));
  FwdView v = whole_view(e);
  return c.dtype == PTTS_BF16 ? score_forward<bf16_t>(e, v, T, io, st) : score_forward<float>(e, v, T, io, st);
}

// ---- continuous session ---------------------------------------------------------------------------------------------------------------
// one body behind both entry points: ptts_session_begin refuses a kv_fp8 engine (its documented behaviour), ptts_session_begin_kv8 any other
static int session_begin(ptts_engine* e, int B, int N, int P, void* stream, bool kv8_entry) {
  PTTS_CHECK(e, PTTS_E_INVALID, "null engine");
  PTTS_TRY(ptts_weights_ready(e));
  const ptts_config& c = e->cfg;
  if (kv8_entry) PTTS_CHECK(c.kv_fp8, PTTS_E_INVALID, "ptts_session_begin_kv8: the engine was created without kv_fp8 (its entry point is ptts_session_begin)");
  else PTTS_CHECK(!c.kv_fp8, PTTS_E_UNSUPPORTED, "continuous sessions do not run on the e4m3 KV cache (kv_fp8)");
  PTTS_CHECK(e->pending_T == 0, PTTS_E_UNSUPPORTED, "a voice prompt is pending (ptts_set_audio_prefix): sessions take none");
  PTTS_TRY(check_call_shape(e, B, N, P, true));
  PTTS_DEVICE(c.device);
  hipStream_t st = pick_stream(e, stream);
  const int H = c.hidden_size, K = c.num_codebooks;
  if (!e->row_maxlen) {  // first session of this engine: the row prefill's own residual rows and per-slot operand tables
    PTTS_TRY(e->alloc(&e->row_maxlen, (size_t)c.max_batch));
    PTTS_TRY(e->alloc(&e->slot_gen, (size_t)c.max_batch));  // with row_maxlen: the step graphs hold a pointer that never changes
    PTTS_TRY(e->alloc(&e->slot_T, (size_t)c.max_batch));    // likewise: a voice admission captures nothing
    PTTS_TRY(e->alloc(&e->dims_adm, (size_t)c.max_batch));  // one per slot: admissions into different slots on different streams share nothing
    PTTS_TRY(e->alloc(&e->h_adm, (size_t)e->max_prompt * H));
    PTTS_TRY(e->alloc(&e->kv_layers_rows, (size_t)c.max_batch * c.num_layers));  // rows_view points into it
    std::vector<KvLayer> kl((size_t)c.max_batch * c.num_layers);
    const size_t kvc = (size_t)e->sc.nkc * c.max_enc * 64 * e->esize;  // one slot's cross K (or V) rows of a layer
    for (int b = 0; b < c.max_batch; ++b)
      for (int l = 0; l < c.num_layers; ++l)
        kl[(size_t)b * c.num_layers + l] = KvLayer{e->L[l].ckv, (char*)e->L[l].k_cross + b * kvc, (char*)e->L[l].v_cross + b * kvc};
    PTTS_HIP(hipMemcpy(e->kv_layers_rows, kl.data(), kl.size() * sizeof(KvLayer), hipMemcpyHostToDevice));
  }
  e->B = B; e->N = N; e->P = P;
  e->session = true;
  e->xfold_valid = false;  // the static cross-attention fold belongs to one utterance: off in a session
  e->session_max_length = e->gp.max_length;
  e->slot_busy.assign(B, 0); e->slot_ub.assign(B, P + 1); e->slot_maxlen.assign(B, e->gp.max_length);
  launch_set_params(e, 0, st);
  hipLaunchKernelGGL(set_slot_gen_kernel, dim3((c.max_batch + 255) / 256), dim3(256), 0, st, e->slot_gen, 0, c.max_batch, SlotGen{});  // no slot has a record of its own
  hipLaunchKernelGGL(fill_int_kernel, dim3(1), dim3(256), 0, st, e->slot_T, 0, (size_t)c.max_batch);  // ... nor a voice prompt
  if (e->pen_on) hipLaunchKernelGGL(set_penalty_kernel, dim3((c.max_batch + 255) / 256), dim3(256), 0, st, e->pen, 0, c.max_batch, e->pen_default);  // ... nor penalties of its own
  if (e->warp_on) hipLaunchKernelGGL(set_warp_kernel, dim3((c.max_batch + 255) / 256), dim3(256), 0, st, e->warp, 0, c.max_batch, e->warp_default);  // ... nor warpers
  if (e->le_on) hipLaunchKernelGGL(copy_logit_edit_kernel, dim3(4, c.max_batch), dim3(256), 0, st, e->le, c.max_batch, 0);  // ... nor logit edits
  if (e->rec_on) {  // ... nor a step record; the session carries both the logits node and the RECORD tail: a slot may ask for either kind
    e->rec_node = e->rec_tail = true;
    hipLaunchKernelGGL(set_step_record_kernel, dim3((c.max_batch + 255) / 256), dim3(256), 0, st, e->rec, 0, c.max_batch, StepRecord{}, 0LL);
  }
  // every slot idle; masks all-ones and step inputs zero so that an idle slot's (discarded) step computes on defined values
  hipLaunchKernelGGL(session_reset_rows_kernel, dim3((B * K + 255) / 256), dim3(256), 0, st, e->ids, e->ids_ld, e->cur_len, e->unfinished, e->has_eos,
                     e->first_unf, e->row_maxlen, 0, B, K, c.bos_token_id, 0, e->gp.max_length);
  hipLaunchKernelGGL(fill_int_kernel, dim3(64), dim3(256), 0, st, e->enc_mask, 1, (size_t)B * c.max_enc);
  hipLaunchKernelGGL(fill_int_kernel, dim3(64), dim3(256), 0, st, e->prompt_mask, 1, (size_t)B * e->max_prompt);
  PTTS_HIP(hipMemsetAsync(e->h, 0, (size_t)B * H * 4, st));
  PTTS_HIP(hipMemsetAsync(e->logits, 0, (size_t)B * K * c.vocab_size * 4, st));
  if (c.kv_fp8) {
    // ... and the K/V rows an idle slot's step attends over: the e4m3 rows and scales of positions [0, P] of its own self arena rows, and the
    // cross rows [0, N) (engine dtype; what a recycled allocation holds may read as NaN). The fused append of an idle or finished slot keeps
    // rewriting its own row (position P, or where the request ended) every step: harmless, an admission rewrites rows [0, P + 1)
    for (const LayerW& w : e->L) {
      hipLaunchKernelGGL(kv8_zero_rows_kernel, dim3(B * e->sc.nkv), dim3(256), 0, st, w.k_self, w.v_self, w.ks_self, w.vs_self, c.max_ctx, P + 1, 4);
      hipLaunchKernelGGL(kv8_zero_rows_kernel, dim3(B * e->sc.nkc), dim3(256), 0, st, w.k_cross, w.v_cross, (float*)nullptr, (float*)nullptr, c.max_enc, N,
                         (int)(64 * e->esize / 16));
    }
    PTTS_TRY(launch_status("kv8_zero_rows"));
  }
  e->kv_ub = P + 1;
  e->kv_bound = kv_bound_of(e, e->kv_ub);
  e->first_recorded = false;
  e->h_ready = true;  // nothing to embed: no slot is live
  e->prefilled = true;
  return PTTS_OK;
}

extern "C" int ptts_session_begin(ptts_engine* e, int32_t B, int32_t N, int32_t P, void* stream) { return session_begin(e, B, N, P, stream, false); }
extern "C" int ptts_session_begin_kv8(ptts_engine* e, int32_t B, int32_t N, int32_t P, void* stream) { return session_begin(e, B, N, P, stream, true); }

// the checks of one request of an admission; *L_out = the request's max_length
static int check_admission(const ptts_engine* e, int row, const float* prompt_dev, int max_length, const ptts_gen_params* gp, int* L_out) {
  PTTS_CHECK(row >= 0 && row < e->B, PTTS_E_INVALID, "slot %d outside the session's %d slots", row, e->B);
  PTTS_CHECK(!e->slot_busy[row], PTTS_E_INVALID, "slot %d still holds a request (ptts_retire_row first)", row);
  PTTS_CHECK(e->pending_T == 0, PTTS_E_UNSUPPORTED, "a voice prompt is pending (ptts_set_audio_prefix): sessions take none");
  PTTS_CHECK(e->P == 0 || prompt_dev, PTTS_E_INVALID, "prompt_dev is null but the session's P > 0");
  const int L = max_length == 0 ? e->session_max_length : max_length;
  PTTS_CHECK(L >= 2, PTTS_E_INVALID, "max_length must be 0 (the session's) or >= 2");
  PTTS_CHECK(L <= e->session_max_length, PTTS_E_CAPACITY, "max_length %d exceeds the session's %d", L, e->session_max_length);
  if (gp) {
    PTTS_TRY(check_sampler_params(gp, true));
    PTTS_CHECK(gp->max_length == 0 || gp->max_length == max_length, PTTS_E_INVALID,
               "gen params max_length %d differs from the max_length argument %d (which rules the slot's end)", gp->max_length, max_length);
  }
  *L_out = L;
  return PTTS_OK;
}

// The per-slot end of an admission, once nothing can refuse it any more: the host's bookkeeping, the request's own sampler record (a slot admitted
// without one kept own = 0 from session begin / its last ptts_retire_row; a refused admission leaves the slot's record cleared), and its tail
static int finish_admission(ptts_engine* e, int row, int L, const ptts_gen_params* gp, bool sample, hipStream_t st, int T = 0) {
  e->slot_busy[row] = 1; e->slot_ub[row] = e->P + 1 + T; e->slot_maxlen[row] = L;  // T voice-prompt positions: the step's fetch bound includes them
  if (gp) hipLaunchKernelGGL(set_slot_gen_kernel, dim3(1), dim3(64), 0, st, e->slot_gen, row, 1, SlotGen{dev_gen_of(*gp, L), 1, 0});
  if (sample) return launch_tail(e, whole_view(e), st, true, row);  // first token of the request + the embedding of its next column into h[row]
  e->h_ready = false;                                               // manual path: the next forward embeds every slot's last column
  return PTTS_OK;
}

extern "C" int ptts_debug_slot_voice(ptts_engine* e, int32_t* frames_host, void* stream) {
  PTTS_CHECK(e && frames_host, PTTS_E_INVALID, "null argument");
  PTTS_CHECK(e->session, PTTS_E_INVALID, "ptts_debug_slot_voice: no continuous session (ptts_session_begin)");
  PTTS_DEVICE(e->cfg.device);
  hipStream_t st = pick_stream(e, stream);
  PTTS_HIP(hipMemcpyAsync(e->host_pinned, e->slot_T, (size_t)e->B * 4, hipMemcpyDeviceToHost, st));
  PTTS_HIP(hipStreamSynchronize(st));
  for (int b = 0; b < e->B; ++b) frames_host[b] = e->host_pinned[b];
  return PTTS_OK;
}

// first group admission of this engine: the residual rows of a group prefill and the operand tables of the move kernels
static int ensure_group_rows(ptts_engine* e) {
  const ptts_config& c = e->cfg;
  if (!e->h_adm_rows) {
    std::vector<AdmitMoveLayer> ml(c.num_layers);
    for (int l = 0; l < c.num_layers; ++l) ml[l] = AdmitMoveLayer{e->L[l].k_self, e->L[l].v_self, e->L[l].k_cross, e->L[l].v_cross};
    PTTS_TRY(e->alloc(&e->move_layers, (size_t)c.num_layers));
    PTTS_HIP(hipMemcpy(e->move_layers, ml.data(), ml.size() * sizeof(AdmitMoveLayer), hipMemcpyHostToDevice));
    if (c.kv_fp8) {
      std::vector<AdmitScaleLayer> sl(c.num_layers);
      for (int l = 0; l < c.num_layers; ++l) sl[l] = AdmitScaleLayer{e->L[l].ks_self, e->L[l].vs_self};
      PTTS_TRY(e->alloc(&e->move_scales, (size_t)c.num_layers));
      PTTS_HIP(hipMemcpy(e->move_scales, sl.data(), sl.size() * sizeof(AdmitScaleLayer), hipMemcpyHostToDevice));
    }
    PTTS_TRY(e->alloc(&e->h_adm_rows, (size_t)(c.max_batch - 1) * e->max_prompt * c.hidden_size));
  }
  return PTTS_OK;
}

// An admission is a list of n requests - slot, max_length, sampler record or none, voice codes and frames or none - and one choice: where its
// prefill pass runs. Everything else is data, and the five entry points below only build the list.
//
// Where. In place: the pass of ONE request runs on the slot's own arena rows (rows_view(e, row, 1)); it needs no spare row. Or on the spare arena
// rows B .. B + n - 1: every array of the engine is batch-outermost and sized for max_batch, so rows_view(e, B, n) is an n-utterance engine and the
// pass is the static prefill forward of a batch of n - the ordinary prefill kernels, chosen by row count - and ONE launch then moves each spare row
// to its slot (admit_move_rows_kernel). The tail runs on the slot itself either way: the draw hash of a slot without a record of its own uses the
// slot index.
//
// Voice prompts. A request that continues a voice prompt of T_j frames is admitted with 1 + T_j given columns: what ptts_set_audio_prefix +
// ptts_prefill do for a static batch. The codes go to the slot's rows of e->prefix, one launch in front of the pass (admit_voice_slots_kernel)
// writes the delay pattern of (BOS + prefix, the request's max_length) to the slot's id columns 1..T_j, its slot_T (which stays set until
// ptts_retire_row; the decode steps read it) and clock, and the DevDims of the row the request runs on; the pass covers P + 1 + Tmax positions per
// row, every row under its own request (FwdView::row_dims: delay pattern, prefix length, logits position), so it feeds the model what the static
// prefill of the same request feeds it. A shorter request is right-padded with PAD columns that causal attention keeps from its own positions, and
// the move carries P + 1 + T_j self rows of request j to its slot and nothing of the padding.
struct Admission {
  const char* call;                    // the entry point, for its refusals
  int n;
  const int32_t* rows;                 // [n] destination slots
  const int32_t* Ls;                   // [n] max_length as given (0: the session's)
  const ptts_gen_params* const* gps;   // null, or [n]: each null or the request's own sampler record
  bool takes_voices;                   // the entry point has voice prompts in its signature: Ts is required
  const int64_t* const* codes;         // null, or [n] device pointers, each null or [K][T_j]
  const int32_t* Ts;                   // null (no request brings a voice prompt), or [n] frames
  bool in_place;                       // n == 1 and the pass runs in the slot itself
  const float* enc; const int32_t* enc_mask; const float* prompt; const int32_t* prompt_mask;  // [n] requests at the session's widths, device
};

static int admit(ptts_engine* e, const Admission& a, bool sample, void* stream) {
  // 1. every check of every request, before anything is launched
  PTTS_CHECK(e, PTTS_E_INVALID, "null engine");
  PTTS_CHECK(e->session, PTTS_E_INVALID, "%s: no continuous session (ptts_session_begin)", a.call);
  PTTS_CHECK(a.n >= 1, PTTS_E_INVALID, "%s: n = %d requests (at least 1)", a.call, a.n);
  PTTS_CHECK(a.enc && a.rows && a.Ls && (a.Ts || !a.takes_voices), PTTS_E_INVALID, "null argument");
  const ptts_config& c = e->cfg;
  const int n = a.n, B = e->B, P = e->P, N = e->N, K = c.num_codebooks;
  std::vector<int> Ls(n), Ts(n, 0);
  int Tmax = 0;
  for (int j = 0; j < n && a.Ts; ++j) {
    const bool given = a.codes && a.codes[j];
    PTTS_CHECK(a.Ts[j] >= 0 && (a.Ts[j] == 0 || given), PTTS_E_INVALID, "request %d: bad voice prompt (T = %d frames, codes %s)", j, a.Ts[j],
               given ? "given" : "null");
    Ts[j] = a.Ts[j];
    Tmax = std::max(Tmax, Ts[j]);
  }
  for (int j = 0; j < n; ++j) {
    PTTS_TRY(check_admission(e, a.rows[j], a.prompt, a.Ls[j], a.gps ? a.gps[j] : nullptr, &Ls[j]));
    for (int i = 0; i < j; ++i) PTTS_CHECK(a.rows[i] != a.rows[j], PTTS_E_INVALID, "slot %d listed twice", a.rows[j]);
    PTTS_CHECK(Ts[j] + 2 <= Ls[j], PTTS_E_INVALID, "request %d: voice prompt of %d frames leaves no room below max_length %d", j, Ts[j], Ls[j]);
  }
  if (!a.in_place)
    PTTS_CHECK(n <= c.max_batch - B, PTTS_E_CAPACITY, "%d requests exceed the %d spare rows behind the session's %d slots (engine max_batch %d)", n,
               c.max_batch - B, B, c.max_batch);
  if (Tmax > 0)
    PTTS_CHECK(P + 1 + Tmax <= e->max_prompt, PTTS_E_CAPACITY, "P + 1 + T = %d positions exceed the engine's prefill capacity %d (max_prompt)", P + 1 + Tmax,
               e->max_prompt);
  PTTS_DEVICE(c.device);
  hipStream_t st = pick_stream(e, stream);
  const int row0 = a.in_place ? a.rows[0] : B;  // first arena row of the pass
  // 2. sampler state (the prefill's embedding reads the BOS column): the spare rows as ptts_prefill prepares a batch of n, every slot under its own
  // max_length. The move touches no sampler state, so the slots could always be reset here; but only a pass in place and the voice preparation read
  // what the reset writes, and n launches in front of the pass are n launch latencies on an idle GPU (a session start in groups of 4 or 8 measured
  // 87 us longer with them there, 37 us without: profiles/admission_one_body.txt), so a plain group resets its slots behind the move, where the
  // pass hides them.
  auto reset_slots = [&] {
    for (int j = 0; j < n; ++j)
      hipLaunchKernelGGL(session_reset_rows_kernel, dim3(1), dim3(256), 0, st, e->ids, e->ids_ld, e->cur_len, e->unfinished, e->has_eos, e->first_unf,
                         e->row_maxlen, a.rows[j], 1, K, c.bos_token_id, 1, Ls[j]);
  };
  const bool reset_first = a.in_place || Tmax > 0;
  if (!a.in_place) {
    PTTS_TRY(ensure_group_rows(e));
    hipLaunchKernelGGL(session_reset_rows_kernel, dim3((n * K + 255) / 256), dim3(256), 0, st, e->ids, e->ids_ld, e->cur_len, e->unfinished, e->has_eos,
                       e->first_unf, e->row_maxlen, B, n, K, c.bos_token_id, 1, e->session_max_length);
  }
  if (reset_first) reset_slots();
  // 3. voice prompts: codes to the slots' prefix rows; id columns, slot_T, clock and the DevDims of the row each request runs on (dims_adm[row0 + j])
  if (Tmax > 0) {
    for (int j = 0; j < n; ++j)
      if (Ts[j] > 0)
        PTTS_HIP(hipMemcpy2DAsync(e->prefix + (size_t)a.rows[j] * K * c.max_ctx, (size_t)c.max_ctx * 8, a.codes[j], (size_t)Ts[j] * 8, (size_t)Ts[j] * 8,
                                  (size_t)K, hipMemcpyDeviceToDevice, st));
    for (int j0 = 0; j0 < n; j0 += ADMIT_ROWS_MAX) {
      const int nj = std::min(n - j0, ADMIT_ROWS_MAX);
      AdmitVoiceSlotsArgs va = {};
      va.ids = e->ids; va.prefix = e->prefix; va.slot_T = e->slot_T; va.cur_len = e->cur_len; va.row_dims = e->dims_adm + row0 + j0;
      va.ids_ld = e->ids_ld; va.prefix_ld = c.max_ctx; va.K = K; va.bos = c.bos_token_id; va.pad = c.pad_token_id; va.P = P; va.N = N;
      for (int j = 0; j < nj; ++j) { va.rows[j] = a.rows[j0 + j]; va.Ts[j] = Ts[j0 + j]; va.Ls[j] = Ls[j0 + j]; }
      hipLaunchKernelGGL(admit_voice_slots_kernel, dim3((K * Tmax + 255) / 256, nj), dim3(256), 0, st, va);
    }
  }
  // 4. the pass: n * (P + 1 + Tmax) residual rows (in place: h_adm; a group: h_adm_rows, at most (max_batch - 1) * max_prompt); the step graphs
  // reference neither
  PTTS_TRY(stage_inputs(e, row0, n, a.enc, a.enc_mask, a.prompt, a.prompt_mask, st));
  FwdView v = rows_view(e, row0, n, a.in_place ? e->h_adm : e->h_adm_rows);
  v.T = Tmax;
  if (Tmax > 0) v.row_dims = e->dims_adm + row0;
  PTTS_TRY(forward_dispatch(e, v, true, st));
  // 5. spare rows to their slots
  if (!a.in_place) {
    const int ru = (int)(64 * e->esize / 16), sru = c.kv_fp8 ? 4 : ru;  // 16-byte units of an arena row: engine dtype; self rows (e4m3: 64 bytes)
    for (int j0 = 0; j0 < n; j0 += ADMIT_ROWS_MAX) {
      const int nj = std::min(n - j0, ADMIT_ROWS_MAX);
      AdmitMoveArgs m = {};
      m.layers = e->move_layers; m.logits = e->logits; m.enc_mask = e->enc_mask; m.prompt_mask = e->prompt_mask;
      m.src0 = B + j0; m.nlayers = c.num_layers; m.nkv = e->sc.nkv; m.nkc = e->sc.nkc;
      m.row_u = sru; m.self_cap_u = c.max_ctx * sru; m.cross_u = N * ru; m.cross_cap_u = c.max_enc * ru;
      m.logit_u = K * c.vocab_size / 4;
      m.enc_n = a.enc_mask ? N : c.max_enc; m.enc_ld = c.max_enc;  // what stage_inputs wrote of each mask row
      m.prompt_n = (a.prompt_mask && P > 0) ? P : e->max_prompt; m.prompt_ld = e->max_prompt;
      for (int j = 0; j < nj; ++j) { m.rows[j] = a.rows[j0 + j]; m.self_rows[j] = P + 1 + Ts[j0 + j]; }
      const int units = 2 * (e->sc.nkv * (P + 1 + Tmax) * sru + e->sc.nkc * m.cross_u);  // of the longest request
      hipLaunchKernelGGL(admit_move_rows_kernel, dim3(std::max(1, std::min(64, (units + 1023) / 1024)), c.num_layers + 1, nj), dim3(256), 0, st, m);
      if (c.kv_fp8) {  // the rows' scales travel with them
        AdmitScaleArgs sa = {};
        sa.layers = e->move_scales; sa.src0 = B + j0; sa.nkv = e->sc.nkv; sa.cap = c.max_ctx;
        for (int j = 0; j < nj; ++j) { sa.rows[j] = a.rows[j0 + j]; sa.ns[j] = P + 1 + Ts[j0 + j]; }
        hipLaunchKernelGGL(admit_move_scales_kernel, dim3(1, c.num_layers, nj), dim3(256), 0, st, sa);
      }
    }
    PTTS_TRY(launch_status("admit_move_rows"));
  }
  if (!reset_first) reset_slots();
  // 6. per slot: bookkeeping, record, tail
  for (int j = 0; j < n; ++j) PTTS_TRY(finish_admission(e, a.rows[j], Ls[j], a.gps ? a.gps[j] : nullptr, sample, st, Ts[j]));
  return PTTS_OK;
}

extern "C" int ptts_admit_row_gen(ptts_engine* e, int32_t row, const float* enc_dev, const int32_t* enc_mask_dev, const float* prompt_dev,
                                  const int32_t* prompt_mask_dev, int32_t max_length, int32_t sample, const ptts_gen_params* gp, void* stream) {
  PTTS_CHECK(e && enc_dev, PTTS_E_INVALID, "null argument");
  return admit(e, Admission{"ptts_admit_row", 1, &row, &max_length, gp ? &gp : nullptr, false, nullptr, nullptr, true, enc_dev, enc_mask_dev, prompt_dev,
                            prompt_mask_dev}, sample != 0, stream);
}

extern "C" int ptts_admit_row(ptts_engine* e, int32_t row, const float* enc_dev, const int32_t* enc_mask_dev, const float* prompt_dev,
                              const int32_t* prompt_mask_dev, int32_t max_length, int32_t sample, void* stream) {
  return ptts_admit_row_gen(e, row, enc_dev, enc_mask_dev, prompt_dev, prompt_mask_dev, max_length, sample, nullptr, stream);
}

extern "C" int ptts_admit_row_voice(ptts_engine* e, int32_t row, const float* enc_dev, const int32_t* enc_mask_dev, const float* prompt_dev,
                                    const int32_t* prompt_mask_dev, const int64_t* codes_dev, int32_t T, int32_t max_length, int32_t sample,
                                    const ptts_gen_params* gp, void* stream) {
  PTTS_CHECK(e && enc_dev, PTTS_E_INVALID, "null argument");
  return admit(e, Admission{"ptts_admit_row_voice", 1, &row, &max_length, gp ? &gp : nullptr, true, &codes_dev, &T, true, enc_dev, enc_mask_dev,
                            prompt_dev, prompt_mask_dev}, sample != 0, stream);
}

// (also n = 1 runs on a spare row: an engine without one keeps refusing the call)
extern "C" int ptts_admit_rows(ptts_engine* e, int32_t n, const int32_t* rows, const float* enc_dev, const int32_t* enc_mask_dev, const float* prompt_dev,
                               const int32_t* prompt_mask_dev, const int32_t* max_lengths, int32_t sample, const ptts_gen_params* const* gps,
                               void* stream) {
  return admit(e, Admission{"ptts_admit_rows", n, rows, max_lengths, gps, false, nullptr, nullptr, false, enc_dev, enc_mask_dev, prompt_dev,
                            prompt_mask_dev}, sample != 0, stream);
}

// (one request that brings a voice prompt runs in place, as ptts_admit_row_voice; a list in which none does is ptts_admit_rows' call)
extern "C" int ptts_admit_rows_voice(ptts_engine* e, int32_t n, const int32_t* rows, const float* enc_dev, const int32_t* enc_mask_dev,
                                     const float* prompt_dev, const int32_t* prompt_mask_dev, const int64_t* const* codes_dev, const int32_t* Ts,
                                     const int32_t* max_lengths, int32_t sample, const ptts_gen_params* const* gps, void* stream) {
  const bool in_place = n == 1 && Ts && Ts[0] > 0;
  return admit(e, Admission{"ptts_admit_rows_voice", n, rows, max_lengths, gps, true, codes_dev, Ts, in_place, enc_dev, enc_mask_dev, prompt_dev,
                            prompt_mask_dev}, sample != 0, stream);
}

extern "C" int ptts_retire_row(ptts_engine* e, int32_t row, void* stream) {
  PTTS_CHECK(e, PTTS_E_INVALID, "null engine");
  PTTS_CHECK(e->session, PTTS_E_INVALID, "ptts_retire_row: no continuous session (ptts_session_begin)");
  PTTS_CHECK(row >= 0 && row < e->B, PTTS_E_INVALID, "slot %d outside the session's %d slots", row, e->B);
  PTTS_DEVICE(e->cfg.device);
  hipLaunchKernelGGL(session_reset_rows_kernel, dim3(1), dim3(256), 0, pick_stream(e, stream), e->ids, e->ids_ld, e->cur_len, e->unfinished, e->has_eos,
                     e->first_unf, e->row_maxlen, row, 1, e->cfg.num_codebooks, e->cfg.bos_token_id, 0, e->session_max_length);
  hipLaunchKernelGGL(set_slot_gen_kernel, dim3(1), dim3(64), 0, pick_stream(e, stream), e->slot_gen, row, 1, SlotGen{});  // the next plain admission samples on the session's
  hipLaunchKernelGGL(fill_int_kernel, dim3(1), dim3(64), 0, pick_stream(e, stream), e->slot_T + row, 0, (size_t)1);  // ... and continues no voice prompt
  if (e->pen_on) hipLaunchKernelGGL(set_penalty_kernel, dim3(1), dim3(64), 0, pick_stream(e, stream), e->pen, row, 1, e->pen_default);  // ... under the session's penalties
  if (e->warp_on) hipLaunchKernelGGL(set_warp_kernel, dim3(1), dim3(64), 0, pick_stream(e, stream), e->warp, row, 1, e->warp_default);  // ... and warpers
  if (e->le_on) hipLaunchKernelGGL(copy_logit_edit_kernel, dim3(4, 1), dim3(256), 0, pick_stream(e, stream), e->le, e->cfg.max_batch, row);  // ... and logit edits
  if (e->rec_on) hipLaunchKernelGGL(set_step_record_kernel, dim3(1), dim3(64), 0, pick_stream(e, stream), e->rec, row, 1, StepRecord{}, 0LL);  // ... and records nothing
  e->slot_busy[row] = 0; e->slot_ub[row] = e->P + 1;
  return PTTS_OK;
}

// ---- history penalties (ptts_penalty.h) --------------------------------------------------------------------------------------------------
static int check_history_penalty(const ptts_history_penalty* hp) {
  PTTS_CHECK(std::isfinite(hp->repetition_penalty) && hp->repetition_penalty > 0.0f, PTTS_E_INVALID, "repetition_penalty must be finite and > 0, got %g",
             (double)hp->repetition_penalty);
  PTTS_CHECK(hp->no_repeat_ngram_size >= 0, PTTS_E_INVALID, "no_repeat_ngram_size must be >= 0, got %d", hp->no_repeat_ngram_size);
  return PTTS_OK;
}

extern "C" int ptts_set_history_penalty(ptts_engine* e, const ptts_history_penalty* hp, void* stream) {
  PTTS_CHECK(e, PTTS_E_INVALID, "null engine");
  if (e->session)  // a session that holds a request is running: its node set was fixed at its begin
    for (char busy : e->slot_busy) PTTS_CHECK(!busy, PTTS_E_INVALID, "ptts_set_history_penalty inside a running session (call it before ptts_session_begin)");
  if (!hp) { e->pen_on = false; e->pen_default = HistoryPenalty{1.0f, 0}; return PTTS_OK; }
  PTTS_TRY(check_history_penalty(hp));
  const ptts_config& c = e->cfg;
  PTTS_CHECK(c.vocab_size <= PTTS_PENALTY_MAX_V, PTTS_E_UNSUPPORTED, "history penalties serve vocabularies up to %d, this engine's is %d", PTTS_PENALTY_MAX_V, c.vocab_size);
  PTTS_DEVICE(c.device);
  if (!e->pen) PTTS_TRY(e->alloc(&e->pen, (size_t)c.max_batch));
  e->pen_default = HistoryPenalty{hp->repetition_penalty, hp->no_repeat_ngram_size};
  hipLaunchKernelGGL(set_penalty_kernel, dim3((c.max_batch + 255) / 256), dim3(256), 0, pick_stream(e, stream), e->pen, 0, c.max_batch, e->pen_default);
  PTTS_TRY(launch_status("set_penalty"));
  e->pen_on = true;
  return PTTS_OK;
}

extern "C" int ptts_set_slot_history_penalty(ptts_engine* e, int32_t row, const ptts_history_penalty* hp, void* stream) {
  PTTS_CHECK(e, PTTS_E_INVALID, "null engine");
  PTTS_CHECK(e->session, PTTS_E_INVALID, "ptts_set_slot_history_penalty: no continuous session (ptts_session_begin)");
  PTTS_CHECK(e->pen_on, PTTS_E_INVALID, "ptts_set_slot_history_penalty: the session was begun without history penalties (ptts_set_history_penalty first)");
  PTTS_CHECK(row >= 0 && row < e->B, PTTS_E_INVALID, "slot %d outside the session's %d slots", row, e->B);
  PTTS_CHECK(!e->slot_busy[row], PTTS_E_INVALID, "slot %d still holds a request (ptts_retire_row first)", row);
  if (hp) PTTS_TRY(check_history_penalty(hp));
  PTTS_DEVICE(e->cfg.device);
  const HistoryPenalty rec = hp ? HistoryPenalty{hp->repetition_penalty, hp->no_repeat_ngram_size} : e->pen_default;
  hipLaunchKernelGGL(set_penalty_kernel, dim3(1), dim3(64), 0, pick_stream(e, stream), e->pen, row, 1, rec);
  return launch_status("set_penalty");
}

// ---- sampling warpers (ptts_warp.h) -------------------------------------------------------------------------------------------------------
static int check_sample_warp(const ptts_sample_warp* w) {
  PTTS_CHECK(std::isfinite(w->min_p) && w->min_p >= 0.0f && w->min_p <= 1.0f, PTTS_E_INVALID, "min_p must lie in [0, 1], got %g", (double)w->min_p);
  PTTS_CHECK(std::isfinite(w->typical_p) && w->typical_p > 0.0f && w->typical_p <= 1.0f, PTTS_E_INVALID, "typical_p must lie in (0, 1], got %g", (double)w->typical_p);
  PTTS_CHECK(std::isfinite(w->epsilon_cutoff) && w->epsilon_cutoff >= 0.0f && w->epsilon_cutoff < 1.0f, PTTS_E_INVALID,
             "epsilon_cutoff must lie in [0, 1), got %g", (double)w->epsilon_cutoff);
  PTTS_CHECK(std::isfinite(w->eta_cutoff) && w->eta_cutoff >= 0.0f && w->eta_cutoff < 1.0f, PTTS_E_INVALID, "eta_cutoff must lie in [0, 1), got %g",
             (double)w->eta_cutoff);
  return PTTS_OK;
}

extern "C" int ptts_set_sample_warp(ptts_engine* e, const ptts_sample_warp* w, void* stream) {
  PTTS_CHECK(e, PTTS_E_INVALID, "null engine");
  if (e->session)  // a session that holds a request is running: its tail instance was fixed at its begin
    for (char busy : e->slot_busy) PTTS_CHECK(!busy, PTTS_E_INVALID, "ptts_set_sample_warp inside a running session (call it before ptts_session_begin)");
  if (!w) { e->warp_on = false; e->warp_default = DevWarp{0.f, 1.f, 0.f, 0.f}; return PTTS_OK; }
  PTTS_TRY(check_sample_warp(w));
  const ptts_config& c = e->cfg;
  PTTS_DEVICE(c.device);
  if (!e->warp) PTTS_TRY(e->alloc(&e->warp, (size_t)c.max_batch));
  e->warp_default = DevWarp{w->min_p, w->typical_p, w->epsilon_cutoff, w->eta_cutoff};
  hipLaunchKernelGGL(set_warp_kernel, dim3((c.max_batch + 255) / 256), dim3(256), 0, pick_stream(e, stream), e->warp, 0, c.max_batch, e->warp_default);
  PTTS_TRY(launch_status("set_warp"));
  e->warp_on = true;
  return PTTS_OK;
}

extern "C" int ptts_set_slot_sample_warp(ptts_engine* e, int32_t row, const ptts_sample_warp* w, void* stream) {
  PTTS_CHECK(e, PTTS_E_INVALID, "null engine");
  PTTS_CHECK(e->session, PTTS_E_INVALID, "ptts_set_slot_sample_warp: no continuous session (ptts_session_begin)");
  PTTS_CHECK(e->warp_on, PTTS_E_INVALID, "ptts_set_slot_sample_warp: the session was begun without sampling warpers (ptts_set_sample_warp first)");
  PTTS_CHECK(row >= 0 && row < e->B, PTTS_E_INVALID, "slot %d outside the session's %d slots", row, e->B);
  PTTS_CHECK(!e->slot_busy[row], PTTS_E_INVALID, "slot %d still holds a request (ptts_retire_row first)", row);
  if (w) PTTS_TRY(check_sample_warp(w));
  PTTS_DEVICE(e->cfg.device);
  const DevWarp rec = w ? DevWarp{w->min_p, w->typical_p, w->epsilon_cutoff, w->eta_cutoff} : e->warp_default;
  hipLaunchKernelGGL(set_warp_kernel, dim3(1), dim3(64), 0, pick_stream(e, stream), e->warp, row, 1, rec);
  return launch_status("set_warp");
}

// ---- step records (ptts_step_record.h) ----------------------------------------------------------------------------------------------------
static int check_step_records(const ptts_step_records* r) {
  PTTS_CHECK(r->cap_steps >= 0, PTTS_E_INVALID, "step records: cap_steps must be >= 0, got %d", r->cap_steps);
  PTTS_CHECK(r->cap_steps > 0 || (!r->scores_dev && !r->logits_dev), PTTS_E_INVALID, "step records: an arena with cap_steps == 0");
  return PTTS_OK;
}

extern "C" int ptts_set_step_records(ptts_engine* e, const ptts_step_records* r, void* stream) {
  PTTS_CHECK(e, PTTS_E_INVALID, "null engine");
  if (e->session)  // a session that holds a request is running: its node set and its tail instance were fixed at its begin
    for (char busy : e->slot_busy) PTTS_CHECK(!busy, PTTS_E_INVALID, "ptts_set_step_records inside a running session (call it before ptts_session_begin)");
  if (!r) { e->rec_on = e->rec_node = e->rec_tail = false; e->rec_call = ptts_step_records{}; return PTTS_OK; }
  PTTS_TRY(check_step_records(r));
  const ptts_config& c = e->cfg;
  PTTS_CHECK(c.vocab_size <= PTTS_SORT_N, PTTS_E_UNSUPPORTED, "step records serve vocabularies up to %d, this engine's is %d", PTTS_SORT_N, c.vocab_size);
  PTTS_DEVICE(c.device);
  if (!e->rec) PTTS_TRY(e->alloc(&e->rec, (size_t)c.max_batch));
  hipLaunchKernelGGL(set_step_record_kernel, dim3((c.max_batch + 255) / 256), dim3(256), 0, pick_stream(e, stream), e->rec, 0, c.max_batch, StepRecord{}, 0LL);
  PTTS_TRY(launch_status("set_step_record"));
  e->rec_call = *r;
  e->rec_on = true;
  // until the next ptts_prefill / ptts_session_begin decides: what a call of this shape will carry (both kinds when no arena is given: a session)
  e->rec_node = r->logits_dev != nullptr || !r->scores_dev;
  e->rec_tail = r->scores_dev != nullptr || !r->logits_dev;
  return PTTS_OK;
}

extern "C" int ptts_set_slot_step_records(ptts_engine* e, int32_t row, const ptts_step_records* r, void* stream) {
  PTTS_CHECK(e, PTTS_E_INVALID, "null engine");
  PTTS_CHECK(e->session, PTTS_E_INVALID, "ptts_set_slot_step_records: no continuous session (ptts_session_begin)");
  PTTS_CHECK(e->rec_on, PTTS_E_INVALID, "ptts_set_slot_step_records: the session was begun without step records (ptts_set_step_records first)");
  PTTS_CHECK(row >= 0 && row < e->B, PTTS_E_INVALID, "slot %d outside the session's %d slots", row, e->B);
  PTTS_CHECK(!e->slot_busy[row], PTTS_E_INVALID, "slot %d still holds a request (ptts_retire_row first)", row);
  if (r) PTTS_TRY(check_step_records(r));
  PTTS_DEVICE(e->cfg.device);
  const long long kv = (long long)e->cfg.num_codebooks * e->cfg.vocab_size;
  const StepRecord rec = r ? StepRecord{r->scores_dev, r->logits_dev, r->cap_steps, 0, kv} : StepRecord{};
  hipLaunchKernelGGL(set_step_record_kernel, dim3(1), dim3(64), 0, pick_stream(e, stream), e->rec, row, 1, rec, 0LL);
  return launch_status("set_step_record");
}

// ---- logit edits (ptts_logit_edit.h) ------------------------------------------------------------------------------------------------------
// one record on the host, as its staging area holds it: header, bias row, decay table, class flags
struct HostLogitEdit {
  LogitEditHeader hdr = {};
  std::vector<float> bias, decay;
  std::vector<unsigned char> flags;
};

// every check of a record, then its arrays; nothing of the engine changes here
static int build_logit_edit(const ptts_engine* e, const ptts_logit_edits* le, HostLogitEdit* out) {
  const int V = e->cfg.vocab_size, eos = e->cfg.eos_token_id, ld_t = e->ids_ld;
  PTTS_CHECK(le->n_bias >= 0 && le->n_bad >= 0 && le->n_suppress >= 0 && le->n_begin_suppress >= 0, PTTS_E_INVALID, "logit edits: a negative count");
  PTTS_CHECK((le->n_bias == 0 || (le->bias_tokens && le->bias_values)) && (le->n_bad == 0 || le->bad_tokens) && (le->n_suppress == 0 || le->suppress_tokens) &&
                 (le->n_begin_suppress == 0 || le->begin_suppress_tokens), PTTS_E_INVALID, "logit edits: a null array with a positive count");
  for (int i = 0; i < le->n_bias; ++i) {
    PTTS_CHECK(le->bias_tokens[i] >= 0 && le->bias_tokens[i] < V, PTTS_E_INVALID, "sequence_bias token %d outside the vocabulary [0, %d)", le->bias_tokens[i], V);
    PTTS_CHECK(std::isfinite(le->bias_values[i]), PTTS_E_INVALID, "sequence_bias of token %d must be finite, got %g", le->bias_tokens[i], (double)le->bias_values[i]);
  }
  for (int i = 0; i < le->n_bad; ++i)
    PTTS_CHECK(le->bad_tokens[i] >= 0 && le->bad_tokens[i] < V, PTTS_E_INVALID, "bad_words_ids token %d outside the vocabulary [0, %d)", le->bad_tokens[i], V);
  if (le->decay_on) {
    PTTS_CHECK(le->decay_start >= 0, PTTS_E_INVALID, "exponential_decay_length_penalty start must be >= 0, got %d", le->decay_start);
    PTTS_CHECK(std::isfinite(le->decay_factor) && le->decay_factor > 0.0, PTTS_E_INVALID, "exponential_decay_length_penalty factor must be finite and > 0, got %g",
               le->decay_factor);
  }
  HostLogitEdit& r = *out;
  r.bias.assign((size_t)V, 0.0f); r.flags.assign((size_t)V, 0); r.decay.clear();
  int mask = 0;
  for (int i = 0; i < le->n_bias; ++i) { r.bias[le->bias_tokens[i]] = le->bias_values[i]; mask |= PTTS_LE_BIAS; }
  for (int i = 0; i < le->n_bad; ++i) {  // NoBadWordsLogitsProcessor drops [eos] and still adds its bias row, all zeros if nothing is left
    mask |= PTTS_LE_BAD;
    if (le->bad_tokens[i] != eos) r.flags[le->bad_tokens[i]] |= PTTS_LEF_BAD;
  }
  for (int i = 0; i < le->n_suppress; ++i) {  // torch.isin over arange(V): a token outside it matches nothing, the stage itself stays
    mask |= PTTS_LE_SUPPRESS;
    if (le->suppress_tokens[i] >= 0 && le->suppress_tokens[i] < V) r.flags[le->suppress_tokens[i]] |= PTTS_LEF_SUPPRESS;
  }
  for (int i = 0; i < le->n_begin_suppress; ++i) {
    mask |= PTTS_LE_BEGIN;
    if (le->begin_suppress_tokens[i] >= 0 && le->begin_suppress_tokens[i] < V) r.flags[le->begin_suppress_tokens[i]] |= PTTS_LEF_BEGIN;
  }
  if (le->decay_on) {  // m[idx] for every idx a clock of this engine can reach (idx < t < ids_ld), with the C library's pow as Python's float pow is
    mask |= PTTS_LE_DECAY;
    r.decay.resize((size_t)ld_t);
    for (int i = 0; i < ld_t; ++i) r.decay[i] = (float)(pow(le->decay_factor, (double)i) - 1.0);
  }
  r.hdr = LogitEditHeader{mask, le->decay_on ? le->decay_start : 0, le->decay_on ? ld_t : 0, 0};
  return PTTS_OK;
}

// First switch-on: the records, their staging areas and events. Every piece is kept in the engine as soon as it exists, so a call that fails half
// way (out of memory) leaves nothing behind that the next call allocates again; the records count as ready (le_ready) only once all of them are
// there and zeroed. The zeroing is ordered on the setter's stream, in front of its first upload.
static int ensure_logit_edit_records(ptts_engine* e, hipStream_t st) {
  if (e->le_ready) return PTTS_OK;
  const ptts_config& c = e->cfg;
  const size_t n = (size_t)c.max_batch + 1, ld_v = (size_t)((c.vocab_size + 3) & ~3), ld_t = (size_t)e->ids_ld;
  const size_t stride = (sizeof(LogitEditHeader) + 4 * ld_v + 4 * ld_t + ld_v + 15) & ~(size_t)15;
  if (!e->le_stage && hipHostMalloc((void**)&e->le_stage, n * stride) != hipSuccess) return ptts_fail(PTTS_E_HIP, "hipHostMalloc failed");
  e->le_stage_stride = stride;
  if (e->le_ev.size() != n) e->le_ev.assign(n, nullptr);
  e->le.ld_v = (int)ld_v; e->le.ld_t = (int)ld_t;
  if (!e->le.bias) PTTS_TRY(e->alloc(&e->le.bias, n * ld_v));
  if (!e->le.decay) PTTS_TRY(e->alloc(&e->le.decay, n * ld_t));
  if (!e->le.flags) PTTS_TRY(e->alloc(&e->le.flags, n * ld_v));
  if (!e->le.hdr) PTTS_TRY(e->alloc(&e->le.hdr, n));
  PTTS_HIP(hipMemsetAsync(e->le.bias, 0, n * ld_v * 4, st));
  PTTS_HIP(hipMemsetAsync(e->le.decay, 0, n * ld_t * 4, st));
  PTTS_HIP(hipMemsetAsync(e->le.flags, 0, n * ld_v, st));
  PTTS_HIP(hipMemsetAsync(e->le.hdr, 0, n * sizeof(LogitEditHeader), st));
  e->le_ready = true;
  return PTTS_OK;
}

// record `rec` of the device arrays = r, ordered on st: through the record's own pinned staging area, so that the caller's arrays are free at return
static int upload_logit_edit(ptts_engine* e, int rec, const HostLogitEdit& r, hipStream_t st) {
  const size_t ld_v = (size_t)e->le.ld_v, ld_t = (size_t)e->le.ld_t, V = (size_t)e->cfg.vocab_size;
  if (e->le_ev[rec]) PTTS_HIP(hipEventSynchronize(e->le_ev[rec]));  // the area's last upload has left it
  else PTTS_HIP(hipEventCreateWithFlags(&e->le_ev[rec], hipEventDisableTiming));
  unsigned char* s = e->le_stage + (size_t)rec * e->le_stage_stride;
  unsigned char *s_bias = s + sizeof(LogitEditHeader), *s_decay = s_bias + 4 * ld_v, *s_flags = s_decay + 4 * ld_t;
  memcpy(s, &r.hdr, sizeof(LogitEditHeader));
  memcpy(s_bias, r.bias.data(), 4 * V);
  memcpy(s_flags, r.flags.data(), V);
  if (!r.decay.empty()) memcpy(s_decay, r.decay.data(), 4 * std::min(r.decay.size(), ld_t));
  // Only the arrays of the stages in the mask travel: the slot's other arrays keep what an earlier request left there, and logit_edit_kernel
  // reads an array only under its stage's mask bit. (Nothing reads the record between these copies, so their order does not matter.)
  if (r.hdr.mask & PTTS_LE_BIAS) PTTS_HIP(hipMemcpyAsync(e->le.bias + rec * ld_v, s_bias, 4 * V, hipMemcpyHostToDevice, st));
  if (r.hdr.mask & (PTTS_LE_BAD | PTTS_LE_SUPPRESS | PTTS_LE_BEGIN)) PTTS_HIP(hipMemcpyAsync(e->le.flags + rec * ld_v, s_flags, V, hipMemcpyHostToDevice, st));
  if (r.hdr.mask & PTTS_LE_DECAY) PTTS_HIP(hipMemcpyAsync(e->le.decay + rec * ld_t, s_decay, 4 * ld_t, hipMemcpyHostToDevice, st));
  PTTS_HIP(hipMemcpyAsync(e->le.hdr + rec, s, sizeof(LogitEditHeader), hipMemcpyHostToDevice, st));
  PTTS_HIP(hipEventRecord(e->le_ev[rec], st));
  return PTTS_OK;
}

extern "C" int ptts_set_logit_edits(ptts_engine* e, const ptts_logit_edits* le, void* stream) {
  PTTS_CHECK(e, PTTS_E_INVALID, "null engine");
  if (e->session)  // a session that holds a request is running: its node set was fixed at its begin
    for (char busy : e->slot_busy) PTTS_CHECK(!busy, PTTS_E_INVALID, "ptts_set_logit_edits inside a running session (call it before ptts_session_begin)");
  if (!le) { e->le_on = false; return PTTS_OK; }
  const ptts_config& c = e->cfg;
  HostLogitEdit r;
  PTTS_TRY(build_logit_edit(e, le, &r));
  PTTS_CHECK(c.vocab_size <= PTTS_LOGIT_EDIT_MAX_V, PTTS_E_UNSUPPORTED, "logit edits serve vocabularies up to %d, this engine's is %d", PTTS_LOGIT_EDIT_MAX_V, c.vocab_size);
  PTTS_DEVICE(c.device);
  hipStream_t st = pick_stream(e, stream);
  PTTS_TRY(ensure_logit_edit_records(e, st));
  PTTS_TRY(upload_logit_edit(e, c.max_batch, r, st));
  hipLaunchKernelGGL(copy_logit_edit_kernel, dim3(4, c.max_batch), dim3(256), 0, st, e->le, c.max_batch, 0);
  PTTS_TRY(launch_status("copy_logit_edit"));
  e->le_on = true;
  return PTTS_OK;
}

extern "C" int ptts_set_slot_logit_edits(ptts_engine* e, int32_t row, const ptts_logit_edits* le, void* stream) {
  PTTS_CHECK(e, PTTS_E_INVALID, "null engine");
  PTTS_CHECK(e->session, PTTS_E_INVALID, "ptts_set_slot_logit_edits: no continuous session (ptts_session_begin)");
  PTTS_CHECK(e->le_on, PTTS_E_INVALID, "ptts_set_slot_logit_edits: the session was begun without logit edits (ptts_set_logit_edits first)");
  PTTS_CHECK(row >= 0 && row < e->B, PTTS_E_INVALID, "slot %d outside the session's %d slots", row, e->B);
  PTTS_CHECK(!e->slot_busy[row], PTTS_E_INVALID, "slot %d still holds a request (ptts_retire_row first)", row);
  HostLogitEdit r;
  if (le) PTTS_TRY(build_logit_edit(e, le, &r));
  PTTS_DEVICE(e->cfg.device);
  hipStream_t st = pick_stream(e, stream);
  if (le) return upload_logit_edit(e, row, r, st);
  hipLaunchKernelGGL(copy_logit_edit_kernel, dim3(4, 1), dim3(256), 0, st, e->le, e->cfg.max_batch, row);
  return launch_status("copy_logit_edit");
}

extern "C" int ptts_row_state(ptts_engine* e, int32_t* cur_len_host, int32_t* live_host, void* stream) {
  PTTS_CHECK(e, PTTS_E_INVALID, "null engine");
  PTTS_CHECK(e->session, PTTS_E_INVALID, "ptts_row_state: no continuous session (ptts_session_begin)");
  PTTS_DEVICE(e->cfg.device);
  hipStream_t st = pick_stream(e, stream);
  const int B = e->B, K = e->cfg.num_codebooks;
  int* hp = e->host_pinned;
  // cur_len[max_batch] and unfinished[max_batch * K] are separate allocations: two enqueued copies, one sync
  PTTS_HIP(hipMemcpyAsync(hp, e->cur_len, (size_t)B * 4, hipMemcpyDeviceToHost, st));
  PTTS_HIP(hipMemcpyAsync(hp + B, e->unfinished, (size_t)B * K * 4, hipMemcpyDeviceToHost, st));
  PTTS_HIP(hipStreamSynchronize(st));
  for (int b = 0; b < B; ++b) {
    int live = 0;
    for (int k = 0; k < K; ++k) live |= hp[B + b * K + k] > 0;
    if (cur_len_host) cur_len_host[b] = hp[b];
    if (live_host) live_host[b] = live;
  }
  return PTTS_OK;
}

extern "C" int ptts_first_token_sync(ptts_engine* e) {
  PTTS_CHECK(e, PTTS_E_INVALID, "null engine");
  PTTS_CHECK(e->prefilled && e->first_recorded, PTTS_E_INVALID, "ptts_first_token_sync: no sampling prefill to wait for");
  PTTS_DEVICE(e->cfg.device);
  PTTS_HIP(hipEventSynchronize(e->ev_first));
  return PTTS_OK;
}

extern "C" int ptts_first_token_times(ptts_engine* e, float* prefill_ms, float* tail_ms) {
  PTTS_CHECK(e && prefill_ms && tail_ms, PTTS_E_INVALID, "null argument");
  PTTS_CHECK(e->prefilled && e->first_recorded, PTTS_E_INVALID, "ptts_first_token_times: no sampling prefill to report on");
  PTTS_DEVICE(e->cfg.device);
  PTTS_HIP(hipEventSynchronize(e->ev_first));
  PTTS_HIP(hipEventElapsedTime(prefill_ms, e->ev_pre0, e->ev_tail0));
  PTTS_HIP(hipEventElapsedTime(tail_ms, e->ev_tail0, e->ev_first));
  return PTTS_OK;
}

extern "C" int ptts_state(ptts_engine* e, int32_t* cur_len, int32_t* all_finished, void* stream) {
  PTTS_CHECK(e, PTTS_E_INVALID, "null engine");
  PTTS_CHECK(e->prefilled, PTTS_E_INVALID, "ptts_state called before ptts_prefill");
  PTTS_DEVICE(e->cfg.device);
  hipStream_t st = pick_stream(e, stream);
  const int n = e->B * e->cfg.num_codebooks;
  int* hp = e->host_pinned;
  PTTS_HIP(hipMemcpyAsync(hp, e->cur_len, 4, hipMemcpyDeviceToHost, st));
  PTTS_HIP(hipMemcpyAsync(hp + 1, e->unfinished, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  PTTS_HIP(hipStreamSynchronize(st));
  if (cur_len) *cur_len = hp[0];
  int any = 0;
  for (int i = 0; i < n; ++i) any |= hp[1 + i] > 0;  // 1 = still generating, -(t + 1) = finished at step t
  if (all_finished) *all_finished = any ? 0 : 1;
  return PTTS_OK;
}

extern "C" int ptts_ids(ptts_engine* e, int64_t** ids_dev, int32_t* row_stride) {
  PTTS_CHECK(e && ids_dev && row_stride, PTTS_E_INVALID, "null argument");
  *ids_dev = reinterpret_cast<int64_t*>(e->ids);
  *row_stride = e->ids_ld;
  return PTTS_OK;
}

extern "C" int ptts_step_forward(ptts_engine* e, void* stream) {
  PTTS_CHECK(e, PTTS_E_INVALID, "null engine");
  PTTS_CHECK(e->prefilled, PTTS_E_INVALID, "ptts_step_forward called before ptts_prefill");
  PTTS_DEVICE(e->cfg.device);
  advance_kv(e);
  return forward_dispatch(e, whole_view(e), false, pick_stream(e, stream));
}

extern "C" int ptts_logits(ptts_engine* e, float** logits_dev) {
  PTTS_CHECK(e && logits_dev, PTTS_E_INVALID, "null argument");
  *logits_dev = e->logits;
  return PTTS_OK;
}

extern "C" int ptts_push_tokens(ptts_engine* e, const int64_t* tokens_dev, const int32_t* finished_dev, void* stream) {
  PTTS_CHECK(e && tokens_dev, PTTS_E_INVALID, "null argument");
  PTTS_CHECK(e->prefilled, PTTS_E_INVALID, "ptts_push_tokens called before ptts_prefill");
  PTTS_DEVICE(e->cfg.device);
  hipStream_t st = pick_stream(e, stream);
  const int n = e->B * e->cfg.num_codebooks;
  if (e->session) {  // only live slots take tokens and move their clock
    hipLaunchKernelGGL(push_tokens_session_kernel, dim3(e->B), dim3(64), 0, st, (const long long*)tokens_dev, finished_dev, e->ids, e->ids_ld, e->cur_len,
                       e->unfinished, e->has_eos, e->row_maxlen, e->cfg.num_codebooks, e->cfg.eos_token_id);
    e->h_ready = false;
    return PTTS_OK;
  }
  hipLaunchKernelGGL(push_tokens_kernel, dim3((n + 255) / 256), dim3(256), 0, st, (const long long*)tokens_dev, finished_dev, e->ids,
                     e->ids_ld, e->cur_len, e->unfinished, e->has_eos, e->B, e->cfg.num_codebooks, e->cfg.eos_token_id);
  hipLaunchKernelGGL(bump_len_kernel, dim3((e->B + 255) / 256), dim3(256), 0, st, e->cur_len, e->B);
  e->h_ready = false;
  return PTTS_OK;
}

#ifdef PTTS_TIMING
// measurement build only: the stamp buffer [layers + 1][5][3][16] (device memory) of the last replayed single-utterance step
extern "C" int ptts_debug_stamps(ptts_engine* e, long long** stamps_dev, int32_t* layers) {
  PTTS_CHECK(e && stamps_dev && layers, PTTS_E_INVALID, "null argument");
  *stamps_dev = e->dbg_stamps;
  *layers = e->cfg.num_layers;
  return PTTS_OK;
}
#endif

extern "C" int ptts_debug_graph_nodes(ptts_engine* e, int32_t* nodes) {
  PTTS_CHECK(e && nodes, PTTS_E_INVALID, "null argument");
  *nodes = e->last_graph_nodes;
  return PTTS_OK;
}

extern "C" int ptts_debug_self_kv(ptts_engine* e, int32_t layer, void** k_dev, void** v_dev, float** kscale_dev, float** vscale_dev, int32_t* row_bytes,
                                  int32_t* kv_heads, int32_t* cap) {
  PTTS_CHECK(e && k_dev && v_dev && kscale_dev && vscale_dev && row_bytes && kv_heads && cap, PTTS_E_INVALID, "null argument");
  PTTS_CHECK(layer >= 0 && layer < e->cfg.num_layers, PTTS_E_INVALID, "layer %d outside the engine's %d layers", layer, e->cfg.num_layers);
  const LayerW& w = e->L[layer];
  *k_dev = w.k_self; *v_dev = w.v_self; *kscale_dev = w.ks_self; *vscale_dev = w.vs_self;
  *row_bytes = (int32_t)(64 * (e->cfg.kv_fp8 ? 1 : e->esize)); *kv_heads = e->sc.nkv; *cap = e->cfg.max_ctx;
  return PTTS_OK;
}

extern "C" int ptts_debug_hidden(ptts_engine* e, float** hidden_dev, int32_t* rows) {
  PTTS_CHECK(e && hidden_dev && rows, PTTS_E_INVALID, "null argument");
  *hidden_dev = e->h;
  *rows = e->B;
  return PTTS_OK;
}
