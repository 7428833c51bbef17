// Which kernels one decoder forward runs: the decision, and nothing else. Host-only, no kernels, no engine pointer, no HIP call - plain values and
// pure functions of the engine's configuration, its environment switches and the shape of the call. ptts_lm.hip computes one plan per forward and
// its walkers (gemv_step, strip_path) only read it, fill argument structs and launch; tests/native/gemv_harness.hip and step_harness.hip hand the
// same plans and predicates to the tests, so a change of the node set of a step is a change here that the tests read, not a restatement.
#pragma once
#include <stddef.h>

#include "../../include/ptts.h"
#include "ptts_gemv.h"

// ---- the environment switches, read once when the engine is created (ptts_lm.hip: read_env_switches) ------------------------
struct StepSwitches {
  int fuse_qa = 1;       // GEMV step: LN1 + QKV rows + self-attention + append as one node (qkv_attn_kernel), PTTS_NO_FUSE_QA=1 = two nodes
  int fuse_qa_max = 3;   // largest batch that runs the fused node (PTTS_FUSE_QA_MAX = 1..8)
  int fuse_x = -1;       // single-utterance GEMV step, folded cross block: LN2 + scores + softmax + U p as one node of per-head partial rows (xfold_attn_kernel),
                         // summed by the LN3 + fc1 node's prologue (GV_LNP). -1 = by width: on up to hidden 1024 (Mini-v1 -1 %: 566 -> 561 us per step), off
                         // above (Large-v1 +8..17 %: every fc1 workgroup pulls 24 x 6 KB of partial rows through the L2; profiles/r04_experiments.txt
                         // call 16); PTTS_FUSE_X=0 / 1 forces it
  int fuse_x_nur = 2;    // rounds of output rows per workgroup of xfold_attn_kernel (PTTS_FUSE_X_NUR = 2 / 4: nheads x 8 / nheads x 4 workgroups at Mini-v1)
  int fuse_xq = 1;       // GEMV step, un-folded cross block: LN2 + cross-q rows + cross-attention as one node (xq_attn_kernel), PTTS_NO_FUSE_XQ=1 = two nodes
  int lnproj = 3;        // decode at batch > 8: LayerNorm + projection as ONE node tiled over 64 weight rows x lnproj_g utterances (lnproj_fused_kernel) instead of
                         // rows_prep + strip GEMM. PTTS_LNPROJ: 0 off, 1 = LN1 + QKV, 2 = + LN3 + fc1 above 32 utterances, 3 = + LN3 + fc1 at 9..32 too instead of
                         // the producer-statistics prologue. On (3) at every batch size above 8: 8 utterances per workgroup up to 40 (round 4: -5.3 % at 32,
                         // -3.2 % at 12; neutral at 64, +12 % at 128 with 8 per workgroup), 16 per workgroup above (round 5, profiles/r05_experiments.txt call 2:
                         // 48 / 64 / 96 / 128 utterances -9.7 / -6.6 / -2.3 / -5.1 % per step)
  int lnproj_g = 0;      // utterances per workgroup of lnproj_fused_kernel: 0 = by batch size (lnproj_group_size), PTTS_LNPROJ_G = 4 / 8 / 16 forces one
  int xattn_g = 0;       // utterances per workgroup of xattn_fused_kernel above 8 utterances: 0 = by batch size (xattn_group_size), PTTS_XATTN_G = 8 / 4 / 2 forces one
  int xattn_groups = 1;  // xattn_fused_kernel also at batch 9..256, in groups of utterances (PTTS_NO_XATTN_GROUPS=1: two nodes; measured: 1386 -> 1360 us per
                         // batch-32 step, profiles/r03_experiments.txt)
};

// ---- what ptts_engine_create derives once from ptts_config --------------------------------------------------------------------------------------------
struct StepConfig {
  int use_gemv;     // decode step at batch <= gemv_rows on the row-per-wave GEMV kernels
  int gemv_rows;    // 1 (fp32 parity engine) or GV_MAX_ROWS
  int w8;           // ptts_config::weights_fp8: e4m3 row-major weights for the GEMV step (the MFMA prefill uses the exact bf16 dequantisation)
  int w8_strips;    // weights_fp8 engine whose decode step runs on the MFMA strips: e4m3 strip copies are allocated
  int xfold_ne;     // > 0: static cross-attention folding available (positions per head in the folded layout)
  int use_lns;      // 8 < batch <= 32 decode: LayerNorm statistics carried by the producer GEMM (no rows_prep node)
  int S_self;       // KV splits of the self-attention of a decode step
  int cross_waves;  // waves per cross-attention workgroup of a decode step: one 8-deep batch of row groups per wave covers max_enc
  int xattn_g_ok;   // the g < 8 instances of xattn_fused_kernel exist for this width (Mini-v1, Large-v1)
  int nkv, nkc;     // self / cross K/V heads (== num_heads unless grouped-query attention)
};

constexpr int step_kt(bool bf16) { return bf16 ? 32 : 16; }  // K elements of one MFMA fragment (Elem<WT>::KT; ptts_lm.hip asserts the equality)
inline int step_esize(const ptts_config& c) { return c.dtype == PTTS_BF16 ? 2 : 4; }
// GEMV mode of the weight matrices, and of the folded cross-attention matrices (in the engine dtype, never e4m3)
inline int step_gemv_mode(const ptts_config& c) { return c.dtype == PTTS_F32 ? GV_F32 : (c.weights_fp8 ? GV_BF16_W8 : GV_BF16); }
inline int step_fold_mode(const ptts_config& c) { return c.dtype == PTTS_F32 ? GV_F32 : GV_BF16; }

// (c: validated by ptts_engine_create - positive sizes, head_dim 64, a known dtype)
inline StepConfig step_config(const ptts_config& c) {
  StepConfig s = {};
  const int H = c.hidden_size, F = c.ffn_dim, nh = c.num_heads, gmode = step_fold_mode(c);
  s.nkv = c.num_kv_heads > 0 ? c.num_kv_heads : nh;
  s.nkc = c.num_cross_kv_heads > 0 ? c.num_cross_kv_heads : s.nkv;
  // decode step on the row-per-wave GEMV kernels: shapes whose rows are whole 1 KiB chunks
  // (an engine created for more than GV_MAX_ROWS utterances never takes the GEMV step: it does not hold the row-major copies either -
  // the model-level cache keeps one engine per batch-size class, each with the weight copies its own decode step streams)
  s.use_gemv = ptts_gemv_k_ok(H, gmode) && ptts_gemv_k_ok(F, gmode) && H <= 2048 && c.max_batch <= GV_MAX_ROWS;
  s.gemv_rows = c.dtype == PTTS_F32 ? 1 : GV_MAX_ROWS;
  s.w8 = c.weights_fp8 != 0;
  s.w8_strips = s.w8 && !s.use_gemv;
  // static cross-attention folding: single utterance, sinusoidal positions (RoPE rotates the cross query by position), <= 64
  // description tokens, full cross K/V heads not required (n_rep handled), folded widths must be GEMV shapes
  s.xfold_ne = (s.use_gemv && !c.rope && c.max_enc <= 64 && ptts_gemv_k_ok(nh * 64, gmode)) ? 64 : 0;
  // split-KV factor: enough workgroups to cover the chip at small batch, none needed at large batch
  int sp = 256 / (c.max_batch * nh);
  if (sp < 1) sp = 1;
  if (sp > 8) sp = 8;
  while (sp > 1 && (sp - 1) * 4 * 8 * 8 >= c.max_ctx) --sp;  // do not split below one 8-deep batch of row groups per wave
  if (s.use_gemv) while (sp & (sp - 1)) --sp;                // the GEMV combine prologue is instantiated for 2 / 4 / 8 splits
  s.S_self = sp;
  const int rows_per_wave = (c.dtype == PTTS_BF16 ? 8 : 4) * 8;  // RPI row groups x 8 loads in flight
  const int need = (c.max_enc + rows_per_wave - 1) / rows_per_wave;
  s.cross_waves = need <= 1 ? 1 : (need <= 2 ? 2 : 4);
  s.use_lns = H == 1024 || H == 1536;
  s.xattn_g_ok = (H == 1024 && ((H / step_kt(c.dtype == PTTS_BF16)) / 2) % 16 == 0) || H == 1536;
  return s;
}

// ---- predicates shared by the plans and the test harnesses, each stated once ------------------------------------------------------------------------------
// PRO_LNS (LayerNorm from the producer GEMM's strip statistics): 9..32 rows that all fit in LDS beside the reduction buffer, hidden 1024 / 1536
inline bool pro_lns_fits(int M, int K, size_t esize) {
  return M > 8 && M <= 32 && (size_t)M * ((size_t)K * esize + 16) + 16 * 1024 <= 159 * 1024 && (K == 1024 || K == 1536);
}
// A GEMM behind a LayerNorm or a split-KV combine: the prologue fused into the strip kernel up to 8 rows; above, the producer's statistics where they
// are carried and the rows fit (PRO_LNS); else a rows_prep node + copy staging (the redundant per-workgroup prologue is 88 % of the GEMM at M = 32:
// tools/phase_probe, profiles/)
enum ProGemm { PG_FUSED = 0, PG_LNS = 1, PG_PREP_COPY = 2 };
inline int pro_gemm(int M, int K, size_t esize, bool lnstat) { return M <= 8 ? PG_FUSED : (lnstat && pro_lns_fits(M, K, esize) ? PG_LNS : PG_PREP_COPY); }
inline int pro_gemm_launches(int how) { return how == PG_PREP_COPY ? 2 : 1; }

// lnproj_fused_kernel: Mini / Large widths whose K halves are whole 8-fragment groups, N in 64-row blocks
inline bool lnproj_width_ok(int H, int kt, int N) { return (H == 1024 || H == 1536) && ((H / kt) / 2) % 8 == 0 && N % 64 == 0; }
// utterances per workgroup of that node: 8 (one row per wave) up to 40, 16 (two rows per wave, the whole MFMA tile, half the weight re-reads) above
inline int lnproj_group_size(int M, int forced) { return forced > 0 ? forced : (M <= 40 ? 8 : 16); }

// xattn_fused_kernel: widths with instances; hidden 512 has the 8-utterance instance only, and up to 8 utterances run one per wave
inline bool xattn_width_ok(int H, int kt) { return (H / kt) % 16 == 0 && (H == 512 || H == 1024 || H == 1536); }
inline bool xattn_group_ok(int H, int gsz, int B) { return (gsz == 8 || gsz == 4 || gsz == 2) && (H != 512 || gsz == 8) && (B > 8 || gsz == 8); }
// utterances per workgroup: 8 (one per wave) up to 8 utterances; above, 8 / 4 / 2: heads x ceil(M / g) workgroups, the 8 / g waves of an utterance
// split the description's row groups. Measured (profiles/r04_experiments.txt, us per step at mid context, g = 8 / 4 / 2): batch 32 1432 / 1381 / 1360,
// batch 128 2596 / 2682 / 2860 -> 2 up to 32 utterances, 4 up to 64, 8 above
inline int xattn_group_size(int M, int forced, bool g_ok) { return (M <= 8 || !g_ok) ? 8 : (forced ? forced : (M <= 32 ? 2 : (M <= 64 ? 4 : 8))); }

// KV splits qkv_attn_kernel may run: the combine prologue of the out_proj node holds S + 1 slots per lane - 12-wave workgroups (5..8 utterances) fit 2
inline int qkvattn_split_cap(int M) { return M == 1 ? 8 : (M <= 4 ? 4 : 2); }

// ---- the GEMV step: 1..gemv_rows utterances ------------------------------------------------------------------------------------------------------------
inline bool step_on_gemv(const StepConfig& s, bool prefill, int B) { return s.use_gemv && !prefill && B <= s.gemv_rows; }

struct GemvNode { int on, pro, epi, S, N, K, mode; };  // one ptts_gemv_launch call (M: the plan's)
enum GemvCross { XFOLD_ONE_NODE = 0, XFOLD_TWO_NODES = 1, XQ_FUSED = 2, PLAIN = 3 };

struct GemvPlan {
  int M, mode, fold_mode;
  int fuse_qa, S_f;   // self-attention block's first half as one node (qkv_attn_kernel) on S_f KV splits; else LN1 + QKV, then attention on S_self splits
  int S_self;
  int cross;          // GemvCross
  int x_fused;        // the cross block left its output as per-head partial rows (XFOLD_ONE_NODE): summed by the LN3 + fc1 node (GV_LNP)
  int fuse_x_nur, cross_waves, xfold_ne;
  GemvNode qkv, out_proj, xscores, xsoftmax, cq, co, fc1, fc2, heads;

  const GemvNode* layer_nodes(int i) const {
    const GemvNode* n[8] = {&qkv, &out_proj, &xscores, &xsoftmax, &cq, &co, &fc1, &fc2};
    return i < 8 ? n[i] : nullptr;
  }
  // kernel launches of one layer: its gemv_kernel nodes + the attention nodes (qkv_attn / attention, xfold_attn / xq_attn / attention)
  int launches() const {
    int n = 1 + (cross == XFOLD_TWO_NODES ? 0 : 1);
    for (int i = 0; i < 8; ++i) n += layer_nodes(i)->on;
    return n;
  }
  int head_launches() const { return 1; }
};

inline GemvPlan gemv_plan(const StepConfig& s, const ptts_config& c, const StepSwitches& sw, int M, int kv_bound, bool xfold_valid) {
  const int H = c.hidden_size, F = c.ffn_dim, nh = c.num_heads, QKV = H + 2 * s.nkv * 64;
  GemvPlan p = {};
  p.M = M; p.mode = step_gemv_mode(c); p.fold_mode = step_fold_mode(c);
  p.S_self = s.S_self; p.fuse_x_nur = sw.fuse_x_nur; p.cross_waves = s.cross_waves; p.xfold_ne = s.xfold_ne;
  auto node = [](int pro, int epi, int S, int N, int K, int mode) { return GemvNode{1, pro, epi, S, N, K, mode}; };
  // single utterance, sinusoidal positions: the two nodes of the self-attention block's first half as one (PTTS_NO_FUSE_QA=1: two nodes)
  // (round 5: 2..8 utterances too - one grid slice per utterance, the slices of a head share its weight rows in the L2; PTTS_FUSE_QA_MAX=1: one only)
  // measured, Mini-v1 us per step at contexts ~210 / ~460 / ~710, fused | two nodes (profiles/r05_experiments.txt call 2): 2 utterances 720 / 756 / 791 |
  // 769 / 777 / 791; 3: 741 / 788 / 862 | 780 / 796 / 821; 4: 777 / 864 / 923 | 803 / 832 / 862; 8: 966 / 1010 / 1068 | 907 / 965 / 1023 (the slices of
  // a head re-read its q / k / v rows from the L2 once per utterance and split): on up to fuse_qa_max utterances (3), PTTS_FUSE_QA_MAX forces a bound
  p.fuse_qa = sw.fuse_qa && (M == 1 || (M <= sw.fuse_qa_max && p.mode != GV_F32)) && !c.rope && ptts_qkvattn_ok(H, p.mode);
  // KV splits of the fused node: the smallest count whose FIRST batch of row groups (8 waves x 4 groups x 8 bf16 / 4 fp32 rows per split,
  // requested before q exists) covers the context bucket this graph is captured for - fewer workgroups recompute the head's q rows, and no
  // split needs a second, dependent K/V batch (context ~210 / ~460 / ~710: 2 splits 554 / 562 / 586 us per step, 4 splits 575 / 577 / 579,
  // 8 splits 645 / 646 / 648; profiles/r04_experiments.txt call 15)
  p.S_f = 1;
  while (p.S_f < qkvattn_split_cap(M) && p.S_f * ptts_qkvattn_rows_per_split(p.mode) < kv_bound) p.S_f *= 2;
  if (p.fuse_qa) {
    p.out_proj = node(GV_ATTN2, GV_RESID, p.S_f, H, H, p.mode);
  } else {
    p.qkv = node(GV_LN, GV_STORE, 1, QKV, H, p.mode);
    p.out_proj = s.S_self == 1 ? node(GV_COPY, GV_RESID, 1, H, H, p.mode) : node(GV_ATTN, GV_RESID, s.S_self, H, H, p.mode);
  }
  const bool folded = xfold_valid && M == 1 && s.xfold_ne > 0;
  if (folded && (sw.fuse_x < 0 ? H <= 1024 : sw.fuse_x != 0) && s.xfold_ne == 64 && ptts_xfoldattn_ok(H, nh, p.fold_mode)) p.cross = XFOLD_ONE_NODE;
  else if (folded) p.cross = XFOLD_TWO_NODES;
  else if (sw.fuse_xq && !c.rope && ptts_xqattn_ok(H, p.mode)) p.cross = XQ_FUSED;
  else p.cross = PLAIN;
  p.x_fused = p.cross == XFOLD_ONE_NODE;
  if (p.cross == XFOLD_TWO_NODES) {  // LN2 + (K Wq) x -> base-2 scores; per-head softmax + (Wo V^T) p + residual
    p.xscores = node(GV_LN, GV_STORE, 1, nh * s.xfold_ne, H, p.fold_mode);
    p.xsoftmax = node(GV_SOFTMAX, GV_RESID, 1, H, nh * s.xfold_ne, p.fold_mode);
  }
  if (p.cross == PLAIN) p.cq = node(GV_LN, GV_STORE, 1, H, H, p.mode);
  if (p.cross == XQ_FUSED || p.cross == PLAIN) p.co = node(GV_COPY, GV_RESID, 1, H, H, p.mode);
  p.fc1 = node(p.x_fused ? GV_LNP : GV_LN, GV_GELU_WT, 1, F, H, p.mode);
  p.fc2 = node(GV_COPY, GV_RESID, 1, H, F, p.mode);
  p.heads = node(GV_LN, GV_STORE, 1, c.num_codebooks * c.vocab_size, H, p.mode);
  return p;
}

// ---- the MFMA strip path: every prefill (Q positions per utterance), and the decode step above gemv_rows utterances ----------------------------------------
enum StripQkv { QKV_LNPROJ = 0, QKV_LNPROJ_KV = 1, QKV_GEMM = 2, QKV_GEMM_KV = 3 };  // _KV: the node's epilogue writes the self K/V cache rows itself
enum StripKvAppend { KVA_NONE = 0, KVA_ENGINE = 1, KVA_E4M3 = 2 };                    // the kv_append node and its instance
enum StripAttn { ATTN_ROWS = 0, ATTN_PREFILL = 1 };                                    // launch_attn | launch_prefill_attn(prefill_attn_mode)
enum StripOutProj { OUT_COPY = 0, OUT_COMBINE_FUSED = 1, OUT_COMBINE_PREP = 2 };
enum StripCross { CROSS_XATTN_FUSED = 0, CROSS_LNPROJ_ATTN = 1, CROSS_GEMM_ATTN = 2 };
enum StripFc { FC_SMALL = 0, FC_LNPROJ = 1, FC_GEMM = 2 };  // SMALL: up to 8 rows, fp32 GELU rows between fc1 and fc2; else engine-dtype rows

struct StripPlan {
  int prefill, B, Q, M;  // M = B * Q rows
  int dec;               // GemmArgs::decode: rows per M pass of the strip GEMMs (msplit_rows)
  int S_used, lns, fo, lnproj_g, prefill_attn_mode, cross_waves;
  int qkv, qkv_how;      // StripQkv; ProGemm of the LayerNorm GEMM
  int kv_append;         // StripKvAppend
  int attn;              // StripAttn, of the self- and the cross-attention node
  int out_proj;          // StripOutProj
  int cross, xattn_g, cq_how;  // StripCross; utterances per workgroup of xattn_fused_kernel; ProGemm of the LN2 + cross-q GEMM
  int fc, fc1_how;       // StripFc; ProGemm of the LN3 + fc1 GEMM
  int heads_x_fo, heads_how;

  int launches() const {  // kernel launches of one layer
    const int qkv_n = (qkv == QKV_GEMM || qkv == QKV_GEMM_KV) ? pro_gemm_launches(qkv_how) : 1;
    const int cross_n = cross == CROSS_XATTN_FUSED ? 1 : (cross == CROSS_LNPROJ_ATTN ? 2 : pro_gemm_launches(cq_how) + 1);
    const int fc_n = (fc == FC_GEMM ? pro_gemm_launches(fc1_how) : 1) + 1;
    return qkv_n + (kv_append != KVA_NONE) + 1 + (out_proj == OUT_COMBINE_PREP ? 2 : 1) + cross_n + 1 + fc_n;
  }
  int head_launches() const { return pro_gemm_launches(heads_how); }
};

inline StripPlan strip_plan(const StepConfig& s, const ptts_config& c, const StepSwitches& sw, bool prefill, int B, int Q, int prefill_attn_mode) {
  const int H = c.hidden_size, F = c.ffn_dim, QKV = H + 2 * s.nkv * 64, M = B * Q, kt = step_kt(c.dtype == PTTS_BF16);
  const size_t es = (size_t)step_esize(c);
  StripPlan p = {};
  p.prefill = prefill; p.B = B; p.Q = Q; p.M = M; p.dec = prefill ? 0 : 1; p.prefill_attn_mode = prefill_attn_mode;
  // KV splits of the self-attention: the engine's split factor at decode (long context, few rows); ONE at prefill - the context is the
  // prompt (tens of positions) and there is one workgroup per (head, position) anyway: splitting 4 ways + a combine kernel cost
  // 15 + 9 us per layer on the time-to-first-token path against ~7 us unsplit (profiles/r03_prefill_kernels.txt)
  p.S_used = prefill ? 1 : s.S_self;
  p.lns = s.use_lns && !prefill && M > 8 && M <= 32;  // LayerNorm statistics carried by the producer GEMM (PRO_LNS)
  // decode at batch > 8: engine-dtype activations travel between kernels in MFMA B-fragment order (ptts_lm_kernels.h: fo_vec_index)
  // (and the prefill while its rows stay on the strip kernels, M <= 256: a single utterance's 33-position prefill is 240 latency-bound
  // launches on the time-to-first-token path)
  p.fo = (M > 8 && (!prefill || M <= 256)) ? 1 : 0;
  // LayerNorm + projection as one node (lnproj_fused_kernel): decode, batch > 8, Mini / Large widths, weights in the engine dtype (e4m3 strips keep
  // streaming bytes through the strip GEMMs)
  // (round 5: the prefill rows of a short prompt, 8 < M <= 40, run the same fused nodes - three rows_prep nodes less per layer on the
  //  time-to-first-token path: prefill 1.41 -> 1.29 ms, first token 2.41 -> 2.28 ms at 33 rows, profiles/r05_experiments.txt call 2)
  const bool lnproj_ok = sw.lnproj > 0 && (!prefill || M <= 40) && M > 8 && !s.w8_strips && lnproj_width_ok(H, kt, QKV) && lnproj_width_ok(H, kt, F);
  p.lnproj_g = lnproj_group_size(M, sw.lnproj_g);
  // prefill rows on the fused LN1 + QKV node, sinusoidal positions, engine-dtype cache: the node's epilogue writes the cache rows itself (no
  // kv_append node: 24 launches of ~4 us + their boundaries off the time-to-first-token path)
  const bool kv_in_qkv = prefill && lnproj_ok && !c.rope && !c.kv_fp8;
  // ... and above 256 rows (a batch's prompts on the > 256-row GEMMs; round 6): the QKV projection's tile epilogue writes them (GemmArgs::kv_col0) -
  // 24 kv_append launches of ~6 us + their boundaries off the time-to-first-token path of a batch. Between 41 and 256 rows the kv_append node stays
  // (fragment-order rows_prep + strips: measured path of round 5).
  const bool kv_in_gemm = prefill && !kv_in_qkv && !lnproj_ok && M > 256 && !c.rope && !c.kv_fp8;
  p.qkv = lnproj_ok ? (kv_in_qkv ? QKV_LNPROJ_KV : QKV_LNPROJ) : (kv_in_gemm ? QKV_GEMM_KV : QKV_GEMM);
  p.qkv_how = pro_gemm(M, H, es, false);
  p.kv_append = (prefill && !kv_in_qkv && !kv_in_gemm) ? (c.kv_fp8 ? KVA_E4M3 : KVA_ENGINE) : KVA_NONE;
  // prefill attention on the tiled kernels (8 query rows per workgroup share the K / V tile; PTTS_PREFILL_ATTN=0: one workgroup per query row, attn_kernel)
  p.attn = (prefill && prefill_attn_mode != 0) ? ATTN_PREFILL : ATTN_ROWS;
  p.cross_waves = prefill ? 4 : s.cross_waves;  // decode: as few waves as cover the description (no LDS combine at 1)
  p.out_proj = p.S_used == 1 ? OUT_COPY : (pro_gemm(M, H, es, false) == PG_FUSED ? OUT_COMBINE_FUSED : OUT_COMBINE_PREP);
  // decode: LN2 + cross q projection + cross-attention fused, one workgroup per (head, group of utterances)
  if (!prefill && (M <= 8 || (sw.xattn_groups && M <= 256)) && xattn_width_ok(H, kt)) p.cross = CROSS_XATTN_FUSED;
  else if (prefill && lnproj_ok) p.cross = CROSS_LNPROJ_ATTN;
  else p.cross = CROSS_GEMM_ATTN;
  p.xattn_g = xattn_group_size(M, sw.xattn_g, s.xattn_g_ok != 0);
  p.cq_how = pro_gemm(M, H, es, p.lns != 0);
  p.fc = M <= 8 ? FC_SMALL : ((lnproj_ok && (sw.lnproj >= 3 || (sw.lnproj == 2 && M > 32))) ? FC_LNPROJ : FC_GEMM);
  p.fc1_how = pro_gemm(M, H, es, p.lns != 0);
  // (the final LayerNorm + LM heads as one lnproj_fused_kernel node at 9..40 utterances measured neutral to +0.6 %: the 20 MB of head weights are
  //  re-read once per group of 8 utterances - profiles/r04_experiments.txt call 23; the rows_prep + strip GEMM pair stays)
  p.heads_x_fo = (B > 8 && (!prefill || B <= 256)) ? 1 : 0;
  p.heads_how = pro_gemm(B, H, es, false);
  return p;
}
