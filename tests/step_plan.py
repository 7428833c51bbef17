"""ctypes mirrors of parler_tts_amd/csrc/ptts_step_plan.h for the two harnesses that hand the product's plans to the tests (tests/gemv_harness.py,
tests/step_harness.py): the switches, the derived engine configuration, the strip plan's fields and its enums. The harnesses report sizeof() of
each struct; the loaders compare."""
import ctypes as C

PTTS_F32, PTTS_BF16 = 0, 1


def _ints(*names):
    return [(n, C.c_int) for n in names]


class StepSwitches(C.Structure):
    """struct StepSwitches: the defaults are the header's (tests/gemv_harness.py compares them with gvh_default_switches when it loads the harness)."""
    _fields_ = _ints("fuse_qa", "fuse_qa_max", "fuse_x", "fuse_x_nur", "fuse_xq", "lnproj", "lnproj_g", "xattn_g", "xattn_groups")
    DEFAULTS = dict(fuse_qa=1, fuse_qa_max=3, fuse_x=-1, fuse_x_nur=2, fuse_xq=1, lnproj=3, lnproj_g=0, xattn_g=0, xattn_groups=1)

    def __init__(self, **kw):
        super().__init__(**{**self.DEFAULTS, **kw})


class StepConfig(C.Structure):
    _fields_ = _ints("use_gemv", "gemv_rows", "w8", "w8_strips", "xfold_ne", "use_lns", "S_self", "cross_waves", "xattn_g_ok", "nkv", "nkc")


class StripPlan(C.Structure):
    _fields_ = _ints("prefill", "B", "Q", "M", "dec", "S_used", "lns", "fo", "lnproj_g", "prefill_attn_mode", "cross_waves", "qkv", "qkv_how", "kv_append",
                     "attn", "out_proj", "cross", "xattn_g", "cq_how", "fc", "fc1_how", "heads_x_fo", "heads_how")


PG_FUSED, PG_LNS, PG_PREP_COPY = 0, 1, 2
XFOLD_ONE_NODE, XFOLD_TWO_NODES, XQ_FUSED, PLAIN = 0, 1, 2, 3
QKV_LNPROJ, QKV_LNPROJ_KV, QKV_GEMM, QKV_GEMM_KV = 0, 1, 2, 3
KVA_NONE, KVA_ENGINE, KVA_E4M3 = 0, 1, 2
ATTN_ROWS, ATTN_PREFILL = 0, 1
OUT_COPY, OUT_COMBINE_FUSED, OUT_COMBINE_PREP = 0, 1, 2
CROSS_XATTN_FUSED, CROSS_LNPROJ_ATTN, CROSS_GEMM_ATTN = 0, 1, 2
FC_SMALL, FC_LNPROJ, FC_GEMM = 0, 1, 2


def config(hidden, heads, ffn, bf16=True, layers=2, max_batch=1, max_ctx=64, max_enc=16, max_prompt=5, kv_heads=0, cross_kv_heads=0, rope=False,
           weights_fp8=False, kv_fp8=False, codebooks=9, vocab=1088):
    """A ptts_config (parler_tts_amd._native.PttsConfig) with the decoder spec's codebooks and vocabulary."""
    from parler_tts_amd._native import PttsConfig

    return PttsConfig(hidden_size=hidden, num_layers=layers, num_heads=heads, ffn_dim=ffn, num_codebooks=codebooks, vocab_size=vocab, max_positions=4096,
                      rope=int(rope), rope_theta=10000.0, pad_token_id=1024, eos_token_id=1024, bos_token_id=1025, dtype=PTTS_BF16 if bf16 else PTTS_F32,
                      max_batch=max_batch, max_ctx=max_ctx, max_enc=max_enc, max_prompt=max_prompt, device=0, num_kv_heads=kv_heads,
                      num_cross_kv_heads=cross_kv_heads, weights_fp8=int(weights_fp8), kv_fp8=int(kv_fp8))
