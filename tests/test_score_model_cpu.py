"""CPU: the teacher-forced forward above the kernel. tests/score_model.py (float64 counting rule + reductions) pinned against the reference's own
``forward`` - live where the reference tree is importable, and against tests/golden/score_ref.npz (tools/make_score_golden.py) everywhere; the
oracle's all-position logits against the fixture's; ``ptts_score.h`` against its ctypes binding, the built library and a torch-free C client;
``ParlerTTSForConditionalGeneration.forward`` on an oracle-backed engine stand-in (the pattern of tests/test_generate_glue_cpu.py)."""
import ctypes
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import parler_tts_amd as P
import score_model as SM
from oracle import decoder_oracle as DO
from oracle.reference_shims import reference_available
from parler_tts_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_score_golden as MSG  # noqa: E402

HEADER = os.path.join(ROOT, "include", "ptts_score.h")
SPEC = MSG.SPEC
RUNS = {"weighted_mean": (MSG.CODEBOOK_WEIGHTS, "mean"), "sum": (None, "sum")}


@pytest.fixture(scope="module")
def gold():
    g = np.load(os.path.join(ROOT, "tests", "golden", "score_ref.npz"))
    return {k: torch.from_numpy(np.array(g[k])) for k in g.files}


# ---- the restatement against the reference ------------------------------------------------------------------------------------------------
def test_fixture_inputs_are_the_tools_and_hold_the_cases(gold):
    enc, enc_mask, prompt, prompt_mask, ids, labels = MSG.inputs()
    for k, v in dict(enc=enc, enc_mask=enc_mask, prompt=prompt, prompt_mask=prompt_mask, input_ids=ids, labels=labels).items():
        assert torch.equal(gold[k], v), k
    cm = SM.counted_mask(ids, labels, SPEC.bos_token_id, SPEC.eos_token_id)
    assert int((labels == SPEC.bos_token_id).sum()) == 1 and not bool(cm[labels == SPEC.bos_token_id].any())
    inp = ids.view(2, 9, -1).transpose(1, 2)
    assert bool(((inp == SPEC.eos_token_id) & (labels != -100)).any()), "an input EOS under a real label"
    assert len({int((labels[b, :, k] == -100).sum()) for b in range(2) for k in range(9)}) > 3, "tails of different lengths"
    assert int(enc_mask.sum()) < enc_mask.numel() and int(prompt_mask.sum()) < prompt_mask.numel()


@pytest.mark.parametrize("run", list(RUNS))
def test_score_model_gives_the_references_loss_on_the_references_logits(gold, run):
    weights, red = RUNS[run]
    loss, per = SM.loss_from_logits(gold[f"{run}__logits"], gold["input_ids"], gold["labels"], SPEC.bos_token_id, SPEC.eos_token_id, red, weights)
    # the reference reduces in fp32: a few ulps of a sum of <= 18 terms of size <= 8
    tol = 1e-5 if red == "mean" else 1e-4
    assert (per - gold[f"{run}__per_codebook_losses"].double()).abs().max() <= tol
    assert abs(float(loss) - float(gold[f"{run}__loss"])) <= tol


@pytest.mark.skipif(not reference_available(), reason="the reference tree is not importable here: the fixture carries its results")
def test_fixture_is_what_the_reference_computes_live(gold):
    live = MSG.reference_results()
    # the reference computes in fp32 and its summation order follows the machine's thread count: 1e-6 on logits of O(0.3), and a few fp32 ulps
    # (2^-23 = 1.2e-7 each) of the losses, which reach 70 as sums
    for k, v in live.items():
        assert np.allclose(gold[k].numpy(), v, rtol=2e-6, atol=1e-6), k


def test_empty_codebook_nan_for_mean_zero_for_sum_and_bad_reduction():
    g = torch.Generator().manual_seed(1)
    logits, ids = torch.randn(4, 5, 16, generator=g), torch.randint(0, 8, (4, 5), generator=g)
    labels = torch.randint(0, 8, (2, 5, 2), generator=g)
    labels[:, :, 1] = -100
    loss, per = SM.loss_from_logits(logits, ids, labels, 9, 10, "mean")
    assert math.isnan(float(per[1])) and math.isnan(float(loss)) and not math.isnan(float(per[0]))
    want = torch.nn.functional.cross_entropy(logits.view(2, 2, 5, 16)[:, 0].reshape(-1, 16).double(), labels[..., 0].reshape(-1), reduction="mean")
    assert abs(float(per[0]) - float(want)) < 1e-12
    loss, per = SM.loss_from_logits(logits, ids, labels, 9, 10, "sum")
    assert float(per[1]) == 0.0 and abs(float(loss) - float(per[0]) / 2) < 1e-12
    with pytest.raises(ValueError):
        SM.reduce_loss(torch.zeros(1, 1, 1), torch.ones(1, 1, 1, dtype=torch.bool), "none")


def test_oracle_logits_at_all_positions_match_the_fixture(gold):
    sd = DO.make_decoder_weights(SPEC, seed=int(gold["weight_seed"]))
    got = DO.DecoderOracle(SPEC, sd).forward(gold["input_ids"], gold["enc"], gold["enc_mask"], gold["prompt"], gold["prompt_mask"])
    real = torch.ones(got.shape[:2], dtype=torch.bool)  # padded-prompt query rows are not compared (oracle/make_golden.py::gen_decoder)
    real[:, :gold["prompt"].shape[1]] = gold["prompt_mask"].bool().repeat_interleave(SPEC.num_codebooks, 0)
    assert float((got - gold["sum__logits"])[real].abs().max()) < 2e-6


# ---- header and bindings -------------------------------------------------------------------------------------------------------------------
def test_header_structure_and_prototype_agree_with_the_binding_and_ptts_h_keeps_its_46():
    hdr = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r'^#include "ptts.h"', hdr, flags=re.M)
    assert sorted(set(re.findall(r"\b(ptts_\w+)\s*\(", code))) == ["ptts_score"] == sorted(_native.SCORE_SYMBOLS)
    assert "ptts_score" not in _native.SYMBOLS and len(_native.SYMBOLS) == 46 and _native.ABI_VERSION == 8
    C = _native.C
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*ptts_score_io\s*;", code)
    fields = [f.split()[-1].lstrip("*") for f in m.group(1).split(";") if f.strip()]
    assert fields == ["input_ids", "labels", "nll", "counted", "logits"] == [n for n, _ in _native.PttsScoreIO._fields_]
    assert all(t is C.c_void_p for _, t in _native.PttsScoreIO._fields_) and ctypes.sizeof(_native.PttsScoreIO) == 5 * ctypes.sizeof(C.c_void_p)
    m = re.search(r"\bint\s+ptts_score\s*\(([^)]*)\)\s*;", code)
    params = [" ".join(p.split()[:-1]).replace(" *", "*") for p in m.group(1).split(",")]
    ctype_of = {"ptts_engine*": C.c_void_p, "void*": C.c_void_p, "int32_t": C.c_int32, "const float*": C.c_void_p, "const int32_t*": C.c_void_p,
                "const ptts_score_io*": C.POINTER(_native.PttsScoreIO)}
    res, args = _native.SCORE_SYMBOLS["ptts_score"]
    assert res is C.c_int and [ctype_of[p] for p in params] == list(args), params
    base = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptts.h")).read(), flags=re.S)
    assert len(set(re.findall(r"\b(ptts_\w+)\s*\(", base))) == 46 and "ptts_score" not in base
    assert '"ptts_score.h"' in open(os.path.join(ROOT, "__graft_entry__.py")).read()  # a change to it rebuilds the library
    assert re.search(r'extern "C" int ptts_score\(', open(os.path.join(ROOT, "parler_tts_amd", "csrc", "ptts_lm.hip")).read())


def _built_library():
    import __graft_entry__

    __graft_entry__.build()  # incremental; cross-compiles without a GPU
    return _native.load_library()


def test_library_exports_ptts_score_and_a_null_engine_is_a_value_error():
    lib = _built_library()
    assert lib.ptts_score.restype is ctypes.c_int and list(lib.ptts_score.argtypes) == _native.SCORE_SYMBOLS["ptts_score"][1]
    io = _native.PttsScoreIO()
    with pytest.raises(ValueError, match="null argument"):
        _native.check(lib.ptts_score(None, None, None, None, None, 1, 1, 0, 1, ctypes.byref(io), None), "ptts_score")


def test_torch_free_c_client_of_the_header_builds_links_and_is_refused_with_a_message(tmp_path):
    gcc, gxx = shutil.which("gcc"), shutil.which("g++")
    if gcc is None or gxx is None:
        pytest.skip("no host compiler")
    _built_library()
    inc = os.path.join(ROOT, "include")
    subprocess.check_call([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER])
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", HEADER])
    src = tmp_path / "client.c"
    src.write_text('#include <stdio.h>\n#include "ptts.h"\n#include "ptts_score.h"\n'
                   "int main(void) {\n"
                   "  ptts_score_io io = {NULL, NULL, NULL, NULL, NULL};\n"
                   "  int a = ptts_score(NULL, NULL, NULL, NULL, NULL, 1, 1, 0, 1, &io, NULL);\n"
                   '  printf("%d %d %s\\n", a != PTTS_OK, (int)(sizeof(io) / sizeof(void*)), ptts_last_error());\n'
                   "  return 0;\n}\n")
    exe = str(tmp_path / "client")
    libdir = os.path.dirname(_native.LIB_PATH)
    torch_lib = os.path.join(os.path.dirname(torch.__file__), "lib")
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", inc, str(src), "-o", exe, "-L" + libdir, "-lptts_hip", "-Wl,-rpath," + libdir,
                        "-Wl,-rpath-link," + torch_lib], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.startswith("1 5 ") and "null argument" in out.stdout, (out.returncode, out.stdout, out.stderr[-500:])


# ---- model.forward on an oracle-backed engine ---------------------------------------------------------------------------------------------
class ScoreEngine:
    """``DecoderEngine.score`` on the oracle: fp32 logits at all positions, fp32 per-token values - what the HIP engine hands back."""

    def __init__(self, spec, sd):
        self.spec, self.sd, self.calls = spec, sd, []

    def score(self, enc, enc_mask, prompt, prompt_mask, input_ids, labels=None, return_logits=False):
        self.calls.append(dict(B=enc.shape[0], N=enc.shape[1], P=0 if prompt is None else prompt.shape[1], T=input_ids.shape[-1], logits=return_logits))
        s = self.spec
        logits = DO.DecoderOracle(s, self.sd).forward(input_ids.reshape(-1, input_ids.shape[-1]), enc, enc_mask, prompt, prompt_mask)
        nll = counted = None
        if labels is not None:
            cm = SM.counted_mask(input_ids, labels, s.bos_token_id, s.eos_token_id, s.vocab_size)
            nll, counted = SM.token_nll(logits, labels, cm)[0].float(), cm.int()
        return nll, counted, logits if return_logits else None


def _model(prompt_cross_attention=False, codebook_weights=None):
    from transformers import T5Config

    torch.manual_seed(0)
    s = SPEC
    t5 = T5Config(vocab_size=128, d_model=128, d_kv=32, d_ff=256, num_layers=2, num_heads=4, feed_forward_proj="gated-gelu")
    dec = P.ParlerTTSDecoderConfig(vocab_size=s.vocab_size, max_position_embeddings=s.max_position_embeddings, num_hidden_layers=2, ffn_dim=256,
                                   num_attention_heads=2, hidden_size=128, num_codebooks=9, pad_token_id=s.pad_token_id, eos_token_id=s.eos_token_id,
                                   bos_token_id=s.bos_token_id, codebook_weights=codebook_weights)
    cfg = P.ParlerTTSConfig.from_sub_models_config(t5, P.DACConfig(latent_dim=64, decoder_dim=256, decoder_rates=[4, 2, 2, 2]), dec, vocab_size=128,
                                                   prompt_cross_attention=prompt_cross_attention)
    m = P.ParlerTTSForConditionalGeneration(cfg)
    sd = DO.make_decoder_weights(s, seed=MSG.WEIGHT_SEED)
    m.decoder.load_state_dict(sd, strict=False)
    eng = ScoreEngine(s, sd)
    m._get_engine = lambda B, N, Pp, L, T=0: eng
    return m, eng


def _fixture_call(gold, **kw):
    return dict(encoder_outputs=(gold["enc"],), attention_mask=gold["enc_mask"], prompt_hidden_states=gold["prompt"],
                prompt_attention_mask=gold["prompt_mask"], **kw)


@pytest.mark.parametrize("run", list(RUNS))
def test_forward_reproduces_the_fixture(gold, run):
    weights, red = RUNS[run]
    m, eng = _model(codebook_weights=weights)
    out = m(**_fixture_call(gold, decoder_input_ids=gold["input_ids"], labels=gold["labels"], loss_reduction=red))
    assert isinstance(out, P.modeling_parler_tts.ParlerTTSSeq2SeqLMOutput)
    tol = 1e-5 if red == "mean" else 1e-4
    assert abs(float(out.loss) - float(gold[f"{run}__loss"])) <= tol
    assert (torch.stack(out.per_codebook_losses) - gold[f"{run}__per_codebook_losses"]).abs().max() <= tol
    assert tuple(out.logits.shape) == tuple(gold[f"{run}__logits"].shape) and out.logits.dtype == torch.float32
    assert torch.equal(out.encoder_last_hidden_state, gold["enc"])
    assert out.past_key_values is None and out.decoder_hidden_states is None and out.cross_attentions is None
    quiet = m(**_fixture_call(gold, decoder_input_ids=gold["input_ids"].view(2, 9, -1), labels=gold["labels"], loss_reduction=red, output_logits=False,
                              use_cache=True))
    assert quiet.logits is None and torch.equal(quiet.loss, out.loss) and eng.calls[-1]["logits"] is False and eng.calls[0]["logits"] is True


def test_forward_from_labels_alone_shifts_them_and_logits_only_without_labels(gold):
    m, eng = _model()
    labels = gold["labels"]
    out = m(**_fixture_call(gold, labels=labels))
    cols = m.prepare_decoder_input_ids_from_labels(labels).reshape(18, -1)
    again = m(**_fixture_call(gold, labels=labels, decoder_input_ids=cols))
    assert torch.equal(out.loss, again.loss) and torch.equal(out.logits, again.logits)
    only = m(**_fixture_call(gold, decoder_input_ids=cols))
    assert only.loss is None and only.per_codebook_losses is None and torch.equal(only.logits, out.logits)
    empty = labels.clone()
    empty[:, :, 3] = -100
    e_mean, e_sum = m(**_fixture_call(gold, labels=empty)), m(**_fixture_call(gold, labels=empty, loss_reduction="sum"))
    assert math.isnan(float(e_mean.per_codebook_losses[3])) and math.isnan(float(e_mean.loss))
    assert float(e_sum.per_codebook_losses[3]) == 0.0 and math.isfinite(float(e_sum.loss))


def test_forward_on_a_prompt_cross_attention_model_joins_the_prompt_to_the_description(gold):
    m, eng = _model(prompt_cross_attention=True)
    g = torch.Generator().manual_seed(2)
    desc, pids = torch.randint(3, 128, (2, 7), generator=g), torch.randint(3, 128, (2, 3), generator=g)
    out = m(input_ids=desc, attention_mask=gold["enc_mask"], prompt_input_ids=pids, prompt_attention_mask=gold["prompt_mask"], labels=gold["labels"])
    assert eng.calls[-1] == dict(B=2, N=10, P=0, T=gold["labels"].shape[1], logits=True)
    enc = m._encode_description(desc, gold["enc_mask"]).float()
    ph = m.embed_prompts(pids).float() + m.embed_positions.weights[:3].float()[None]
    logits = DO.DecoderOracle(SPEC, eng.sd).forward(m.prepare_decoder_input_ids_from_labels(gold["labels"]).reshape(18, -1), torch.cat([enc, ph], 1),
                                                    torch.cat([gold["enc_mask"], gold["prompt_mask"]], 1), None, None)
    loss, _ = SM.loss_from_logits(logits, m.prepare_decoder_input_ids_from_labels(gold["labels"]).reshape(18, -1), gold["labels"], SPEC.bos_token_id,
                                  SPEC.eos_token_id)
    assert abs(float(out.loss) - float(loss)) < 1e-5


def test_forward_refusals(gold):
    m, _ = _model()
    with pytest.raises(NotImplementedError, match="generate"):
        m()
    with pytest.raises(NotImplementedError, match="generate"):
        m(input_ids=torch.zeros(2, 7, dtype=torch.long))
    ok = _fixture_call(gold, labels=gold["labels"])
    for name in ("decoder_attention_mask", "decoder_position_ids", "decoder_inputs_embeds", "inputs_embeds", "past_key_values", "head_mask",
                 "decoder_head_mask", "cross_attn_head_mask"):
        with pytest.raises(NotImplementedError, match=name):
            m(**ok, **{name: torch.ones(1)})
    with pytest.raises(NotImplementedError, match="return_dict"):
        m(**ok, return_dict=False)
    for name in ("output_attentions", "output_hidden_states"):
        with pytest.raises(NotImplementedError, match="output_"):
            m(**ok, **{name: True})
    with pytest.raises(ValueError, match="loss_reduction"):
        m(**ok, loss_reduction="none")
    with pytest.raises(ValueError):
        m(**_fixture_call(gold, labels=gold["labels"][:, :-1], decoder_input_ids=gold["input_ids"]))
    with pytest.raises(NotImplementedError):
        m.decoder.forward(input_ids=gold["input_ids"])
