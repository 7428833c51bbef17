"""Single-utterance step: the split-KV combine prologue of the out_proj node (GV_ATTN2) on one wave per 256 columns of the row instead of
one wave for the whole row (tests/split3_cases.py: shapes, contexts, inputs). The arithmetic per column did not move, so the step is
bit-identical to the parent commit's.

(The issue this file was written for also proposed a 3-way KV split for buckets 576..768. Measured on top of the combine change it was
neutral - profiles/split3_combine_ab.txt - and is not in the tree; its parity cases went with it.)

Tolerance against the two-node path: 2e-2 on the logits, the bound tests/test_lm_gpu.py (test_fused_qkv_attention_node_*) holds the bf16
fused step to against the two-node step."""
import json
import os

import pytest
import torch

import split3_cases as SC
from conftest import GOLD
from oracle import decoder_oracle as DO

pytestmark = pytest.mark.gpu

TOL = 2e-2


class _Engines:
    """One engine per path ("fused" = the default, "two" = the two-node path: PTTS_NO_FUSE_QA is read when an engine is created)."""

    def __init__(self):
        self.sd, self.eng, self.cache = SC.weights(), {}, {}

    def get(self, key):
        if key not in self.eng:
            mp = pytest.MonkeyPatch()
            try:
                mp.delenv("PTTS_NO_FUSE_QA", raising=False)
                if key == "two":
                    mp.setenv("PTTS_NO_FUSE_QA", "1")
                self.eng[key] = SC.engine(self.sd)
            finally:
                mp.undo()
        return self.eng[key]

    def logits(self, key, P, steps):
        """Computed once per (path, prompt length), shared by the tests and left unchanged."""
        if (key, P, steps) not in self.cache:
            self.cache[(key, P, steps)] = SC.step_logits(self.get(key), P, steps)
        return self.cache[(key, P, steps)]

    def close(self):
        for e in self.eng.values():
            e.close()


@pytest.fixture(scope="module")
def engines():
    e = _Engines()
    yield e
    e.close()


@pytest.mark.parametrize("window", sorted(SC.WINDOWS))
def test_combine_on_slab_waves_is_bit_identical_to_the_one_wave_prologue(window, engines):
    """The logits of 6 teacher-forced steps at contexts straddling a bucket edge (251..256: 1 -> 2 splits; 511..516: 2 -> 4), of 6 steps on
    2 splits and of 2 steps on 8, against the logits the parent commit's library gave for the same inputs
    (tests/golden/split3_combine_parent.json, written by tools/make_split3_combine_golden.py: sha256 of the fp32 logits of each step).
    Exact equality: the combine's arithmetic per column did not move, only the wave that holds the column."""
    P, steps, splits = SC.WINDOWS[window]
    gold = json.load(open(os.path.join(GOLD, "split3_combine_parent.json")))[window]
    assert gold["prompt"] == P and gold["splits"] == splits and len(gold["sha256"]) == steps
    got = [SC.digest(x) for x in engines.logits("fused", P, steps)]
    assert got == gold["sha256"], [i for i, (a, b) in enumerate(zip(got, gold["sha256"])) if a != b]


@pytest.mark.parametrize("window", sorted(SC.WINDOWS))
def test_fused_step_matches_the_two_node_path(window, engines):
    """The same windows against the two-node path (PTTS_NO_FUSE_QA=1), whose combine (gv_attn_wave) did not change."""
    P, steps, _ = SC.WINDOWS[window]
    a, b = engines.logits("fused", P, steps), engines.logits("two", P, steps)
    d = max(float((x - y).abs().max()) for x, y in zip(a, b))
    print(f"{window}: max |logits(fused) - logits(two nodes)| = {d:.3e}")
    assert d < TOL and all(torch.isfinite(x).all() for x in a), (window, d)


def test_greedy_ids_across_the_two_to_four_split_edge_match_the_two_node_path(engines):
    """40 free-running greedy steps through the captured step graphs from context 500 to 540 (2 splits up to 511, 4 from 512: one graph per
    64-position bucket, each captured with the count of its bucket) against the two-node path's ids. Input seed chosen on the CPU oracle
    (bf16 precision): the min top-2 margin of the run is checked here, far above a last-bit difference between the two paths."""
    enc, prompt, _ = SC.inputs(499, seed=SC.GREEDY_SEED)
    ref = DO.sample_loop(DO.DecoderOracle(SC.spec(), engines.sd, precision="bf16"), enc, None, prompt, None, DO.GenParams(max_length=42, min_new_tokens=41))
    assert ref.min_margin >= SC.GREEDY_MARGIN, ref.min_margin
    ids = {}
    for key in ("fused", "two"):
        eng = engines.get(key)
        eng.set_gen_params(max_length=42, min_new_tokens=41)
        eng.prefill(enc, None, prompt, None, sample=True)
        eng.decode_steps(40)
        ids[key] = eng.ids().cpu()
    assert ids["fused"].shape == (9, 42)
    assert torch.equal(ids["fused"], ids["two"]), (ids["fused"] != ids["two"]).nonzero()[:4]
