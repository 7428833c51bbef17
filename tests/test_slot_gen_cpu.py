"""CPU: per-request sampler records - the new harness (tests/native/slot_gen_harness.hip) cross-compiles for gfx950 without a GPU and exports
exactly its entry points; ptts_admit_row_gen is declared, bound and exported under ABI version 8; and the inputs of the GPU cases
(tests/slot_gen_cases.py) keep the ambiguous draws under the cap on the host model alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sampler_cases as SC
import slot_gen_cases as GC
import slot_gen_harness as SG
import tail_harness as TH
from parler_tts_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return SG.Harness(SG.build(str(tmp_path_factory.mktemp("slot_gen_harness"))))


def test_harness_cross_compiles_and_exports_its_entry_points(harness):
    for n in SG.ENTRY_POINTS:
        assert hasattr(harness.lib, n), n
    # every other symbol stays hidden: the harness's own copy of ptts_fail cannot interpose on the product library's
    out = subprocess.run(["nm", "-D", "--defined-only", harness.lib._name], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert exported == set(SG.ENTRY_POINTS), exported ^ set(SG.ENTRY_POINTS)
    assert C.sizeof(SG.SlotGen) == 48 and C.sizeof(TH.DevGen) == 40  # DevGen's layout did not move; a record is one 48-byte load


def test_admit_row_gen_is_declared_bound_and_exported_under_abi_8():
    hdr = open(os.path.join(ROOT, "include", "ptts.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"#define\s+PTTS_ABI_VERSION\s+8\b", hdr) and _native.ABI_VERSION == 8  # additive: the version does not move
    decl = {n: re.search(r"\bint\s+" + n + r"\s*\(([^)]*)\)\s*;", code) for n in ("ptts_admit_row", "ptts_admit_row_gen")}
    assert decl["ptts_admit_row_gen"], "ptts_admit_row_gen is not declared in include/ptts.h"
    params = {n: [" ".join(p.split()[:-1]) for p in m.group(1).split(",")] for n, m in decl.items()}
    # ptts_admit_row plus the request's parameters, in front of the stream
    assert params["ptts_admit_row_gen"] == params["ptts_admit_row"][:-1] + ["const ptts_gen_params*"] + params["ptts_admit_row"][-1:]
    assert "ptts_admit_row_gen" in _native.SYMBOLS
    (res, args), (res0, args0) = _native.SYMBOLS["ptts_admit_row_gen"], _native.SYMBOLS["ptts_admit_row"]
    assert res is C.c_int and res0 is C.c_int
    assert args == args0[:-1] + [C.POINTER(_native.PttsGenParams)] + args0[-1:]  # one pointer more
    assert len(re.findall(r"^\s*(?:const\s+char\s*\*|int32_t|int|void)\s+ptts_\w+\s*\(", code, flags=re.M)) == len(_native.SYMBOLS) == 46
    src = open(os.path.join(ROOT, "parler_tts_amd", "csrc", "ptts_lm.hip")).read()
    assert re.search(r'extern "C" int ptts_admit_row_gen\(', src)

    import __graft_entry__

    __graft_entry__.build()  # incremental; cross-compiles without a GPU
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {"ptts_admit_row", "ptts_admit_row_gen"} <= exported
    assert _native.load_library().ptts_abi_version() == 8


@pytest.mark.parametrize("V,K", GC.SHAPES)
def test_the_model_alone_stays_under_the_ambiguous_cap_on_the_mixed_case(V, K):
    """The inputs of tests/test_slot_gen_tail_gpu.py::test_mixed_slots_in_one_launch are chosen on the reference: its draws (the same ones the
    device makes: they follow from the seeds, the columns and the scripted logits) are ambiguous in at most 4 % of the cases."""
    m = GC.run_mixed_on_the_model(V, K)
    st = m.stats
    assert st["draws"] >= 30 * K and st["ambiguous"] / st["draws"] <= SC.AMBIGUOUS_CAP, st
    GC.assert_slot4_waits_for_its_own_bound(m, K, V)
    f = m.full
    assert sorted(m.own) == [0, 1, 2, 4] and [int(f.cur_len[b]) for b in range(4)] == [14, 12, 9, 14] and f.cur_len[4] >= GC.MIN_NEW_4 + 2
    assert (f.unfinished[5 * K:] == 0).all() and f.cur_len[5] == 1  # the idle slot
    # the records: own = 1 and row_base 0 where a request brought one, all zero elsewhere
    own = np.array([b in m.own for b in range(GC.SLOTS)])
    assert (m.recs[own, 10] == 1).all() and (m.recs[own, 11] == 0).all() and not m.recs[~own].any()


def test_the_models_draws_follow_the_record_not_the_slot():
    """The contract on the model alone: a slot with a record draws from (its seed, t, k) - the same tokens in slot 0 and in slot 4 - and
    a slot without one from (session seed, t, b * K + k), which differ between the two slots."""
    V, K = 64, 4
    ids = {}
    for rec in (True, False):
        for slot, at in ((0, 0), (4, 3)):
            m = GC.SlotSession(GC.SLOTS, K, V, GC.MAXLEN + 3, GC.session_gen(), GC.SESSION_SEED)
            for ev in GC.placement_events(V, K, slot, at, rec):
                if ev[0] == "reset":
                    m.reset(*ev[1:])
                elif ev[0] != "clear":
                    m.step(ev[2], slots=[ev[1]] if ev[0] == "admit" else None, choose=lambda row, acc: min(acc))
            assert m.full.cur_len[slot] == 2 + GC.PLACE_STEPS and (slot in m.own) == rec
            ids[rec, slot] = m.full.ids[slot * K:(slot + 1) * K, :2 + GC.PLACE_STEPS].copy()
    assert np.array_equal(ids[True, 0], ids[True, 4])
    assert not np.array_equal(ids[False, 0], ids[False, 4])
    assert not np.array_equal(ids[True, 0], ids[False, 0])
