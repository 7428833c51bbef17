"""CPU: the decode-step test harness (tests/native/step_harness.hip) cross-compiles for gfx950 without a GPU, exports exactly its entry points,
agrees with the Python side on its struct layouts, and reaches every lnproj_fused_kernel, xattn_fused_kernel, rows_prep_kernel and e4m3
gemm_strip_kernel instance that the product library contains - an instance added to launch_lnproj, launch_xattn_fused, launch_prep's callers or
ptts_lm_w8.hip without a case fails here. Symbol names only; no instruction is read. The case lists of tests/step_cases.py are chosen at collection
time, before any harness exists, so they keep their Python form; here they are held to the product's own plan of a strip-path forward
(ptts_step_plan.h: strip_plan and its predicates, through the harness's host-only entry points): every list names rows at which the plan picks the
node the list is about."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import step_cases as SC
import step_harness as SH
import step_plan as SP

LLVM = "/opt/rocm/lib/llvm/bin"
# template arguments in the mangled names: t = bf16_t (uint16_t), f = float, Li<n>E an int, Lb<0|1>E a bool
PATTERNS = {
    "lnproj_fused_kernel": r"_Z19lnproj_fused_kernelI([tf])Li(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EE",
    "xattn_fused_kernel": r"_Z18xattn_fused_kernelI([tf])Li(\d+)ELi(\d+)ELi(\d+)EE",
    "rows_prep_kernel": r"_Z16rows_prep_kernelI([tf])Li(\d+)EE",
    "gemm_strip_kernel_w8": r"_Z17gemm_strip_kernelI(t)Li(\d+)ELi(\d+)ELi(\d+)ELb1ELb1EE",
}
AT_LEAST = {"lnproj_fused_kernel": 36, "xattn_fused_kernel": 16, "rows_prep_kernel": 4, "gemm_strip_kernel_w8": 13}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return SH.Harness(SH.build(str(tmp_path_factory.mktemp("step_harness"))))


def _instances_in(lib, tmp_path):
    """{kind: {template arguments}} over the gfx950 code objects of `lib` (the method of test_gemm_harness_cpu.py / test_attn_harness_cpu.py)."""
    assert os.path.exists(os.path.join(LLVM, "llvm-objdump")), "llvm-objdump of the ROCm toolchain is needed to list the library's kernels"
    os.makedirs(str(tmp_path), exist_ok=True)
    shutil.copy(lib, str(tmp_path / "lib.so"))
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", str(tmp_path / "lib.so")], capture_output=True, cwd=str(tmp_path), check=True)
    objs = [str(tmp_path / f) for f in os.listdir(tmp_path) if "amdgcn" in f]
    assert objs, "no embedded gfx950 code objects found"
    found = {k: set() for k in PATTERNS}
    for obj in objs:
        syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--symbols", obj], capture_output=True, text=True, check=True).stdout
        for name, pat in PATTERNS.items():
            for m in re.finditer(pat, syms):
                args = tuple(int(x) for x in m.groups()[1:])
                found[name].add(args if name == "gemm_strip_kernel_w8" else (int(m.group(1) == "t"),) + args)
    # rows_prep_kernel<WT, PRO_RMS> is the T5 description encoder's (ptts_t5.hip; tests/test_t5_gpu.py), not a node of the decode step
    found["rows_prep_kernel"] = {t for t in found["rows_prep_kernel"] if t[1] != SH.PRO_RMS}
    return found


def test_harness_cross_compiles_and_exports_its_entry_points(harness):
    names = SH.entry_points()
    for n in names:
        assert hasattr(harness.lib, n), n
    # every other symbol stays hidden: the harness's own copies of ptts_fail and ptts_strip_w8_launch cannot interpose on the product library's
    out = subprocess.run(["nm", "-D", "--defined-only", harness.lib._name], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert exported == names, exported ^ names
    assert len(SH.parts()) == 2 + 2 * (len(SH.GEMM_PAIRS) + 3)


def test_struct_layouts_match_the_python_side(harness):
    for which, st in enumerate(SH.STRUCTS):
        assert harness.lib.sh_args_size(which) == C.sizeof(st), st.__name__
    assert harness.lib.sh_args_size(len(SH.STRUCTS)) == -1
    assert harness.lib.sh_instances(len(SH.KINDS), None, 0) == -1


def test_harness_reaches_every_decode_step_instance_of_the_product(harness, tmp_path):
    from parler_tts_amd import _native as N

    import __graft_entry__

    __graft_entry__.build()  # incremental: a library older than its sources must not hide a newly added instance
    product = _instances_in(N.LIB_PATH, tmp_path / "product")
    direct = harness.instances()
    held = _instances_in(harness.lib._name, tmp_path / "harness")
    for name in SH.KINDS:
        assert len(direct[name]) == len(set(direct[name])), (name, direct[name])
        assert len(product[name]) >= AT_LEAST[name], (name, product[name])
        assert set(direct[name]) == product[name], \
            f"{name}: only in the product {sorted(product[name] - set(direct[name]))}; only in the harness {sorted(set(direct[name]) - product[name])}"
        # and the harness library itself holds the same instances: it launches what it lists
        assert held[name] == product[name], (name, held[name] ^ product[name])


def test_every_listed_instance_has_a_case(harness):
    """tests/step_cases.py names, per family, the instances its case lists reach by the launch functions' own selection rules; an instance that no
    case reaches must be one of the documented unreachable ones."""
    direct = harness.instances()
    for name in SH.KINDS:
        reached = SC.reached_instances(name)
        missing = set(direct[name]) - reached - SC.UNREACHABLE[name]
        assert not missing, f"{name}: no case in tests/step_cases.py reaches {sorted(missing)}"
        assert reached <= set(direct[name]), (name, sorted(reached - set(direct[name])))


def test_host_checks_decline_unsafe_shapes(harness):
    """Null pointers and shapes outside the strip path are PTTS_E_INVALID before any launch (no GPU is touched)."""
    a = SH.ShGemm()
    for d in (True, False):
        for p, e in SH.GEMM_PAIRS:
            assert harness.gemm(d, p, e, a, None) == SH.PTTS_E_INVALID and "sh_gemm" in harness.error()
        assert harness.rows_prep(d, SH.PRO_LN, a, None) == SH.PTTS_E_INVALID
        assert harness.lnproj(d, SH.EPI_STORE, 8, SH.ShLnProj(), None) == SH.PTTS_E_INVALID
        assert harness.xattn(d, 8, SH.ShXAttn(), None) == SH.PTTS_E_INVALID
    assert harness.pack(True, None, None, 16, 32, None) == SH.PTTS_E_INVALID
    assert harness.pack_w8(None, None, 16, 64, None) == SH.PTTS_E_INVALID
    # addressable pointers (never dereferenced on the host), shapes the nodes do not serve
    p = 4096
    g = SH.ShGemm(W=p, x=p, out=p, gamma=p, beta=p, lnstat=p, M=9, N=64, K=1024, x_ld=1024, out_ld=64, x_row_mul=1)
    assert harness.gemm(True, SH.PRO_LN, SH.EPI_STORE, g, None) == SH.PTTS_E_INVALID          # fused LayerNorm above 8 rows
    g.M = 33
    assert harness.gemm(True, SH.PRO_LNS, SH.EPI_STORE, g, None) == SH.PTTS_E_INVALID         # producer statistics above 32 rows
    g.M, g.K, g.x_ld = 16, 512, 512
    assert harness.gemm(True, SH.PRO_LNS, SH.EPI_STORE, g, None) == SH.PTTS_E_INVALID         # ... at a width without an instance
    g.M, g.K, g.x_ld = 257, 1024, 1024
    assert harness.gemm(True, SH.PRO_COPY, SH.EPI_STORE, g, None) == SH.PTTS_E_INVALID        # above 256 rows: the other harness
    g.M, g.out_fo = 16, 1
    assert harness.gemm(True, SH.PRO_COPY, SH.EPI_STORE, g, None) == SH.PTTS_E_INVALID        # fragment-order output of an fp32 epilogue
    ln = SH.ShLnProj(W=p, x=p, gamma=p, beta=p, out=p, M=9, N=64, K=512, x_ld=512, out_ld=64)
    assert harness.lnproj(True, SH.EPI_STORE, 8, ln, None) == SH.PTTS_E_INVALID               # hidden 512
    ln.K = ln.x_ld = 1024
    assert harness.lnproj(True, SH.EPI_STORE, 5, ln, None) == SH.PTTS_E_INVALID               # group size
    xa = SH.ShXAttn(W=p, x=p, gamma=p, beta=p, kcache=p, vcache=p, dims=p, out=p, B=9, K=512, x_ld=512, x_row_mul=1, cap=8, nheads=8, kv_heads=8, n_rep=1)
    assert harness.xattn(True, 4, xa, None) == SH.PTTS_E_INVALID                              # hidden 512 has the 8-utterance instance only
    xa.K = xa.x_ld = 1024
    assert harness.xattn(True, 4, xa, None) == SH.PTTS_E_INVALID                              # heads * 64 != K


# ---- the case lists against the product's plan ---------------------------------------------------------------------------------------------------------
def _cfg(H, bf16=True, **kw):
    return SP.config(H, H // 64, 4 * H, bf16=bf16, **kw)


def _decode(harness, H, B, bf16=True, **switches):
    """The plan of a decode step of B utterances on an engine created for them (for at least 9: up to 8 would take the GEMV step)."""
    r = harness.strip_plan(_cfg(H, bf16, max_batch=max(B, 9)), SP.StepSwitches(**switches), False, B)
    assert r is not None, harness.error()
    return r


def test_lns_fits_is_the_product_s_predicate(harness):
    for bf16 in SC.ENGINES:
        for K in (512, 1024, 1536):
            for M in range(1, 65):
                assert SC.lns_fits(M, K, bf16) == harness.lns_fits(M, K, bf16), (M, K, bf16)
    assert harness.lns_fits(32, 1536, True) and not harness.lns_fits(32, 1536, False) and harness.lns_fits(23, 1536, False)


def test_plan_picks_the_nodes_the_case_lists_are_about(harness):
    for bf16 in SC.ENGINES:
        for H in SC.WIDTHS_FULL:
            # LayerNorm + projection as one node: 8 utterances per workgroup up to 40 rows, 16 above; PTTS_LNPROJ_G forces the size
            for g, rows in SC.LNPROJ_ROWS.items():
                for M in rows:
                    forced, _, _ = _decode(harness, H, M, bf16, lnproj_g=g)
                    plan, layer, head = _decode(harness, H, M, bf16)
                    assert (forced.qkv, forced.fc, forced.lnproj_g) == (SP.QKV_LNPROJ, SP.FC_LNPROJ, g), (H, M, g)
                    assert (plan.qkv, plan.fc, plan.lnproj_g) == (SP.QKV_LNPROJ, SP.FC_LNPROJ, 8 if M <= 40 else 16), (H, M)
                    assert g == 4 or plan.lnproj_g == g, (M, g)                       # the 8- and 16-utterance lists are the default policy's rows
                    assert (layer, head, plan.fo, plan.kv_append, plan.attn) == (6 + (1 if plan.out_proj == SP.OUT_COPY else 2), 2, 1, SP.KVA_NONE, SP.ATTN_ROWS)
            for M, g in ((9, 8), (40, 8), (41, 16), (128, 16)):
                assert _decode(harness, H, M, bf16)[0].lnproj_g == g
            # PTTS_LNPROJ=0: the producer's statistics at 9..32 rows where they fit (PRO_LNS), rows_prep + PRO_COPY on fragment-order rows elsewhere
            for M in sorted(set(SC.ROWS_LNS) | set(SC.ROWS_COPY_FO) | set(range(9, 34))):
                plan, layer, _ = _decode(harness, H, M, bf16, lnproj=0, xattn_groups=0)
                lns = SP.PG_LNS if SC.lns_fits(M, H, bf16) else SP.PG_PREP_COPY
                assert (plan.qkv, plan.qkv_how, plan.fo) == (SP.QKV_GEMM, SP.PG_PREP_COPY, 1), (H, M)
                assert (plan.cross, plan.cq_how, plan.fc, plan.fc1_how, plan.lns) == (SP.CROSS_GEMM_ATTN, lns, SP.FC_GEMM, lns, int(M <= 32)), (H, M, bf16)
                assert layer == 2 + 1 + (1 if plan.out_proj == SP.OUT_COPY else 2) + 2 * (2 if lns == SP.PG_PREP_COPY else 1) + 1 + 1 + 1
                assert SC.lns_fits(M, H, bf16) or M not in SC.ROWS_LNS or (H, bf16, M) == (1536, False, 32)
            # up to 8 rows on a wide engine: every prologue fused into its strip kernel
            for M in SC.ROWS_FUSED:
                plan, layer, head = _decode(harness, H, M, bf16)
                assert (plan.qkv, plan.qkv_how, plan.fc, plan.fo, plan.cross, plan.xattn_g) == (SP.QKV_GEMM, SP.PG_FUSED, SP.FC_SMALL, 0, SP.CROSS_XATTN_FUSED, 8)
                assert plan.out_proj in (SP.OUT_COPY, SP.OUT_COMBINE_FUSED) and (layer, head) == (7, 1)
            # a short prompt's prefill (B = 3, Q = 11; sinusoidal positions, engine-dtype cache): the LN1 + QKV node writes the cache rows itself
            B, Q = SC.LNPROJ_PREFILL["B"], SC.LNPROJ_PREFILL["Q"]
            cfg = _cfg(H, bf16, max_batch=B, max_prompt=Q)
            plan, layer, _ = harness.strip_plan(cfg, SP.StepSwitches(), True, B, Q)
            assert (plan.qkv, plan.kv_append, plan.cross, plan.attn, plan.S_used, plan.lnproj_g) == (SP.QKV_LNPROJ_KV, SP.KVA_NONE, SP.CROSS_LNPROJ_ATTN, SP.ATTN_PREFILL, 1, 8)
            assert layer == 8  # QKV, attention, out_proj, LN2 + q, attention, out_proj, LN3 + fc1, fc2
            rope = harness.strip_plan(_cfg(H, bf16, max_batch=B, max_prompt=Q, rope=True), SP.StepSwitches(), True, B, Q)[0]
            assert (rope.qkv, rope.kv_append) == (SP.QKV_LNPROJ, SP.KVA_ENGINE)
            assert harness.strip_plan(cfg, SP.StepSwitches(), True, B, Q, prefill_attn_mode=0)[0].attn == SP.ATTN_ROWS
            # above 256 prefill rows the QKV GEMM's tile epilogue writes them; up to 256 the kv_append node stays
            for rows, qkv, kva in ((256, SP.QKV_GEMM, SP.KVA_ENGINE), (257, SP.QKV_GEMM_KV, SP.KVA_NONE)):
                plan = harness.strip_plan(_cfg(H, bf16, max_batch=1, max_ctx=512, max_prompt=rows), SP.StepSwitches(), True, 1, rows)[0]
                assert (plan.qkv, plan.qkv_how, plan.kv_append, plan.fo) == (qkv, SP.PG_PREP_COPY, kva, int(rows <= 256)), rows
    kv8 = harness.strip_plan(_cfg(1024, max_batch=9, max_ctx=512, max_prompt=300, kv_fp8=True), SP.StepSwitches(), True, 1, 257)[0]
    assert (kv8.qkv, kv8.kv_append) == (SP.QKV_GEMM, SP.KVA_E4M3)
    # the fused cross block: utterances per workgroup by batch size (2 up to 32, 4 up to 64, 8 above; 8 up to 8 utterances), PTTS_XATTN_G forces one
    for bf16 in SC.ENGINES:
        for g, rows in SC.XATTN_ROWS.items():
            for B in rows:
                policy = 8 if B <= 8 else 2 if B <= 32 else 4 if B <= 64 else 8
                for H in SC.WIDTHS_FULL:
                    plan, forced = _decode(harness, H, B, bf16)[0], _decode(harness, H, B, bf16, xattn_g=g)[0]
                    assert (plan.cross, plan.xattn_g) == (SP.CROSS_XATTN_FUSED, policy), (H, B)
                    assert (forced.cross, forced.xattn_g) == (SP.CROSS_XATTN_FUSED, g if B > 8 else 8), (H, B, g)
                    assert g in (plan.xattn_g, forced.xattn_g)
                assert _decode(harness, SC.WIDTH_GENERIC, B, bf16, xattn_g=g)[0].xattn_g == 8   # hidden 512: the 8-utterance instance only
        assert _decode(harness, 1024, 9, bf16, xattn_groups=0)[0].cross == SP.CROSS_GEMM_ATTN
        assert _decode(harness, 1024, 257, bf16)[0].cross == SP.CROSS_GEMM_ATTN


def test_plan_entry_declines_what_is_no_strip_forward(harness):
    sw = SP.StepSwitches()
    assert harness.strip_plan(_cfg(1024, max_batch=8), sw, False, 3) is None                 # the GEMV step
    assert harness.strip_plan(_cfg(1024, max_batch=8), sw, True, 3, 5) is not None           # its prefill runs the strips
    assert harness.strip_plan(_cfg(1024, bf16=False, max_batch=8), sw, False, 3) is not None  # the fp32 GEMV step serves one utterance
    assert harness.strip_plan(_cfg(1024, max_batch=9), sw, False, 10) is None                # more utterances than the engine holds
    assert harness.strip_plan(_cfg(1024, max_batch=9), sw, False, 9, 2) is None              # a decode step has one position
    assert harness.strip_plan(_cfg(1024, max_batch=9), sw, True, 9, 6) is None               # past max_prompt
    assert harness.strip_plan(_cfg(1024, max_batch=8, kv_fp8=True), sw, True, 1, 5) is None  # a config ptts_engine_create refuses
