"""CPU: the GEMV decode-step harness (tests/native/gemv_harness.hip) cross-compiles for gfx950 without a GPU, exports exactly its entry points, agrees
with the Python side on its struct layouts, holds the same gemv_kernel / qkv_attn_kernel / xfold_attn_kernel / xq_attn_kernel instances as the
product library, and tests/gemv_cases.py's restatement of the instance selection names only instances that exist and reaches, with a test case,
every instance that a node of its node table reaches. That table is tied to the product by the product's own plan of the step
(ptts_step_plan.h: gemv_plan, through the harness's host-only entry points): swept over the table's widths, batch sizes, contexts and every switch,
the launches the plan lists are exactly gemv_cases.nodes() minus gemv_cases.UNREACHED_NODES - a node gemv_step starts or stops issuing fails here.
The scan of ptts_qkvattn_ok / ptts_xqattn_ok / ptts_xfoldattn_ok / ptts_gemv_k_ok and GV_MAX_ROWS ties the widths themselves (a fused width, a chunk
count or a larger batch added there fails here), and every named instance is looked up among the library's symbols. Symbol names only; no
instruction is read. Unsafe launches are declined on the host before anything touches a device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import gemv_cases as GC
import gemv_harness as GH
import step_plan as SP

LLVM = "/opt/rocm/lib/llvm/bin"
KERNELS = ("gemv_kernel", "qkv_attn_kernel", "xfold_attn_kernel", "xq_attn_kernel")
# the mangled name up to the end of the template argument list (t = bf16_t, f = float, Li<n>E an int, Lb<0|1>E a bool)
PATTERN = r"_Z\d+(" + "|".join(KERNELS) + r")I[tf](?:L[ib]\d+E)+E"
AT_LEAST = {"gemv_kernel": 267, "qkv_attn_kernel": 8, "xfold_attn_kernel": 8, "xq_attn_kernel": 8}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    import __graft_entry__

    __graft_entry__.build()  # incremental: the harness links the objects it leaves beside the sources; a stale library must not hide an instance
    return GH.Harness(GH.build(str(tmp_path_factory.mktemp("gemv_harness"))))


def _instances_in(lib, tmp_path):
    """{kernel: {mangled instance names}} over the gfx950 code objects of `lib` (the method of test_attn_harness_cpu.py)."""
    assert os.path.exists(os.path.join(LLVM, "llvm-objdump")), "llvm-objdump of the ROCm toolchain is needed to list the library's kernels"
    os.makedirs(str(tmp_path), exist_ok=True)
    shutil.copy(lib, str(tmp_path / "lib.so"))
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", str(tmp_path / "lib.so")], capture_output=True, cwd=str(tmp_path), check=True)
    objs = [str(tmp_path / f) for f in os.listdir(tmp_path) if "amdgcn" in f]
    assert objs, "no embedded gfx950 code objects found"
    found = {k: set() for k in KERNELS}
    for obj in objs:
        syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--symbols", "--wide", obj], capture_output=True, text=True, check=True).stdout
        for m in re.finditer(PATTERN, syms):
            found[m.group(1)].add(m.group(0))
    return found


@pytest.fixture(scope="module")
def instances(harness, tmp_path_factory):
    from parler_tts_amd import _native as N

    d = tmp_path_factory.mktemp("gemv_symbols")
    return _instances_in(N.LIB_PATH, d / "product"), _instances_in(harness.lib._name, d / "harness")


def test_harness_cross_compiles_and_exports_its_entry_points(harness):
    for n in GH.ENTRY_POINTS:
        assert hasattr(harness.lib, n), n
    # every other symbol stays local: the harness's copies of ptts_gemv_launch and its kin cannot interpose on the product library's
    out = subprocess.run(["nm", "-D", "--defined-only", harness.lib._name], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert exported == set(GH.ENTRY_POINTS), exported ^ set(GH.ENTRY_POINTS)
    assert set(GH.build.reused) == set(GH.UNITS), f"after build() the product's own objects are linked, not recompiled: {GH.build.reused}"


def test_struct_layouts_and_constants_match_the_python_side(harness):
    for which, st in enumerate(GH.STRUCTS):
        assert harness.lib.gvh_args_size(which) == C.sizeof(st), st.__name__
    assert harness.lib.gvh_args_size(len(GH.STRUCTS)) == -1
    assert (harness.PMAX, harness.MAX_ROWS) == (GC.GV_PMAX, GC.GV_MAX_ROWS)
    # what the product itself states about its shapes, scanned: the hidden sizes the fused nodes serve are the case table's WIDTHS, the chunk
    # counts gemv_kernel is built for are NCH_BUILT, the utterances per launch GV_MAX_ROWS. A fused width, a chunk count or a larger batch added to
    # the product fails here; a new model width inside the same chunk counts is not something the product states, and is not noticed.
    hidden = {w[0] for w in GC.WIDTHS}
    for mode in GH.MODES:
        assert harness.rows_per_split(mode) == GC.rows_per_split(mode)
        fused = {Hd for Hd in range(64, 4097, 64) if harness.qkvattn_ok(Hd, mode)}
        assert fused == {Hd for Hd in range(64, 4097, 64) if harness.xqattn_ok(Hd, mode)} == {Hd for Hd in hidden if GC.qa_ok(Hd, mode)}, (mode, fused)
        assert fused <= hidden
        if mode != GH.GV_BF16_W8:
            folded = {Hd for Hd in range(64, 4097, 64) if harness.xfoldattn_ok(Hd, Hd // 64, mode)}
            assert folded == {Hd for Hd in hidden if GC.xfold_ok(Hd, Hd // 64, mode)}, (mode, folded)
        e = GC.epl(mode)
        built = {K // (64 * e) for K in range(64, 64 * e * 32 + 1, 64) if harness.gemv_k_ok(K, mode)}
        assert built == set(GC.NCH_BUILT), (mode, built)


# every switch the GEMV step reads, on both sides, one at a time beside the defaults
GEMV_SWITCHES = ({}, dict(fuse_qa=0), dict(fuse_qa_max=1), dict(fuse_qa_max=8), dict(fuse_x=0), dict(fuse_x=1), dict(fuse_x_nur=4), dict(fuse_xq=0))


def test_the_product_s_plan_issues_the_node_table(harness):
    """gemv_plan over WIDTHS x {all K/V heads, half} x the three modes x M = 1..8 (fp32: 1) x max_batch in {M, 8} x max_ctx in {64, 300, 1100, 2048}
    (S_self takes every value it can) x every 64-position bucket edge up to max_ctx x folded or not x each switch on both sides: what it lists is a
    subset of gemv_cases.nodes(), and what is left over is exactly UNREACHED_NODES."""
    listed, splits = set(), set()
    for Hd, nh, F in GC.WIDTHS:
        for nkv in (nh, nh // 2):
            for mode in GH.MODES:
                for M in range(1, (1 if mode == GH.GV_F32 else GC.GV_MAX_ROWS) + 1):
                    for max_batch in sorted({M, GC.GV_MAX_ROWS}):
                        for max_ctx in (64, 300, 1100, 2048):
                            cfg = SP.config(Hd, nh, F, bf16=mode != GH.GV_F32, max_batch=max_batch, max_ctx=max_ctx, kv_heads=0 if nkv == nh else nkv,
                                            weights_fp8=mode == GH.GV_BF16_W8)
                            sc = harness.step_config(cfg)
                            assert sc.use_gemv and (sc.nkv, sc.gemv_rows) == (nkv, 1 if mode == GH.GV_F32 else GC.GV_MAX_ROWS), (Hd, nkv, mode)
                            splits.add(sc.S_self)
                            for kv_bound in sorted({min(max_ctx, 64 * k) for k in range(1, max_ctx // 64 + 2)}):
                                for xfold_valid in (False, True):
                                    for kw in GEMV_SWITCHES:
                                        plan = harness.gemv_plan(cfg, SP.StepSwitches(**kw), M, kv_bound, xfold_valid)
                                        assert plan is not None, (Hd, nkv, mode, M, max_batch, max_ctx, kv_bound, harness.error())
                                        assert all(n[3] == M for n in plan[0]) and plan[5] <= (8 if M == 1 else 4 if M <= 4 else 2)
                                        listed |= set(plan[0])
    assert splits == {1, 2, 4, 8}
    assert listed <= GC.nodes(), sorted(listed - GC.nodes())[:4]
    assert GC.nodes() - listed == GC.UNREACHED_NODES, sorted((GC.nodes() - listed) ^ GC.UNREACHED_NODES)[:4]
    # a call the engine would not run as a GEMV step is declined: more utterances than the engine holds, or than the fp32 step serves
    cfg = SP.config(1024, 16, 4096, max_batch=4)
    assert harness.gemv_plan(cfg, SP.StepSwitches(), 5, 64, False) is None
    assert harness.gemv_plan(SP.config(1024, 16, 4096, bf16=False, max_batch=4), SP.StepSwitches(), 2, 64, False) is None
    assert harness.gemv_plan(SP.config(1024, 16, 4096, max_batch=9), SP.StepSwitches(), 1, 64, False) is None


def test_plan_launch_counts_of_the_default_step(harness):
    """Default switches, hidden 1024, 2 layers: 5 / 6 / 6 / 7 launches per layer at 1 / 2 / 3 / 4 utterances plus one for the head projection - the
    numbers tests/test_lm_gpu.py reads off the captured step graphs (there with the sampler tail as one more node)."""
    for M, per_layer in ((1, 5), (2, 6), (3, 6), (4, 7)):
        cfg = SP.config(1024, 16, 4096, layers=2, max_batch=M, max_ctx=64, max_enc=16, max_prompt=5)
        launches, layer, head, cross, fuse_qa, S_f = harness.gemv_plan(cfg, SP.StepSwitches(), M, 64, M == 1)
        assert (layer, head) == (per_layer, 1), (M, layer, head)
        assert cross == (SP.XFOLD_ONE_NODE if M == 1 else SP.XQ_FUSED) and fuse_qa == int(M <= 3) and S_f == 1
        # the gemv_kernel launches among them: all but the two attention nodes of a layer (qkv_attn or attention, xfold_attn or xq_attn)
        assert len(launches) == 2 * (per_layer - 2) + 1


def test_harness_holds_the_product_s_instances(instances):
    product, held = instances
    for k in KERNELS:
        assert len(product[k]) >= AT_LEAST[k], (k, len(product[k]))
        assert held[k] == product[k], f"{k}: only in the product {sorted(product[k] - held[k])[:4]}; only in the harness {sorted(held[k] - product[k])[:4]}"


def test_restated_selection_names_existing_instances(instances):
    product, _ = instances
    names = product["gemv_kernel"]
    # every instance the restatement can name for a shape the dispatch serves: over the built chunk counts, row counts on both sides of every
    # pick_rows threshold, every (prologue, epilogue, S), M = 1, 3, 8 and the three modes
    named = set()
    for mode in GH.MODES:
        for nch in GC.NCH_BUILT:
            K = nch * 64 * GC.epl(mode)
            for pro, epi in ((GH.GV_LN, GH.GV_STORE), (GH.GV_LN, GH.GV_GELU_WT), (GH.GV_COPY, GH.GV_RESID), (GH.GV_SOFTMAX, GH.GV_RESID),
                             (GH.GV_ATTN, GH.GV_RESID), (GH.GV_ATTN2, GH.GV_RESID), (GH.GV_LNP, GH.GV_GELU_WT)):
                for S in (1, 2, 4, 8):
                    for M in (1, 3, 8):
                        for N in [1 + 1024 * i for i in range(11)] + [1024 * i for i in range(1, 12)]:
                            inst = GC.instance_of(pro, epi, S, M, N, K, mode)
                            if inst is not None:
                                named.add(inst)
    assert len(named) > len(GC.reached_by_nodes())
    missing = [i for i in sorted(named) if GC.symbol_of(i) not in names]
    assert not missing, f"instance_of names {len(missing)} instances the product does not hold, e.g. {missing[:4]}"
    missing = [i for i in sorted(GC.reached_by_nodes()) if GC.symbol_of(i) not in names]
    assert not missing, missing[:4]


def test_every_instance_a_node_reaches_has_a_case():
    reached, covered = set(GC.reached_by_nodes()), GC.reached_by_cases()
    assert len(reached) >= AT_LEAST["gemv_kernel"]
    assert not reached - covered, f"no case in tests/gemv_cases.py reaches {sorted(reached - covered)[:4]}"
    cases = GC.gemv_cases()
    for pro, epi, S, M, N, K, mode in cases:
        R = GC.instance_of(pro, epi, S, M, N, K, mode)[2]
        product_n = N == GC.LM_HEAD_ROWS or (N, K) == (2048, 1024)
        assert product_n or (N % (4 * R) and N > 4 * R), (pro, epi, S, M, N, K, mode)   # the row clamp of the last workgroup is exercised
    assert any(c[4] == GC.LM_HEAD_ROWS and GC.LM_HEAD_ROWS % (4 * GC.instance_of(*c)[2]) for c in cases)  # the product's own clamp: 9792 rows at R = 10
    assert any(c[4] == 1024 + 2 * 8 * 64 for c in cases)                                                   # a grouped-query QKV width
    for c in GC.group_cases():
        assert GC.groups_of(GC.instance_of(*c))[1] > 1
    # the fused attention nodes: every (dtype, NCH, W8) instance of the product has a shape
    assert {(m, Hd) for m, Hd, *_ in GC.QKV_SHAPES} == {(m, Hd) for m in GH.MODES for Hd in (512, 1024, 1536) if GC.qa_ok(Hd, m) and not (m == GH.GV_BF16_W8 and Hd == 1536)}
    assert {(m, Hd) for m, Hd, _ in GC.XFOLD_SHAPES} == {(m, Hd) for m in (GH.GV_F32, GH.GV_BF16) for Hd in (512, 1024, 1536) if GC.xfold_ok(Hd, Hd // 64, m)}


def test_host_checks_decline_unsafe_launches(harness):
    """Null pointers, extents that do not cover what the kernel can index, and combinations outside the dispatch are PTTS_E_INVALID before any
    launch (no GPU is touched: the pointers are never dereferenced on the host)."""
    E = GH.PTTS_E_INVALID
    assert harness.gemv(GH.GvhGemv(), None) == E and "gvh_gemv" in harness.error()
    assert harness.qkvattn(GH.GvhQkvAttn(), None) == E and harness.xfoldattn(GH.GvhXfold(), None) == E and harness.xqattn(GH.GvhXq(), None) == E
    p = 4096

    def gemv(**kw):
        base = dict(W=p, out=p, x=p, gamma=p, beta=p, n_W=70 * 512 * 2, n_x=520, n_gamma=512, n_out=78, mode=GH.GV_BF16, pro=GH.GV_LN, epi=GH.GV_STORE,
                    S=1, M=1, N=70, K=512, x_ld=520, out_ld=78)
        base.update(kw)
        return harness.gemv(GH.GvhGemv(**base), None)

    assert gemv(n_W=70 * 512 * 2 - 1) == E                      # the last weight row
    assert gemv(n_out=69) == E and gemv(out_ld=64) == E          # N, out_ld
    assert gemv(M=3, n_out=78 * 2 + 69) == E                     # the last utterance's row
    assert gemv(x_ld=508) == E and gemv(M=2, n_x=520 + 511) == E
    assert gemv(mode=GH.GV_F32, M=2, n_W=70 * 512 * 4, n_x=1040, n_out=156) == E   # the fp32 engine serves one utterance
    assert gemv(K=2560, n_W=70 * 2560 * 2) == E and gemv(K=4096, n_W=70 * 4096 * 2, n_x=4104, n_gamma=4096, x_ld=4104) == E  # no such chunk count; LN above 2048
    assert gemv(mode=GH.GV_BF16_W8, n_W=70 * 512) == E           # e4m3 rows without scales
    assert gemv(pro=GH.GV_COPY, epi=GH.GV_RESID, xw=p, xw_ld=516, n_xw=516) == E       # rows not 16-byte aligned
    assert gemv(pro=GH.GV_COPY, epi=GH.GV_RESID, xw=p, xw_ld=520, n_xw=511) == E
    assert gemv(pro=GH.GV_COPY, epi=GH.GV_RESID, xw=p, xw_ld=520, n_xw=520, resid=p, n_resid=69) == E
    at = dict(pro=GH.GV_ATTN2, epi=GH.GV_RESID, part=p, stats=p, nheads=8, S=4, n_part=5 * 512, n_stats=5 * 8 * 2)
    assert gemv(**{**at, "n_part": 5 * 512 - 1}) == E and gemv(**{**at, "n_stats": 5 * 16 - 1}) == E       # M x (S + 1) slots
    assert gemv(**{**at, "nheads": 7}) == E and gemv(**{**at, "S": 3}) == E
    assert gemv(**{**at, "M": 5, "n_part": 25 * 512, "n_stats": 400, "n_out": 5 * 78}) == E              # 5..8 utterances: up to 2 splits
    assert gemv(**{**at, "pro": GH.GV_ATTN, "S": 1}) == E
    sm = dict(pro=GH.GV_SOFTMAX, epi=GH.GV_RESID, n_valid=p, ne=64, mask=p, n_mask=64)
    assert gemv(**{**sm, "ne": 48}) == E and gemv(**{**sm, "n_mask": 63}) == E and gemv(**{**sm, "n_valid": None}) == E
    lp = dict(pro=GH.GV_LNP, epi=GH.GV_GELU_WT, part=p, npart=24, n_part=24 * 512, hsum=p, n_hsum=512)
    assert gemv(**{**lp, "npart": 25, "n_part": 25 * 512}) == E and gemv(**{**lp, "n_part": 24 * 512 - 1}) == E and gemv(**{**lp, "n_hsum": 511}) == E

    def qkv(**kw):
        base = dict(W=p, x=p, gamma=p, beta=p, kcache=p, vcache=p, cur_len=p, P=p, part=p, stats=p, n_W=1536 * 512 * 2, n_x=512, n_gamma=512,
                    n_cache=8 * 300 * 64, n_cur_len=1, n_part=3 * 512, n_stats=3 * 16, mode=GH.GV_BF16, S=2, M=1, H=512, nheads=8, kv_heads=8, x_ld=512,
                    cap=300, kv_bound=300, scale=0.125)
        base.update(kw)
        return harness.qkvattn(GH.GvhQkvAttn(**base), None)

    assert qkv(kv_bound=301) == E and qkv(n_cache=8 * 300 * 64 - 1) == E           # the K/V fetch stays below kv_bound <= cap
    assert qkv(n_part=3 * 512 - 1) == E and qkv(n_stats=47) == E and qkv(S=3) == E  # M x (S + 1) slots
    assert qkv(mask=p, mask_ld=8, n_mask=7) == E and qkv(kv_heads=3) == E and qkv(H=2048, nheads=32) == E
    assert qkv(M=5, S=4, n_x=5 * 512, n_cur_len=5, n_cache=5 * 8 * 300 * 64, n_part=25 * 512, n_stats=400) == E
    assert qkv(mode=GH.GV_F32, H=1536, nheads=24, kv_heads=24) == E

    def xf(**kw):
        base = dict(Mw=p, Uw=p, x=p, gamma=p, beta=p, n_valid=p, xpart=p, n_Mw=512 * 512, n_Uw=512 * 512, n_x=512, n_gamma=512, n_xpart=8 * 512,
                    mode=GH.GV_BF16, H=512, nheads=8, nur=2)
        base.update(kw)
        return harness.xfoldattn(GH.GvhXfold(**base), None)

    assert xf(nur=3) == E and xf(n_xpart=8 * 512 - 1) == E and xf(mode=GH.GV_BF16_W8) == E and xf(mask=p, n_mask=63) == E and xf(mode=GH.GV_F32, H=1024, nheads=16) == E

    def xq(**kw):
        base = dict(W=p, x=p, gamma=p, beta=p, kcache=p, vcache=p, n_valid=p, out=p, n_W=512 * 512 * 2, n_x=512, n_gamma=512, n_cache=8 * 80 * 64, n_out=512,
                    mode=GH.GV_BF16, M=1, H=512, nheads=8, kv_heads=8, x_ld=512, out_ld=512, cap=80, scale=0.125)
        base.update(kw)
        return harness.xqattn(GH.GvhXq(**base), None)

    assert xq(n_cache=8 * 80 * 64 - 1) == E and xq(out_ld=508) == E and xq(M=9) == E and xq(mask=p, mask_ld=80, n_mask=79) == E and xq(n_valid=None) == E
