"""CPU: the decode-step test harness (tests/native/step_harness.hip) cross-compiles for gfx950 without a GPU, exports exactly its entry points,
agrees with the Python side on its struct layouts, and reaches every lnproj_fused_kernel, xattn_fused_kernel, rows_prep_kernel and e4m3
gemm_strip_kernel instance that the product library contains - an instance added to launch_lnproj, launch_xattn_fused, launch_prep's callers or
ptts_lm_w8.hip without a case fails here. Symbol names only; no instruction is read."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import step_cases as SC
import step_harness as SH

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
