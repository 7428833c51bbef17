"""CPU: the attention test harness (tests/native/attn_harness.hip) cross-compiles for gfx950 without a GPU, exports exactly its entry points,
and reaches every instance of the six attention kernels that the product library contains - an instance added to launch_attn,
launch_prefill_attn or the T5 forward without a test fails here."""
import os
import re
import shutil
import subprocess

import pytest

import attn_harness as AH

LLVM = "/opt/rocm/lib/llvm/bin"
# template arguments in the mangled names: t = bf16_t (uint16_t), f = float, Li<n>E an int, Lb<0|1>E a bool; the T5 kernels live in an unnamed namespace
PATTERNS = {
    "attn_kernel": r"_Z11attn_kernelI([tf])Li(\d+)ELb([01])EE",
    "prefill_attn_kernel": r"_Z19prefill_attn_kernelI([tf])Lb([01])EE",
    "prefill_attn_mfma_kernel": r"_Z24prefill_attn_mfma_kernelI([tf])Li(\d+)EE",
    "kv_append_kernel": r"_Z16kv_append_kernelI([tf])Lb([01])EE",
    "t5_attn_kernel": r"_ZN12_GLOBAL__N_114t5_attn_kernelI([tf])EE",
    "t5_attn_mfma_kernel": r"_ZN12_GLOBAL__N_119t5_attn_mfma_kernelI([tf])EE",
}
AT_LEAST = {"attn_kernel": 7, "prefill_attn_kernel": 3, "prefill_attn_mfma_kernel": 8, "kv_append_kernel": 3, "t5_attn_kernel": 2, "t5_attn_mfma_kernel": 2}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return AH.Harness(AH.build(str(tmp_path_factory.mktemp("attn_harness"))))


def _instances_in(lib, tmp_path):
    """{kernel: {(bf16, further template arguments...)}} over the gfx950 code objects of `lib` (the method of test_tail_harness_cpu.py)."""
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
                found[name].add((int(m.group(1) == "t"),) + tuple(int(x) for x in m.groups()[1:]))
    return found


def test_harness_cross_compiles_and_exports_its_entry_points(harness):
    for n in AH.ENTRY_POINTS:
        assert hasattr(harness.lib, n), n
    # every other symbol stays hidden: the harness's own copy of ptts_fail cannot interpose on the product library's
    out = subprocess.run(["nm", "-D", "--defined-only", harness.lib._name], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert exported == set(AH.ENTRY_POINTS), exported ^ set(AH.ENTRY_POINTS)


def test_harness_reaches_every_attention_kernel_instance_of_the_product(harness, tmp_path):
    from parler_tts_amd import _native as N

    import __graft_entry__

    __graft_entry__.build()  # incremental: a library older than its sources must not hide a newly added instance
    product = _instances_in(N.LIB_PATH, tmp_path / "product")
    direct = harness.instances()
    held = _instances_in(harness.lib._name, tmp_path / "harness")
    for name in AH.KINDS:
        assert len(direct[name]) == len(set(direct[name])), (name, direct[name])
        assert len(product[name]) >= AT_LEAST[name], (name, product[name])
        assert set(direct[name]) == product[name], \
            f"{name}: only in the product {sorted(product[name] - set(direct[name]))}; only in the harness {sorted(set(direct[name]) - product[name])}"
        # and the harness library itself holds the same instances: it launches what it lists
        assert held[name] == product[name], (name, held[name] ^ product[name])
