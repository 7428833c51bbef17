"""CPU: the sampler-tail test harness (tests/native/tail_harness.hip) cross-compiles for gfx950 without a GPU, exports exactly its entry
points, and reaches every tail_kernel instance the product library contains - an instance added to ptts_tail_launch.h without a test
fails here."""
import os
import re
import shutil
import subprocess

import pytest

import tail_harness as TH

LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return TH.Harness(TH.build(str(tmp_path_factory.mktemp("tail_harness"))))


def _tail_instances_in(lib, tmp_path):
    """(NV, SESSION) of every tail_kernel in the gfx950 code objects of `lib` (the method of test_gemm_harness_cpu.py)."""
    assert os.path.exists(os.path.join(LLVM, "llvm-objdump")), "llvm-objdump of the ROCm toolchain is needed to list the library's kernels"
    os.makedirs(str(tmp_path), exist_ok=True)
    shutil.copy(lib, str(tmp_path / "lib.so"))
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", str(tmp_path / "lib.so")], capture_output=True, cwd=str(tmp_path), check=True)
    objs = [str(tmp_path / f) for f in os.listdir(tmp_path) if "amdgcn" in f]
    assert objs, "no embedded gfx950 code objects found"
    found = set()
    for obj in objs:
        syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--symbols", obj], capture_output=True, text=True, check=True).stdout
        for m in re.finditer(r"_Z11tail_kernelILi(\d+)ELb([01])EE", syms):
            found.add((int(m.group(1)), int(m.group(2))))
    return found


def test_harness_cross_compiles_and_exports_its_entry_points(harness):
    for n in TH.ENTRY_POINTS:
        assert hasattr(harness.lib, n), n
    # every other symbol stays hidden: the harness's own copy of ptts_fail cannot interpose on the product library's
    out = subprocess.run(["nm", "-D", "--defined-only", harness.lib._name], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert exported == set(TH.ENTRY_POINTS), exported ^ set(TH.ENTRY_POINTS)


def test_harness_reaches_every_tail_kernel_instance_of_the_product(harness, tmp_path):
    from parler_tts_amd import _native as N

    import __graft_entry__

    __graft_entry__.build()  # incremental: a library older than its sources must not hide a newly added instance
    product = _tail_instances_in(N.LIB_PATH, tmp_path / "product")
    direct = harness.tail_instances()
    assert len(direct) == len(set(direct)), direct
    assert len(product) >= 6, product
    assert set(direct) == product, f"only in the product: {sorted(product - set(direct))}; only in the harness: {sorted(set(direct) - product)}"
    # and the harness library itself holds the same instances: it launches what it lists
    assert _tail_instances_in(harness.lib._name, tmp_path / "harness") == product
