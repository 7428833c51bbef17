"""CPU: the harness of the WARP instances of the sampler tail (tests/native/warp_tail_harness.hip) cross-compiles for gfx950 without a GPU,
exports exactly its entry points, and holds every tail_warp_kernel instance the product library contains (what tests/test_tail_harness_cpu.py
checks for tail_kernel, whose six instances keep their names)."""
import os
import re
import shutil
import subprocess

import pytest

import test_tail_harness_cpu as TT
import warp_tail_harness as WH

ENTRY_POINTS = ("wh_last_error", "wh_args_size", "wh_tail", "wh_set_warp", "wh_set_slot_gen")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return WH.Harness(WH.build(str(tmp_path_factory.mktemp("warp_tail_harness"))))


def _kernels_in(lib, tmp_path, pattern):
    os.makedirs(str(tmp_path), exist_ok=True)
    shutil.copy(lib, str(tmp_path / "lib.so"))  # the code objects are written next to the file they come from
    subprocess.run([os.path.join(TT.LLVM, "llvm-objdump"), "--offloading", str(tmp_path / "lib.so")], capture_output=True, cwd=str(tmp_path), check=True)
    objs = [str(tmp_path / f) for f in os.listdir(tmp_path) if "amdgcn" in f]
    assert objs, "no embedded gfx950 code objects found"
    found = set()
    for obj in objs:
        syms = subprocess.run([os.path.join(TT.LLVM, "llvm-readelf"), "--symbols", obj], capture_output=True, text=True, check=True).stdout
        found |= {(int(a), int(b)) for a, b in re.findall(pattern, syms)}
    return found


def test_harness_cross_compiles_and_exports_its_entry_points(harness):
    out = subprocess.run(["nm", "-D", "--defined-only", harness.lib._name], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert exported == set(ENTRY_POINTS), exported ^ set(ENTRY_POINTS)


def test_harness_holds_every_warp_instance_of_the_product_and_tail_kernel_keeps_its_six(harness, tmp_path):
    from parler_tts_amd import _native as N

    import __graft_entry__

    __graft_entry__.build()  # incremental: a library older than its sources must not hide a newly added instance
    warp = r"_Z16tail_warp_kernelILi(\d+)ELb([01])EE"
    want = {(nv, s) for nv in (8, 18, 32) for s in (0, 1)}
    assert _kernels_in(N.LIB_PATH, tmp_path / "product", warp) == want == _kernels_in(harness.lib._name, tmp_path / "harness", warp)
    assert TT._tail_instances_in(N.LIB_PATH, tmp_path / "product2") == want  # tail_kernel<NV, SESSION>: the names of the parent commit
