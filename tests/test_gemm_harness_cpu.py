"""CPU: the GEMM test harness (tests/native/gemm_harness.hip) cross-compiles for gfx950 without a GPU, and it launches directly every
gemm_glds_kernel instance the product library contains - a tile policy added to ptts_gemm_glds.h without a test case fails here."""
import os
import re
import shutil
import subprocess

import pytest

import gemm_harness as GH

LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return GH.Harness(GH.build(str(tmp_path_factory.mktemp("gemm_harness"))))


def _glds_instances_in(lib, tmp_path):
    """Template arguments of every gemm_glds_kernel in the gfx950 code objects of `lib` (the method of test_native_abi.py)."""
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("no llvm-objdump in this image")
    shutil.copy(lib, str(tmp_path / "lib.so"))
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", str(tmp_path / "lib.so")], capture_output=True, cwd=str(tmp_path), check=True)
    objs = [str(tmp_path / f) for f in os.listdir(tmp_path) if "amdgcn" in f]
    assert objs, "no embedded gfx950 code objects found"
    found = set()
    for obj in objs:
        syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--symbols", obj], capture_output=True, text=True, check=True).stdout
        for m in re.finditer(r"16gemm_glds_kernelI((?:Li\d+E){7})E", syms):
            found.add(tuple(int(v) for v in re.findall(r"Li(\d+)E", m.group(1))))
    return found


def test_harness_cross_compiles_and_exports_its_entry_points(harness):
    names = {"gh_pack", "gh_glds_instances", "gh_last_error", "gh_args_size"}
    for d in "tf":
        for e in GH.EPIS:
            names |= {f"gh_gemm_{d}{e}", f"gh_tile_{d}{e}", f"gh_block_{d}{e}", f"gh_strip_{d}{e}"}
    names |= {f"gh_glds_t{e}" for e in GH.EPIS} | {f"gh_glds_dispatch_t{e}" for e in GH.EPIS}
    for n in names:
        assert hasattr(harness.lib, n), n
    # every other symbol stays hidden: the harness's own copies of ptts_fail & co. cannot interpose on the product library's
    out = subprocess.run(["nm", "-D", "--defined-only", harness.lib._name], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert exported == names, exported ^ names


def test_harness_launches_every_glds_instance_of_the_product(harness, tmp_path):
    from parler_tts_amd import _native as N

    if not os.path.exists(N.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    product = _glds_instances_in(N.LIB_PATH, tmp_path)
    direct = harness.glds_instances()
    assert len(direct) == len(set(direct)), direct
    assert len(product) >= 17, product
    assert set(direct) == product, f"only in the product: {sorted(product - set(direct))}; only in the harness: {sorted(set(direct) - product)}"
