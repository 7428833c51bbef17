"""CPU: the DAC kernel harness (tests/native/dac_harness.hip) cross-compiles for gfx950 without a GPU, exports exactly its entry points and reaches
every instance of the codec's templated kernels that the product library holds; and the codec's dispatch (ptts_dac_launch.h: dac_conv_plan,
dac_resunit_fusable, dac_resunit_xin_width, dac_resunit_plan, dac_conv_out_plan, dac_pack_plan) - pure host functions - selects every convolution
instance for some workload of the two codec shapes, with its thresholds where the comments put them."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import dac_harness as DH
from oracle import dac_oracle as DA

LLVM = "/opt/rocm/lib/llvm/bin"
# template arguments in the mangled names: Li<n>E an int, Lb<0|1>E a bool; the kernels live in an unnamed namespace
PATTERNS = {
    "conv_mfma_kernel": r"_ZN12_GLOBAL__N_116conv_mfma_kernelILi(\d+)ELb([01])EE",
    "conv_lds_kernel": r"_ZN12_GLOBAL__N_115conv_lds_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EE",
    "resunit_lds_kernel": r"_ZN12_GLOBAL__N_118resunit_lds_kernelILi(\d+)ELi(\d+)ELb([01])ELb([01])ELb([01])ELb([01])EE",
    "conv_out_tanh_kernel": r"_ZN12_GLOBAL__N_120conv_out_tanh_kernelILb([01])EE",
    "conv_out_tanh_lds_kernel": r"_ZN12_GLOBAL__N_124conv_out_tanh_lds_kernelILb([01])EE",
    "rvq_gather_kernel": r"_ZN12_GLOBAL__N_117rvq_gather_kernelILb([01])EE",
}
AT_LEAST = {"conv_mfma_kernel": 10, "conv_lds_kernel": 6, "resunit_lds_kernel": 19, "conv_out_tanh_kernel": 2, "conv_out_tanh_lds_kernel": 2, "rvq_gather_kernel": 2}
PLAIN = ("conv_in_kernel", "cb_normalize_kernel", "rvq_encode_kernel", "rvq_table_kernel", "pack_conv_kernel", "pack_conv_bf16_kernel", "inv_alpha_kernel")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return DH.Harness(DH.build(str(tmp_path_factory.mktemp("dac_harness"))))


def _symbols(lib, tmp_path):
    assert os.path.exists(os.path.join(LLVM, "llvm-objdump")), "llvm-objdump of the ROCm toolchain is needed to list the library's kernels"
    os.makedirs(str(tmp_path), exist_ok=True)
    shutil.copy(lib, str(tmp_path / "lib.so"))
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", str(tmp_path / "lib.so")], capture_output=True, cwd=str(tmp_path), check=True)
    objs = [str(tmp_path / f) for f in os.listdir(tmp_path) if "amdgcn" in f]
    assert objs, "no embedded gfx950 code objects found"
    return "\n".join(subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--symbols", o], capture_output=True, text=True, check=True).stdout for o in objs)


def _instances_in(syms):
    return {name: {tuple(int(x) for x in m.groups()) for m in re.finditer(pat, syms)} for name, pat in PATTERNS.items()}


def test_harness_cross_compiles_and_exports_its_entry_points(harness):
    for n in DH.ENTRY_POINTS:
        assert hasattr(harness.lib, n), n
    out = subprocess.run(["nm", "-D", "--defined-only", harness.lib._name], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert exported == set(DH.ENTRY_POINTS), exported ^ set(DH.ENTRY_POINTS)


def test_harness_reaches_every_dac_kernel_instance_of_the_product(harness, tmp_path):
    from parler_tts_amd import _native as N

    import __graft_entry__

    __graft_entry__.build()  # incremental: a library older than its sources must not hide a newly added instance
    psyms, hsyms = _symbols(N.LIB_PATH, tmp_path / "product"), _symbols(harness.lib._name, tmp_path / "harness")
    product, held, direct = _instances_in(psyms), _instances_in(hsyms), harness.instances()
    for name in DH.KINDS:
        assert len(direct[name]) == len(set(direct[name])), (name, direct[name])
        assert len(product[name]) >= AT_LEAST[name], (name, product[name])
        assert set(direct[name]) == product[name], \
            f"{name}: only in the product {sorted(product[name] - set(direct[name]))}; only in the harness {sorted(set(direct[name]) - product[name])}"
        assert held[name] == product[name], (name, held[name] ^ product[name])
    for name in PLAIN:  # the untemplated kernels: held by both
        assert re.search(rf"_ZN12_GLOBAL__N_1\d+{name}E", psyms) and re.search(rf"_ZN12_GLOBAL__N_1\d+{name}E", hsyms), name


# ---- the dispatch rules ---------------------------------------------------------------------------------------------------------------
def _layers(spec, bf16):
    """(shape, rows per latent frame, kind) of every MFMA convolution of the codec, as ptts_dac_create lists them; the encoder runs fp32 only."""
    S, out = DH.ConvShape, []
    ch, mul = spec.decoder_dim, 1
    out.append((S(spec.latent_dim, ch, 7, 1, 1, 0, bf16, -1), 1, "dec"))
    for bi, s in enumerate(spec.decoder_rates):
        cin, cout = ch >> bi, ch >> (bi + 1)
        out.append((S(cin, cout, 2 * s, 1, s, 1, bf16, -1), mul, "dec"))
        mul *= s
        for dil in (1, 3, 9):
            out.append((S(cout, cout, 7, dil, 1, 0, bf16, -1), mul, "dec"))
            out.append((S(cout, cout, 1, 1, 1, 0, bf16, -1), mul, "dec"))
    if not bf16:
        dim, rows = spec.encoder_dim, spec.hop_length
        for st in spec.encoder_rates:
            for dil in (1, 3, 9):
                out.append((S(dim, dim, 7, dil, 1, 0, 0, -1), rows, "enc"))
                out.append((S(dim, dim, 1, 1, 1, 0, 0, -1), rows, "enc"))
            out.append((S(dim, 2 * dim, 2 * st, 1, st, 0, 0, (st + 1) // 2), rows, "enc"))
            dim, rows = 2 * dim, rows // st
        out.append((S(dim, spec.latent_dim, 3, 1, 1, 0, 0, 1), rows, "enc"))
    return out


WORKLOADS = [(1, 1), (1, 8), (2, 37), (1, 56), (1, 100), (4, 100), (1, 430), (1, 860), (2, 860), (4, 860), (8, 860), (32, 860)]  # batch x latent frames


def test_conv_plan_selects_every_instance_for_some_workload(harness):
    """Every layer of DAC_44KHZ and DAC_TINY in both operand modes, from 1 x 1 to 32 x 860 frames and the streamer's 56-frame window: each plan is
    one the launcher accepts, and together they select every conv_mfma_kernel / conv_lds_kernel instance the product holds on every wave count."""
    selected = set()
    for spec in (DA.DAC_44KHZ, DA.DAC_TINY):
        for bf16 in (0, 1):
            for shape, mul, _ in _layers(spec, bf16):
                for B, T in WORKLOADS:
                    p = harness.conv_plan(shape, B, T * mul)
                    selected.add(p.instance())
                    if p.kernel == DH.CONV_LDS:
                        assert shape.bf16 and shape.Cout % (48 * p.p[1]) == 0 and p.block == 64 * p.p[1] and p.grid_y == shape.Cout // (48 * p.p[1]), (p.instance(), shape.Cout)
                        assert shape.Cin % (32 * p.p[2]) == 0
                    else:
                        assert (shape.Cout // 16) % p.p[0] == 0 and p.p[1] == shape.bf16 and p.block == 64 * p.p[2] and p.grid_y == shape.Cout // (16 * p.p[0])
    inst = harness.instances()
    mfma = {(DH.CONV_MFMA, cs, bf) for cs, bf in inst["conv_mfma_kernel"]}
    assert {s[:3] for s in selected if s[0] == DH.CONV_MFMA} == mfma, mfma ^ {s[:3] for s in selected if s[0] == DH.CONV_MFMA}
    assert {s[3] for s in selected if s[0] == DH.CONV_MFMA} == {1, 2, 4}  # waves per workgroup
    lds = {(DH.CONV_LDS,) + t for t in inst["conv_lds_kernel"]}
    assert {s for s in selected if s[0] == DH.CONV_LDS} == lds, lds ^ {s for s in selected if s[0] == DH.CONV_LDS}


def test_conv_plan_thresholds(harness):
    S = DH.ConvShape
    k1 = S(768, 768, 1, 1, 1, 0, 1, -1)  # the un-fused units of the C = 768 block: LDS-tiled from 32 768 rows per launch
    assert harness.conv_plan(k1, 1, 32767).instance()[:3] == (DH.CONV_MFMA, 8, 1)
    assert harness.conv_plan(k1, 1, 32768).instance() == (DH.CONV_LDS, 3, 4, 3, 2, 8)
    assert harness.conv_plan(k1, 32, 1023).instance()[0] == DH.CONV_MFMA and harness.conv_plan(k1, 32, 1024).instance()[0] == DH.CONV_LDS
    assert harness.conv_plan(S(768, 768, 1, 1, 1, 0, 0, -1), 1, 40000).instance()[:3] == (DH.CONV_MFMA, 8, 0)  # fp32 operands: never
    k7 = S(192, 192, 7, 3, 1, 0, 1, -1)  # one workgroup column: FT = 4 below 320 workgroups of 128 frames
    assert harness.conv_plan(k7, 1, 128 * 319).instance() == (DH.CONV_LDS, 3, 4, 1, 54, 4)
    p = harness.conv_plan(k7, 1, 128 * 319)
    assert (p.grid_x, p.grid_y, p.block) == (2 * 319, 1, 256)
    p = harness.conv_plan(k7, 1, 128 * 319 + 1)
    assert p.instance() == (DH.CONV_LDS, 3, 4, 1, 54, 8) and (p.grid_x, p.grid_y) == (320, 1)
    up = S(1536, 768, 16, 1, 8, 1, 1, -1)  # 8 phases x 4 workgroup columns: 9 tiles x 32 = 288 < 320 <= 10 tiles
    assert harness.conv_plan(up, 1, 128 * 9).instance() == (DH.CONV_LDS, 3, 4, 3, 2, 4) and harness.conv_plan(up, 1, 128 * 10).instance() == (DH.CONV_LDS, 3, 4, 3, 2, 8)
    assert harness.conv_plan(S(192, 96, 4, 1, 2, 1, 1, -1), 1, 64).instance() == (DH.CONV_LDS, 3, 2, 1, 2, 8)  # two-wave instances: 128-frame tiles only
    assert harness.conv_plan(S(96, 96, 7, 9, 1, 0, 1, -1), 1, 64).instance() == (DH.CONV_LDS, 3, 2, 1, 54, 8)
    assert harness.conv_plan(S(96, 96, 7, 10, 1, 0, 1, -1), 1, 64).instance()[:3] == (DH.CONV_MFMA, 6, 1)  # halo 60 > 54
    assert harness.conv_plan(S(64, 64, 7, 1, 1, 0, 1, -1), 1, 64).instance()[:3] == (DH.CONV_MFMA, 4, 1)  # below 96 channels
    e = S(128, 128, 1, 1, 1, 0, 0, -1)  # one strip column of CS = 8: waves halve below 1 536 workgroups
    assert harness.conv_plan(e, 1, 128 * 1536).instance() == (DH.CONV_MFMA, 8, 0, 4, 0, 0)
    assert harness.conv_plan(e, 1, 128 * 1536 - 128).instance() == (DH.CONV_MFMA, 8, 0, 2, 0, 0)
    assert harness.conv_plan(e, 1, 64 * 1536 - 64).instance() == (DH.CONV_MFMA, 8, 0, 1, 0, 0)
    p = harness.conv_plan(e, 3, 100)
    assert (p.grid_x, p.grid_y, p.block) == (4 * 3, 1, 64)
    d = harness.conv_plan(S(64, 128, 4, 1, 2, 0, 0, 1), 2, 200)  # a down-sampling conv: rows per launch are the OUTPUT rows
    assert d.instance()[:3] == (DH.CONV_MFMA, 8, 0) and d.grid_x == 2 * 4  # Tn = (200 + 2 - 4) / 2 + 1 = 100 rows -> 4 one-wave tiles


def test_resunit_dispatch(harness):
    S = DH.ConvShape
    unit = lambda Cw, dil=1, bf=1: (S(Cw, Cw, 7, dil, 1, 0, bf, -1), S(Cw, Cw, 1, 1, 1, 0, bf, -1))
    for Cw, fusable in ((96, True), (192, True), (384, True), (768, False), (48, False)):
        assert harness.resunit_plan(*unit(Cw))[0] is fusable, Cw
    assert harness.resunit_plan(*unit(96, 9))[0] and not harness.resunit_plan(*unit(96, 10))[0]  # 6 * dil <= 54
    assert not harness.resunit_plan(*unit(96, 1, 0))[0]  # fp32 operands
    assert not any(harness.resunit_plan(*unit(Cw), no_fuse=1)[0] for Cw in (96, 192, 384))  # PTTS_DAC_NO_FUSE_RES=1
    assert [harness.resunit_plan(*unit(Cw), no_fuse=2)[0] for Cw in (96, 192, 384)] == [True, True, False]
    # the XIN mask: C = 96 always, all three widths from 2 x 860 latent frames; PTTS_DAC_XIN overrides
    for frames, want in ((1, [True, False, False]), (1719, [True, False, False]), (1720, [True, True, True]), (32 * 860, [True, True, True])):
        assert [harness.resunit_plan(*unit(Cw), frames=frames)[1] for Cw in (96, 192, 384)] == want, frames
    assert [harness.resunit_plan(*unit(Cw), frames=5000, xin_mask=0)[1] for Cw in (96, 192, 384)] == [False] * 3
    assert [harness.resunit_plan(*unit(Cw), frames=1, xin_mask=6)[1] for Cw in (96, 192, 384)] == [False, True, True]
    # every resunit_lds_kernel instance is the plan of some (width, outputs), and nothing else is
    planned = set()
    for Cw in (96, 192, 384):
        for raw in (0, 1):
            for f32 in (0, 1):
                for xin in (0, 1):
                    for act in (0, 1):
                        _, _, p = harness.resunit_plan(*unit(Cw), B=2, T=129, raw=raw, act_f32=f32, xin=xin, act=act)
                        if p is None:
                            assert (not act and not (xin and raw)) or (f32 and Cw != 96)
                            continue
                        assert (p.grid_x, p.block) == (4, Cw // 48 * 64) and p.lds >= 2 * (128 + 54) * 96
                        planned.add(p.instance())
    assert planned == set(harness.instances()["resunit_lds_kernel"]), planned ^ set(harness.instances()["resunit_lds_kernel"])
    assert harness.resunit_plan(*unit(384), B=1, T=1)[2].lds == 128 * (384 * 2 + 32)  # 100 KB: the y tile


def test_final_conv_choice_and_tap_table(harness):
    p = harness.conv_out_plan(96, 2, 130)
    assert (p.lds_kernel, p.grid_x, p.grid_y, p.block, p.lds) == (1, 3, 2, 64, 0)
    p = harness.conv_out_plan(96, 2, 130, force_direct=True)
    assert (p.lds_kernel, p.grid_x, p.grid_y, p.block, p.lds) == (0, 1, 1, 256, 7 * 96 * 4)
    assert harness.conv_out_plan(32, 2, 130).lds_kernel == 0 and harness.conv_out_plan(96, 65536, 4).lds_kernel == 0
    # the per-phase tap table of the pack kernels
    k16 = harness.pack_plan(DH.ConvShape(64, 128, 16, 1, 8, 0, 0, 4))  # the 16-tap strided conv: rows 0 and 1 of the table
    assert list(k16.ktap[:16]) == list(range(16)) and (k16.ntaps, k16.nphase, k16.s_co, k16.s_ci, k16.s_k) == (16, 1, 64 * 16, 16, 1)
    for s in (2, 4, 8):
        t = harness.pack_plan(DH.ConvShape(192, 96, 2 * s, 1, s, 1, 1, -1))
        assert (t.ntaps, t.nphase, t.s_co, t.s_ci, t.s_k) == (2, s, 2 * s, 96 * 2 * s, 1)
        pad = (s + 1) // 2
        for ph in range(s):  # output row j * s + ph takes kernel index r from input row j + c0 and r + s from row j + c0 - 1: (j + c0) * s - pad + r = j * s + ph
            r = t.ktap[ph * DH.MAXTAPS]
            assert t.ktap[ph * DH.MAXTAPS + 1] == r + s and 0 <= r < s and ((ph + pad) // s) * s - pad + r == ph


def test_forced_instances_are_refused_where_they_cannot_serve(harness):
    """dh_conv with a forced instance: the launcher's limits (strip count, Cin % 32 / % 96, halo <= 54 / 2, stride, operand mode). A refusal comes
    before any device call, so the pointers are never used."""
    fake = 0x1000

    def forced(shape, kernel, p, T=64):
        a = DH.DhConv(x=fake, w=fake, bias=fake, out_raw=fake, Wp=fake, ktap=fake, shape=shape, B=2, Tin=T, len_mul=1, forced=1)
        a.plan.kernel = kernel
        a.plan.p[:] = p
        return harness.conv(a, None)

    S = DH.ConvShape
    U = DH.PTTS_E_UNSUPPORTED
    assert forced(S(96, 96, 7, 1, 1, 0, 1, -1), DH.CONV_LDS, (3, 4, 1, 54, 8)) == U  # 6 strips: no four-wave column
    assert "strips" in harness.error()
    assert forced(S(96, 192, 7, 10, 1, 0, 1, -1), DH.CONV_LDS, (3, 4, 1, 54, 8)) == U  # halo 60
    assert forced(S(96, 192, 7, 1, 1, 0, 1, -1), DH.CONV_LDS, (3, 4, 3, 2, 8)) == U  # halo 6 on the MAXHALO = 2 instance
    assert forced(S(64, 192, 1, 1, 1, 0, 1, -1), DH.CONV_LDS, (3, 4, 3, 2, 8)) == U  # Cin % 96
    assert forced(S(192, 192, 1, 1, 1, 0, 0, -1), DH.CONV_LDS, (3, 4, 3, 2, 8)) == U  # fp32 operands
    assert forced(S(192, 192, 7, 1, 1, 0, 1, -1), DH.CONV_LDS, (3, 4, 2, 54, 8)) == U  # no such instance
    assert forced(S(192, 192, 7, 1, 1, 0, 1, -1), DH.CONV_LDS, (3, 2, 1, 54, 4)) == U  # FT = 4 exists on four waves only
    assert forced(S(96, 96, 1, 1, 1, 0, 0, -1), DH.CONV_MFMA, (8, 0, 4, 0, 0)) == U  # 6 strips % 8
    assert forced(S(96, 96, 1, 1, 1, 0, 0, -1), DH.CONV_MFMA, (6, 0, 3, 0, 0)) == U  # three waves
    assert forced(S(96, 96, 1, 1, 1, 0, 0, -1), DH.CONV_MFMA, (6, 1, 4, 0, 0)) == U  # operand mode
    assert forced(S(48, 96, 1, 1, 1, 0, 1, -1), DH.CONV_MFMA, (6, 1, 4, 0, 0)) == U  # Cin % 32 with bf16 operands
    assert forced(S(64, 192, 4, 1, 2, 0, 1, 1), DH.CONV_LDS, (3, 4, 1, 54, 8)) == U  # a strided conv
    assert "stride 2" in harness.error()
