"""CPU: the one composed bound of tests/test_gemv_kernels_gpu.py - gemv_cases.lnp_gelu_bound, the normalised row of GV_LNP seen through its only
epilogue, the GELU - holds for a float32 torch restatement of the node on the GPU cases' own inputs, in both engine dtypes, and is not vacuous:
the same restatement on a row sum that lacks its last partial row, and on a LayerNorm without beta, exceeds it many times over."""
import pytest
import torch

import gemv_cases as GC
import step_model as SM

F64 = torch.float64


def restate(hs, gamma, beta, c, pi, bf16):
    """GV_LNP + GV_GELU_WT through one selection matrix in float32 torch: LayerNorm of the summed row, the row in the engine dtype, c y (exact),
    the GELU as the engine evaluates it (bf16: the fp32 formula, rounded to bf16; fp32: the double-precision form rounded once). -> float64 [1, N]"""
    y = torch.nn.functional.layer_norm(hs.float()[None, :], (hs.numel(),), gamma.float(), beta.float(), SM.EPS)
    y = y.bfloat16().float() if bf16 else y
    u = c.float()[None, :] * y[:, pi]
    if bf16:
        return (0.5 * u * (1.0 + torch.erf(u * 0.70710678118654752440))).bfloat16().to(F64)
    return SM.gelu_erf64(u).float().to(F64)


@pytest.mark.parametrize("bf16", (True, False), ids=("bf16", "fp32"))
@pytest.mark.parametrize("K,npart", GC.LNP_SHAPES)
def test_float32_restatement_stays_inside_the_lnp_gelu_bound(K, npart, bf16):
    x, part, gamma, beta = GC.lnp_inputs(K, npart)
    hs = GC.lnp_row_sum(x, part)
    y64 = SM.layer_norm64(hs[None, :], gamma, beta)
    bar, _ = SM.ln_tolerance_fp32(hs[None, :], gamma, beta, y64)
    rows_bound = SM.ln_rows_bound(y64, bar, bf16)
    worst, wrong = 0.0, {"row sum without its last partial row": 0.0, "LayerNorm without beta": 0.0}
    for _, pi, c in GC.selection_weights(256, K, 3510 + K):
        ref, tol = GC.lnp_gelu_bound(y64, rows_bound, c, pi, bf16)
        assert bool((tol > 0).all())
        worst = max(worst, float(((restate(hs, gamma, beta, c, pi, bf16) - ref).abs() / tol).max()))
        short = restate(GC.lnp_row_sum(x, part[:-1]), gamma, beta, c, pi, bf16)
        nobeta = restate(hs, gamma, torch.zeros_like(beta), c, pi, bf16)
        wrong["row sum without its last partial row"] = max(wrong["row sum without its last partial row"], float(((short - ref).abs() / tol).max()))
        wrong["LayerNorm without beta"] = max(wrong["LayerNorm without beta"], float(((nobeta - ref).abs() / tol).max()))
    print(f"K={K} npart={npart} {'bf16' if bf16 else 'fp32'}: float32 restatement error / bound {worst:.3f}; wrong variants {wrong}")
    assert worst <= 1.0, f"the float32 restatement leaves the bound: {worst:.2f} x"
    for what, r in wrong.items():
        assert r > 4.0, f"{what} stays within {r:.2f} x the bound: the check would not see it"
