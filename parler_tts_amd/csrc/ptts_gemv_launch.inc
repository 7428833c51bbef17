// Instantiation + dispatch of gemv_kernel for ONE (engine dtype, weight format) pair: included by ptts_gemv_bf16.hip,
// ptts_gemv_f32.hip and ptts_gemv_w8.hip with GV_WT / GV_W8 / GV_FN defined (three translation units compiled in parallel).
#include <algorithm>

#include "ptts_gemv_kernels.h"

namespace {

// rows per wave: enough that N / R waves is ~1024 (4 per CU), bounded by the loads a wave keeps in flight (R * NCH <= 40)
inline int pick_rows(int N, int nch, int rcap) {
  static const int sup[] = {1, 2, 3, 4, 5, 6, 8, 10};
  const int want = (N + 1023) / 1024;
  const int maxr = std::min(rcap, std::max(1, 40 / nch));
  int r = 1;
  for (int s : sup)
    if (s <= maxr) { r = s; if (s >= want) break; }
  return r;
}

template <int PRO, int EPI, int S, int RCAP, int MB, int NCH, int R>
int launch_inst(const GemvArgs& a, hipStream_t st) {
  // prologue kernels reduce over K = hidden_size (NF4 <= 8); with 4 utterances the epilogue needs MB * R <= 64 lanes
  // MB = 8 runs 12 waves per workgroup (168 VGPRs per lane): at most 4 weight rows per wave (3 with the e4m3 convert temporaries) stay spill-free
  if constexpr (R * NCH <= 40 && R <= RCAP && MB * R <= 64 && (MB < 8 || R <= (GV_W8 ? 3 : 4)) && (PRO == GV_COPY || NCH * Elem<GV_WT>::EPL <= 32)) {
    const int waves = (a.N + R - 1) / R;
    const int npw = gv_prologue_waves<PRO, MB>(NCH * Elem<GV_WT>::EPL / 4);
    const dim3 grid((waves + 3) / 4), block((npw + 4) * 64);
    const size_t sh = PRO == GV_COPY ? 0 : (size_t)MB * a.K * sizeof(GV_WT);
    if constexpr (PRO == GV_COPY && MB == 8 && MB * NCH > 40 && MB * NCH * 1024 <= 64 * 1024) {
      // 5..8 utterances, activations streamed from memory: staged in LDS once per workgroup where the rows do not fit the registers in one
      // group (Mini fc2: batch 8 step 1054 -> 967 us, batch 5 935 -> 891; profiles/r03_experiments.txt; staging every GV_COPY node measured
      // equal). Up to the 64 KiB of dynamic LDS a launch gets without opting in: the 96 KiB tile of the Large-v1 fc2 (one workgroup per CU)
      // measured no gain over the register groups and stays on them.
      constexpr size_t tile = (size_t)MB * NCH * 1024;  // MB rows of K * sizeof(WT) = NCH KiB
      ptts_klaunch(gemv_kernel<GV_WT, NCH, R, PRO, EPI, S, MB, GV_W8, true>, grid, block, tile, st, a);
      return 0;
    }
    ptts_klaunch(gemv_kernel<GV_WT, NCH, R, PRO, EPI, S, MB, GV_W8>, grid, block, sh, st, a);
    return 0;
  } else {
    return -1;
  }
}
template <int PRO, int EPI, int S, int RCAP, int MB, int NCH>
int launch_nch(const GemvArgs& a, hipStream_t st) {
  switch (pick_rows(a.N, NCH, MB >= 8 ? std::min(RCAP, GV_W8 ? 3 : 4) : (MB > 1 ? std::min(RCAP, 64 / MB) : RCAP))) {
    case 1: return launch_inst<PRO, EPI, S, RCAP, MB, NCH, 1>(a, st);
    case 2: return launch_inst<PRO, EPI, S, RCAP, MB, NCH, 2>(a, st);
    case 3: return launch_inst<PRO, EPI, S, RCAP, MB, NCH, 3>(a, st);
    case 4: return launch_inst<PRO, EPI, S, RCAP, MB, NCH, 4>(a, st);
    case 5: return launch_inst<PRO, EPI, S, RCAP, MB, NCH, 5>(a, st);
    case 6: return launch_inst<PRO, EPI, S, RCAP, MB, NCH, 6>(a, st);
    case 8: return launch_inst<PRO, EPI, S, RCAP, MB, NCH, 8>(a, st);
    default: return launch_inst<PRO, EPI, S, RCAP, MB, NCH, 10>(a, st);
  }
}
// NCH (16-byte activation chunks per lane per row: K / (64 * EPL)) instantiated: hidden sizes 512 / 1024 / 1536 / 2048 and
// ffn sizes 4096 / 6144 in bf16 (1, 2, 3, 4, 8, 12), the same widths in fp32 (2, 4, 6, 8, 16, 24)
template <int PRO, int EPI, int S, int RCAP, int MB>
int launch_k(const GemvArgs& a, hipStream_t st) {
  switch (a.K / (64 * Elem<GV_WT>::EPL)) {
    case 1: return launch_nch<PRO, EPI, S, RCAP, MB, 1>(a, st);
    case 2: return launch_nch<PRO, EPI, S, RCAP, MB, 2>(a, st);
    case 3: return launch_nch<PRO, EPI, S, RCAP, MB, 3>(a, st);
    case 4: return launch_nch<PRO, EPI, S, RCAP, MB, 4>(a, st);
    case 6: return launch_nch<PRO, EPI, S, RCAP, MB, 6>(a, st);
    case 8: return launch_nch<PRO, EPI, S, RCAP, MB, 8>(a, st);
    case 12: return launch_nch<PRO, EPI, S, RCAP, MB, 12>(a, st);
    case 16: return launch_nch<PRO, EPI, S, RCAP, MB, 16>(a, st);
    case 24: return launch_nch<PRO, EPI, S, RCAP, MB, 24>(a, st);
    default: return -1;
  }
}
template <int PRO, int EPI, int S, int RCAP>
int launch_m(const GemvArgs& a, hipStream_t st) {
  if (a.M == 1) return launch_k<PRO, EPI, S, RCAP, 1>(a, st);
#ifdef GV_MULTI  // batch 2..4 and 5..8 instances (not built for the fp32 parity engine: one utterance only)
  if (a.M <= 4) return launch_k<PRO, EPI, S, RCAP, 4>(a, st);
  if (a.M <= GV_MAX_ROWS) return launch_k<PRO, EPI, S, RCAP, GV_MAX_ROWS>(a, st);
#endif
  return -1;
}

}  // namespace

int GV_FN(int pro, int epi, int S, GemvArgs a, hipStream_t st) {
  a.invK = 1.0f / (float)a.K;
  if (!a.resid) a.resid = a.out;
  int rc = -1;
  if (pro == GV_LN && epi == GV_STORE) rc = launch_m<GV_LN, GV_STORE, 1, 10>(a, st);
  else if (pro == GV_LN && epi == GV_GELU_WT) rc = launch_m<GV_LN, GV_GELU_WT, 1, 10>(a, st);
  else if (pro == GV_COPY && epi == GV_RESID) rc = launch_m<GV_COPY, GV_RESID, 1, 2>(a, st);
  else if (pro == GV_SOFTMAX && epi == GV_RESID && a.M == 1) rc = launch_k<GV_SOFTMAX, GV_RESID, 1, 2, 1>(a, st);
  else if (pro == GV_ATTN && epi == GV_RESID && S == 2) rc = launch_m<GV_ATTN, GV_RESID, 2, 2>(a, st);
  else if (pro == GV_ATTN && epi == GV_RESID && S == 4) rc = launch_m<GV_ATTN, GV_RESID, 4, 2>(a, st);
  else if (pro == GV_ATTN && epi == GV_RESID && S == 8) rc = launch_m<GV_ATTN, GV_RESID, 8, 2>(a, st);
  else if (pro == GV_LNP && epi == GV_GELU_WT && a.M == 1 && a.npart <= GV_PMAX) rc = launch_k<GV_LNP, GV_GELU_WT, 1, 10, 1>(a, st);
  else if (pro == GV_ATTN2 && epi == GV_RESID && S == 1) rc = launch_m<GV_ATTN2, GV_RESID, 1, 2>(a, st);
  else if (pro == GV_ATTN2 && epi == GV_RESID && S == 2) rc = launch_m<GV_ATTN2, GV_RESID, 2, 2>(a, st);
  else if (pro == GV_ATTN2 && epi == GV_RESID && S == 4 && a.M <= 4) rc = launch_m<GV_ATTN2, GV_RESID, 4, 2>(a, st);  // 5..8 utterances: 12 waves, the 4-split combine spills
  else if (pro == GV_ATTN2 && epi == GV_RESID && a.M == 1 && S == 8) rc = launch_k<GV_ATTN2, GV_RESID, 8, 2, 1>(a, st);
  if (rc != 0) return rc;
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// qkv_attn_kernel: hidden sizes 512 / 1024 / 1536 in bf16 (NCH 1 .. 3), 512 / 1024 in fp32 (NCH 2 / 4); U = 4 K/V row groups per wave in flight
// (a split's first batch covers 8 waves x 4 groups x RPI rows = 256 bf16 / 128 fp32 positions). U = 8 with half the splits measured 5 % SLOWER at
// Mini-v1 (584 vs 557 us per step) and 3 % at Large-v1 (profiles/r04_experiments.txt call 17): the instances were dropped. bf16 at H = 2048 (NCH 4)
// keeps the two nodes (its 8 weight rows per wave + the K/V batch spill).
namespace {
template <int NCH>
int launch_qa(const QkvAttnArgs& a, hipStream_t st) {
  ptts_klaunch(qkv_attn_kernel<GV_WT, NCH, GV_W8, 4>, dim3(a.nheads, a.S + 3, a.M), dim3(512), 0, st, a);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
}  // namespace
int GV_QA_FN(QkvAttnArgs a, hipStream_t st) {
  a.invK = 1.0f / (float)a.H;
  if (a.M < 1) a.M = 1;
  if (a.x_ld <= 0) a.x_ld = a.H;
  if (a.H % (64 * Elem<GV_WT>::EPL)) return -1;
  const int nch = a.H / (64 * Elem<GV_WT>::EPL);
  if constexpr (sizeof(GV_WT) == 4) {
    if (nch == 2) return launch_qa<2>(a, st);
    if (nch == 4) return launch_qa<4>(a, st);
    return -1;
  } else {
    switch (nch) {
      case 1: return launch_qa<1>(a, st);
      case 2: return launch_qa<2>(a, st);
      case 3: return launch_qa<3>(a, st);
      default: return -1;
    }
  }
}

// xq_attn_kernel: the widths of qkv_attn_kernel
namespace {
template <int NCH>
int launch_xq(const XqAttnArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((xq_attn_kernel<GV_WT, NCH, GV_W8>), dim3(a.nheads, a.M), dim3(512), 0, st, a);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
}  // namespace
int GV_XQ_FN(XqAttnArgs a, hipStream_t st) {
  a.invK = 1.0f / (float)a.H;
  if (a.H % (64 * Elem<GV_WT>::EPL)) return -1;
  const int nch = a.H / (64 * Elem<GV_WT>::EPL);
  if constexpr (sizeof(GV_WT) == 4) {
    if (nch == 2) return launch_xq<2>(a, st);
    if (nch == 4) return launch_xq<4>(a, st);
    return -1;
  } else {
    switch (nch) {
      case 1: return launch_xq<1>(a, st);
      case 2: return launch_xq<2>(a, st);
      case 3: return launch_xq<3>(a, st);
      default: return -1;
    }
  }
}

#ifdef GV_XA_FN
// xfold_attn_kernel: hidden sizes 512 / 1024 / 1536 in bf16 (NCH 1 .. 3), 512 in fp32 (NCH 2); NUR = 2 or 4 rounds of output rows per workgroup
namespace {
template <int NCH, int NUR>
int launch_xa(const XfoldAttnArgs& a, hipStream_t st) {
  constexpr int rows_per_wg = NUR * 8 * (Elem<GV_WT>::EPL);  // NUR rounds x 8 waves x 64 / LPR rows
  if (a.H % rows_per_wg) return -1;
  ptts_klaunch(xfold_attn_kernel<GV_WT, NCH, NUR>, dim3(a.nheads, a.H / rows_per_wg), dim3(512), 0, st, a);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
template <int NCH>
int launch_xa_n(const XfoldAttnArgs& a, hipStream_t st) {
  return a.nur == 4 ? launch_xa<NCH, 4>(a, st) : launch_xa<NCH, 2>(a, st);
}
}  // namespace
int GV_XA_FN(XfoldAttnArgs a, hipStream_t st) {
  a.invK = 1.0f / (float)a.H;
  if (a.H % (64 * Elem<GV_WT>::EPL)) return -1;
  const int nch = a.H / (64 * Elem<GV_WT>::EPL);
  if constexpr (sizeof(GV_WT) == 4) {
    return nch == 2 ? launch_xa_n<2>(a, st) : -1;
  } else {
    switch (nch) {
      case 1: return launch_xa_n<1>(a, st);
      case 2: return launch_xa_n<2>(a, st);
      case 3: return launch_xa_n<3>(a, st);
      default: return -1;
    }
  }
}
#endif
