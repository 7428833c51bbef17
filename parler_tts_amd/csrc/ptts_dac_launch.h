// Host dispatch of the DAC codec's kernels (ptts_dac_kernels.h), in two halves per kernel family:
//   * a PLAN: a pure host function (no HIP call) from a layer's shape, the launch size and the two environment switches' values to the kernel
//     instance with its grid, block and dynamic LDS - what tests/test_dac_harness_cpu.py sweeps without a device;
//   * a LAUNCHER that takes a plan and the kernel's argument struct. It can be handed a forced instance (dac_conv_plan_for) and refuses what that
//     instance cannot serve (strip count, Cin % 32 / % 96, halo, stride).
// ptts_dac.hip reads the switches (PTTS_DAC_NO_FUSE_RES, PTTS_DAC_XIN) per call and passes their values in; tests/native/dac_harness.hip calls the
// same functions on buffers of its own.
#pragma once
#include "ptts_dac_kernels.h"

namespace {

// a Conv1d / ConvTranspose1d as the checkpoint describes it; pad < 0: "same" padding (k - 1) * dil / 2 (transposed: (stride + 1) / 2 always)
struct DacConvShape {
  int Cin, Cout, ksize, dil, stride, transposed, bf16, pad;
};

enum { DAC_CONV_MFMA = 0, DAC_CONV_LDS = 1 };
// conv_mfma_kernel<CS, BF> on `waves` waves (p = {CS, BF, waves, 0, 0}), or conv_lds_kernel<CSW, NW, KS, MAXHALO, FT> (p = the five arguments)
struct DacConvPlan {
  int kernel;
  int p[5];
  unsigned grid_x, grid_y, block, lds;
};

// the shape's part of ConvArgs: taps, phases, offsets and the rows per phase of a launch on B x Tin input rows
inline void dac_conv_geometry(const DacConvShape& L, int B, int Tin, ConvArgs& a) {
  a.B = B; a.Tin = Tin; a.Cin = L.Cin; a.Cout = L.Cout;
  if (!L.transposed) {
    a.ntaps = L.ksize; a.nphase = 1; a.dil = L.dil; a.pad = L.pad >= 0 ? L.pad : (L.ksize - 1) * L.dil / 2; a.transposed = 0;
    a.stride = L.stride; a.Tn = L.stride > 1 ? (Tin + 2 * a.pad - L.ksize) / L.stride + 1 : Tin;
  } else {  // to = j*s + ph = ti*s - pad + k  =>  tap 0 (k = r): ti = j + c0 ; tap 1 (k = r + s): ti = j + c0 - 1, c0 = (ph + pad)/s
    a.ntaps = 2; a.nphase = L.stride; a.dil = 1; a.pad = (L.stride + 1) / 2; a.transposed = 1;
    a.stride = 1; a.Tn = Tin;
  }
}

// grid, block and LDS of instance (kernel, p) on the geometry in `a` (no check: dac_conv_launch refuses what the instance cannot serve)
inline DacConvPlan dac_conv_plan_for(int kernel, const int* p, const ConvArgs& a) {
  DacConvPlan pl = {};
  pl.kernel = kernel;
  for (int i = 0; i < 5; ++i) pl.p[i] = p[i];
  const int nstrips = a.Cout / 16;
  if (kernel == DAC_CONV_LDS) {
    const int nw = p[1] > 0 ? p[1] : 1, tfr = p[4] * 16 > 0 ? p[4] * 16 : 128;
    pl.grid_x = (unsigned)(((a.Tn + tfr - 1) / tfr) * a.nphase * a.B);
    pl.grid_y = (unsigned)(nstrips / (3 * nw));
    pl.block = (unsigned)(nw * 64);
  } else {
    const int cs = p[0] > 0 ? p[0] : 1, nwb = p[2] > 0 ? p[2] : 1;
    pl.grid_x = (unsigned)(((a.Tn + 32 * nwb - 1) / (32 * nwb)) * a.nphase * a.B);
    pl.grid_y = (unsigned)(nstrips / cs);
    pl.block = (unsigned)(64 * nwb);
  }
  return pl;
}

// which instance a layer gets at B x Tin input rows
inline DacConvPlan dac_conv_plan(const DacConvShape& L, int B, int Tin) {
  ConvArgs a = {};
  dac_conv_geometry(L, B, Tin, a);
  const int nstrips = L.Cout / 16;
  // LDS-tiled kernel where it wins (rocprof per layer, profiles/r02_dac_layers.txt): every k7 conv (2x the direct kernel) and the
  // transposed convs into >= 192 channels. The last transposed conv is bound by its epilogue traffic (two writes per element) and runs as fast
  // on the direct kernel's 4-5 waves per SIMD as on this one's 2 (round 2 said the same of the k1 convs; see lds_k1 below).
  // k1 convs (the un-fused units of the C = 768 block): on the LDS-tiled kernel from 32 K rows per launch (round 5) - with the whole-row epilogue
  // through LDS it beats the direct kernel at batch 32 (63.1 -> 61.3 ms per decode) and loses 1 % on a single utterance's 6880 rows (2.69 vs 2.71 ms;
  // profiles/r05_experiments.txt calls 13 / 15).
  const bool lds_k1 = (long long)B * Tin >= 32768;
  // the last transposed conv (-> 96 channels): on the LDS-tiled kernel since round 5. Round 4 measured it equal to the direct kernel (5.19 ms per
  // batch-32 launch) - with the 96-channel staging instance, which needs 324 VGPRs and ran one wave per SIMD; with 32-channel staging chunks
  // (conv_lds_kernel<3, 2, 1, 2>, 228 VGPRs, two waves per SIMD) the batch-32 decode drops 61.3 -> 59.3 ms, 860 frames 2.71 -> 2.67 ms
  // (profiles/r05_experiments.txt call 15).
  const bool lds_ok = a.ntaps > 2 ? L.Cout >= 96 : ((a.transposed && L.Cout >= 96) || (lds_k1 && !a.transposed && a.ntaps == 1));
  if (L.bf16 && lds_ok && a.stride == 1 && nstrips % 6 == 0) {
    const int nw = nstrips % 12 == 0 ? 4 : 2;
    const int halo = a.transposed ? a.ntaps - 1 : (a.ntaps - 1) * a.dil;
    // 64-frame tiles (FT = 4) where 128-frame tiles would leave the launch with about one workgroup per CU or fewer (round 5: the first block of a
    // single utterance ran 56-224 workgroups on 256 CUs; the streamer's short windows even fewer): 860 frames 2.34 -> 2.27 ms, a 56-frame window
    // 0.91 -> 0.82 ms; at 432-448 workgroups (two utterances) the smaller tiles LOSE 3.5 % (profiles/r05_experiments.txt call 18), hence the bound.
    // Four-wave instances only.
    const bool ft4 = nw == 4 && (long long)((a.Tn + 127) / 128) * a.nphase * B * (nstrips / (3 * nw)) < 320;
    if (a.ntaps > 2 && halo <= 54 && a.Cin % 32 == 0) {
      const int p[5] = {3, nw, 1, 54, ft4 ? 4 : 8};
      return dac_conv_plan_for(DAC_CONV_LDS, p, a);
    } else if (a.ntaps <= 2 && a.Cin % 96 == 0 && nw == 4) {
      const int p[5] = {3, 4, 3, 2, ft4 ? 4 : 8};
      return dac_conv_plan_for(DAC_CONV_LDS, p, a);
    } else if (a.ntaps <= 2 && a.Cin % 96 == 0) {
      // two-wave workgroups (Cout = 96: the last transposed conv): 32-channel staging chunks - a 96-channel instance staged 13 16-byte pieces per
      // thread, needed 324 VGPRs and ran ONE wave per SIMD (round 5: 5.59 vs 3.35 ms per batch-32 launch; the instance is gone since round 6)
      const int p[5] = {3, 2, 1, 2, 8};
      return dac_conv_plan_for(DAC_CONV_LDS, p, a);
    }
  }
  // strips per wave: the largest of {8, 6, 4, 2, 1} that divides the layer (real DAC widths: 96/48/24/12/6 strips)
  const int CS = nstrips % 8 == 0 ? 8 : (nstrips % 6 == 0 ? 6 : (nstrips % 4 == 0 ? 4 : (nstrips % 2 == 0 ? 2 : 1)));
  // waves per workgroup: fewer (finer tiles) when the launch would otherwise put < ~6 workgroups on each CU, so the
  // 256 CUs finish together (324 four-wave workgroups on 256 CUs = 63 % balance; 1296 one-wave ones = 84 %+)
  int nwb = 4;
  auto blocks = [&](int nw) { return (long long)((a.Tn + 32 * nw - 1) / (32 * nw)) * a.nphase * B * (nstrips / CS); };
  while (nwb > 1 && blocks(nwb) < 256LL * 6) nwb >>= 1;
  const int p[5] = {CS, L.bf16 ? 1 : 0, nwb, 0, 0};
  return dac_conv_plan_for(DAC_CONV_MFMA, p, a);
}

// can instance `pl` serve `a`? Pure host. An instance that cannot is refused (PTTS_E_UNSUPPORTED), an instance that does not exist too
inline int dac_conv_check(const DacConvPlan& pl, const ConvArgs& a) {
  const int nstrips = a.Cout / 16;
  if (a.Cout < 16 || a.Cout % 16 != 0 || a.B <= 0 || a.Tin <= 0 || a.Tn <= 0 || a.ntaps <= 0 || a.nphase <= 0)
    return ptts_fail(PTTS_E_INVALID, "conv: Cout=%d B=%d Tin=%d Tn=%d taps=%d phases=%d", a.Cout, a.B, a.Tin, a.Tn, a.ntaps, a.nphase);
  if (pl.kernel == DAC_CONV_LDS) {
    const int nw = pl.p[1], ks = pl.p[2], maxhalo = pl.p[3], ft = pl.p[4];
    const int halo = a.transposed ? a.ntaps - 1 : (a.ntaps - 1) * a.dil;
    const bool known = pl.p[0] == 3 && ((nw == 4 && ks == 1 && maxhalo == 54 && (ft == 4 || ft == 8)) || (nw == 2 && ks == 1 && maxhalo == 54 && ft == 8) ||
                                        (nw == 4 && ks == 3 && maxhalo == 2 && (ft == 4 || ft == 8)) || (nw == 2 && ks == 1 && maxhalo == 2 && ft == 8));
    if (!known) return ptts_fail(PTTS_E_UNSUPPORTED, "conv_lds_kernel<%d, %d, %d, %d, %d> is not built", pl.p[0], nw, ks, maxhalo, ft);
    if (a.stride != 1 || nstrips % (3 * nw) != 0 || a.Cin % (32 * ks) != 0 || halo > maxhalo || halo > 54 || (unsigned)(nw * 64) != pl.block ||
        pl.grid_y != (unsigned)(nstrips / (3 * nw)) || pl.grid_x != (unsigned)(((a.Tn + ft * 16 - 1) / (ft * 16)) * a.nphase * a.B))
      return ptts_fail(PTTS_E_UNSUPPORTED, "conv_lds_kernel<3, %d, %d, %d, %d> cannot serve stride %d, %d strips, Cin %d, halo %d", nw, ks, maxhalo, ft, a.stride,
                       nstrips, a.Cin, halo);
  } else if (pl.kernel == DAC_CONV_MFMA) {
    const int CS = pl.p[0], bf = pl.p[1], nwb = pl.p[2];
    if (!(CS == 8 || CS == 6 || CS == 4 || CS == 2 || CS == 1) || !(nwb == 1 || nwb == 2 || nwb == 4) || (bf != 0 && bf != 1))
      return ptts_fail(PTTS_E_UNSUPPORTED, "conv_mfma_kernel<%d, %d> on %d waves is not built", CS, bf, nwb);
    if (nstrips % CS != 0 || a.Cin % (bf ? 32 : 16) != 0 || a.stride < 1 || (unsigned)(64 * nwb) != pl.block || pl.grid_y != (unsigned)(nstrips / CS) ||
        pl.grid_x != (unsigned)(((a.Tn + 32 * nwb - 1) / (32 * nwb)) * a.nphase * a.B))
      return ptts_fail(PTTS_E_UNSUPPORTED, "conv_mfma_kernel<%d, %d> cannot serve %d strips, Cin %d", CS, bf, nstrips, a.Cin);
  } else {
    return ptts_fail(PTTS_E_INVALID, "conv: unknown kernel %d", pl.kernel);
  }
  return PTTS_OK;
}

// launch `pl` on `a` after dac_conv_check
inline int dac_conv_launch(const DacConvPlan& pl, const ConvArgs& a, hipStream_t st) {
  PTTS_TRY(dac_conv_check(pl, a));
  const dim3 grid(pl.grid_x, pl.grid_y), blk(pl.block);
  if (pl.kernel == DAC_CONV_LDS) {
    const int nw = pl.p[1], ks = pl.p[2], maxhalo = pl.p[3], ft = pl.p[4];
    if (ks == 1 && maxhalo == 54) {
      if (nw == 4 && ft == 4) hipLaunchKernelGGL((conv_lds_kernel<3, 4, 1, 54, 4>), grid, blk, 0, st, a);
      else if (nw == 4) hipLaunchKernelGGL((conv_lds_kernel<3, 4, 1, 54>), grid, blk, 0, st, a);
      else hipLaunchKernelGGL((conv_lds_kernel<3, 2, 1, 54>), grid, blk, 0, st, a);
    } else if (ks == 3) {
      if (ft == 4) hipLaunchKernelGGL((conv_lds_kernel<3, 4, 3, 2, 4>), grid, blk, 0, st, a);
      else hipLaunchKernelGGL((conv_lds_kernel<3, 4, 3, 2>), grid, blk, 0, st, a);
    } else {
      hipLaunchKernelGGL((conv_lds_kernel<3, 2, 1, 2>), grid, blk, 0, st, a);
    }
  } else {
    const int CS = pl.p[0], bf = pl.p[1];
#define PTTS_CONV_LAUNCH(CSV)                                                                     \
  do {                                                                                            \
    if (bf) hipLaunchKernelGGL((conv_mfma_kernel<CSV, true>), grid, blk, 0, st, a);               \
    else hipLaunchKernelGGL((conv_mfma_kernel<CSV, false>), grid, blk, 0, st, a);                 \
  } while (0)
    if (CS == 8) PTTS_CONV_LAUNCH(8);
    else if (CS == 6) PTTS_CONV_LAUNCH(6);
    else if (CS == 4) PTTS_CONV_LAUNCH(4);
    else if (CS == 2) PTTS_CONV_LAUNCH(2);
    else PTTS_CONV_LAUNCH(1);
#undef PTTS_CONV_LAUNCH
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ptts_fail(PTTS_E_HIP, "conv launch failed: %s", hipGetErrorString(e));
  return PTTS_OK;
}

// one residual unit (k7 dilated conv -> Snake -> k1 conv -> + skip -> Snake) in one launch? `no_fuse`: the value of PTTS_DAC_NO_FUSE_RES (0 when
// unset) - 1: every unit as two launches; 2: only the C = 384 block's units (round 3's baseline). `alphas`: both convs carry a Snake.
inline bool dac_resunit_fusable(const DacConvShape& c7, const DacConvShape& c1, bool alphas, int no_fuse) {
  const int off = no_fuse;
  const bool on = off != 1;
  // the C = 384 block's units too (8 waves, 100 KB of LDS, one workgroup per CU): batch 32 83.3 -> 77.9 ms, 860 frames 3.39 -> 3.28 ms
  // (profiles/r03_pmc_dac_mfma.txt)
  const bool fuse384 = off != 2;
  return on && c7.bf16 && c1.bf16 && !c7.transposed && !c1.transposed && c7.stride == 1 && c1.stride == 1 && c7.ksize == 7 && c1.ksize == 1 &&
         c7.Cin == c7.Cout && c1.Cin == c7.Cout && c1.Cout == c7.Cout && (c7.Cout == 192 || c7.Cout == 96 || (c7.Cout == 384 && fuse384)) && 6 * c7.dil <= 54 &&
         alphas;
}
// Which widths run their residual units as XIN units (input = the fp32 stream, see resunit_lds_kernel): bit 0: C = 96, bit 1: C = 192, bit 2: C = 384.
// Measured on MI355X (profiles/r06_dac_xin_ab.txt, r06_dac_up_order_ab.txt; ms per decode of 860 frames, mask 0 | 1 | 3 | 7): 32 utterances 56.16 | 54.86 |
// 54.35 | 53.99, 8: - | 14.30 | - | 14.13, 4: - | 7.69 | - | 7.55, one utterance 2.409 | 2.316 | 2.335 | 2.349 - the wider units gain only where the launch
// is bandwidth-bound, hence by the latent frames of the call. `xin_mask`: the value of PTTS_DAC_XIN, negative when unset (every mask gives the same bits).
inline bool dac_resunit_xin_width(int C, long long frames, int xin_mask) {
  const int m = xin_mask >= 0 ? xin_mask : (frames >= 2 * 860 ? 7 : 1);
  return (C == 96 && (m & 1)) || (C == 192 && (m & 2)) || (C == 384 && (m & 4));
}

// resunit_lds_kernel<NW, WD, RAW, F32, XIN, ACT>
struct DacResPlan {
  int NW, WD, RAW, F32, XIN, ACT;
  unsigned grid_x, block, lds;
};
// instances by (width, stream written?, fp32 activation?, input from the stream?, activation written?): compile-time in the kernel (its epilogue is
// straight-line code). The two-register-set weight prefetch (WD = 1, round 3) serves the XIN instances at C = 96 (registers: see the kernel).
inline int dac_resunit_plan(int C, int B, int T, bool raw, bool act_f32, bool xin, bool act, DacResPlan* out) {
  if (!act && !(xin && raw)) return ptts_fail(PTTS_E_INVALID, "residual unit: no activation output");
  if (C != 96 && C != 192 && C != 384) return ptts_fail(PTTS_E_UNSUPPORTED, "residual unit: width %d", C);
  if (act_f32 && C != 96) return ptts_fail(PTTS_E_UNSUPPORTED, "residual unit: fp32 activations only at the last block's width");
  DacResPlan p = {};
  p.NW = C / 48;
  p.WD = xin ? (p.NW == 2 ? ResunitXinWD<2>::value : p.NW == 4 ? ResunitXinWD<4>::value : ResunitXinWD<8>::value) : 3;
  p.XIN = xin ? 1 : 0;
  // (stream written, activation written) of an XIN unit: (1, 0) units 1 and 2 of a block, (0, 1) unit 3, (1, 1) the parity probe's stop stage
  p.RAW = raw ? 1 : 0;
  p.ACT = act ? 1 : 0;
  p.F32 = act && act_f32 ? 1 : 0;
  p.grid_x = (unsigned)(((T + 127) / 128) * B);
  p.block = (unsigned)(p.NW * 64);
  p.lds = (unsigned)(p.NW == 2 ? ResunitLds<2>::bytes : p.NW == 4 ? ResunitLds<4>::bytes : ResunitLds<8>::bytes);
  *out = p;
  return PTTS_OK;
}

// `r.alpha_in` != null: an XIN unit - x is the fp32 stream (= skip) and alpha_in the [alpha | 1 / alpha] of the Snake in front of the unit; out_raw must
// then be a DIFFERENT buffer (neighbouring workgroups read x's halo rows). out_act may be null for a unit whose consumer is an XIN unit.
inline int dac_resunit_launch(const DacResPlan& p, const ResArgs& r, hipStream_t st) {
  const bool raw = r.out_raw != nullptr, xin = r.alpha_in != nullptr, act = r.out_act != nullptr;
  const int C = p.NW * 48;
  if (raw != (p.RAW != 0) || xin != (p.XIN != 0) || act != (p.ACT != 0) || (act && (r.act_f32 != 0) != (p.F32 != 0)) || r.a.Cin != C || r.a.Cout != C ||
      r.a.ntaps != 7 || r.a.nphase != 1 || r.a.stride != 1 || r.a.transposed || 6 * r.a.dil > 54 || r.a.pad != 3 * r.a.dil || r.a.Tn != r.a.Tin ||
      p.grid_x != (unsigned)(((r.a.Tin + 127) / 128) * r.a.B) || p.block != (unsigned)(p.NW * 64) || !r.skip)
    return ptts_fail(PTTS_E_UNSUPPORTED, "resunit_lds_kernel<%d, %d, %d, %d, %d, %d> cannot serve C=%d dil=%d raw=%d act=%d f32=%d xin=%d", p.NW, p.WD, p.RAW,
                     p.F32, p.XIN, p.ACT, r.a.Cout, r.a.dil, (int)raw, (int)act, r.act_f32, (int)xin);
  if (xin && ((const void*)r.skip != r.a.x || (const void*)r.out_raw == r.a.x))
    return ptts_fail(PTTS_E_INVALID, "residual unit on the stream: x must be the skip buffer, out_raw another one");
  const dim3 grid(p.grid_x);
#define PTTS_RU_LAUNCH(NWV, RAWV, F32V) \
  hipLaunchKernelGGL((resunit_lds_kernel<NWV, 3, RAWV, F32V>), grid, dim3(NWV * 64), ResunitLds<NWV>::bytes, st, r)
#define PTTS_RU_LAUNCH_XIN(NWV, RAWV, F32V, ACTV) \
  hipLaunchKernelGGL((resunit_lds_kernel<NWV, ResunitXinWD<NWV>::value, RAWV, F32V, true, ACTV>), grid, dim3(NWV * 64), ResunitLds<NWV>::bytes, st, r)
#define PTTS_RU_XIN_BY_OUT(NWV, F32V)                                   \
  do {                                                                  \
    if (raw && !act) PTTS_RU_LAUNCH_XIN(NWV, true, false, false);       \
    else if (raw) PTTS_RU_LAUNCH_XIN(NWV, true, F32V, true);            \
    else PTTS_RU_LAUNCH_XIN(NWV, false, F32V, true);                    \
  } while (0)
  if (C == 384) {
    static PttsPerDeviceOnce attr_once;  // 100 KB of dynamic LDS needs the opt-in
    const int attr_dev = PttsPerDeviceOnce::device();
    if (attr_once.need(attr_dev)) {
      constexpr int WDX = ResunitXinWD<8>::value;
      const void* fns[] = {reinterpret_cast<const void*>(&resunit_lds_kernel<8, 3, true, false>), reinterpret_cast<const void*>(&resunit_lds_kernel<8, 3, false, false>),
                           reinterpret_cast<const void*>(&resunit_lds_kernel<8, WDX, true, false, true, false>),
                           reinterpret_cast<const void*>(&resunit_lds_kernel<8, WDX, true, false, true, true>),
                           reinterpret_cast<const void*>(&resunit_lds_kernel<8, WDX, false, false, true, true>)};
      for (const void* fn : fns) {
        const hipError_t ea = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, ResunitLds<8>::bytes);
        if (ea != hipSuccess) return ptts_fail(PTTS_E_HIP, "hipFuncSetAttribute(max dynamic LDS) failed: %s", hipGetErrorString(ea));
      }
      attr_once.done(attr_dev);
    }
    if (xin) PTTS_RU_XIN_BY_OUT(8, false);
    else if (raw) PTTS_RU_LAUNCH(8, true, false); else PTTS_RU_LAUNCH(8, false, false);
  } else if (C == 192) {
    if (xin) PTTS_RU_XIN_BY_OUT(4, false);
    else if (raw) PTTS_RU_LAUNCH(4, true, false); else PTTS_RU_LAUNCH(4, false, false);
  } else if (r.act_f32) {
    if (xin) PTTS_RU_XIN_BY_OUT(2, true);
    else if (raw) PTTS_RU_LAUNCH(2, true, true); else PTTS_RU_LAUNCH(2, false, true);
  } else {
    if (xin) PTTS_RU_XIN_BY_OUT(2, false);
    else if (raw) PTTS_RU_LAUNCH(2, true, false); else PTTS_RU_LAUNCH(2, false, false);
  }
#undef PTTS_RU_XIN_BY_OUT
#undef PTTS_RU_LAUNCH_XIN
#undef PTTS_RU_LAUNCH
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ptts_fail(PTTS_E_HIP, "residual-unit launch failed: %s", hipGetErrorString(e));
  return PTTS_OK;
}

// final Conv1d(C -> 1, k7) + tanh: LDS-tiled at the 44.1 kHz width, otherwise the per-thread kernel
struct DacOutPlan {
  int lds_kernel;
  unsigned grid_x, grid_y, block, lds;
};
inline DacOutPlan dac_conv_out_plan(int C, int B, int T, bool force_direct = false) {
  DacOutPlan p = {};
  if (C == OUT_C && B <= 65535 && !force_direct) {
    p.lds_kernel = 1; p.grid_x = (unsigned)((T + OUT_TILE - 1) / OUT_TILE); p.grid_y = (unsigned)B; p.block = OUT_TILE; p.lds = 0;
  } else {
    const size_t n = (size_t)B * ((T + OUT_OS - 1) / OUT_OS);
    p.lds_kernel = 0; p.grid_x = (unsigned)((n + 255) / 256); p.grid_y = 1; p.block = 256; p.lds = (unsigned)((size_t)7 * C * 4);
  }
  return p;
}
template <bool ROWS>
inline int dac_conv_out_launch(const DacOutPlan& p, const float* x, const float* w, const float* bias, float* out, int B, int T, int C,
                               typename EmitArg<ROWS>::T skip_of, long long out_ld, typename EmitArg<ROWS>::T t_end_of, const int* lens, int len_mul,
                               hipStream_t st) {
  if (p.lds_kernel) {
    if (C != OUT_C || B > 65535) return ptts_fail(PTTS_E_UNSUPPORTED, "conv_out_tanh_lds_kernel serves C = %d and B <= 65535 (C=%d B=%d)", OUT_C, C, B);
    hipLaunchKernelGGL((conv_out_tanh_lds_kernel<ROWS>), dim3(p.grid_x, p.grid_y), dim3(p.block), 0, st, x, w, bias, out, T, skip_of, out_ld, t_end_of, lens,
                       len_mul);
  } else {
    if (C % 4 != 0) return ptts_fail(PTTS_E_UNSUPPORTED, "conv_out_tanh_kernel: C = %d is no multiple of 4", C);
    hipLaunchKernelGGL((conv_out_tanh_kernel<ROWS>), dim3(p.grid_x), dim3(p.block), p.lds, st, x, w, bias, out, B, T, C, 7, skip_of, out_ld, t_end_of, lens,
                       len_mul);
  }
  return PTTS_OK;
}

// The pack kernels' view of a checkpoint weight: the per-phase tap table ktap[phase * MAXTAPS + tap] -> kernel index (a plain conv, one phase,
// may use up to 16 entries of row 0 / 1) and the strides of element (co, ci, k) in the source.
struct DacPackPlan {
  int ktap[MAXTAPS * 8];
  long long s_co, s_ci, s_k;
  int ntaps, nphase;
};
inline DacPackPlan dac_pack_plan(const DacConvShape& L) {
  DacPackPlan p;
  memset(p.ktap, 0, sizeof p.ktap);
  const int k = L.ksize;
  p.s_k = 1;
  if (!L.transposed) {  // torch Conv1d weight [Cout][Cin][k]
    p.s_co = (long long)L.Cin * k; p.s_ci = k; p.ntaps = k; p.nphase = 1;
    for (int t = 0; t < k; ++t) p.ktap[t] = t;
  } else {  // torch ConvTranspose1d weight [Cin][Cout][2s]
    p.s_ci = (long long)L.Cout * k; p.s_co = k; p.ntaps = 2; p.nphase = L.stride;
    const int s = L.stride, pad = (s + 1) / 2;
    for (int ph = 0; ph < s; ++ph) { const int r = (ph + pad) % s; p.ktap[ph * MAXTAPS + 0] = r; p.ktap[ph * MAXTAPS + 1] = r + s; }
  }
  return p;
}
// pack `src` (the checkpoint's layout) into `Wp`; `d_ktap` (MAXTAPS * 8 ints on the device) must hold p.ktap when the kernel runs
inline void dac_pack_launch(const DacConvShape& L, const DacPackPlan& p, const float* src, void* Wp, const int* d_ktap, hipStream_t st) {
  const size_t total = (size_t)p.nphase * (L.Cout / 16) * p.ntaps * (L.Cin / 16) * 64;
  if (L.bf16) {
    const size_t tb = (size_t)p.nphase * (L.Cout / 16) * p.ntaps * (L.Cin / 32) * 64;
    hipLaunchKernelGGL(pack_conv_bf16_kernel, dim3((unsigned)((tb + 255) / 256)), dim3(256), 0, st, src, reinterpret_cast<bf16_t*>(Wp), L.Cout,
                       L.Cin, p.ntaps, p.nphase, d_ktap, p.s_co, p.s_ci, p.s_k);
  } else {
    hipLaunchKernelGGL(pack_conv_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, src, reinterpret_cast<float*>(Wp), L.Cout, L.Cin, p.ntaps,
                       p.nphase, d_ktap, p.s_co, p.s_ci, p.s_k);
  }
}

}  // namespace
