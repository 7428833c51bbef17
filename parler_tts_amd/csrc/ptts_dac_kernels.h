// The DAC codec's device code - argument structs, snake_f, the convolution / residual-unit / final-convolution kernels, the RVQ kernels and the
// weight pack kernels - apart from ptts_dac.hip so that tests/native/dac_harness.hip launches the same code on buffers of its own. The kernels
// live in an unnamed namespace, as they did in that file: every includer gets instances of its own. Host dispatch: ptts_dac_launch.h.
#pragma once
#include <limits.h>

#include <type_traits>

#include "ptts_common.h"

namespace {

constexpr int MAXTAPS = 8;

struct ConvArgs {
  const void* x;       // activated input, channels-last [B][Tin][Cin]: fp32, or bf16 in the bf16-operand mode
  const void* Wp;      // packed [phase][Cout/16][ntaps*Cin/16][64][4] fp32, or [..][ntaps*Cin/32][64][8] bf16
  const float* bias;   // [Cout]
  const float* skip;   // optional residual [B][Tout][Cout] (may alias out_raw)
  float* out_raw;      // optional
  void* out_act;       // optional: snake(alpha) of the result (bf16 in the bf16-operand mode unless act_f32)
  int act_f32;         // bf16 mode: write out_act as fp32 (the layer feeding the final Conv1d(C -> 1) + tanh)
  const float* alpha;  // [Cout] for out_act
  int dil, pad, transposed;  // tap offset: conv  tap*dil - pad ; transposed (stride = nphase)  (ph + pad)/nphase - tap
  int B, Tin, Cin, Cout, ntaps, nphase;
  int stride, Tn;      // input stride of a down-sampling conv (else 1); output frames per phase (Tin unless strided)
  const int* lens;     // ragged decode (ptts_dac_decode_ragged): latent frames per utterance [B] on the device, or null. Utterance b then has
  int len_mul;         // lens[b] * len_mul valid input rows (= output rows per phase): rows beyond read as the zero padding, tiles beyond exit
};

// valid input rows of utterance b (buffers keep the full stride a.Tin)
__device__ __forceinline__ int valid_rows(const ConvArgs& a, int b) { return a.lens ? min(a.Tin, max(a.lens[b], 0) * a.len_mul) : a.Tin; }  // lengths clamped to [0, T]

// FAST (bf16-operand mode, whose activations are rounded to bf16 anyway): v_sin_f32 on a*x / 2pi instead of the ~100-instruction
// exact sinf - the Snake epilogue of the 42 M-element layers was ~100 us of VALU per layer (profiles/r02_dac_layers.txt).
// inv = 1.0f / (al + 1e-9f), computed ONCE per channel at load time (inv_alpha_kernel: the same correctly rounded fp32 division the
// epilogues evaluated per element - ~10 VALU instructions beside a sin; the Snake of the fused units was 7.3 ms of a 69 ms batch-32 decode,
// profiles/r04_experiments.txt call 8). Stored right behind the alphas: alpha[C + c].
template <bool FAST>
__device__ __forceinline__ float snake_f(float x, float al, float inv) {
  float s;
  if constexpr (FAST) s = __sinf(al * x);
  else s = sinf(al * x);
  return x + inv * (s * s);
}
__device__ __forceinline__ float4 ld_inv4(const float* alpha, int C, int c) { return *reinterpret_cast<const float4*>(alpha + C + c); }
__global__ void inv_alpha_kernel(float* __restrict__ alpha, int C) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < C) alpha[C + i] = 1.0f / (alpha[i] + 1e-9f);
}

// workgroup: 4 waves = 4 consecutive 32-frame tiles; every wave owns the SAME CS 16-channel output strips (CS = 6 or 8
// divides every decoder width / 16: 96, 48, 24, 12, 6 strips), so each activation fragment is reused CS times from
// registers and the 4 waves read identical weight fragments (L1 broadcast). First mapping (waves over strips, one
// shared tile) left 25 % of the waves idle on the 6/12/24-strip layers and ran at 43 % of the f32-MFMA peak.
// BF: bf16 MFMA operands (v_mfma_f32_16x16x32_bf16: 32 channels per step, activations and weights stored in bf16), fp32
// accumulate, bias / skip / Snake in fp32 - at least the precision of the reference run in bf16, where every conv output
// is rounded to bf16. BF = false is the exact-f32 parity mode.
template <int CS, bool BF>
__global__ void __launch_bounds__(256) conv_mfma_kernel(ConvArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = lane >> 4, j = lane & 15;
  const int fpb = 32 * (int)(blockDim.x >> 6);  // frames per workgroup: 32 per wave, 1/2/4 waves (host picks for balance)
  const int ntile = (a.Tn + fpb - 1) / fpb;
  const int tile = blockIdx.x % ntile, ph = (blockIdx.x / ntile) % a.nphase, b = blockIdx.x / (ntile * a.nphase);
  const int strip0 = blockIdx.y * CS;
  const int nstrips = a.Cout / 16;
  const int Tv = valid_rows(a, b), Tnv = a.lens ? Tv : a.Tn;  // ragged decode: this utterance's rows
  if (tile * fpb + wave * 32 >= Tnv) return;
  constexpr int KC = BF ? 32 : 16;      // channels per k-step
  const int cpt = a.Cin / KC;           // k-steps per tap
  const int nk = a.ntaps * cpt;
  const char* xb = reinterpret_cast<const char*>(a.x) + (size_t)b * a.Tin * a.Cin * (BF ? 2 : 4);
  const float4* Wp = reinterpret_cast<const float4*>(a.Wp) + ((size_t)ph * nstrips * nk) * 64 + lane;  // 16 B per lane either way
  const int j0 = tile * fpb + wave * 32;

  f32x4 acc[CS][2];
#pragma unroll
  for (int s = 0; s < CS; ++s) { acc[s][0] = f32x4{0, 0, 0, 0}; acc[s][1] = f32x4{0, 0, 0, 0}; }

  // software-pipelined k loop over (tap, 16-channel chunk): the fragments of step ks+1 are in flight while the
  // 8*CS MFMAs of step ks issue (measured: neutral, 65.5 -> 66.9 TFLOP/s -- L2 latency was already hidden by occupancy)
  const int nks = nk;
  // (a macro, not a lambda: array-by-reference parameters kept the CS = 8 fragment arrays in scratch)
#define PTTS_DAC_LOAD_STEP(KS, WF, B0, B1)                                                                              \
  do {                                                                                                                  \
    const int tap_ = (KS) / cpt, cc_ = (KS) - tap_ * cpt;                                                                \
    const int off_ = a.transposed ? (ph + a.pad) / a.nphase - tap_ : tap_ * a.dil - a.pad;                               \
    const int ti0_ = (j0 + j) * a.stride + off_, ti1_ = ti0_ + 16 * a.stride;                                            \
    B0 = make_float4(0, 0, 0, 0);                                                                                        \
    B1 = make_float4(0, 0, 0, 0);                                                                                        \
    if (ti0_ >= 0 && ti0_ < Tv) B0 = *reinterpret_cast<const float4*>(xb + ((size_t)ti0_ * a.Cin + cc_ * KC) * (BF ? 2 : 4) + q * 16);  \
    if (ti1_ >= 0 && ti1_ < Tv) B1 = *reinterpret_cast<const float4*>(xb + ((size_t)ti1_ * a.Cin + cc_ * KC) * (BF ? 2 : 4) + q * 16);  \
    _Pragma("unroll") for (int s_ = 0; s_ < CS; ++s_) WF[s_] = Wp[((size_t)(strip0 + s_) * nk + (KS)) * 64];             \
  } while (0)
  float4 wf[CS], b0, b1;
  PTTS_DAC_LOAD_STEP(0, wf, b0, b1);
  for (int ks = 0; ks < nks; ++ks) {
    float4 wn[CS], n0, n1;
    if (ks + 1 < nks) PTTS_DAC_LOAD_STEP(ks + 1, wn, n0, n1);
#pragma unroll
    for (int s = 0; s < CS; ++s) {
      if constexpr (BF) {
        acc[s][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wf[s]), __builtin_bit_cast(bf16x8, b0), acc[s][0], 0, 0, 0);
        acc[s][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wf[s]), __builtin_bit_cast(bf16x8, b1), acc[s][1], 0, 0, 0);
      } else {
        acc[s][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s].x, b0.x, acc[s][0], 0, 0, 0);
        acc[s][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s].x, b1.x, acc[s][1], 0, 0, 0);
        acc[s][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s].y, b0.y, acc[s][0], 0, 0, 0);
        acc[s][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s].y, b1.y, acc[s][1], 0, 0, 0);
        acc[s][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s].z, b0.z, acc[s][0], 0, 0, 0);
        acc[s][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s].z, b1.z, acc[s][1], 0, 0, 0);
        acc[s][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s].w, b0.w, acc[s][0], 0, 0, 0);
        acc[s][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s].w, b1.w, acc[s][1], 0, 0, 0);
      }
    }
    if (ks + 1 < nks) {
#pragma unroll
      for (int s = 0; s < CS; ++s) wf[s] = wn[s];
      b0 = n0;
      b1 = n1;
    }
  }
  // epilogue: D[row = co_local = q*4 + r][col = frame j]. A helper called with compile-time (s, half) keeps `acc`
  // statically indexed: the big inlined snake bodies otherwise stop the unroller at CS = 8 and push acc to scratch.
  const int Tout = a.Tn * a.nphase;
  auto emit = [&](const f32x4& av, int s, int half) {
    const int jj = j0 + half * 16 + j;
    if (jj >= Tnv) return;
    const int co = (strip0 + s) * 16 + q * 4;
    const float4 bs = *reinterpret_cast<const float4*>(a.bias + co);
    const size_t o = ((size_t)b * Tout + (size_t)jj * a.nphase + ph) * a.Cout + co;
    float4 v = make_float4(av[0] + bs.x, av[1] + bs.y, av[2] + bs.z, av[3] + bs.w);
    if (a.skip) {
      const float4 sk = *reinterpret_cast<const float4*>(a.skip + o);
      v.x += sk.x; v.y += sk.y; v.z += sk.z; v.w += sk.w;
    }
    if (a.out_raw) *reinterpret_cast<float4*>(a.out_raw + o) = v;
    if (a.out_act) {
      const float4 al = *reinterpret_cast<const float4*>(a.alpha + co), ia = ld_inv4(a.alpha, a.Cout, co);
      const float4 sv = make_float4(snake_f<BF>(v.x, al.x, ia.x), snake_f<BF>(v.y, al.y, ia.y), snake_f<BF>(v.z, al.z, ia.z), snake_f<BF>(v.w, al.w, ia.w));
      if (BF && !a.act_f32) *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(a.out_act) + o) = make_uint2(pack_bf16x2(sv.x, sv.y), pack_bf16x2(sv.z, sv.w));
      else *reinterpret_cast<float4*>(reinterpret_cast<float*>(a.out_act) + o) = sv;
    }
  };
  if (CS >= 1) { emit(acc[0][0], 0, 0); emit(acc[0][1], 0, 1); }
  if (CS >= 2) { emit(acc[1 % CS][0], 1, 0); emit(acc[1 % CS][1], 1, 1); }
  if (CS >= 4) { emit(acc[2 % CS][0], 2, 0); emit(acc[2 % CS][1], 2, 1); emit(acc[3 % CS][0], 3, 0); emit(acc[3 % CS][1], 3, 1); }
  if (CS >= 6) { emit(acc[4 % CS][0], 4, 0); emit(acc[4 % CS][1], 4, 1); emit(acc[5 % CS][0], 5, 0); emit(acc[5 % CS][1], 5, 1); }
  if (CS >= 8) { emit(acc[6 % CS][0], 6, 0); emit(acc[6 % CS][1], 6, 1); emit(acc[7 % CS][0], 7, 0); emit(acc[7 % CS][1], 7, 1); }
}

// The staged-slab MFMA accumulation of conv_lds_kernel and of resunit_lds_kernel's k7 phase, written once:
//   acc[s][f] += sum over (chunk c, tap, kk) of W[strip s][tap][c * KCH + kk * 32 ..] * x[frame tile f + rel(tap)][same channels]
// for the calling wave's CSW strips and the workgroup's FT 16-frame tiles. `slab`: two buffers of MAXROWS * RS bytes in LDS; `xb`: the utterance's
// activation rows; `Wp`: the packed fragments of this wave's first strip (+ lane), strips nk * 64 float4 apart. Every thread of the workgroup calls it
// (barriers inside); the last chunk's barrier has retired every slab read when it returns.
//   * chunk c + 1 is fetched into the staging registers at step 0 of chunk c and committed to the other buffer before the ONE barrier of the chunk;
//   * weight fragments are requested WD k-steps ahead, also across chunks, into WD + 1 register sets that ROTATE (never copied: a copy makes the
//     compiler wait for the loads it has just issued). WD = 3: four sets; WD = 1: two sets, where the registers do not reach (see ResunitXinWD).
//     A k-step is 24 MFMAs = 384 cycles per wave, ~770 with the SIMD's second wave interleaved: one step ahead is ~0.3 us, less than an L2 round
//     trip - and the fragments DO come from the L2 every time (a wave re-streams its 3 strips x 7 taps x C channels = 129 KB at C = 192 per tile
//     through a 32 KB L1 shared by 8 waves), so with WD = 1 every k-step waited for its weights: MFMA pipe 23-28 % busy (profiles/r03_pmc_dac_mfma.txt);
//   * B fragments are read in two halves of FT / 2 frame tiles, each half in flight under the other half's MFMAs.
// XIN: `xb` is the fp32 residual stream; a staged slot is 32 bytes of it (two uint4) that become the slot's 16 bytes of bf16 at commit time
// (Snake with `s_ain` = [alpha | 1 / (alpha + 1e-9)] of all Cin channels in LDS, rounded once). Rows outside the utterance read as zeros either
// way (Snake(0) = 0: the conv's zero padding).
// C7 = 0: channels, taps, dilation and the transposed conv's phase addressing (`ph`) come from `a` at run time (conv_lds_kernel). C7 = C: a plain k7
// conv over C channels (the residual unit): k-steps per chunk, chunks and their product are compile-time constants.
template <int CSW, int NW, int KS, int FT, int MAXHALO, int WD, bool XIN, int C7>
__device__ __forceinline__ void slab_mfma_loop(f32x4 (&acc)[CSW][FT], unsigned char* const slab, const float* const s_ain, const ConvArgs& a,
                                               const char* const xb, const float4* const Wp, const int nk, const int t0, const int Tv, const int ph) {
  static_assert(FT == 8 || FT == 4, "frame tiles per workgroup");
  static_assert(WD == 3 || WD == 1, "weight prefetch depth: four or two rotating register sets");
  constexpr int TF = FT * 16, HF = FT / 2;
  constexpr int KCH = 32 * KS;          // channels per staged chunk
  constexpr int RS = KS * 64 + 32;      // slab row stride in bytes: RS / 32 is odd (conflict-free ds_read_b128 for any row base)
  constexpr int SL = KS * 4;            // 16-byte slots per slab row
  constexpr int NT = NW * 64;
  constexpr int MAXROWS = TF + MAXHALO;
  constexpr int NST = (MAXROWS * SL + NT - 1) / NT;  // staged slots per thread and chunk
  constexpr bool K7 = C7 != 0;
  static_assert(C7 % KCH == 0, "chunk width");
  const int tid = threadIdx.x, q = (tid & 63) >> 4, j = tid & 15;
  const int Cin = K7 ? C7 : a.Cin;
  const int cpt = Cin / 32, nchunk = Cin / KCH;
  const int NS = (K7 ? 7 : a.ntaps) * KS;  // k-steps per chunk
  const int total = nchunk * NS;
  // slab row r holds input frame t0 + o0 + r; tap `tap` of output frame t0 + f reads row f + rel(tap)
  const bool tr = !K7 && a.transposed;
  const int o0 = tr ? (ph + a.pad) / a.nphase - (a.ntaps - 1) : -a.pad;
  const int halo = tr ? a.ntaps - 1 : (a.ntaps - 1) * a.dil;
  const int nslot = (TF + halo) * SL;
  const int lrow = j * RS + q * 16;

  uint4 stg[XIN ? 2 * NST : NST];
#define PTTS_SLAB_FETCH(C)                                                                                              \
  _Pragma("unroll") for (int i_ = 0; i_ < NST; ++i_) {                                                                    \
    const int idx_ = tid + i_ * NT, r_ = idx_ / SL, sl_ = idx_ - r_ * SL, ti_ = t0 + o0 + r_;                              \
    const bool ok_ = idx_ < nslot && ti_ >= 0 && ti_ < Tv;                                                                \
    if constexpr (XIN) {                                                                                                  \
      stg[2 * i_] = make_uint4(0, 0, 0, 0); stg[2 * i_ + 1] = make_uint4(0, 0, 0, 0);                                     \
      if (ok_) {                                                                                                          \
        const uint4* p_ = reinterpret_cast<const uint4*>(xb + ((size_t)ti_ * Cin + (size_t)(C) * KCH) * 4 + sl_ * 32);    \
        stg[2 * i_] = p_[0]; stg[2 * i_ + 1] = p_[1];                                                                     \
      }                                                                                                                   \
    } else {                                                                                                              \
      stg[i_] = make_uint4(0, 0, 0, 0);                                                                                   \
      if (ok_) stg[i_] = *reinterpret_cast<const uint4*>(xb + ((size_t)ti_ * Cin + (size_t)(C) * KCH) * 2 + sl_ * 16);    \
    }                                                                                                                     \
  }
#define PTTS_SLAB_COMMIT(BUFP, C)                                                                                       \
  {                                                                                                                     \
    float4 al0_, al1_, ia0_, ia1_;                                                                                        \
    if constexpr (XIN) {  /* the thread's slot column is the same for every i_ (NT % SL == 0): 8 channels of chunk C */    \
      const float* ap_ = s_ain + (C) * KCH + (tid % SL) * 8;                                                              \
      al0_ = *reinterpret_cast<const float4*>(ap_); al1_ = *reinterpret_cast<const float4*>(ap_ + 4);                      \
      ia0_ = *reinterpret_cast<const float4*>(ap_ + Cin); ia1_ = *reinterpret_cast<const float4*>(ap_ + Cin + 4);          \
    }                                                                                                                     \
    _Pragma("unroll") for (int i_ = 0; i_ < NST; ++i_) {                                                                  \
      const int idx_ = tid + i_ * NT, r_ = idx_ / SL, sl_ = idx_ - r_ * SL;                                                \
      uint4 v_;                                                                                                           \
      if constexpr (XIN) {                                                                                                \
        const uint4 lo_ = stg[2 * i_], hi_ = stg[2 * i_ + 1];                                                             \
        v_ = make_uint4(pack_bf16x2(snake_f<true>(__uint_as_float(lo_.x), al0_.x, ia0_.x), snake_f<true>(__uint_as_float(lo_.y), al0_.y, ia0_.y)), \
                        pack_bf16x2(snake_f<true>(__uint_as_float(lo_.z), al0_.z, ia0_.z), snake_f<true>(__uint_as_float(lo_.w), al0_.w, ia0_.w)), \
                        pack_bf16x2(snake_f<true>(__uint_as_float(hi_.x), al1_.x, ia1_.x), snake_f<true>(__uint_as_float(hi_.y), al1_.y, ia1_.y)), \
                        pack_bf16x2(snake_f<true>(__uint_as_float(hi_.z), al1_.z, ia1_.z), snake_f<true>(__uint_as_float(hi_.w), al1_.w, ia1_.w))); \
      } else {                                                                                                            \
        v_ = stg[i_];                                                                                                     \
      }                                                                                                                   \
      if (idx_ < nslot) *reinterpret_cast<uint4*>((BUFP) + r_ * RS + sl_ * 16) = v_;                                       \
    }                                                                                                                     \
  }
  // weight fragments of global k-step G = chunk * NS + step: ks = tap * cpt + chunk * KS + kk
#define PTTS_W_FETCH(WF, G)                                                                                             \
  do {                                                                                                                  \
    const int c_ = (G) / NS, s_ = (G) - c_ * NS, tap_ = s_ / KS, kk_ = s_ - tap_ * KS;                                    \
    const float4* wp_ = Wp + (size_t)(tap_ * cpt + c_ * KS + kk_) * 64;                                                   \
    _Pragma("unroll") for (int w_ = 0; w_ < CSW; ++w_) WF[w_] = wp_[(size_t)w_ * nk * 64];                               \
  } while (0)
  // B fragments (HF frame tiles from F0) of step S out of buffer SB
#define PTTS_B_FETCH(BV, SB, S, F0)                                                                                     \
  do {                                                                                                                  \
    const int tap_ = (S) / KS, kk_ = (S) - tap_ * KS;                                                                     \
    const int rel_ = tr ? (a.ntaps - 1 - tap_) : tap_ * a.dil;                                                            \
    const unsigned char* sp_ = (SB) + (rel_ + (F0) * 16) * RS + kk_ * 64 + lrow;                                          \
    _Pragma("unroll") for (int f_ = 0; f_ < HF; ++f_) BV[f_] = *reinterpret_cast<const uint4*>(sp_ + f_ * 16 * RS);       \
  } while (0)
#define PTTS_MFMA_HALF(WC, BV, F0)                                                                                      \
  _Pragma("unroll") for (int f_ = 0; f_ < HF; ++f_) _Pragma("unroll") for (int s_ = 0; s_ < CSW; ++s_)                     \
    acc[s_][(F0) + f_] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, WC[s_]), __builtin_bit_cast(bf16x8, BV[f_]), acc[s_][(F0) + f_], 0, 0, 0);
  // One k-step: MFMAs of (chunk c, step st) with the weight fragments WC while WN receives those of k-step gi + WD (possibly of a later chunk).
  // That fetch is unconditional (a valid re-fetch of the last k-step at the very end): a branch here would merge into a conservative vmcnt on
  // the MFMAs below. The last step of a chunk commits the staged slab and holds the chunk's barrier.
#define PTTS_STEP(WC, WN)                                                                                               \
  {                                                                                                                     \
    const unsigned char* sb_ = slab + (c & 1) * (MAXROWS * RS);                                                           \
    unsigned char* nb_ = slab + ((c + 1) & 1) * (MAXROWS * RS);                                                           \
    const bool more_ = c + 1 < nchunk, lastst_ = st + 1 == NS;                                                            \
    if (st == 0 && more_) { PTTS_SLAB_FETCH(c + 1); }                                                                     \
    PTTS_W_FETCH(WN, min(gi + WD, total - 1));                                                                            \
    PTTS_B_FETCH(bB, sb_, st, HF);                                                                                        \
    PTTS_MFMA_HALF(WC, bA, 0)                                                                                             \
    if (!lastst_) PTTS_B_FETCH(bA, sb_, st + 1, 0);                                                                       \
    PTTS_MFMA_HALF(WC, bB, HF)                                                                                            \
    if (lastst_) {                                                                                                        \
      if (more_) { PTTS_SLAB_COMMIT(nb_, c + 1); }                                                                        \
      __syncthreads();                                                                                                    \
      if (more_) PTTS_B_FETCH(bA, nb_, 0, 0);                                                                             \
      ++c;                                                                                                                \
      st = 0;                                                                                                             \
    } else {                                                                                                              \
      ++st;                                                                                                               \
    }                                                                                                                     \
    ++gi;                                                                                                                 \
  }
  float4 w0[CSW], w1[CSW], w2[CSW], w3[CSW];  // WD = 3: k-step g computes out of w[g % 4] while the fragments of k-step g + 3 land in w[(g + 3) % 4]
  uint4 bA[HF], bB[HF];
  PTTS_W_FETCH(w0, 0);
  if constexpr (WD == 3) {
    PTTS_W_FETCH(w1, min(1, total - 1));
    PTTS_W_FETCH(w2, min(2, total - 1));
  }
  PTTS_SLAB_FETCH(0);
  PTTS_SLAB_COMMIT(slab, 0);
  __syncthreads();
  PTTS_B_FETCH(bA, slab, 0, 0);
  int c = 0, st = 0, gi = 0;
  if constexpr (WD == 3) {
    for (int g = 0; g < total; g += 4) {
      PTTS_STEP(w0, w3)
      if (g + 1 < total) PTTS_STEP(w1, w0)
      if (g + 2 < total) PTTS_STEP(w2, w1)
      if (g + 3 < total) PTTS_STEP(w3, w2)
    }
  } else {
    for (int g = 0; g < total; g += 2) {
      PTTS_STEP(w0, w1)
      if (g + 1 < total) PTTS_STEP(w1, w0)
    }
  }
#undef PTTS_STEP
#undef PTTS_MFMA_HALF
#undef PTTS_B_FETCH
#undef PTTS_W_FETCH
#undef PTTS_SLAB_COMMIT
#undef PTTS_SLAB_FETCH
}

// LDS-tiled variant of the bf16-operand kernel for the stride-1 layers of the 44.1 kHz stack (k7 dilated convs, k1 convs,
// the 2-tap phases of the transposed convs): the kernel above fetches every activation fragment from L1/L2 once per TAP and
// every weight fragment once per WAVE (10 KB per wave per 256 MFMA cycles = 160 B/clk/CU asked of a 64 B/clk L1), and ran at
// 10 % of the bf16 MFMA peak. Here a workgroup owns 128 consecutive frames x NW*CSW 16-channel strips:
//   * the activation slab of one KCH-channel chunk ([128 + halo] rows x KCH bf16, KCH = 32 * KS) is staged ONCE into LDS and read by all
//     taps (7x fewer global reads) and all waves; rows are RS = KCH*2 + 32 bytes apart: RS/32 is odd, so the 16 lanes of each
//     ds_read_b128 service group land on 16 distinct 16-byte bank slots for ANY row base (the tap offset tap*dil is arbitrary);
//   * waves split the output strips (CSW each) and share the frames, so every wave's weight fragments are its own: CSW KB
//     per wave per k-step from L2/L1 (24 B/clk/CU at CSW = 3), prefetched three k-steps ahead in registers, also across chunks;
//   * two LDS buffers, one barrier per chunk, B fragments in two halves: slab_mfma_loop above, shared with resunit_lds_kernel.
// Per k-step and wave: 24 MFMAs 16x16x32 (384 cycles) against 8 ds_read_b128 + 3 global 16-B loads.
// MAXHALO: the largest (ntaps - 1) * dil the instance serves (sizes the slab).
// FT (round 5): 16-frame tiles per workgroup - 8 (128 frames), or 4 where 128-frame tiles leave the launch with fewer than two workgroups per CU (the
// first block of a single utterance: 56-224 workgroups on 256 CUs; the short windows of the streamer). Same k order per output: bit-identical.
template <int CSW, int NW, int KS, int MAXHALO, int FT = 8>
__global__ void __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(2, 2))) conv_lds_kernel(ConvArgs a) {
  constexpr int TF = FT * 16, RS = KS * 64 + 32, NT = NW * 64, MAXROWS = TF + MAXHALO;  // as slab_mfma_loop's
  __shared__ __attribute__((aligned(16))) unsigned char slab[2][MAXROWS * RS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = lane >> 4, j = lane & 15;
  const int ntile = (a.Tn + TF - 1) / TF;
  // (round 6, profiles/r06_dac_up_order_ab.txt: the phases of a transposed conv as neighbours in ONE XCD's queue - sharing its L2 copy of the input tile -
  //  or the phase as the slowest index - one phase's weights L2-resident at a time - measured equal to this order, 54.2-54.7 vs 53.8-54.2 ms per batch-32
  //  decode, bit-identical: the re-fetched bytes the PMC table shows for these layers do not cost time. Not kept.)
  const int tile = blockIdx.x % ntile, ph = (blockIdx.x / ntile) % a.nphase, b = blockIdx.x / (ntile * a.nphase);
  const int nstrips = a.Cout / 16;
  const int strip0 = (blockIdx.y * NW + wave) * CSW;
  const int nk = a.ntaps * (a.Cin / 32);
  const int t0 = tile * TF;
  const int Tv = valid_rows(a, b), Tnv = a.lens ? Tv : a.Tn;  // ragged decode: this utterance's rows (workgroup-uniform)
  if (t0 >= Tnv) return;
  const char* xb = reinterpret_cast<const char*>(a.x) + (size_t)b * a.Tin * a.Cin * 2;
  const float4* Wp = reinterpret_cast<const float4*>(a.Wp) + ((size_t)ph * nstrips + strip0) * nk * 64 + lane;

  f32x4 acc[CSW][FT];
#pragma unroll
  for (int s = 0; s < CSW; ++s)
#pragma unroll
    for (int f = 0; f < FT; ++f) acc[s][f] = f32x4{0, 0, 0, 0};
  slab_mfma_loop<CSW, NW, KS, FT, MAXHALO, 3, false, 0>(acc, &slab[0][0], nullptr, a, xb, Wp, nk, t0, Tv, ph);
  const int Tout = a.Tn * a.nphase;
  // epilogue through LDS (as resunit_lds_kernel's): the workgroup's output tile [128 frames][NW * 48 channels] goes through the slab
  // memory in passes of EF frames as fp32 rows, and every lane then moves 16 CONSECUTIVE bytes of a row (a row of the tile = NW * 192 bytes of
  // an output row; the rows of a transposed conv's phase are `nphase` rows apart). Why not straight out of the accumulators: DESIGN.md §5.
  constexpr int CW = NW * CSW * 16, RSE = CW * 4 + 16, SLB = 2 * MAXROWS * RS, VPR = CW / 4;
  constexpr int EF0 = SLB / RSE;
  constexpr int EF1 = EF0 >= 128 ? 128 : (EF0 >= 64 ? 64 : (EF0 >= 32 ? 32 : 16)), EF = EF1 > TF ? TF : EF1, TPP = EF / 16;
  static_assert(EF0 >= 16, "one 16-frame pass of the output tile fits the slab memory");
  unsigned char* et = &slab[0][0];  // the last chunk's barrier has retired every slab read
  const int c0 = blockIdx.y * CW;
  // Round 5 (as resunit_lds_kernel's epilogue): the Snake parameters of this workgroup's CW channels go through LDS, and a pass over EF whole
  // rows is ONE straight-line block per (residual?, stream?, activation format) - no load from global memory and no branch between the stores,
  // so no s_waitcnt vmcnt(0) (= "until my last stores are acknowledged") in front of every row piece.
  constexpr int NPT = EF * VPR / NT;
  static_assert(EF * VPR % NT == 0, "row pieces per thread and pass");
  int tid_e = tid;  // an opaque copy for the epilogue's address arithmetic: computed from `tid` it is hoisted above the MFMA loop and spilled there
  asm volatile("" : "+v"(tid_e));
  static_assert(EF * RSE + 2 * CW * 4 <= SLB, "LDS: one pass of the output tile + the Snake parameters");
  float* s_al = reinterpret_cast<float*>(et + EF * RSE);  // [2][CW]: alpha | 1 / (alpha + 1e-9)
  if (a.out_act)
    for (int i = tid; i < 2 * VPR; i += NT) {
      const int hf = i / VPR, c4 = i - hf * VPR;
      reinterpret_cast<float4*>(s_al)[i] = *reinterpret_cast<const float4*>(a.alpha + (size_t)hf * a.Cout + c0 + c4 * 4);
    }
  typedef std::integral_constant<int, 0> I0_;
  typedef std::integral_constant<int, 1> I1_;
  typedef std::integral_constant<int, 2> I2_;
  auto pass = [&](auto skip_c, auto raw_c, auto act_c, const int r0, const int rows) __attribute__((always_inline)) {
    constexpr bool SK = decltype(skip_c)::value != 0, RW = decltype(raw_c)::value != 0;
    constexpr int AC = decltype(act_c)::value;  // 0: no activation output, 1: bf16, 2: fp32
    auto offs = [&](const int i) { const int rr = i / VPR, cv = i - rr * VPR; return ((size_t)b * Tout + (size_t)(r0 + rr) * a.nphase + ph) * a.Cout + c0 + cv * 4; };
    auto piece = [&](const int i, const size_t o, const float4 sk) __attribute__((always_inline)) {
      const int rr = i / VPR, cv = i - rr * VPR;
      float4 v = *reinterpret_cast<const float4*>(et + rr * RSE + cv * 16);
      if constexpr (SK) { v.x += sk.x; v.y += sk.y; v.z += sk.z; v.w += sk.w; }
      if constexpr (RW) *reinterpret_cast<float4*>(a.out_raw + o) = v;
      if constexpr (AC != 0) {
        const float4 al = *reinterpret_cast<const float4*>(s_al + cv * 4), ia = *reinterpret_cast<const float4*>(s_al + CW + cv * 4);
        const float4 sv = make_float4(snake_f<true>(v.x, al.x, ia.x), snake_f<true>(v.y, al.y, ia.y), snake_f<true>(v.z, al.z, ia.z), snake_f<true>(v.w, al.w, ia.w));
        if constexpr (AC == 1) *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(a.out_act) + o) = make_uint2(pack_bf16x2(sv.x, sv.y), pack_bf16x2(sv.z, sv.w));
        else *reinterpret_cast<float4*>(reinterpret_cast<float*>(a.out_act) + o) = sv;
      }
    };
    if (rows == EF) {
      constexpr int GP = NPT > 6 ? 6 : NPT;  // residual values in flight per group (registers: acc is still live for the next pass)
      static_assert(NPT % GP == 0, "row pieces per group");
#pragma unroll
      for (int k0 = 0; k0 < NPT; k0 += GP) {
        float4 skp[SK ? GP : 1];
        if constexpr (SK) {
#pragma unroll
          for (int k = 0; k < GP; ++k) skp[k] = *reinterpret_cast<const float4*>(a.skip + offs(tid_e + (k0 + k) * NT));
        }
#pragma unroll
        for (int k = 0; k < GP; ++k) piece(tid_e + (k0 + k) * NT, offs(tid_e + (k0 + k) * NT), SK ? skp[SK ? k : 0] : make_float4(0.f, 0.f, 0.f, 0.f));
      }
    } else {
#pragma unroll 2
      for (int k = 0; k < NPT; ++k) {
        const int i = tid_e + k * NT;
        if (i / VPR < rows) {
          const size_t o = offs(i);
          float4 sk = make_float4(0.f, 0.f, 0.f, 0.f);
          if constexpr (SK) sk = *reinterpret_cast<const float4*>(a.skip + o);
          piece(i, o, sk);
        }
      }
    }
  };
  auto by_act = [&](auto skip_c, auto raw_c, const int r0, const int rows) __attribute__((always_inline)) {
    if (!a.out_act) pass(skip_c, raw_c, I0_(), r0, rows);
    else if (a.act_f32) pass(skip_c, raw_c, I2_(), r0, rows);
    else pass(skip_c, raw_c, I1_(), r0, rows);
  };
  // (explicitly instantiated per pass: inside a `#pragma unroll` loop the dispatch below stopped the unroller and `acc` went to scratch)
  auto do_pass = [&](auto p0_c) __attribute__((always_inline)) {
    constexpr int p0 = decltype(p0_c)::value;
    if constexpr (p0 < FT) {
#pragma unroll
    for (int s = 0; s < CSW; ++s) {
      const float4 bs = *reinterpret_cast<const float4*>(a.bias + (strip0 + s) * 16 + q * 4);
#pragma unroll
      for (int f = 0; f < TPP; ++f) {
        const f32x4 av = acc[s][p0 + f];
        *reinterpret_cast<float4*>(et + (f * 16 + j) * RSE + ((wave * CSW + s) * 16 + q * 4) * 4) = make_float4(av[0] + bs.x, av[1] + bs.y, av[2] + bs.z, av[3] + bs.w);
      }
    }
    __syncthreads();
    const int r0 = t0 + p0 * 16, rows = min(EF, Tnv - r0);
    if (a.skip) { if (a.out_raw) by_act(I1_(), I1_(), r0, rows); else by_act(I1_(), I0_(), r0, rows); }
    else { if (a.out_raw) by_act(I0_(), I1_(), r0, rows); else by_act(I0_(), I0_(), r0, rows); }
    if (p0 + TPP < FT) __syncthreads();  // the tile memory is rewritten by the next pass
    }
  };
  do_pass(std::integral_constant<int, 0>()); do_pass(std::integral_constant<int, TPP>()); do_pass(std::integral_constant<int, 2 * TPP>());
  do_pass(std::integral_constant<int, 3 * TPP>()); do_pass(std::integral_constant<int, 4 * TPP>()); do_pass(std::integral_constant<int, 5 * TPP>());
  do_pass(std::integral_constant<int, 6 * TPP>()); do_pass(std::integral_constant<int, 7 * TPP>());
}

// Fused residual unit (default; PTTS_DAC_NO_FUSE_RES=1 restores the two-launch path for A/B): one residual unit of the three narrower blocks
// (C = 384 / 192 / 96) in ONE launch (measured on MI355X, profiles/r03_experiments.txt: 860 frames 3.62 -> 3.25 ms, batch 32 109.4 -> 97.5 ms):
//   y = Snake_a(conv_k7_dil(x) + b7)  ->  bf16 tile in LDS  ->  out = skip + conv_k1(y) + b1 ; act = Snake_a1(out)
// The workgroup owns all C channels of 128 frames (NW * 3 strips = C / 16), so the k1 GEMM's operand never leaves the CU: the unit's
// HBM traffic drops from 16 to 12 bytes per element (no bf16 round trip of y) and one launch per unit goes away (per-layer table,
// profiles/r02_dac_layers.txt: k7 + k1 = 339 us at C = 192, 260 us at C = 96, the k1 half bound by its epilogue traffic).
// Phase A is slab_mfma_loop as conv_lds_kernel<3, NW, 1, 54> runs it; the y tile overlays the two slab buffers once the last chunk's barrier has passed.
// weight prefetch depth (slab_mfma_loop's WD) of the XIN instances per width (registers: an XIN unit stages twice the bytes per slab slot)
template <int NW> struct ResunitXinWD { static constexpr int value = NW == 2 ? 1 : 3; };
struct ResArgs {
  ConvArgs a;           // the k7 conv (x, Wp, bias, alpha = Snake between the two convs, dil, pad, B, Tin, Cin = Cout = C)
  const void* Wp1;      // k1 weights, packed [C/16][C/32][64][8 bf16]
  const float* bias1;
  const float* alpha1;  // Snake of the unit's output (the next layer's input activation)
  const float* skip;    // fp32 residual stream [B][T][C]
  float* out_raw;       // fp32 residual stream after the unit (may alias skip), or null
  void* out_act;        // activated output, bf16 (fp32 if act_f32): NOT the buffer x lives in (neighbouring tiles read x's halo rows)
  int act_f32;
  const float* alpha_in;  // XIN instances: [alpha | 1 / (alpha + 1e-9)] of the Snake that turns the fp32 stream `a.x` into this unit's input activation
};

// dynamic LDS of resunit_lds_kernel<NW>: the two slab buffers of phase A, overlaid by the y tile [128 frames][C bf16 + pad] of phase B
// (NW = 8, C = 384: 100 KB - above the 64 KB a static __shared__ array may declare, hence dynamic for every instance)
template <int NW> struct ResunitLds {
  static constexpr int C = NW * 3 * 16, slabs = 2 * (128 + 54) * 96, ytile = 128 * (C * 2 + 32);
  static constexpr int etile = 64 * (C * 4 + 16);  // epilogue: half of the output tile as fp32 rows (16 bytes of padding: the 16 frames of one store hit 16 different bank groups)
  static constexpr int ain = slabs + 2 * C * 4;  // XIN instances: the input Snake's [alpha | 1 / alpha] behind the two slabs
  static constexpr int bytes0 = ain > ytile ? ain : ytile;
  static constexpr int bytes = bytes0 > etile ? bytes0 : etile;
};
// WD: how many k-steps ahead a wave requests its weight fragments (slab_mfma_loop: 3, or 1 for the XIN instances at C = 96).
// RAW / F32 (round 5): does the launch write the fp32 stream, and is the activation written as fp32 (the unit feeding the final conv)? Compile-time,
// so that the epilogue's pass over a whole half tile is ONE straight-line block (see there).
// XIN / ACT (round 6): the codec is HBM-bound at batch 32 (profiles/r06_pmc_dac_bs32.txt: 195.7 GB per decode, the C = 96 units at 4.5-4.6 TB/s), so bytes
// are what is left to cut. An XIN unit takes its input straight from the fp32 residual stream (`a.x` = `skip`): the Snake of the PREVIOUS layer's
// output is evaluated on the way into the LDS slab (same function on the same fp32 values, rounded to bf16 once: bit-identical to reading the bf16
// activation the producer would have written), and a producer whose consumer is an XIN unit does not write that activation at all (ACT = false):
// per element and unit 12 C -> ~9.7 C bytes (halo rows of the stream are fp32 now, the bf16 copy is neither written nor read).
template <int NW, int WD = 3, bool RAW = true, bool F32 = false, bool XIN = false, bool ACT = true>
__global__ void __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(2, 2))) resunit_lds_kernel(ResArgs ra) {
  constexpr int CSW = 3, FT = 8, TF = FT * 16, MAXHALO = 54;
  constexpr int C = NW * CSW * 16;
  constexpr int RS = 96, NT = NW * 64, MAXROWS = TF + MAXHALO;  // slab_mfma_loop's at KS = 1: 32-channel chunks, 64-byte slab rows + 32
  constexpr int RS2 = C * 2 + 32;  // y tile row stride: an odd multiple of 32 bytes, conflict-free ds_read_b128 like the slab
  constexpr int NK1 = C / 32;      // k-steps of the k1 GEMM
  static_assert(ResunitLds<NW>::bytes >= 2 * MAXROWS * RS && ResunitLds<NW>::bytes >= TF * RS2, "LDS size");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const ConvArgs& a = ra.a;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = lane >> 4, j = lane & 15;
  const int ntile = (a.Tn + TF - 1) / TF;
  const int tile = blockIdx.x % ntile, b = blockIdx.x / ntile;
  const int strip0 = wave * CSW;
  const int nk = a.ntaps * (C / 32);
  const int t0 = tile * TF;
  const int Tv = valid_rows(a, b);  // ragged decode: this utterance's rows (workgroup-uniform)
  if (t0 >= Tv) return;
  const char* xb = reinterpret_cast<const char*>(a.x) + (size_t)b * a.Tin * C * (XIN ? 4 : 2);
  float* s_ain = reinterpret_cast<float*>(lds + 2 * MAXROWS * RS);  // XIN: [2][C]
  if constexpr (XIN) {
    for (int i = tid; i < 2 * C / 4; i += NT) reinterpret_cast<float4*>(s_ain)[i] = reinterpret_cast<const float4*>(ra.alpha_in)[i];
    __syncthreads();
  }
  const float4* Wp = reinterpret_cast<const float4*>(a.Wp) + (size_t)strip0 * nk * 64 + lane;

  f32x4 acc[CSW][FT];
#pragma unroll
  for (int s = 0; s < CSW; ++s)
#pragma unroll
    for (int f = 0; f < FT; ++f) acc[s][f] = f32x4{0, 0, 0, 0};
  // ---- phase A: the k7 conv (the unit's first conv is k7: run_resunit), k-steps and chunks known at compile time
  slab_mfma_loop<CSW, NW, 1, FT, MAXHALO, WD, XIN, C>(acc, lds, s_ain, a, xb, Wp, nk, t0, Tv, 0);
  // ---- phase A epilogue: y = Snake(acc + b7) as bf16 into the LDS tile [frame][C] (the loop's last barrier has retired every slab read)
  unsigned char* ytile = lds;
  auto put_y = [&](const f32x4 av, const int s, const int f) {
    const int co = (strip0 + s) * 16 + q * 4;
    const float4 bs = *reinterpret_cast<const float4*>(a.bias + co);
    const float4 al = *reinterpret_cast<const float4*>(a.alpha + co), ia = ld_inv4(a.alpha, C, co);
    const float4 sv = make_float4(snake_f<true>(av[0] + bs.x, al.x, ia.x), snake_f<true>(av[1] + bs.y, al.y, ia.y), snake_f<true>(av[2] + bs.z, al.z, ia.z),
                                  snake_f<true>(av[3] + bs.w, al.w, ia.w));
    *reinterpret_cast<uint2*>(ytile + (f * 16 + j) * RS2 + co * 2) = make_uint2(pack_bf16x2(sv.x, sv.y), pack_bf16x2(sv.z, sv.w));
  };
#define RU_PUT_ROW(S)                                                                                                   \
  put_y(acc[S][0], S, 0); put_y(acc[S][1], S, 1); put_y(acc[S][2], S, 2); put_y(acc[S][3], S, 3);                         \
  put_y(acc[S][4], S, 4); put_y(acc[S][5], S, 5); put_y(acc[S][6], S, 6); put_y(acc[S][7], S, 7);
  RU_PUT_ROW(0)
  RU_PUT_ROW(1)
  RU_PUT_ROW(2)
#undef RU_PUT_ROW
  __syncthreads();
  // the epilogue's residual rows: thread i owns float4 i, i + NT, ... of the [64][C] half tile, all 12 loads of a half in flight at once.
  // (Requesting them BEFORE the k1 GEMM, and 64-channel staging chunks, were measured and dropped: 72.3 vs 70.2 ms per batch-32 decode,
  // profiles/r04_experiments.txt - the units are not short of bytes in flight.)
  constexpr int VPRH = C / 4, NPT = 64 * VPRH / NT;  // float4 per row; per thread and half tile (= 12 for every NW)
  float4 skp[NPT];
  auto load_skip = [&](const int hh) __attribute__((always_inline)) {
    const int r0_ = t0 + hh * 64, rows_ = min(64, Tv - r0_);
    const float* sb_ = ra.skip + ((size_t)b * a.Tn + r0_) * C;
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
      const int i_ = tid + k * NT;
      skp[k] = (i_ / VPRH) < rows_ ? *reinterpret_cast<const float4*>(sb_ + (size_t)i_ * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  // ---- phase B: the k1 conv as a [C x C] GEMM over the tile; A = this wave's 3 strips of W1, B = y rows out of LDS
  const float4* W1 = reinterpret_cast<const float4*>(ra.Wp1) + (size_t)strip0 * NK1 * 64 + lane;
#pragma unroll
  for (int s = 0; s < CSW; ++s)
#pragma unroll
    for (int f = 0; f < FT; ++f) acc[s][f] = f32x4{0, 0, 0, 0};
  const unsigned char* yl = ytile + j * RS2 + q * 16;
#pragma unroll
  for (int kk = 0; kk < NK1; ++kk) {
    float4 wk[CSW];
#pragma unroll
    for (int s = 0; s < CSW; ++s) wk[s] = W1[((size_t)s * NK1 + kk) * 64];
#pragma unroll
    for (int f = 0; f < FT; ++f) {
      const uint4 bv = *reinterpret_cast<const uint4*>(yl + f * 16 * RS2 + kk * 64);
#pragma unroll
      for (int s = 0; s < CSW; ++s)
        acc[s][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wk[s]), __builtin_bit_cast(bf16x8, bv), acc[s][f], 0, 0, 0);
    }
  }
  // ---- phase B epilogue: + bias + residual, fp32 stream out, Snake of the unit's output.
  // Through LDS: a lane's accumulators are 4 channels of ONE frame, so stored straight from them the fp32 stream moves in 64-byte pieces
  // (rows C * 4 bytes apart; that form and its figures: DESIGN.md §5). Here the output tile goes through LDS in two halves of 64 frames
  // ([64][C fp32], rows padded by 16 bytes) and every lane then owns 16 CONSECUTIVE bytes of a row: the residual read, the stream write and
  // the activation write are whole rows (tools/epilogue_probe.hip: 64-frame halves; 128-frame tiles do not pay).
  constexpr int RSE = C * 4 + 16, VPR = C / 4;
  unsigned char* et = lds;
  // The output Snake's [alpha | 1 / (alpha + 1e-9)] go through LDS (round 5): fetched from global memory inside the loop below, every iteration's
  // s_waitcnt vmcnt() for them also waited for the STORES of the iteration before (loads and stores retire in order on one counter) - 24 store
  // round trips in a row per workgroup, ~2/3 of the time the three fused units spent outside their MFMA loops (found in the ISA, not in a counter).
  static_assert(ResunitLds<NW>::bytes >= 64 * RSE + 2 * C * 4, "LDS: half output tile + the output Snake's parameters");
  float* s_al = reinterpret_cast<float*>(lds + 64 * RSE);  // [2][C]
  __syncthreads();  // every wave has finished reading the y tile
  if constexpr (ACT)
    for (int i = tid; i < 2 * C / 4; i += NT) reinterpret_cast<float4*>(s_al)[i] = reinterpret_cast<const float4*>(ra.alpha1)[i];
  // (requesting the residual rows before the transposition, and the second half's as the first half's registers free up, measured SLOWER:
  //  C = 96 unit 4228 -> 4735 us, profiles/r04_experiments.txt call 7; they are requested after the tile's barrier, 12 loads at once)
#pragma unroll
  for (int hh = 0; hh < 2; ++hh) {
#pragma unroll
    for (int s = 0; s < CSW; ++s) {
      const int co = (strip0 + s) * 16 + q * 4;
      const float4 bs = *reinterpret_cast<const float4*>(ra.bias1 + co);
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        const f32x4 av = acc[s][hh * 4 + f];
        *reinterpret_cast<float4*>(et + (f * 16 + j) * RSE + co * 4) = make_float4(av[0] + bs.x, av[1] + bs.y, av[2] + bs.z, av[3] + bs.w);
      }
    }
    __syncthreads();
    const int r0 = t0 + hh * 64;
    const int rows = min(64, Tv - r0);
    const size_t base = ((size_t)b * a.Tn + r0) * C;
    // A whole half tile (every tile but an utterance's last) is ONE straight-line block: 12 unconditional residual loads, then per row piece
    // LDS reads -> add -> store(s) -> Snake -> store, no load from global memory and no branch in between. With the stream / activation format
    // decided by branches inside the loop (and the Snake parameters loaded from global memory there), the compiler's wait-count bookkeeping
    // put an s_waitcnt vmcnt(0) - "until my last STORES are acknowledged", loads and stores retire in order on one counter - in front of every
    // row piece: 24 store round trips in a row per workgroup.
    auto piece = [&](const int k, const float4 sk) __attribute__((always_inline)) {
      const int i = tid + k * NT;
      const int rr = i / VPR, cv = i - rr * VPR;
      const float4 av = *reinterpret_cast<const float4*>(et + rr * RSE + cv * 16);
      const size_t o = base + (size_t)i * 4;  // the rows of a tile are contiguous in memory: i * 4 == rr * C + cv * 4
      const float4 v = make_float4(av.x + sk.x, av.y + sk.y, av.z + sk.z, av.w + sk.w);
      if constexpr (RAW) *reinterpret_cast<float4*>(ra.out_raw + o) = v;
      if constexpr (ACT) {  // ACT = false: the consumer is an XIN unit and evaluates this Snake itself, out of the stream
        const float4 al = *reinterpret_cast<const float4*>(s_al + cv * 4), ia = *reinterpret_cast<const float4*>(s_al + C + cv * 4);
        const float4 sv = make_float4(snake_f<true>(v.x, al.x, ia.x), snake_f<true>(v.y, al.y, ia.y), snake_f<true>(v.z, al.z, ia.z), snake_f<true>(v.w, al.w, ia.w));
        if constexpr (!F32) *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(ra.out_act) + o) = make_uint2(pack_bf16x2(sv.x, sv.y), pack_bf16x2(sv.z, sv.w));
        else *reinterpret_cast<float4*>(reinterpret_cast<float*>(ra.out_act) + o) = sv;
      }
    };
    if (rows == 64) {
      const float* sb_ = ra.skip + base;
#pragma unroll
      for (int k = 0; k < NPT; ++k) skp[k] = *reinterpret_cast<const float4*>(sb_ + (size_t)(tid + k * NT) * 4);
#pragma unroll
      for (int k = 0; k < NPT; ++k) piece(k, skp[k]);
    } else {
      load_skip(hh);
#pragma unroll
      for (int k = 0; k < NPT; ++k)
        if ((tid + k * NT) / VPR < rows) piece(k, skp[k]);
    }
    if (hh == 0) __syncthreads();  // the tile is rewritten by the second half
  }
}

// final Conv1d(C -> 1, k7, pad 3) + tanh; weights [7][C] in LDS. One thread per OS = 4 consecutive output samples: the 10 input rows
// they touch are read once (60 float4 loads per sample instead of 168; the kernel was 187 us of the 860-frame decode, L1-bound on
// the 7x re-read). Per sample the fma order is unchanged (bias, then tap 0..6 x channel 0..C-1), so the exact-f32 mode is bit-identical.
// samples [skip, t_end) of every utterance are written to out[b * out_ld + (t - skip)] (skip > 0: the halo frames of a chunk)
// ROWS (the streaming pass out of a session): the emit range is [skip[b], t_end[b]) per row instead of one range for the batch
constexpr int OUT_OS = 4;
template <bool ROWS> struct EmitArg { using T = int; };
template <> struct EmitArg<true> { using T = const int* __restrict__; };
__device__ __forceinline__ int emit_of(int v, int) { return v; }
__device__ __forceinline__ int emit_of(const int* v, int b) { return v[b]; }

template <bool ROWS>
__global__ void conv_out_tanh_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                     float* __restrict__ out, int B, int T, int C, int ktaps, typename EmitArg<ROWS>::T skip_of, long long out_ld,
                                     typename EmitArg<ROWS>::T t_end_of, const int* __restrict__ lens, int len_mul) {
  extern __shared__ float sw[];
  for (int i = threadIdx.x; i < ktaps * C; i += blockDim.x) sw[i] = w[i];
  __syncthreads();
  const int TG = (T + OUT_OS - 1) / OUT_OS;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)B * TG) return;
  const int b = (int)(idx / TG), t0 = (int)(idx % TG) * OUT_OS;
  const int Tv = lens ? min(T, lens[b] * len_mul) : T;  // ragged decode: samples of this utterance (rows beyond are the zero padding)
  const int skip = emit_of(skip_of, b), t_end = min(emit_of(t_end_of, b), Tv);
  if (t0 + OUT_OS <= skip || t0 >= t_end) return;
  float acc[OUT_OS];
#pragma unroll
  for (int s = 0; s < OUT_OS; ++s) acc[s] = bias[0];
  const int half = ktaps / 2;
  for (int r = 0; r < OUT_OS + ktaps - 1; ++r) {  // input row t0 - half + r feeds sample s with tap r - s
    const int ti = t0 - half + r;
    if (ti < 0 || ti >= Tv) continue;
    const float4* xr = reinterpret_cast<const float4*>(x + ((size_t)b * T + ti) * C);
    for (int c4 = 0; c4 < C / 4; ++c4) {
      const float4 xv = xr[c4];
#pragma unroll
      for (int s = 0; s < OUT_OS; ++s) {
        const int tap = r - s;
        if (tap >= 0 && tap < ktaps) {
          const float4 wv = reinterpret_cast<const float4*>(sw + tap * C)[c4];
          acc[s] = fmaf(xv.x, wv.x, acc[s]); acc[s] = fmaf(xv.y, wv.y, acc[s]); acc[s] = fmaf(xv.z, wv.z, acc[s]); acc[s] = fmaf(xv.w, wv.w, acc[s]);
        }
      }
    }
  }
#pragma unroll
  for (int s = 0; s < OUT_OS; ++s) {
    const int t = t0 + s;
    if (t < Tv && t >= skip && t < t_end) out[(size_t)b * out_ld + (t - skip)] = tanhf(acc[s]);
  }
}

// The same final convolution, LDS-tiled (C == 96, k7: the 44.1 kHz decoder). conv_out_tanh_kernel's threads each walk their own
// input rows (a wave-load touches 64 different 384-byte rows: 169 MB at 1.4 TB/s, 121 us of the 860-frame decode). Here a workgroup
// owns OUT_TILE consecutive samples: the (OUT_TILE + 6) x 96 input tile is ONE contiguous 27 KB block, staged into LDS with coalesced
// float4 loads; rows are 100 floats apart (400 B = 36 dwords mod 64: the 16 lanes of a ds_read_b128 service group hit 16 distinct
// 4-bank slots), the 7 x 96 weights are read as wave-uniform broadcasts. Thread t then computes sample t with EXACTLY the fma order
// of the reference restatement (bias, tap 0..6 x channel 0..95): the exact-f32 mode stays bit-identical to the direct kernel.
constexpr int OUT_TILE = 64, OUT_C = 96, OUT_ROW = 100;  // 64 samples per (one-wave) workgroup: 28 KB of LDS, 5 workgroups per CU
template <bool ROWS>
__global__ void __launch_bounds__(OUT_TILE) conv_out_tanh_lds_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                                     float* __restrict__ out, int T, typename EmitArg<ROWS>::T skip_of, long long out_ld,
                                                                     typename EmitArg<ROWS>::T t_end_of, const int* __restrict__ lens, int len_mul) {
  __shared__ __attribute__((aligned(16))) float sx[(OUT_TILE + 6) * OUT_ROW];
  __shared__ __attribute__((aligned(16))) float sw[7 * OUT_C];
  const int b = blockIdx.y, t0 = blockIdx.x * OUT_TILE, tid = threadIdx.x;
  const int Tv = lens ? min(T, lens[b] * len_mul) : T;  // ragged decode: samples of this utterance (rows beyond are the zero padding)
  const int skip = emit_of(skip_of, b), t_end = min(emit_of(t_end_of, b), Tv);
  if (t0 + OUT_TILE <= skip || t0 >= t_end) return;  // workgroup-uniform: nothing of this tile is emitted
  for (int i = tid; i < 7 * OUT_C / 4; i += OUT_TILE) reinterpret_cast<float4*>(sw)[i] = reinterpret_cast<const float4*>(w)[i];
  const float4* xb = reinterpret_cast<const float4*>(x + (size_t)b * T * OUT_C);
  constexpr int NV = (OUT_TILE + 6) * (OUT_C / 4), UL = 9;  // 1680 float4 of the tile (rows t0 - 3 .. t0 + OUT_TILE + 2), 9 loads in flight per thread
  for (int i0 = tid; i0 < NV; i0 += UL * OUT_TILE) {
    float4 v[UL];
#pragma unroll
    for (int u = 0; u < UL; ++u) {
      const int i = min(i0 + u * OUT_TILE, NV - 1), r = i / (OUT_C / 4), ti = t0 - 3 + r;
      v[u] = (ti >= 0 && ti < Tv) ? xb[(size_t)ti * (OUT_C / 4) + (i - r * (OUT_C / 4))] : make_float4(0.f, 0.f, 0.f, 0.f);  // zero outside [0, Tv)
    }
#pragma unroll
    for (int u = 0; u < UL; ++u) {
      const int i = i0 + u * OUT_TILE, r = i / (OUT_C / 4);
      if (i < NV) *reinterpret_cast<float4*>(sx + r * OUT_ROW + (i - r * (OUT_C / 4)) * 4) = v[u];
    }
  }
  __syncthreads();
  const int t = t0 + tid;
  if (t >= Tv || t < skip || t >= t_end) return;
  float acc = bias[0];
#pragma unroll 1
  for (int tap = 0; tap < 7; ++tap) {
    const int ti = t - 3 + tap;
    if (ti < 0 || ti >= Tv) continue;  // the direct kernel skips out-of-range rows too (no fma with the zero padding)
    const float* xr = sx + (tid + tap) * OUT_ROW;
    const float* wr = sw + tap * OUT_C;
#pragma unroll
    for (int c4 = 0; c4 < OUT_C / 4; ++c4) {
      const float4 xv = *reinterpret_cast<const float4*>(xr + c4 * 4), wv = *reinterpret_cast<const float4*>(wr + c4 * 4);
      acc = fmaf(xv.x, wv.x, acc); acc = fmaf(xv.y, wv.y, acc); acc = fmaf(xv.z, wv.z, acc); acc = fmaf(xv.w, wv.w, acc);
    }
  }
  out[(size_t)b * out_ld + (t - skip)] = tanhf(acc);
}

// first encoder Conv1d(1 -> C, k7, pad 3) on the raw waveform: one thread per (sample, 4 channels); writes the raw
// result (residual skip of the first unit) and its Snake. HBM-bound (C floats out per sample), trivially parallel.
__global__ void conv_in_kernel(const float* __restrict__ wave, const float* __restrict__ w /*[C][7]*/, const float* __restrict__ bias,
                               const float* __restrict__ alpha, float* __restrict__ out_raw, float* __restrict__ out_act, int B, int L, int C) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int c4n = C / 4;
  if (idx >= (size_t)B * L * c4n) return;
  const int c4 = (int)(idx % c4n);
  const size_t bt = idx / c4n;
  const int t = (int)(bt % L), b = (int)(bt / L);
  float xs[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) { const int ti = t + k - 3; xs[k] = (ti >= 0 && ti < L) ? wave[(size_t)b * L + ti] : 0.f; }
  float o[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int c = c4 * 4 + e;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 7; ++k) acc = fmaf(w[c * 7 + k], xs[k], acc);
    o[e] = acc + bias[c];
  }
  const size_t off = bt * C + c4 * 4;
  *reinterpret_cast<float4*>(out_raw + off) = make_float4(o[0], o[1], o[2], o[3]);
  const float4 al = *reinterpret_cast<const float4*>(alpha + c4 * 4), ia = ld_inv4(alpha, C, c4 * 4);
  *reinterpret_cast<float4*>(out_act + off) = make_float4(snake_f<false>(o[0], al.x, ia.x), snake_f<false>(o[1], al.y, ia.y), snake_f<false>(o[2], al.z, ia.z), snake_f<false>(o[3], al.w, ia.w));
}

// F.normalize(codebook) rows: c / max(||c||_2, 1e-12)
__global__ void cb_normalize_kernel(const float* __restrict__ cb, float* __restrict__ cbn, float* __restrict__ cbn_sq, int ncodes, int cdim) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ncodes) return;
  float ss = 0.f;
  for (int d = 0; d < cdim; ++d) ss += cb[(size_t)i * cdim + d] * cb[(size_t)i * cdim + d];
  const float inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
  float s2 = 0.f;
  for (int d = 0; d < cdim; ++d) { const float v = cb[(size_t)i * cdim + d] * inv; cbn[(size_t)i * cdim + d] = v; s2 += v * v; }
  cbn_sq[i] = s2;  // the ||c||^2 term of the reference's distance (1 up to rounding, kept so that near-ties order the same way)
}

// Residual VQ encode (ResidualVectorQuantize.forward, eval mode), one workgroup per latent frame, all stages in sequence:
//   p = in_proj_i(residual); idx = argmax_c <normalize(p), normalize(codebook_i[c])> (first index on ties);
//   z_q = out_proj_i(p + (codebook_i[idx] - p));  residual -= z_q.
// in_w [K][cdim][latent], in_b [K][cdim], cb/cbn [K][codes][cdim], out_w [K][latent][cdim], out_b [K][latent]. cdim <= 16.
constexpr int RVQ_MAXD = 16;
__global__ void __launch_bounds__(256) rvq_encode_kernel(const float* __restrict__ z /*[B][T][latent]*/, const float* __restrict__ in_w,
                                                         const float* __restrict__ in_b, const float* __restrict__ cb, const float* __restrict__ cbn,
                                                         const float* __restrict__ cbn_sq, const float* __restrict__ out_w, const float* __restrict__ out_b,
                                                         long long* __restrict__ codes /*[B][nq][T]*/, int T, int latent, int cdim, int ncodes, int nq) {
  extern __shared__ float s_res[];  // [latent] residual, then [4 waves][RVQ_MAXD] partials
  __shared__ float s_part[4][RVQ_MAXD];
  __shared__ float s_p[RVQ_MAXD], s_e[RVQ_MAXD], s_q[RVQ_MAXD];
  __shared__ float s_ee;
  __shared__ float s_best[4];
  __shared__ int s_bidx[4];
  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* zr = z + ((size_t)b * T + t) * latent;
  for (int c = tid; c < latent; c += 256) s_res[c] = zr[c];
  __syncthreads();
  for (int i = 0; i < nq; ++i) {
    const float* W = in_w + (size_t)i * cdim * latent;
    // 1. p[d] = b[d] + sum_c W[d][c] * r[c]
    float part[RVQ_MAXD];
#pragma unroll
    for (int d = 0; d < RVQ_MAXD; ++d) part[d] = 0.f;
    for (int c = tid; c < latent; c += 256) {
      const float r = s_res[c];
#pragma unroll
      for (int d = 0; d < RVQ_MAXD; ++d)
        if (d < cdim) part[d] = fmaf(W[(size_t)d * latent + c], r, part[d]);
    }
#pragma unroll
    for (int d = 0; d < RVQ_MAXD; ++d) {
      if (d < cdim) {
        const float v = wave_sum(part[d]);
        if (lane == 0) s_part[wave][d] = v;
      }
    }
    __syncthreads();
    if (tid < cdim) s_p[tid] = ((s_part[0][tid] + s_part[1][tid]) + (s_part[2][tid] + s_part[3][tid])) + in_b[(size_t)i * cdim + tid];
    __syncthreads();
    if (tid == 0) {
      float ss = 0.f;
      for (int d = 0; d < cdim; ++d) ss += s_p[d] * s_p[d];
      const float inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
      float ee = 0.f;
      for (int d = 0; d < cdim; ++d) { s_e[d] = s_p[d] * inv; ee += s_e[d] * s_e[d]; }
      s_ee = ee;
    }
    __syncthreads();
    // 2. nearest code: argmax of -(||e||^2 - 2 e.c + ||c||^2) over the normalised codebook, first index on ties
    float best = -INFINITY;
    int bidx = 0;
    const float ee = s_ee;
    for (int c = tid; c < ncodes; c += 256) {
      const float* cr = cbn + ((size_t)i * ncodes + c) * cdim;
      float dot = 0.f;
      for (int d = 0; d < cdim; ++d) dot = fmaf(s_e[d], cr[d], dot);
      const float score = -((ee - 2.0f * dot) + cbn_sq[(size_t)i * ncodes + c]);
      if (score > best) { best = score; bidx = c; }
    }
    const float wb = wave_max(best);
    // lowest code index among the lanes holding the wave maximum
    int cand = best == wb ? bidx : 0x7fffffff;
    for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o));
    if (lane == 0) { s_best[wave] = wb; s_bidx[wave] = cand; }
    __syncthreads();
    if (tid == 0) {
      float bb = s_best[0]; int bi = s_bidx[0];
      for (int w2 = 1; w2 < 4; ++w2)
        if (s_best[w2] > bb || (s_best[w2] == bb && s_bidx[w2] < bi)) { bb = s_best[w2]; bi = s_bidx[w2]; }
      codes[((size_t)b * nq + i) * T + t] = bi;
      const float* cr = cb + ((size_t)i * ncodes + bi) * cdim;
      for (int d = 0; d < cdim; ++d) { const float diff = cr[d] - s_p[d]; s_q[d] = s_p[d] + diff; }  // straight-through expression
    }
    __syncthreads();
    // 3. residual -= out_proj(q)
    const float* OW = out_w + (size_t)i * latent * cdim;
    for (int c = tid; c < latent; c += 256) {
      float acc = 0.f;
      for (int d = 0; d < cdim; ++d) acc = fmaf(OW[(size_t)c * cdim + d], s_q[d], acc);
      s_res[c] -= acc + out_b[(size_t)i * latent + c];
    }
    __syncthreads();
  }
}

// RVQ table: table[i][code][c] = bias_i[c] + sum_d W_i[c][d] * codebook_i[code][d]
__global__ void rvq_table_kernel(const float* __restrict__ cb, const float* __restrict__ w, const float* __restrict__ bias,
                                 float* __restrict__ table, int ncodes, int cdim, int latent) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)ncodes * latent) return;
  const int code = (int)(idx / latent), c = (int)(idx % latent);
  float acc = 0.f;
  for (int d = 0; d < cdim; ++d) acc = fmaf(w[(size_t)c * cdim + d], cb[(size_t)code * cdim + d], acc);
  table[idx] = acc + bias[c];
}

// streaming out of a continuous session (ptts_dac_stream_decode): one pass's plan, [row] arrays written by stream_absorb_kernel
struct StreamPlan {
  const int *tab, *lens, *start, *skip, *tend, *slot;
  int cap;
};
template <bool STREAM> struct GatherSrc { using T = const long long* __restrict__; };
template <> struct GatherSrc<true> { using T = StreamPlan; };

// z[b][t][c] = sum_i table[i][codes[b][i][t]][c]   (sequential over i, like from_codes)
// codes rows have stride `ld` frames and the window starts at frame `t0` (chunked / streaming decode reads a slice in place)
// STREAM: row b's window [start[b], start[b] + lens[b]) of its slot's kept codes instead (ld / t0 unused, lens == src.lens)
template <bool STREAM>
__global__ void rvq_gather_kernel(typename GatherSrc<STREAM>::T src, const float* __restrict__ table, void* __restrict__ z,
                                  int K, int T, int ncodes, int latent, int z_bf16, long long ld, int t0, const int* __restrict__ lens) {
  const int t = blockIdx.x, b = blockIdx.y;
  if (lens && t >= lens[b]) return;  // ragged decode: frames beyond the utterance's length are never read
  __shared__ int s_code[32];
  if (threadIdx.x < K) {
    long long cde;
    if constexpr (STREAM) cde = src.tab[((size_t)src.slot[b] * K + threadIdx.x) * src.cap + src.start[b] + t];
    else cde = src[((size_t)b * K + threadIdx.x) * ld + t0 + t];
    if (cde < 0) cde = 0;
    if (cde >= ncodes) cde = ncodes - 1;
    s_code[threadIdx.x] = (int)cde;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < latent; c += blockDim.x) {
    float acc = 0.f;
    for (int i = 0; i < K; ++i) acc += table[((size_t)i * ncodes + s_code[i]) * latent + c];
    if (z_bf16) reinterpret_cast<bf16_t*>(z)[((size_t)b * T + t) * latent + c] = f32_to_bf16(acc);
    else reinterpret_cast<float*>(z)[((size_t)b * T + t) * latent + c] = acc;
  }
}

// pack conv weights into MFMA A-fragment order. src element (co, ci, k) at src[co*s_co + ci*s_ci + k*s_k].
__global__ void pack_conv_kernel(const float* __restrict__ src, float* __restrict__ dst, int Cout, int Cin, int ntaps, int nphase,
                                 const int* __restrict__ ktap /*[phase][tap] -> kernel index*/, long long s_co, long long s_ci, long long s_k) {
  const int cpt = Cin / 16, nk = ntaps * cpt, nstrips = Cout / 16;
  const size_t total = (size_t)nphase * nstrips * nk * 64;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int lane = idx & 63;
  size_t r = idx >> 6;
  const int ks = (int)(r % nk); r /= nk;
  const int strip = (int)(r % nstrips);
  const int ph = (int)(r / nstrips);
  const int tap = ks / cpt, cc = ks % cpt;
  const int co = strip * 16 + (lane & 15);
  const int kidx = ktap[ph * MAXTAPS + tap];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int ci = cc * 16 + (lane >> 4) * 4 + e;
    dst[idx * 4 + e] = src[co * s_co + ci * s_ci + kidx * s_k];
  }
}

// bf16-operand mode: [phase][Cout/16][ntaps*Cin/32][64 lanes][8 bf16]; lane: row = lane & 15, channels (lane >> 4) * 8 .. + 8
__global__ void pack_conv_bf16_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst, int Cout, int Cin, int ntaps, int nphase,
                                      const int* __restrict__ ktap, long long s_co, long long s_ci, long long s_k) {
  const int cpt = Cin / 32, nk = ntaps * cpt, nstrips = Cout / 16;
  const size_t total = (size_t)nphase * nstrips * nk * 64;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int lane = idx & 63;
  size_t r = idx >> 6;
  const int ks = (int)(r % nk); r /= nk;
  const int strip = (int)(r % nstrips);
  const int ph = (int)(r / nstrips);
  const int tap = ks / cpt, cc = ks % cpt;
  const int co = strip * 16 + (lane & 15);
  const int kidx = ktap[ph * MAXTAPS + tap];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int ci = cc * 32 + (lane >> 4) * 8 + e;
    dst[idx * 8 + e] = f32_to_bf16(src[co * s_co + ci * s_ci + kidx * s_k]);
  }
}

}  // namespace
