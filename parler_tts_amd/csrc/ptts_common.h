// Shared host/device helpers for libptts_hip.so (gfx950 only; wave = 64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <string.h>
#include <stdlib.h>
#include <string>
#include <atomic>

#include "../../include/ptts.h"

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef uint16_t bf16_t;  // raw bf16 bits

// ---- error plumbing: no exception crosses the C ABI ------------------------------------------------
extern thread_local std::string g_ptts_err;
int ptts_fail(int code, const char* fmt, ...);
#define PTTS_HIP(call)                                                                       \
  do {                                                                                       \
    hipError_t _e = (call);                                                                  \
    if (_e != hipSuccess) return ptts_fail(PTTS_E_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); \
  } while (0)
#define PTTS_CHECK(cond, code, ...) \
  do {                              \
    if (!(cond)) return ptts_fail(code, __VA_ARGS__); \
  } while (0)
#define PTTS_TRY(expr)       \
  do {                       \
    int _r = (expr);         \
    if (_r != PTTS_OK) return _r; \
  } while (0)

// Every C-ABI entry point runs on the engine's device and restores the caller's current device on return (the engine
// may live on cuda:N while torch's current device is another one).
struct PttsDeviceGuard {
  int prev = -1;
  bool ok = false;
  explicit PttsDeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    ok = prev == dev || hipSetDevice(dev) == hipSuccess;
    if (prev == dev) prev = -1;  // nothing to restore
  }
  ~PttsDeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
#define PTTS_DEVICE(dev)            \
  PttsDeviceGuard _ptts_dg(dev);    \
  if (!_ptts_dg.ok) return ptts_fail(PTTS_E_HIP, "hipSetDevice(%d) failed (%s:%d)", (int)(dev), __FILE__, __LINE__)

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) applies to the CURRENT device's function object: the opt-in is tracked per
// (kernel instantiation, device), so a second engine on another GPU of the same process gets it too. Two threads racing
// on the first launch both set the attribute: idempotent.
struct PttsPerDeviceOnce {
  std::atomic<unsigned long long> mask{0};
  static int device() { int d = 0; (void)hipGetDevice(&d); return d < 0 ? 0 : (d > 63 ? 63 : d); }
  bool need(int dev) const { return !((mask.load(std::memory_order_acquire) >> dev) & 1ull); }
  void done(int dev) { mask.fetch_or(1ull << dev, std::memory_order_release); }
};

// ---- environment switches ------------------------------------------------------------------------------------------------------
// The product library reads FIFTEEN PTTS_* variables with getenv: each selects the un-fused / alternative side of a node that a parity test
// compares with the default path (table in DESIGN.md section 6; tests/test_host_logic.py counts them). The other switches that rounds 1-6 used
// for A/B measurements were removed with the paths they selected; their measurements live in profiles/.

// ---- kernel-argument preload (gfx950) ---------------------------------------------------------------------------------------------
// A wave's first instructions are s_load of its kernel arguments: one scalar round trip before the first global load can be addressed.
// gfx950's command processor can instead write the first 14 argument dwords of a dispatch into user SGPRs before the first wave starts
// (LLVM: -mllvm -amdgpu-kernarg-preload-count=14, set in __graft_entry__.build), but only for arguments the kernel takes as SCALARS - a
// by-value struct stays behind s_load. Measured on a chain of dependent GEMV nodes: -0.075 us per node (profiles/r05_experiments.txt call 9).
// The nodes of the decode step therefore take the first 56 bytes of their argument struct A - its HEAD - as scalar parameters of their own
// types (pointers stay pointers: re-assembled from integers they would lose their address space and every load would become a flat_load)
// and the rest of A as KTail<A>; A's fields are ordered so that everything a wave needs to address its FIRST loads sits in the head.
//
// Each head is declared once, as a list <H>_KHEAD(X) of entries KIND(X, ...) in parameter order. A kind hands the selector X its entry's five forms,
// X(member, parameter, join, argument, join0): the struct member (PTTS_KMEMBERS), ", type k_name" (PTTS_KPARAMS), the device join of the parameter into
// h_ (the head re-assembled in registers: SROA, no memory), ", value" for the host launch (ptts_klaunch), and what fills the struct a_ behind the head
// first. KF(X, type, name): a parameter that is the member of that name and type; KTAIL(X, A): the last parameter, KTail<A> (a head-only struct has
// none); other kinds are hooks of one declaration, defined next to it. A head is A's own first 56 bytes (PTTS_KMEMBERS opens A; PTTS_KJOIN,
// PTTS_KLAUNCH), or a struct H of its own in front of A's tail (PTTS_KJOIN_VIA: h_ and `A a`, H::unpack(a) writes what the kernel reads of A's head;
// PTTS_KLAUNCH_VIA: ptts_klaunch(kernel, ..., h, a) with h from H::pack). PTTS_KMEMBERS checks that the head is exactly 56 bytes.
typedef unsigned long long ptts_u64;
template <typename A> struct KTail {
  static_assert(sizeof(A) > 56 && sizeof(A) % 8 == 0, "argument struct: more than the 56 preloaded bytes, a multiple of 8");
  ptts_u64 w[(sizeof(A) - 56) / 8];
};
// A tail field first used by the EPILOGUE (the output pointer) would be fetched by an s_load right in front of the store - a scalar round trip at
// the end of the node's critical path. PTTS_KTOUCH(v), placed behind the wave's load burst, makes the compiler fetch it there, in the burst's shadow.
#define PTTS_KTOUCH(v) asm volatile("" ::"s"(v))
template <typename A> inline KTail<A> ptts_ktail(const A& a) {
  KTail<A> t;
  memcpy(&t, reinterpret_cast<const char*>(&a) + 56, sizeof(t));
  return t;
}

#define PTTS_KCOMMA ,  // a form's leading comma, produced only after the selector has split its arguments
#define PTTS_KSEL_MEMBER(m, p, j, g, j0) m
#define PTTS_KSEL_PARAM(m, p, j, g, j0) p
#define PTTS_KSEL_JOIN(m, p, j, g, j0) j
#define PTTS_KSEL_ARG(m, p, j, g, j0) g
#define PTTS_KSEL_JOIN0(m, p, j, g, j0) j0
#define KF(X, T, n) X(T n;, PTTS_KCOMMA T k_##n, h_.n = k_##n;, PTTS_KCOMMA h_.n, )
#define KTAIL(X, A) X(, PTTS_KCOMMA KTail<A> k_tail, , PTTS_KCOMMA ptts_ktail(a_), __builtin_memcpy(reinterpret_cast<char*>(&a_) + 56, &k_tail, sizeof(k_tail));)

#define PTTS_KMEMBERS(H)                                                                                              \
  struct KHeadEnd_ { H##_KHEAD(PTTS_KSEL_MEMBER) char end_; };                                                        \
  static_assert(offsetof(KHeadEnd_, end_) == 56, #H ": the head is exactly the 56 preloaded bytes (14 dwords)");       \
  H##_KHEAD(PTTS_KSEL_MEMBER)
#define PTTS_KDROP1_(x, ...) __VA_ARGS__
#define PTTS_KDROP1(...) PTTS_KDROP1_(__VA_ARGS__)
#define PTTS_KPARAMS(H) PTTS_KDROP1(H##_KHEAD(PTTS_KSEL_PARAM))
#define PTTS_KJOIN(A, a) A a; { A& a_ = a; A& h_ = a; A##_KHEAD(PTTS_KSEL_JOIN0) A##_KHEAD(PTTS_KSEL_JOIN) }
#define PTTS_KJOIN_VIA(H, A, a) A a; H h_; { A& a_ = a; H##_KHEAD(PTTS_KSEL_JOIN0) H##_KHEAD(PTTS_KSEL_JOIN) } h_.unpack(a);
#define PTTS_KLAUNCH(A) template <typename Kn> inline void ptts_klaunch(Kn kern, dim3 grid, dim3 block, size_t shmem, hipStream_t st, const A& a_) {   \
    const A& h_ = a_;                                                                                                            \
    hipLaunchKernelGGL(kern, grid, block, shmem, st A##_KHEAD(PTTS_KSEL_ARG));                                                   \
  }
#define PTTS_KLAUNCH_VIA(H, A) template <typename Kn> inline void ptts_klaunch(Kn kern, dim3 grid, dim3 block, size_t shmem, hipStream_t st, const H& h_, const A& a_) { \
    hipLaunchKernelGGL(kern, grid, block, shmem, st H##_KHEAD(PTTS_KSEL_ARG));                                                               \
  }

// ---- bf16 <-> f32 (round-to-nearest-even, identical to torch's .to(bfloat16)) -------------------------
__host__ __device__ __forceinline__ bf16_t f32_to_bf16(float f) {
  uint32_t u;
#if defined(__HIP_DEVICE_COMPILE__)
  u = __float_as_uint(f);
#else
  memcpy(&u, &f, 4);
#endif
  if ((u & 0x7fffffffu) > 0x7f800000u) return (bf16_t)0x7fc0;  // NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (bf16_t)(u >> 16);
}
__device__ __forceinline__ float bf16_to_f32(bf16_t h) { return __uint_as_float(((uint32_t)h) << 16); }
// two fp32 -> packed bf16 pair with ONE v_cvt_pk_bf16_f32 (gfx950; round-to-nearest-even like f32_to_bf16 above)
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
  typedef __attribute__((ext_vector_type(2))) float f32x2_t;
  typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
  const f32x2_t v = {lo, hi};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_t));
}

// element traits of the engine dtype
template <typename WT> struct Elem;
template <> struct Elem<float> {
  static constexpr int KT = 16;   // k per packed weight fragment (4 x mfma_f32_16x16x4f32)
  static constexpr int EPL = 4;   // elements per 16-byte lane load
  static __device__ __forceinline__ float ld(const float* p) { return *p; }
  static __device__ __forceinline__ float rnd(float v) { return v; }  // value as stored in this dtype
};
template <> struct Elem<bf16_t> {
  static constexpr int KT = 32;   // 1 x mfma_f32_16x16x32_bf16
  static constexpr int EPL = 8;
  static __device__ __forceinline__ float ld(const bf16_t* p) { return bf16_to_f32(*p); }
  static __device__ __forceinline__ float rnd(float v) { return bf16_to_f32(f32_to_bf16(v)); }
};

// unpack a 16-byte lane load into EPL floats
__device__ __forceinline__ void unpack16(const uint4& v, float (&o)[4], float) {
  o[0] = __uint_as_float(v.x); o[1] = __uint_as_float(v.y); o[2] = __uint_as_float(v.z); o[3] = __uint_as_float(v.w);
}
__device__ __forceinline__ void unpack16(const uint4& v, float (&o)[8], bf16_t) {
  o[0] = __uint_as_float(v.x << 16); o[1] = __uint_as_float(v.x & 0xffff0000u);
  o[2] = __uint_as_float(v.y << 16); o[3] = __uint_as_float(v.y & 0xffff0000u);
  o[4] = __uint_as_float(v.z << 16); o[5] = __uint_as_float(v.z & 0xffff0000u);
  o[6] = __uint_as_float(v.w << 16); o[7] = __uint_as_float(v.w & 0xffff0000u);
}
__device__ __forceinline__ uint4 pack16(const float (&o)[4], float) {
  return make_uint4(__float_as_uint(o[0]), __float_as_uint(o[1]), __float_as_uint(o[2]), __float_as_uint(o[3]));
}
__device__ __forceinline__ uint4 pack16(const float (&o)[8], bf16_t) {
  return make_uint4(pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]), pack_bf16x2(o[4], o[5]), pack_bf16x2(o[6], o[7]));
}

// 16-byte non-temporal (streamed-once) global load: weights are read exactly once per decode step
__device__ __forceinline__ uint4 ld_nt16(const uint4* p) {
  typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
  const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
  return make_uint4(v.x, v.y, v.z, v.w);
}

// 8 OCP e4m3 bytes -> 8 packed bf16 (exact: 3 mantissa bits into 7), 4 x v_cvt_scalef32_pk_bf16_fp8 with scale 1.0
__device__ __forceinline__ uint4 e4m3x8_to_bf16x8(uint32_t lo, uint32_t hi) {
  typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
  const bf16x2_t a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false), b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true);
  const bf16x2_t c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false), d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true);
  return make_uint4(__builtin_bit_cast(uint32_t, a), __builtin_bit_cast(uint32_t, b), __builtin_bit_cast(uint32_t, c), __builtin_bit_cast(uint32_t, d));
}

// ---- cross-lane reductions without LDS ---------------------------------------------------------------------
// __shfl_xor lowers to ds_bpermute (an LDS round trip, ~100 cycles each; 12 of them were most of the LayerNorm
// chain in the first profile). These use DPP row operations inside a 16-lane row and v_permlane16/32_swap (gfx950)
// across rows: 6 dependent VALU ops for a full wave64 reduction, result in EVERY lane.
template <int CTRL> __device__ __forceinline__ float dpp_mov(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xf, 0xf, true));
}
struct OpSum { static __device__ __forceinline__ float f(float a, float b) { return a + b; } };
struct OpMax { static __device__ __forceinline__ float f(float a, float b) { return fmaxf(a, b); } };

template <typename Op> __device__ __forceinline__ float swap16_reduce(float v) {  // combine adjacent 16-lane rows
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return Op::f(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
template <typename Op> __device__ __forceinline__ float swap32_reduce(float v) {  // combine the two 32-lane halves
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return Op::f(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
// reduce within aligned groups of G lanes (G = 8 or 16), result in every lane of the group
template <typename Op, int G> __device__ __forceinline__ float group_reduce(float v) {
  v = Op::f(v, dpp_mov<0xB1>(v));   // quad_perm [1,0,3,2]
  v = Op::f(v, dpp_mov<0x4E>(v));   // quad_perm [2,3,0,1]
  v = Op::f(v, dpp_mov<0x141>(v));  // row_half_mirror: other quad of the 8-lane half
  if (G == 16) v = Op::f(v, dpp_mov<0x140>(v));  // row_mirror: other half of the row
  return v;
}
// lane-wise reduction across the 64/G aligned groups of G lanes (lane c of every group combines with lane c of the
// others), result in every lane
template <typename Op, int G> __device__ __forceinline__ float across_groups_reduce(float v) {
  if (G == 8) v = Op::f(v, dpp_mov<0x128>(v));  // row_ror:8 == xor 8 inside a 16-lane row
  v = swap16_reduce<Op>(v);
  return swap32_reduce<Op>(v);
}
template <typename Op> __device__ __forceinline__ float wave_reduce(float v) {
  return across_groups_reduce<Op, 16>(group_reduce<Op, 16>(v));
}
__device__ __forceinline__ float wave_sum(float v) { return wave_reduce<OpSum>(v); }
__device__ __forceinline__ float wave_max(float v) { return wave_reduce<OpMax>(v); }

// Both LayerNorm sums in ONE reduction tree: a permlane32 swap puts sum-halves of s1 in lanes 0-31 and of s2 in lanes
// 32-63, five more steps finish both (6 dependent cross-lane ops instead of 12); read back with v_readlane.
__device__ __forceinline__ void gv_pair_sum(float& s1, float& s2) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(s1), __float_as_uint(s2), false, false);
  float t = __uint_as_float(r[0]) + __uint_as_float(r[1]);  // lanes 0-31: s1[l] + s1[l+32]; lanes 32-63: s2[l-32] + s2[l]
  t = swap16_reduce<OpSum>(t);
  t = group_reduce<OpSum, 16>(t);
  s1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t), 0));
  s2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t), 32));
}

// ---- phases the decode-step kernels share ------------------------------------------------------------------------------------------
// One function per phase; the kernels of ptts_lm_kernels.h and ptts_gemv_kernels.h call it with values they have already loaded (where a
// load is issued - row first, rendezvous, weights - is each kernel's own business) and store through a functor. Whatever changes a rounding
// is a template parameter: two kernels that pass the same parameters compute the same bits. The few call sites where the call moved the
// kernel's loop shape or register count keep the phase written out, under a comment that names the function here.

// LayerNorm of a row (nn.LayerNorm, eps 1e-5): mean and variance from ONE pass of sum(x - c) and sum((x - c)^2) with the shift c = x[0]
// (shifted-data variance: no catastrophic cancellation, error ~ eps * (1 + (mean - c)^2 / var)).
__device__ __forceinline__ void ln_accum4(const float4& t, float c, float& s1, float& s2) {
  const float d0 = t.x - c, d1 = t.y - c, d2 = t.z - c, d3 = t.w - c;
  s1 += (d0 + d1) + (d2 + d3);
  s2 += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
}
// the row in registers, NF4 float4 per lane (element (lane + 64 i) * 4); EXACT: K == NF4 * 256, otherwise the lanes at or beyond K count as zero
template <int NF4, bool EXACT = true>
__device__ __forceinline__ void ln_row_sums(const float4 (&v)[NF4], int lane, int K, float& c, float& s1, float& s2) {
  c = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v[0].x)));
  s1 = 0.f; s2 = 0.f;
#pragma unroll
  for (int i = 0; i < NF4; ++i) {
    if constexpr (EXACT) {
      ln_accum4(v[i], c, s1, s2);
    } else {
      const float msk = (lane + 64 * i) * 4 < K ? 1.f : 0.f;
      const float d0 = (v[i].x - c) * msk, d1 = (v[i].y - c) * msk, d2 = (v[i].z - c) * msk, d3 = (v[i].w - c) * msk;
      s1 += (d0 + d1) + (d2 + d3);
      s2 += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    }
  }
}
// The two reduction trees in use round differently: two full wave reductions (MFMA-strip kernels), or both sums in one tree (GEMV kernels).
struct LnWaveSums { static __device__ __forceinline__ void reduce(float& s1, float& s2) { s1 = wave_sum(s1); s2 = wave_sum(s2); } };
struct LnPairSum { static __device__ __forceinline__ void reduce(float& s1, float& s2) { gv_pair_sum(s1, s2); } };
__device__ __forceinline__ void ln_mean_rstd(float c, float s1, float s2, float invK, float& mean, float& rstd) {
  const float dm = s1 * invK;
  mean = c + dm;
  rstd = rsqrtf(fmaxf(s2 * invK - dm * dm, 0.f) + 1e-5f);
}
template <typename Tree, int NF4>
__device__ __forceinline__ void ln_row_stats(const float4 (&v)[NF4], float invK, float& mean, float& rstd) {
  float c, s1, s2;
  ln_row_sums<NF4>(v, 0, 0, c, s1, s2);
  Tree::reduce(s1, s2);
  ln_mean_rstd(c, s1, s2, invK, mean, rstd);
}
__device__ __forceinline__ float ln_norm(float x, float mean, float rstd, float g, float b) { return (x - mean) * rstd * g + b; }
// st(k, a, b, c, d): elements k .. k + 3 of the normalised row
template <int NF4, typename Store>
__device__ __forceinline__ void ln_row_store(const float4 (&v)[NF4], const float4 (&g)[NF4], const float4 (&bt)[NF4], float mean, float rstd, int lane, Store&& st) {
#pragma unroll
  for (int i = 0; i < NF4; ++i)
    st((lane + 64 * i) * 4, ln_norm(v[i].x, mean, rstd, g[i].x, bt[i].x), ln_norm(v[i].y, mean, rstd, g[i].y, bt[i].y), ln_norm(v[i].z, mean, rstd, g[i].z, bt[i].z),
       ln_norm(v[i].w, mean, rstd, g[i].w, bt[i].w));
}

// RW weight rows of this wave (chunk c * 64 + lane of each row, in registers) against the prepared row in LDS (engine dtype): chunk-parity
// accumulators, one wave reduction per row, row rr's dot product in lane rr (gemv_kernel's order). Dot = GvDot<WT, W8> (ptts_gemv_kernels.h).
template <typename Dot, int RW, int NCH, typename WV>
__device__ __forceinline__ float wave_rows_dot(const WV (&wv)[RW][NCH], const char* s_x, int lane) {
  uint4 xv[NCH];
#pragma unroll
  for (int cc = 0; cc < NCH; ++cc) xv[cc] = *reinterpret_cast<const uint4*>(s_x + (size_t)(cc * 64 + lane) * 16);
  float acc[RW], acc2[RW];
#pragma unroll
  for (int rr = 0; rr < RW; ++rr) { acc[rr] = 0.f; acc2[rr] = 0.f; }
#pragma unroll
  for (int cc = 0; cc < NCH; ++cc)
#pragma unroll
    for (int rr = 0; rr < RW; ++rr) {
      if (cc & 1) acc2[rr] = Dot::run(wv[rr][cc], xv[cc], acc2[rr]);
      else acc[rr] = Dot::run(wv[rr][cc], xv[cc], acc[rr]);
    }
  float v = 0.f;
#pragma unroll
  for (int rr = 0; rr < RW; ++rr) {
    const float t = wave_sum(acc[rr] + acc2[rr]);
    v = lane == rr ? t : v;
  }
  return v;
}

// ---- single-query attention over K / V row groups (attn_kernel, qkv_attn_kernel, xq_attn_kernel, xattn_fused_kernel) --------------------------
// A wave-load covers RPI = 64 / LPR rows of 64 elements: lane (r, c) = (lane / LPR, lane % LPR) holds chunk c (EPL elements) of row r.
__device__ __forceinline__ void kv8_unpack8(const uint2& v, float (&o)[8]) {
  const auto a = __builtin_amdgcn_cvt_pk_f32_fp8((int)v.x, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)v.x, true);
  const auto c = __builtin_amdgcn_cvt_pk_f32_fp8((int)v.y, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)v.y, true);
  o[0] = a[0]; o[1] = a[1]; o[2] = b[0]; o[3] = b[1]; o[4] = c[0]; o[5] = c[1]; o[6] = d[0]; o[7] = d[1];
}
struct AttnExp2 { static __device__ __forceinline__ float f(float x) { return __builtin_amdgcn_exp2f(x); } };  // scores in log2 units
struct AttnExpE { static __device__ __forceinline__ float f(float x) { return expf(x); } };
// Online-softmax update for one batch of U row groups already in registers: scores of the (scaled) query chunk qv, block maximum, rescale of the
// running (m, l, o), accumulation. visible(u): the caller's predicate for row group u (an invisible row weighs 0 and its data is never used -
// it may be NaN / garbage). KV8: rows are 64 e4m3 bytes, the K row's scale ksc multiplies the score, the V row's vsc rides on the probability.
template <typename WT, typename Exp, bool KV8, int U, typename KVV, int NS, int EPL, typename Vis>
__device__ __forceinline__ void attn_online_update(const KVV (&kf)[U], const KVV (&vf)[U], Vis&& visible, const float (&ksc)[NS], const float (&vsc)[NS],
                                                   const float (&qv)[EPL], float& m_run, float& l_run, float (&o)[EPL]) {
  constexpr int LPR = 64 / EPL;
  bool ok[U];
  float sc[U], bm = -INFINITY;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    ok[u] = visible(u);
    float kx[EPL];
    if constexpr (KV8) kv8_unpack8(kf[u], kx);
    else unpack16(kf[u], kx, WT());
    float d = 0.f;
#pragma unroll
    for (int e = 0; e < EPL; ++e) d = fmaf(qv[e], kx[e], d);
    d = group_reduce<OpSum, LPR>(d);
    if constexpr (KV8) d *= ksc[u];
    sc[u] = ok[u] ? d : -INFINITY;
    bm = fmaxf(bm, sc[u]);
  }
  bm = across_groups_reduce<OpMax, LPR>(bm);
  const float m_new = fmaxf(m_run, bm);
  if (m_new == -INFINITY) return;  // wave-uniform: nothing visible yet
  const float alpha = (m_run == -INFINITY) ? 0.f : Exp::f(m_run - m_new);
  l_run *= alpha;
#pragma unroll
  for (int e = 0; e < EPL; ++e) o[e] *= alpha;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const float p = ok[u] ? Exp::f(sc[u] - m_new) : 0.f;
    float vx[EPL];
    if constexpr (KV8) kv8_unpack8(vf[u], vx);
    else unpack16(vf[u], vx, WT());
    l_run += p;
    const float pv = KV8 ? p * vsc[KV8 ? u : 0] : p;
#pragma unroll
    for (int e = 0; e < EPL; ++e) o[e] = ok[u] ? fmaf(pv, vx[e], o[e]) : o[e];
  }
  m_run = m_new;
}
template <typename WT, typename Exp, int U, int EPL, typename Vis>  // rows in the engine dtype: no row scales
__device__ __forceinline__ void attn_online_update(const uint4 (&kf)[U], const uint4 (&vf)[U], Vis&& visible, const float (&qv)[EPL], float& m_run, float& l_run, float (&o)[EPL]) {
  const float none[1] = {1.f};
  attn_online_update<WT, Exp, false>(kf, vf, visible, none, none, qv, m_run, l_run, o);
}
// sum over the RPI row slots of the wave (lanes sharing chunk c), result in every lane
template <int EPL>
__device__ __forceinline__ void attn_row_slots_sum(float& l_run, float (&o)[EPL]) {
  l_run = across_groups_reduce<OpSum, 64 / EPL>(l_run);
#pragma unroll
  for (int e = 0; e < EPL; ++e) o[e] = across_groups_reduce<OpSum, 64 / EPL>(o[e]);
}
// this wave's partial context and (max, sumexp) into its slots so[64] / sml[2] of the workgroup's merge buffers
template <int EPL>
__device__ __forceinline__ void attn_wave_publish(float* so, float* sml, int r, int c, float m_run, float l_run, const float (&o)[EPL]) {
  if (r == 0) {
#pragma unroll
    for (int e = 0; e < EPL; ++e) so[c * EPL + e] = o[e];
    if (c == 0) { sml[0] = m_run; sml[1] = l_run; }
  }
}
// merge of NW consecutive waves' partials (fixed order: deterministic): columns col0 .. col0 + NC - 1 of the context, the maximum and the sum
template <typename Exp, int NW, int NC>
__device__ __forceinline__ void attn_waves_merge(const float* so, const float* sml, int col0, float& M, float& l, float (&o)[NC]) {
  M = -INFINITY;
#pragma unroll
  for (int i = 0; i < NW; ++i) M = fmaxf(M, sml[i * 2]);
  l = 0.f;
#pragma unroll
  for (int e = 0; e < NC; ++e) o[e] = 0.f;
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const float mi = sml[i * 2];
    const float wgt = (mi == -INFINITY) ? 0.f : Exp::f(mi - M);
    l += wgt * sml[i * 2 + 1];
#pragma unroll
    for (int e = 0; e < NC; ++e) o[e] += wgt * so[i * 64 + col0 + e];
  }
}

// ---- 64-key block of the f32-MFMA attention kernels (prefill_attn_mfma_kernel, t5_attn_mfma_kernel) ----------------------------------
// K / V tiles in LDS as fp32 [64 keys][16 slots of 16 B], slot XOR-swizzled by key & 15; lane (j = l & 15, g = l >> 4).
// Round 6, call 46: the compiler had scheduled each fragment read directly in front of its MFMAs - ds_read -> s_waitcnt lgkmcnt(0) -> MFMA, 16 + 64 LDS
// round trips in a row per key block (~5 us of a 14 us launch for 1.7 us of MFMA issue). Now every fragment of a phase is requested before the first
// MFMA of that phase (a scheduling barrier keeps the order; the waits become counted), and V is read as ONE b128 per (key, lane) instead of four b32:
// output tile dt of lane j is column d = 4 j + dt (was 16 dt + j) - which lane holds which column changes, the sum of each output does not.
// S^T = K Q^T: lane ends up with the scores of query j against keys 16 kt + 4 g + r; k order d = 16 c + e + 4 g over (c, e) then g.
__device__ __forceinline__ void attn_block_scores(const float4* sK4, int j, int g, const float4 (&qr)[4], f32x4 (&st)[4]) {
  float4 kr[4][4];
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) kr[c][kt] = sK4[(16 * kt + j) * 16 + ((4 * c + g) ^ j)];
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) st[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 4; ++c) {  // four independent accumulator chains interleaved; each chain's own order is (c, e) as before
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) st[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(kr[c][kt].x, qr[c].x, st[kt], 0, 0, 0);
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) st[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(kr[c][kt].y, qr[c].y, st[kt], 0, 0, 0);
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) st[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(kr[c][kt].z, qr[c].z, st[kt], 0, 0, 0);
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) st[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(kr[c][kt].w, qr[c].w, st[kt], 0, 0, 0);
  }
}
// V rows of this lane's 16 keys, columns 4 j .. 4 j + 3: requested behind the score MFMAs, in flight under the softmax
__device__ __forceinline__ void attn_block_v_request(const float4* sV4, int j, int g, float4 (&vb)[4][4]) {
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * kt + 4 * g + r;
      vb[kt][r] = sV4[row * 16 + (j ^ (row & 15))];
    }
  __builtin_amdgcn_sched_barrier(0);
}
// O += P V with the lane's own probabilities as the A operand (the MFMA sums over g): o[dt][r] = query 4 g + r, column 4 j + dt;
// k order keys 16 kt + r + 4 g over (kt, r) then g
__device__ __forceinline__ void attn_block_pv(const f32x4 (&p)[4], const float4 (&vb)[4][4], f32x4 (&o)[4]) {
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      o[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[kt][r], vb[kt][r].x, o[0], 0, 0, 0);
      o[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[kt][r], vb[kt][r].y, o[1], 0, 0, 0);
      o[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[kt][r], vb[kt][r].z, o[2], 0, 0, 0);
      o[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[kt][r], vb[kt][r].w, o[3], 0, 0, 0);
    }
}
