// The T5 description encoder's attention kernels (t5_attn_kernel, t5_attn_mfma_kernel) and their argument struct, apart from ptts_t5.hip so that
// tests/native/attn_harness.hip launches the same code on buffers of its own. The kernels live in an unnamed namespace, as they did in that
// file: every includer gets instances of its own.
#pragma once
#include "ptts_common.h"
#include "ptts_lm_kernels.h"

namespace {

// The attention kernels take the whole struct as SCALAR parameters (14 dwords = exactly what the command processor preloads into SGPRs before the first
// wave starts, -mllvm -amdgpu-kernarg-preload-count=14, ptts_common.h): no s_load in front of the wave's first loads (call 54). Head only: no tail.
#define T5AttnArgs_KHEAD(X)                                                                                                             \
  KF(X, const float*, qkv)    /* [B*N][ld] fp32: q at column h*64, k at inner + h*64, v at 2*inner + h*64 */                            \
  KF(X, int, ld) KF(X, int, inner)                                                                                                      \
  KF(X, const float*, bias)   /* [heads][bias_ld], entry (key - query) + bias_zero */                                                   \
  KF(X, int, bias_ld) KF(X, int, bias_zero)                                                                                             \
  KF(X, const int*, mask)     /* [B][N] int32 (1 = keep) or null */                                                                     \
  KF(X, void*, out)           /* [B*N][inner] engine dtype, row-major or MFMA B-fragment order */                                       \
  KF(X, int, N)                                                                                                                         \
  KF(X, int, out_fo)
struct T5AttnArgs {
  PTTS_KMEMBERS(T5AttnArgs)
};
PTTS_KLAUNCH(T5AttnArgs)

// T5Attention.forward, encoder self-attention: scores = q k^T (NO 1/sqrt(d) scale) + position_bias (+ (1 - mask) * finfo.min), softmax in fp32,
// context = p v. One workgroup = 8 queries of one (utterance, head): 4 waves x 2 queries; keys in tiles of 64 (lane = key), K / V tiles staged in
// LDS once per workgroup, online softmax across tiles. A masked key keeps the score -FLT_MAX exactly as the additive mask leaves it (a fully
// masked row is therefore uniform over all N keys, like the reference); keys beyond N do not exist.
template <typename WT>
__global__ void __launch_bounds__(256) t5_attn_kernel(PTTS_KPARAMS(T5AttnArgs)) {
  PTTS_KJOIN(T5AttnArgs, a)
  constexpr int QW = 2, QB = 4 * QW, EPL = Elem<WT>::EPL;
  __shared__ float sK[64 * 65];
  __shared__ __attribute__((aligned(16))) float sV[64 * 64];
  __shared__ float sQ[QB][64];
  __shared__ float sP[QB][64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int h = blockIdx.y, b = blockIdx.z, i0 = blockIdx.x * QB;
  const float* base = a.qkv + (size_t)b * a.N * a.ld;
  for (int e = tid; e < QB * 64; e += 256) {
    const int qi = e >> 6, d = e & 63, i = min(i0 + qi, a.N - 1);
    sQ[qi][d] = base[(size_t)i * a.ld + h * 64 + d];
  }
  float m_run[QW], l_run[QW], o[QW];
#pragma unroll
  for (int q = 0; q < QW; ++q) { m_run[q] = -INFINITY; l_run[q] = 0.f; o[q] = 0.f; }
  for (int j0 = 0; j0 < a.N; j0 += 64) {
    __syncthreads();  // the previous tile is consumed (first pass: sQ is visible)
    for (int e = tid; e < 64 * 16; e += 256) {
      const int r = e >> 4, c4 = e & 15, j = j0 + r;
      float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
      if (j < a.N) {
        kv = *reinterpret_cast<const float4*>(base + (size_t)j * a.ld + a.inner + h * 64 + c4 * 4);
        vv = *reinterpret_cast<const float4*>(base + (size_t)j * a.ld + 2 * a.inner + h * 64 + c4 * 4);
      }
      float* kd = sK + r * 65 + c4 * 4;
      kd[0] = kv.x; kd[1] = kv.y; kd[2] = kv.z; kd[3] = kv.w;
      *reinterpret_cast<float4*>(sV + r * 64 + c4 * 4) = vv;
    }
    __syncthreads();
    const int j = j0 + lane;
    const bool exists = j < a.N;
    const bool kept = exists && (!a.mask || a.mask[(size_t)b * a.N + j] != 0);
    float s[QW];
#pragma unroll
    for (int q = 0; q < QW; ++q) s[q] = 0.f;
    for (int d = 0; d < 64; ++d) {
      const float kd = sK[lane * 65 + d];
#pragma unroll
      for (int q = 0; q < QW; ++q) s[q] = fmaf(sQ[w * QW + q][d], kd, s[q]);
    }
#pragma unroll
    for (int q = 0; q < QW; ++q) {
      const int i = min(i0 + w * QW + q, a.N - 1);
      const float bias = a.bias[(size_t)h * a.bias_ld + (min(j, a.N - 1) - i) + a.bias_zero];
      const float sc = !exists ? -INFINITY : (kept ? s[q] + bias : -3.402823466e38f);
      const float m_new = fmaxf(m_run[q], wave_max(sc));
      const float alpha = m_run[q] == -INFINITY ? 0.f : expf(m_run[q] - m_new);
      const float p = exists ? expf(sc - m_new) : 0.f;
      l_run[q] = l_run[q] * alpha + wave_sum(p);
      o[q] *= alpha;
      m_run[q] = m_new;
      sP[w * QW + q][lane] = p;
    }
    __syncthreads();
    for (int jj = 0; jj < 64; ++jj) {
      const float v = sV[jj * 64 + lane];
#pragma unroll
      for (int q = 0; q < QW; ++q) o[q] = fmaf(sP[w * QW + q][jj], v, o[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < QW; ++q) {
    const int i = i0 + w * QW + q;
    if (i >= a.N) continue;
    const int m = b * a.N + i, kcol = h * 64 + lane;
    WT* dst = reinterpret_cast<WT*>(a.out);
    if (a.out_fo) dst += fo_vec_index<WT>(m, kcol & ~(EPL - 1), a.inner / Elem<WT>::KT) * EPL + (kcol & (EPL - 1));
    else dst += (size_t)m * a.inner + kcol;
    store_from_f32<WT>(dst, o[q] / l_run[q]);
  }
}

// t5_attn_mfma_kernel (round 6): the same attention on the f32-input MFMA (v_mfma_f32_16x16x4_f32: exact fp32, an fmaf chain per output - the
// arithmetic of the kernel above in another summation order), for batches that fill the chip: t5_attn_kernel spends 34 us per block at 32 x 64 tokens
// (16 TFLOP/s of VALU fmaf behind one LDS read per fmaf pair; profiles/r06_prefill_kernels_bs32_v1.txt). One workgroup = 64 queries of one
// (utterance, head), one wave = 16 queries x ALL keys, key blocks of 64 with the K / V tiles in LDS (fp32, 16-byte slots XOR-swizzled by row & 15:
// the b128 fragment reads of K and the b32 reads of V are both conflict-free without padding):
//   S^T = K Q^T   A = K[key][d], B = Q[query][d] (Q fragments live in registers): lane (i = l & 15, g = l >> 4) ends up holding the scores of
//                 query i against keys 16 kt + 4 g + r - 16 of the block's 64 keys, the other 48 in the three lanes with the same i
//   softmax       per query across those 4 lanes (permlane swaps), online across key blocks
//   O = P V       A = P: step (kt, r) takes the lane's OWN register P[i][16 kt + 4 g + r] (the MFMA sums over g: no transpose, no LDS round trip
//                 for the probabilities), B = V[16 kt + 4 g + r][4 j + dt] (one b128 read per key: ptts_common.h, attn_block_*)
// k order of the q.k sums: d = 16 c + e + 4 g over (c, e) then g (fixed, deterministic); of the p.v sums: keys 16 kt + r + 4 g over (kt, r) then g.
template <typename WT>
__global__ void __launch_bounds__(256) t5_attn_mfma_kernel(PTTS_KPARAMS(T5AttnArgs)) {
  PTTS_KJOIN(T5AttnArgs, a)
  __shared__ __attribute__((aligned(16))) float sK[64 * 64];
  __shared__ __attribute__((aligned(16))) float sV[64 * 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, j = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, b = blockIdx.z, i0 = blockIdx.x * 64 + w * 16;
  const float* base = a.qkv + (size_t)b * a.N * a.ld;
  const int iq = min(i0 + j, a.N - 1);  // clamped queries are computed and dropped
  float4 qr[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) qr[c] = *reinterpret_cast<const float4*>(base + (size_t)iq * a.ld + h * 64 + 16 * c + 4 * g);
  float m_run = -INFINITY, l_run = 0.f;
  f32x4 o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float4* sK4 = reinterpret_cast<const float4*>(sK);
  for (int j0 = 0; j0 < a.N; j0 += 64) {
    if (j0) __syncthreads();  // the previous tiles are consumed
    // (call 38) every global load is unconditional on a clamped address and selected afterwards: inside per-lane conditions each one had been compiled into
    // its own branch + s_waitcnt vmcnt(0) - 8 + 32 dependent round trips per key block (tools/isa_load_chains.py)
    float4 kq[4], vq[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = tid + 256 * u, r = e >> 4, sl = e & 15, key = min(j0 + r, a.N - 1);
      kq[u] = *reinterpret_cast<const float4*>(base + (size_t)key * a.ld + a.inner + h * 64 + sl * 4);
      vq[u] = *reinterpret_cast<const float4*>(base + (size_t)key * a.ld + 2 * a.inner + h * 64 + sl * 4);
    }
    // bias and key flags of this lane's 16 (query, key) pairs: independent of the tiles, in flight across the barrier
    float bias[4][4];
    int flag[4][4];  // 0: no such key, 1: masked, 2: kept
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int kc = min(j0 + 16 * kt + 4 * g + r, a.N - 1);
        bias[kt][r] = a.bias[(size_t)h * a.bias_ld + (kc - iq) + a.bias_zero];
        flag[kt][r] = 2;
      }
    if (a.mask) {  // wave-uniform
      int mv[4][4];
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) mv[kt][r] = a.mask[(size_t)b * a.N + min(j0 + 16 * kt + 4 * g + r, a.N - 1)];
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) flag[kt][r] = mv[kt][r] != 0 ? 2 : 1;
    }
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (j0 + 16 * kt + 4 * g + r >= a.N) flag[kt][r] = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = tid + 256 * u, r = e >> 4, sl = e & 15;
      const bool live = j0 + r < a.N;
      reinterpret_cast<float4*>(sK)[r * 16 + (sl ^ (r & 15))] = live ? kq[u] : make_float4(0.f, 0.f, 0.f, 0.f);
      reinterpret_cast<float4*>(sV)[r * 16 + (sl ^ (r & 15))] = live ? vq[u] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    f32x4 st[4];
    attn_block_scores(sK4, j, g, qr, st);
    float4 vb[4][4];
    attn_block_v_request(reinterpret_cast<const float4*>(sV), j, g, vb);
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float sc = flag[kt][r] == 0 ? -INFINITY : (flag[kt][r] == 2 ? st[kt][r] + bias[kt][r] : -3.402823466e38f);
        st[kt][r] = sc;
        mx = fmaxf(mx, sc);
      }
    const float m_new = fmaxf(m_run, across_groups_reduce<OpMax, 16>(mx));
    const float alpha = m_run == -INFINITY ? 0.f : expf(m_run - m_new);
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pv = flag[kt][r] == 0 ? 0.f : expf(st[kt][r] - m_new);
        st[kt][r] = pv;
        sum += pv;
      }
    l_run = l_run * alpha + across_groups_reduce<OpSum, 16>(sum);
    m_run = m_new;
    if (j0) {  // the accumulators hold queries 4 g + r; their factors live in the lanes whose l & 15 is that query
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float ar = __shfl(alpha, 4 * g + r);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt][r] *= ar;
      }
    }
    attn_block_pv(st, vb, o);
  }
  WT* dst0 = reinterpret_cast<WT*>(a.out);
#pragma unroll
  for (int r = 0; r < 4; ++r) {  // o[dt][r]: query 4 g + r, column 4 j + dt of the head - four consecutive elements per lane
    const float lr = __shfl(l_run, 4 * g + r);
    const int i = i0 + 4 * g + r;
    if (i >= a.N) continue;
    act_store4<WT>(dst0, b * a.N + i, h * 64 + 4 * j, a.inner, a.out_fo, o[0][r] / lr, o[1][r] / lr, o[2][r] / lr, o[3][r] / lr);
  }
}

}  // namespace
