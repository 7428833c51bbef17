// Teacher-forced scoring (include/ptts_score.h): the raw-column embedding and the final LayerNorm + LM heads + cross-entropy kernel.
//
// score_heads_kernel<WT, MT, STORE>: one workgroup owns 16 * MT scored rows and ONE codebook (grid = (row tiles, K)). The rows' final LayerNorm
// output is staged once in LDS in the engine dtype (the rounding model of the PRO_LN prologue: fp32 statistics, one rounding to WT), then every
// wave walks its share of the codebook's V / 16 weight strips (e->heads, the fragment order pack_weight_kernel writes) and multiplies each strip
// against all MT row tiles: mfma_f32_16x16x4f32 (fp32 engine) / mfma_f32_16x16x32_bf16 (bf16 engine), A = 16 vocabulary rows of the strip,
// B = 16 residual rows, so lane (q, j) = (lane >> 4, lane & 15) holds logits of row j at columns strip * 16 + q * 4 + {0..3}. The K reduction
// stays inside one wave (one accumulator chain order per logit, whatever the wave count). Each lane keeps a running (max, sum) in base 2 and the
// label's logit for the rows it owns; the 4 * waves partials of a row meet once, in a fixed order, through LDS at the end of the codebook:
//   nll = ln2 * (max2 + log2(sum)) - logit[label]
// No logits and no partials go through memory. STORE = true is the same kernel with one more float4 store per lane and strip: the optional
// logits output [B * K][Q_out][V] of ptts_score comes from this flag, not from a second projection, so both instances give the same nll bits.
#pragma once
#include "ptts_lm_kernels.h"

// Residual rows of a teacher-forced pass: P prompt rows (prompt embedding + position, as embed_kernel's prefill rows), then the T given columns as
// they are - no delay pattern, no BOS column: sum_k E_k[input_ids[b * K + k][j]] + position P + j  (modeling:1433, :1506-1511)
struct EmbedRawArgs {
  const void* tables;      // [K][V+1][H] engine dtype
  const float* pos_table;  // [max_pos][H] or null (RoPE)
  const float* prompt;     // [B][P][H] or null
  const long long* ids;    // [B*K][T]
  float* h;                // [B][P + T][H]
  int H, K, V1, P, T;
};

template <typename WT>
__global__ void embed_raw_kernel(EmbedRawArgs a) {
  const int b = blockIdx.y, qi = blockIdx.x, Q = a.P + a.T;
  float* out = a.h + ((size_t)b * Q + qi) * a.H;
  if (qi < a.P) {
    const float* pr = a.prompt + ((size_t)b * a.P + qi) * a.H;
    for (int d = threadIdx.x; d < a.H; d += blockDim.x) out[d] = pr[d] + (a.pos_table ? a.pos_table[(size_t)qi * a.H + d] : 0.f);
    return;
  }
  __shared__ int s_tok[32];
  if (threadIdx.x < a.K) {
    const long long t = a.ids[((size_t)b * a.K + threadIdx.x) * a.T + (qi - a.P)];
    s_tok[threadIdx.x] = (int)(t < 0 ? 0 : (t >= a.V1 ? a.V1 - 1 : t));  // the caller validates ids; an id outside the table never leaves it
  }
  __syncthreads();
  const WT* tab = reinterpret_cast<const WT*>(a.tables);
  for (int d = threadIdx.x; d < a.H; d += blockDim.x) {
    float acc = 0.f;
    for (int k = 0; k < a.K; ++k) acc += Elem<WT>::ld(tab + ((size_t)k * a.V1 + s_tok[k]) * a.H + d);  // sum([...]) order :1433
    if (a.pos_table) acc += a.pos_table[(size_t)qi * a.H + d];
    out[d] = acc;
  }
}

struct ScoreArgs {
  const float* x;          // residual rows fp32 [B * Q][x_ld]
  const float* gamma;      // final LayerNorm
  const float* beta;
  const void* W;           // packed heads [K * V / 16 strips][H / KT fragments][64 lanes][16 B]
  const long long* ids;    // [B * K][T] decoder input columns (the EOS test of the counting rule), or null with labels
  const long long* labels; // [B][T][K], or null: logits only
  float* nll;              // [B][T][K]
  int* counted;            // [B][T][K]
  float* logits;           // STORE: [B * K][Qs][V]
  int x_ld;                // floats between residual rows
  int H, K, V;
  int B, Q, Qs, T;         // Q rows per utterance in x; the last Qs of them are projected (Qs = T, or Q with logits); the last T carry labels
  int bos, eos;
  float invH;
};

constexpr int SCORE_WAVES = 8;

template <typename WT, int MT, bool STORE>
__global__ void __launch_bounds__(SCORE_WAVES * 64) score_heads_kernel(ScoreArgs a) {
  constexpr int KT = Elem<WT>::KT, U = 8;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, j = lane & 15;
  const int row_bytes = a.H * (int)sizeof(WT) + 16;  // 16-byte pad: conflict-free b128 reads of 16 different rows
  char* s_x = smem_raw;                                                                // [16 * MT][row_bytes]
  float* s_part = reinterpret_cast<float*>(smem_raw + (size_t)16 * MT * row_bytes);  // [SCORE_WAVES][MT][64][3] = (max2, sum, label logit)
  int* s_lab = reinterpret_cast<int*>(s_part + (size_t)SCORE_WAVES * MT * 64 * 3);     // [16 * MT] the row's label where its position counts, else -1
  const int M = a.B * a.Qs, m0 = blockIdx.x * 16 * MT, nrows = min(16 * MT, M - m0), cb = blockIdx.y;
  // scored row m -> utterance b, position jj of the Qs projected ones, residual row b * Q + (Q - Qs) + jj
  auto xrow = [&](int m) { const int b = m / a.Qs, jj = m - b * a.Qs; return a.x + (size_t)(b * a.Q + (a.Q - a.Qs) + jj) * a.x_ld; };

  // 1. final LayerNorm of this tile's rows -> LDS, engine dtype (ln_rows' arithmetic without the EXACT shortcut: any H <= 2048, H % 4 == 0)
  for (int r = wave; r < nrows; r += SCORE_WAVES) {
    const float* xr = xrow(m0 + r);
    float4 v[LN_MAX_F4];
#pragma unroll
    for (int i = 0; i < LN_MAX_F4; ++i) {
      const int k = (lane + 64 * i) * 4;
      v[i] = *reinterpret_cast<const float4*>(xr + (k < a.H ? k : 0));
    }
    float c, s1, s2, mean, rstd;
    ln_row_sums<LN_MAX_F4, false>(v, lane, a.H, c, s1, s2);
    LnWaveSums::reduce(s1, s2);
    ln_mean_rstd(c, s1, s2, a.invH, mean, rstd);
#pragma unroll
    for (int i = 0; i < LN_MAX_F4; ++i) {
      const int k = (lane + 64 * i) * 4;
      if (k < a.H) {
        const float4 g = *reinterpret_cast<const float4*>(a.gamma + k), bt = *reinterpret_cast<const float4*>(a.beta + k);
        lds_store4<WT>(s_x + (size_t)r * row_bytes, k, ln_norm(v[i].x, mean, rstd, g.x, bt.x), ln_norm(v[i].y, mean, rstd, g.y, bt.y),
                       ln_norm(v[i].z, mean, rstd, g.z, bt.z), ln_norm(v[i].w, mean, rstd, g.w, bt.w));
      }
    }
  }
  // 2. this lane's rows (one per row tile): label, whether the position counts, where its logits go
  int label[MT];
  float* lrow[MT];
  const char* brow[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int rloc = mt * 16 + j, m = m0 + min(rloc, nrows - 1);  // rows past the tile's end are clamped: nothing of theirs is stored
    const int b = m / a.Qs, jj = m - b * a.Qs, t = jj - (a.Qs - a.T);
    label[mt] = -1;
    if (a.labels && rloc < nrows && t >= 0) {
      const long long lb = a.labels[((size_t)b * a.T + t) * a.K + cb];
      const long long in = a.ids[((size_t)b * a.K + cb) * a.T + t];
      // modeling:1935-1938: the label is neither the ignore index nor BOS, and the input column is not EOS; a label outside the vocabulary never counts
      if (lb != -100 && lb != a.bos && in != a.eos && lb >= 0 && lb < a.V) label[mt] = (int)lb;
    }
    lrow[mt] = STORE ? a.logits + ((size_t)(b * a.K + cb) * a.Qs + jj) * a.V : nullptr;
    brow[mt] = s_x + (size_t)min(rloc, nrows - 1) * row_bytes + (size_t)q * 16;
    if (wave == 0 && q == 0) s_lab[rloc] = label[mt];  // the counting rule is stated once, here; the merge reads its outcome
  }
  __syncthreads();

  // 3. the codebook's strips, SCORE_WAVES at a time; the whole K reduction of a strip in this wave
  const int nfrag = a.H / KT, nstrips = a.V >> 4;
  float mx[MT], sm[MT], pick[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) { mx[mt] = -3.0e38f; sm[mt] = 0.f; pick[mt] = 0.f; }
  for (int s = wave; s < nstrips; s += SCORE_WAVES) {
    const uint4* Wp = reinterpret_cast<const uint4*>(a.W) + ((size_t)(cb * nstrips + s) * nfrag) * 64 + lane;
    f32x4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    uint4 afr[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (u < nfrag) afr[u] = Wp[(size_t)u * 64];
    for (int tb = 0; tb < nfrag; tb += U) {
      uint4 cur[U];
#pragma unroll
      for (int u = 0; u < U; ++u) cur[u] = afr[u];
      if (tb + U < nfrag) {  // the next group's weights are in flight under this group's MFMAs
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (tb + U + u < nfrag) afr[u] = Wp[(size_t)(tb + U + u) * 64];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (tb + u < nfrag) {
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            const uint4 bf = *reinterpret_cast<const uint4*>(brow[mt] + (size_t)(tb + u) * (KT * sizeof(WT)));
            acc[mt] = MfmaStep<WT>::run(cur[u], bf, acc[mt]);
          }
        }
      }
    }
    const int n = s * 16 + q * 4;  // D[row = q * 4 + e][col = j]: columns n .. n + 3 of row j
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const f32x4 r = acc[mt];
      if (STORE && mt * 16 + j < nrows) *reinterpret_cast<float4*>(lrow[mt] + n) = make_float4(r[0], r[1], r[2], r[3]);
      const float x0 = r[0] * 1.44269504088896340736f, x1 = r[1] * 1.44269504088896340736f, x2 = r[2] * 1.44269504088896340736f,
                  x3 = r[3] * 1.44269504088896340736f;
      const float mn = fmaxf(fmaxf(mx[mt], fmaxf(x0, x1)), fmaxf(x2, x3));
      sm[mt] = sm[mt] * __builtin_amdgcn_exp2f(mx[mt] - mn) +
               ((__builtin_amdgcn_exp2f(x0 - mn) + __builtin_amdgcn_exp2f(x1 - mn)) + (__builtin_amdgcn_exp2f(x2 - mn) + __builtin_amdgcn_exp2f(x3 - mn)));
      mx[mt] = mn;
      const int d = label[mt] - n;
      if (d >= 0 && d < 4) pick[mt] = d == 0 ? r[0] : (d == 1 ? r[1] : (d == 2 ? r[2] : r[3]));
    }
  }
  if (!a.labels) return;  // logits only (uniform over the workgroup)
  // 4. one merge per row: 4 column groups x SCORE_WAVES partials, fixed order
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    float* p = s_part + (((size_t)wave * MT + mt) * 64 + lane) * 3;
    p[0] = mx[mt]; p[1] = sm[mt]; p[2] = pick[mt];
  }
  __syncthreads();
  for (int rloc = threadIdx.x; rloc < nrows; rloc += blockDim.x) {
    const int mt = rloc >> 4, jr = rloc & 15, m = m0 + rloc;
    const int b = m / a.Qs, jj = m - b * a.Qs, t = jj - (a.Qs - a.T);
    if (t < 0) continue;
    const size_t o = ((size_t)b * a.T + t) * a.K + cb;
    const bool cnt = s_lab[rloc] >= 0;
    float M2 = -3.0e38f;
    for (int w = 0; w < SCORE_WAVES; ++w)
      for (int qq = 0; qq < 4; ++qq) M2 = fmaxf(M2, s_part[(((size_t)w * MT + mt) * 64 + qq * 16 + jr) * 3]);
    float S = 0.f, pk = 0.f;
    for (int w = 0; w < SCORE_WAVES; ++w)
      for (int qq = 0; qq < 4; ++qq) {
        const float* p = s_part + (((size_t)w * MT + mt) * 64 + qq * 16 + jr) * 3;
        S += p[1] * __builtin_amdgcn_exp2f(p[0] - M2);
        pk += p[2];  // exactly one partial holds the label's logit, the others 0
      }
    a.nll[o] = cnt ? (M2 + __builtin_amdgcn_logf(S)) * 0.69314718055994530942f - pk : 0.f;
    a.counted[o] = cnt ? 1 : 0;
  }
}
