// Test-only harness of the attention kernels (tests/test_attn_kernels_gpu.py, tests/test_attn_harness_cpu.py).
// It includes the product headers and launches the product's own kernels - attn_kernel<WT, NW, KV8> through launch_attn and
// prefill_attn_kernel<WT, KV8> / prefill_attn_mfma_kernel<WT, NW> through launch_prefill_attn (the functions the engine calls),
// kv_append_kernel<WT, KV8> as ptts_lm.hip launches it, t5_attn_kernel<WT> / t5_attn_mfma_kernel<WT> as ptts_t5.hip launches them - on
// device pointers that the test allocates with torch. No kernel code of its own. Built by the tests with build()'s hipcc flags as one
// translation unit. Every entry returns a PTTS_* status; the message is in ah_last_error().
#include "ptts_common.h"
#include "ptts_lm_kernels.h"
#include "ptts_gemm_launch.h"
#include "ptts_t5_kernels.h"

#define AH_API extern "C" __attribute__((visibility("default")))

// the operands of one decoder attention / append launch: AttnArgs flattened, plus the launch's own choices; DevDims lives in device memory,
// written by the test as raw bytes
struct AhArgs {
  const float* q;
  const float* knew;
  const float* vnew;
  void* kcache;
  void* vcache;
  const int* cur_len;
  const void* dims;  // DevDims
  const int* mask;
  const float* cos;
  const float* sin;
  float* part;
  void* direct_out;
  float* stats;
  float* kscale;
  float* vscale;
  int q_ld, kv_ld, cap, kv_bound, mask_ld, S, Q, nheads, H, kv_heads, n_rep, cross, fused_append, out_fo, hostP, hostN;
  int B;      // utterances: the grid is (S, nheads, B * Q) / (query tiles, nheads, B)
  int bf16;   // engine dtype: 1 = bf16_t, 0 = float
  int waves;  // ah_attn: launch_attn's `waves`
  int mode;   // ah_prefill_attn: launch_prefill_attn's `mode`
  float scale;
};

// one T5 attention launch (T5AttnArgs + grid)
struct AhT5Args {
  const float* qkv;
  const float* bias;
  const int* mask;
  void* out;
  int ld, inner, bias_ld, bias_zero, N, out_fo, B, nheads, bf16, mfma;
};

thread_local std::string g_ptts_err;
int ptts_fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_ptts_err = buf;
  return code;
}

static int ah_launched(const char* what) {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? PTTS_OK : ptts_fail(PTTS_E_HIP, "%s launch failed: %s", what, hipGetErrorString(e));
}

AH_API const char* ah_last_error(void) { return g_ptts_err.c_str(); }
// 0: AhArgs, 1: AhT5Args, 2: DevDims
AH_API int ah_args_size(int which) { return which == 0 ? (int)sizeof(AhArgs) : which == 1 ? (int)sizeof(AhT5Args) : which == 2 ? (int)sizeof(DevDims) : -1; }

// every instance the harness reaches, three ints per instance; returns the number of instances of `kind`
//   0 attn_kernel (bf16, NW, KV8)   1 prefill_attn_kernel (bf16, KV8, 0)   2 prefill_attn_mfma_kernel (bf16, NW, 0)
//   3 kv_append_kernel (bf16, KV8, 0)   4 t5_attn_kernel (bf16, 0, 0)   5 t5_attn_mfma_kernel (bf16, 0, 0)
AH_API int ah_instances(int kind, int* out, int cap) {
  int n = 0;
  auto put = [&](int a, int b, int c) {
    if (n < cap) { out[3 * n] = a; out[3 * n + 1] = b; out[3 * n + 2] = c; }
    ++n;
  };
  for (int bf = 0; bf < 2; ++bf) {
    if (kind == 0) {
      for (int nw = 1; nw <= 4; nw *= 2) put(bf, nw, 0);
      if (bf) put(1, 4, 1);
    } else if (kind == 1 || kind == 3) {
      put(bf, 0, 0);
      if (bf) put(1, 1, 0);
    } else if (kind == 2) {
      for (int nw = 1; nw <= 4; ++nw) put(bf, nw, 0);
    } else if (kind == 4 || kind == 5) {
      put(bf, 0, 0);
    } else {
      return -1;
    }
  }
  return n;
}

// what the host can check of a launch's addressing (the lengths behind dims / cur_len are the test's to keep inside cap, mask_ld and the tables)
static int ah_check(const AhArgs& g, const char* who) {
  if (!g.kcache || !g.vcache) return ptts_fail(PTTS_E_INVALID, "%s: null cache pointer", who);
  if (g.B <= 0 || g.Q <= 0 || g.nheads <= 0 || g.kv_heads <= 0 || g.n_rep <= 0 || g.kv_heads * g.n_rep != g.nheads || g.H != g.nheads * 64 || g.cap <= 0 ||
      (!g.kscale) != (!g.vscale) || (!g.cos) != (!g.sin) || (g.kscale && !g.bf16))
    return ptts_fail(PTTS_E_INVALID, "%s: B=%d Q=%d heads=%d x %d / %d H=%d cap=%d", who, g.B, g.Q, g.kv_heads, g.n_rep, g.nheads, g.H, g.cap);
  return PTTS_OK;
}

static void ah_fill(const AhArgs& g, AttnArgs& a) {
  a.q = g.q; a.q_ld = g.q_ld; a.knew = g.knew; a.vnew = g.vnew; a.kv_ld = g.kv_ld; a.kcache = g.kcache; a.vcache = g.vcache;
  a.cap = g.cap; a.kv_bound = g.kv_bound; a.cur_len = g.cur_len; a.dims = reinterpret_cast<const DevDims*>(g.dims); a.mask = g.mask; a.mask_ld = g.mask_ld;
  a.cos = g.cos; a.sin = g.sin; a.part = g.part; a.direct_out = g.direct_out; a.stats = g.stats; a.S = g.S; a.Q = g.Q; a.nheads = g.nheads; a.H = g.H;
  a.kv_heads = g.kv_heads; a.n_rep = g.n_rep; a.cross = g.cross; a.fused_append = g.fused_append; a.scale = g.scale; a.out_fo = g.out_fo;
  a.kscale = g.kscale; a.vscale = g.vscale; a.hostP = g.hostP; a.hostN = g.hostN;
}

static int ah_check_attn(const AhArgs& g, const char* who) {
  if (int rc = ah_check(g, who)) return rc;
  if (!g.q || !g.dims || g.q_ld < g.H || g.q_ld % 4 || g.kv_bound <= 0 || g.kv_bound > g.cap || g.S <= 0 || (g.mask && g.mask_ld <= 0) ||
      (g.S > 1 && (g.direct_out || !g.part || !g.stats)) || (g.S == 1 && !g.direct_out && (!g.part || !g.stats)))
    return ptts_fail(PTTS_E_INVALID, "%s: q_ld=%d kv_bound=%d cap=%d S=%d mask_ld=%d", who, g.q_ld, g.kv_bound, g.cap, g.S, g.mask_ld);
  if (g.fused_append && (!g.knew || !g.vnew || !g.cur_len || g.cross || g.Q != 1 || g.kv_ld < g.kv_heads * 64 || g.kv_ld % 4))
    return ptts_fail(PTTS_E_INVALID, "%s: fused append needs knew / vnew / cur_len, Q = 1, self-attention (kv_ld=%d)", who, g.kv_ld);
  return PTTS_OK;
}

// launch_attn<WT>: the engine's instance choice from `waves` and the e4m3 scales
AH_API int ah_attn(const AhArgs* g, void* stream) {
  if (int rc = ah_check_attn(*g, "ah_attn")) return rc;
  AttnArgs a = {};
  ah_fill(*g, a);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return g->bf16 ? launch_attn<bf16_t>(a, g->B, st, g->waves) : launch_attn<float>(a, g->B, st, g->waves);
}

// launch_prefill_attn<WT>: mode 1 = the VALU kernel, 2 = the MFMA kernel, 3 = by batch
AH_API int ah_prefill_attn(const AhArgs* g, void* stream) {
  if (int rc = ah_check_attn(*g, "ah_prefill_attn")) return rc;
  if (g->S != 1 || !g->direct_out || g->fused_append || g->cur_len || g->mode < 1 || g->mode > 3 || (g->cross ? g->hostN <= 0 || g->hostN > g->cap : g->Q > g->cap))
    return ptts_fail(PTTS_E_INVALID, "ah_prefill_attn: S=%d mode=%d Q=%d N=%d cap=%d (unsplit, direct_out, no append, no cur_len)", g->S, g->mode, g->Q, g->hostN, g->cap);
  AttnArgs a = {};
  ah_fill(*g, a);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return g->bf16 ? launch_prefill_attn<bf16_t>(a, g->B, st, g->mode) : launch_prefill_attn<float>(a, g->B, st, g->mode);
}

// kv_append_kernel<WT, KV8> on rows [B][Q] of knew / vnew: positions 0 .. Q - 1 of every (utterance, K/V head); KV8 when the scales are given
AH_API int ah_kv_append(const AhArgs* g, void* stream) {
  if (int rc = ah_check(*g, "ah_kv_append")) return rc;
  if (!g->knew || !g->vnew || g->Q > g->cap || g->kv_ld < g->kv_heads * 64)
    return ptts_fail(PTTS_E_INVALID, "ah_kv_append: Q=%d cap=%d kv_ld=%d", g->Q, g->cap, g->kv_ld);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(g->Q, g->kv_heads, g->B), block(64);
  if (g->kscale)
    hipLaunchKernelGGL((kv_append_kernel<bf16_t, true>), grid, block, 0, st, g->knew, g->vnew, g->kv_ld, g->kcache, g->vcache, g->cap, g->Q, g->kv_heads, g->cos,
                       g->sin, g->kscale, g->vscale);
  else if (g->bf16)
    hipLaunchKernelGGL((kv_append_kernel<bf16_t>), grid, block, 0, st, g->knew, g->vnew, g->kv_ld, g->kcache, g->vcache, g->cap, g->Q, g->kv_heads, g->cos, g->sin);
  else
    hipLaunchKernelGGL((kv_append_kernel<float>), grid, block, 0, st, g->knew, g->vnew, g->kv_ld, g->kcache, g->vcache, g->cap, g->Q, g->kv_heads, g->cos, g->sin);
  return ah_launched("kv_append_kernel");
}

// t5_attn_kernel<WT> (mfma = 0) / t5_attn_mfma_kernel<WT> (mfma = 1) on the grid and block of the encoder's forward
AH_API int ah_t5_attn(const AhT5Args* g, void* stream) {
  if (!g->qkv || !g->bias || !g->out || g->B <= 0 || g->N <= 0 || g->nheads <= 0 || g->inner != g->nheads * 64 || g->ld < 3 * g->inner || g->ld % 4 ||
      g->bias_zero < g->N - 1 || g->bias_ld < g->bias_zero + g->N)
    return ptts_fail(PTTS_E_INVALID, "ah_t5_attn: B=%d N=%d heads=%d inner=%d ld=%d bias_ld=%d bias_zero=%d", g->B, g->N, g->nheads, g->inner, g->ld, g->bias_ld,
                     g->bias_zero);
  T5AttnArgs a = {};
  a.qkv = g->qkv; a.ld = g->ld; a.inner = g->inner; a.bias = g->bias; a.bias_ld = g->bias_ld; a.bias_zero = g->bias_zero;
  a.mask = g->mask; a.out = g->out; a.out_fo = g->out_fo; a.N = g->N;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int N = g->N;
  if (g->mfma) {
    if (g->bf16) ptts_klaunch(t5_attn_mfma_kernel<bf16_t>, dim3((N + 63) / 64, g->nheads, g->B), dim3(256), 0, st, a);
    else ptts_klaunch(t5_attn_mfma_kernel<float>, dim3((N + 63) / 64, g->nheads, g->B), dim3(256), 0, st, a);
  } else {
    if (g->bf16) ptts_klaunch(t5_attn_kernel<bf16_t>, dim3((N + 7) / 8, g->nheads, g->B), dim3(256), 0, st, a);
    else ptts_klaunch(t5_attn_kernel<float>, dim3((N + 7) / 8, g->nheads, g->B), dim3(256), 0, st, a);
  }
  return ah_launched(g->mfma ? "t5_attn_mfma_kernel" : "t5_attn_kernel");
}
