// Test-only harness of the DAC codec's kernels (tests/test_dac_kernels_gpu.py, tests/test_dac_harness_cpu.py).
// It includes the product headers (ptts_dac_kernels.h, ptts_dac_launch.h) and launches the product's own kernels through the product's own plan and
// launch functions, on device pointers that the test allocates with torch. Weights arrive in the checkpoint's layout and go through the product's
// pack kernels and tap table, the Snake's 1 / (alpha + 1e-9) through inv_alpha_kernel. The only kernel of its own is the one-line Snake probe.
// Built by the tests with build()'s hipcc flags as three translation units (-DDH_PART_CONV / _RES / _MISC). Every launcher returns a PTTS_* status;
// the message is in dh_last_error().
#include "ptts_common.h"
#include "ptts_dac_kernels.h"
#include "ptts_dac_launch.h"

#define DH_API extern "C" __attribute__((visibility("default")))
#if !defined(DH_PART_CONV) && !defined(DH_PART_RES) && !defined(DH_PART_MISC)
#define DH_PART_CONV
#define DH_PART_RES
#define DH_PART_MISC
#endif

// one convolution: the layer's shape, the launch, and (forced != 0) the instance to run instead of the planned one
struct DhConv {
  const void* x;
  const float* w;      // checkpoint layout: [Cout][Cin][k], transposed [Cin][Cout][k]
  const float* bias;
  const float* skip;
  float* out_raw;
  void* out_act;
  float* alpha;        // [2 * Cout]: the harness fills the second half with inv_alpha_kernel
  const int* lens;
  void* Wp;            // room for the packed weights
  int* ktap;           // 64 ints on the device
  DacConvShape shape;
  int B, Tin, len_mul, act_f32;
  int forced;
  DacConvPlan plan;    // forced: kernel and p[] in; always: the plan that ran, out
};

// one fused residual unit; alpha_in != null: an XIN unit
struct DhRes {
  const void* x;
  const float *w7, *b7;
  float* alpha7;       // [2C]
  const float *w1, *b1;
  float* alpha1;       // [2C]
  const float* skip;
  float* out_raw;
  void* out_act;
  float* alpha_in;     // [2C] or null
  const int* lens;
  void *Wp7, *Wp1;
  int* ktap;
  int C, dil, B, T, len_mul, act_f32;
  DacResPlan plan;     // out
};

struct DhOut {
  const float* x;
  const float* w;      // checkpoint layout [1][C][7]
  const float* bias;
  float* wt;           // room for [7][C]
  float* out;
  const int *skip_of, *t_end_of;  // rows != 0: per-row emit ranges
  const int* lens;
  long long out_ld;
  int B, T, C, skip, t_end, len_mul, rows, force_direct;
};

struct DhGather {
  const long long* codes;
  const int *tab, *p_lens, *start, *slot;  // stream != 0
  const float* table;
  void* z;
  const int* lens;
  long long ld;
  int cap, K, T, B, ncodes, latent, z_bf16, t0, stream;
};

struct DhEncode {
  const float *z, *in_w, *in_b, *cb, *cbn, *cbn_sq, *out_w, *out_b;
  long long* codes;
  int B, T, latent, cdim, ncodes, nq;
};

#ifdef DH_PART_MISC
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
DH_API const char* dh_last_error(void) { return g_ptts_err.c_str(); }
#endif

static int dh_launched(const char* what) {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? PTTS_OK : ptts_fail(PTTS_E_HIP, "%s launch failed: %s", what, hipGetErrorString(e));
}
static void dh_inv_alpha(float* alpha, int C, hipStream_t st) {
  if (alpha) hipLaunchKernelGGL(inv_alpha_kernel, dim3((C + 255) / 256), dim3(256), 0, st, alpha, C);
}
// the product's load path of one conv weight: tap table to the device, pack kernel, and the wait before the table is reused
static int dh_pack(const DacConvShape& L, const float* w, void* Wp, int* ktap, hipStream_t st) {
  if (!w || !Wp || !ktap) return ptts_fail(PTTS_E_INVALID, "null weight / pack / tap-table pointer");
  if (L.Cout % 16 || L.Cin % (L.bf16 ? 32 : 16) || L.ksize < 1 || (L.transposed ? (L.ksize != 2 * L.stride || L.stride < 2 || L.stride > 8) : L.ksize > 16))
    return ptts_fail(PTTS_E_UNSUPPORTED, "conv %d -> %d k%d stride %d", L.Cin, L.Cout, L.ksize, L.stride);
  const DacPackPlan pk = dac_pack_plan(L);
  PTTS_HIP(hipMemcpyAsync(ktap, pk.ktap, sizeof pk.ktap, hipMemcpyHostToDevice, st));
  dac_pack_launch(L, pk, w, Wp, ktap, st);
  PTTS_HIP(hipStreamSynchronize(st));
  return dh_launched("pack");
}

#ifdef DH_PART_MISC
// 0: DhConv 1: DhRes 2: DhOut 3: DhGather 4: DhEncode 5: DacConvShape 6: DacConvPlan 7: DacResPlan 8: DacOutPlan 9: DacPackPlan
DH_API int dh_sizes(int which) {
  const int s[] = {(int)sizeof(DhConv), (int)sizeof(DhRes), (int)sizeof(DhOut), (int)sizeof(DhGather), (int)sizeof(DhEncode), (int)sizeof(DacConvShape),
                   (int)sizeof(DacConvPlan), (int)sizeof(DacResPlan), (int)sizeof(DacOutPlan), (int)sizeof(DacPackPlan)};
  return which >= 0 && which < 10 ? s[which] : -1;
}

// ---- pure host: no device touched ---------------------------------------------------------------------------------------------------
DH_API void dh_conv_plan(const DacConvShape* L, int B, int Tin, DacConvPlan* out) { *out = dac_conv_plan(*L, B, Tin); }
// the residual unit's dispatch: fusable under PTTS_DAC_NO_FUSE_RES = no_fuse? (bit 0 of the result); XIN at `frames` latent frames under
// PTTS_DAC_XIN = xin_mask (negative: unset)? (bit 1); *out: the instance of (raw, act_f32, xin, act), bit 2 set where dac_resunit_plan refuses them
DH_API int dh_resunit_plan(const DacConvShape* c7, const DacConvShape* c1, int no_fuse, int xin_mask, long long frames, int B, int T, int raw, int act_f32,
                           int xin, int act, DacResPlan* out) {
  const int bits = (dac_resunit_fusable(*c7, *c1, true, no_fuse) ? 1 : 0) | (dac_resunit_xin_width(c7->Cout, frames, xin_mask) ? 2 : 0);
  if (out && dac_resunit_plan(c7->Cout, B, T, raw != 0, act_f32 != 0, xin != 0, act != 0, out) != PTTS_OK) return bits | 4;
  return bits;
}
DH_API void dh_conv_out_plan(int C, int B, int T, int force_direct, DacOutPlan* out) { *out = dac_conv_out_plan(C, B, T, force_direct != 0); }
DH_API void dh_pack_plan(const DacConvShape* L, DacPackPlan* out) { *out = dac_pack_plan(*L); }

// every instance the harness reaches, six ints per instance; returns the number of instances of `kind`
//   0 conv_mfma_kernel (CS, BF)   1 conv_lds_kernel (CSW, NW, KS, MAXHALO, FT)   2 resunit_lds_kernel (NW, WD, RAW, F32, XIN, ACT)
//   3 conv_out_tanh_kernel (ROWS)   4 conv_out_tanh_lds_kernel (ROWS)   5 rvq_gather_kernel (STREAM)
DH_API int dh_instances(int kind, int* out, int cap) {
  int n = 0;
  auto put = [&](int a, int b = 0, int c = 0, int d = 0, int e = 0, int f = 0) {
    if (n < cap) { int* o = out + 6 * n; o[0] = a; o[1] = b; o[2] = c; o[3] = d; o[4] = e; o[5] = f; }
    ++n;
  };
  if (kind == 0) {
    for (int cs : {1, 2, 4, 6, 8}) for (int bf = 0; bf < 2; ++bf) put(cs, bf);
  } else if (kind == 1) {
    put(3, 4, 1, 54, 4); put(3, 4, 1, 54, 8); put(3, 2, 1, 54, 8); put(3, 4, 3, 2, 4); put(3, 4, 3, 2, 8); put(3, 2, 1, 2, 8);
  } else if (kind == 2) {
    for (int nw : {2, 4, 8}) {
      const int wdx = nw == 2 ? 1 : 3;
      for (int f32 = 0; f32 < (nw == 2 ? 2 : 1); ++f32) {
        put(nw, 3, 1, f32, 0, 1); put(nw, 3, 0, f32, 0, 1);
        put(nw, wdx, 1, f32, 1, 1); put(nw, wdx, 0, f32, 1, 1);
      }
      put(nw, wdx, 1, 0, 1, 0);
    }
  } else if (kind == 3 || kind == 4 || kind == 5) {
    put(0); put(1);
  } else {
    return -1;
  }
  return n;
}
#endif  // DH_PART_MISC

#ifdef DH_PART_CONV
// one convolution as planned (forced == 0) or on the instance in g->plan (kernel, p[]); the plan that ran is written back
DH_API int dh_conv(DhConv* g, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const DacConvShape& L = g->shape;
  if (!g->x || !g->bias || g->B <= 0 || g->Tin <= 0 || g->len_mul < 1 || (!g->out_raw && !g->out_act) || (g->out_act && !g->alpha))
    return ptts_fail(PTTS_E_INVALID, "dh_conv: B=%d Tin=%d len_mul=%d", g->B, g->Tin, g->len_mul);
  ConvArgs a = {};
  a.act_f32 = g->act_f32; a.lens = g->lens; a.len_mul = g->len_mul;
  a.x = g->x; a.Wp = g->Wp; a.bias = g->bias; a.skip = g->skip; a.out_raw = g->out_raw; a.out_act = g->out_act; a.alpha = g->alpha;
  dac_conv_geometry(L, g->B, g->Tin, a);
  if (a.Tn <= 0) return ptts_fail(PTTS_E_INVALID, "dh_conv: no output rows");
  if (g->forced && g->plan.kernel == DAC_CONV_LDS && !L.bf16) return ptts_fail(PTTS_E_UNSUPPORTED, "conv_lds_kernel takes bf16 operands");
  if (g->forced && g->plan.kernel == DAC_CONV_MFMA && g->plan.p[1] != L.bf16) return ptts_fail(PTTS_E_UNSUPPORTED, "operand mode of the instance and of the layer differ");
  g->plan = g->forced ? dac_conv_plan_for(g->plan.kernel, g->plan.p, a) : dac_conv_plan(L, g->B, g->Tin);
  if (int rc = dac_conv_check(g->plan, a)) return rc;  // a refused instance touches no device
  if (int rc = dh_pack(L, g->w, g->Wp, g->ktap, st)) return rc;
  if (g->out_act) dh_inv_alpha(g->alpha, L.Cout, st);
  return dac_conv_launch(g->plan, a, st);
}
#endif  // DH_PART_CONV

#ifdef DH_PART_RES
DH_API int dh_resunit(DhRes* g, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!g->x || !g->b7 || !g->b1 || !g->alpha7 || !g->alpha1 || !g->skip || g->B <= 0 || g->T <= 0 || g->len_mul < 1)
    return ptts_fail(PTTS_E_INVALID, "dh_resunit: B=%d T=%d", g->B, g->T);
  const int C = g->C;
  const DacConvShape c7 = {C, C, 7, g->dil, 1, 0, 1, -1}, c1 = {C, C, 1, 1, 1, 0, 1, -1};
  if (!dac_resunit_fusable(c7, c1, true, 0)) return ptts_fail(PTTS_E_UNSUPPORTED, "dh_resunit: C=%d dil=%d is not fusable", C, g->dil);
  if (int rc = dh_pack(c7, g->w7, g->Wp7, g->ktap, st)) return rc;
  if (int rc = dh_pack(c1, g->w1, g->Wp1, g->ktap, st)) return rc;
  dh_inv_alpha(g->alpha7, C, st); dh_inv_alpha(g->alpha1, C, st); dh_inv_alpha(g->alpha_in, C, st);
  ResArgs r = {};
  r.a.lens = g->lens; r.a.len_mul = g->len_mul;
  r.a.x = g->x; r.a.Wp = g->Wp7; r.a.bias = g->b7; r.a.alpha = g->alpha7; r.a.dil = g->dil; r.a.pad = 3 * g->dil;
  r.a.B = g->B; r.a.Tin = g->T; r.a.Tn = g->T; r.a.Cin = C; r.a.Cout = C; r.a.ntaps = 7; r.a.nphase = 1; r.a.stride = 1;
  r.Wp1 = g->Wp1; r.bias1 = g->b1; r.alpha1 = g->alpha1; r.skip = g->skip; r.out_raw = g->out_raw; r.out_act = g->out_act; r.act_f32 = g->act_f32;
  r.alpha_in = g->alpha_in;
  PTTS_TRY(dac_resunit_plan(C, g->B, g->T, g->out_raw != nullptr, g->act_f32 != 0, g->alpha_in != nullptr, g->out_act != nullptr, &g->plan));
  return dac_resunit_launch(g->plan, r, st);
}
#endif  // DH_PART_RES

#ifdef DH_PART_MISC
// final Conv1d(C -> 1, k7) + tanh: the planned kernel, or the direct one (force_direct) where the LDS-tiled one would run
DH_API int dh_conv_out(const DhOut* g, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!g->x || !g->w || !g->bias || !g->wt || !g->out || g->B <= 0 || g->T <= 0 || g->C <= 0 || g->C % 4 || g->len_mul < 1 || (g->rows && (!g->skip_of || !g->t_end_of)))
    return ptts_fail(PTTS_E_INVALID, "dh_conv_out: B=%d T=%d C=%d", g->B, g->T, g->C);
  for (int k = 0; k < 7; ++k)  // [1][C][7] -> [7][C], as ptts_dac_load_weight does
    PTTS_HIP(hipMemcpy2DAsync(g->wt + (size_t)k * g->C, 4, g->w + k, 7 * 4, 4, g->C, hipMemcpyDeviceToDevice, st));
  const DacOutPlan p = dac_conv_out_plan(g->C, g->B, g->T, g->force_direct != 0);
  int rc;
  if (g->rows) rc = dac_conv_out_launch<true>(p, g->x, g->wt, g->bias, g->out, g->B, g->T, g->C, g->skip_of, g->out_ld, g->t_end_of, g->lens, g->len_mul, st);
  else rc = dac_conv_out_launch<false>(p, g->x, g->wt, g->bias, g->out, g->B, g->T, g->C, g->skip, g->out_ld, g->t_end, g->lens, g->len_mul, st);
  return rc != PTTS_OK ? rc : dh_launched("conv_out_tanh");
}

DH_API int dh_conv_in(const float* wave, const float* w, const float* bias, float* alpha, float* out_raw, float* out_act, int B, int L, int C, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!wave || !w || !bias || !alpha || !out_raw || !out_act || B <= 0 || L <= 0 || C <= 0 || C % 4) return ptts_fail(PTTS_E_INVALID, "dh_conv_in: B=%d L=%d C=%d", B, L, C);
  dh_inv_alpha(alpha, C, st);
  const size_t n = (size_t)B * L * (C / 4);
  hipLaunchKernelGGL(conv_in_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, wave, w, bias, alpha, out_raw, out_act, B, L, C);
  return dh_launched("conv_in_kernel");
}

DH_API int dh_rvq_table(const float* cb, const float* w, const float* bias, float* table, int ncodes, int cdim, int latent, void* stream) {
  if (!cb || !w || !bias || !table || ncodes <= 0 || cdim <= 0 || latent <= 0) return ptts_fail(PTTS_E_INVALID, "dh_rvq_table: null or empty");
  const size_t n = (size_t)ncodes * latent;
  hipLaunchKernelGGL(rvq_table_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), cb, w, bias, table, ncodes, cdim,
                     latent);
  return dh_launched("rvq_table_kernel");
}

DH_API int dh_rvq_gather(const DhGather* g, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!g->table || !g->z || g->K <= 0 || g->K > 32 || g->T <= 0 || g->B <= 0 || g->ncodes <= 0 || g->latent <= 0 ||
      (g->stream ? (!g->tab || !g->p_lens || !g->start || !g->slot || g->lens != g->p_lens || g->cap <= 0) : (!g->codes || g->ld < g->t0 + g->T)))
    return ptts_fail(PTTS_E_INVALID, "dh_rvq_gather: K=%d T=%d B=%d", g->K, g->T, g->B);
  if (g->stream) {
    StreamPlan sp = {};
    sp.tab = g->tab; sp.lens = g->p_lens; sp.start = g->start; sp.slot = g->slot; sp.cap = g->cap;
    hipLaunchKernelGGL((rvq_gather_kernel<true>), dim3(g->T, g->B), dim3(256), 0, st, sp, g->table, g->z, g->K, g->T, g->ncodes, g->latent, g->z_bf16, g->ld, g->t0,
                       g->lens);
  } else {
    hipLaunchKernelGGL((rvq_gather_kernel<false>), dim3(g->T, g->B), dim3(256), 0, st, g->codes, g->table, g->z, g->K, g->T, g->ncodes, g->latent, g->z_bf16, g->ld,
                       g->t0, g->lens);
  }
  return dh_launched("rvq_gather_kernel");
}

DH_API int dh_cb_normalize(const float* cb, float* cbn, float* cbn_sq, int ncodes, int cdim, void* stream) {
  if (!cb || !cbn || !cbn_sq || ncodes <= 0 || cdim <= 0) return ptts_fail(PTTS_E_INVALID, "dh_cb_normalize: null or empty");
  hipLaunchKernelGGL(cb_normalize_kernel, dim3((ncodes + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), cb, cbn, cbn_sq, ncodes, cdim);
  return dh_launched("cb_normalize_kernel");
}

DH_API int dh_rvq_encode(const DhEncode* g, void* stream) {
  if (!g->z || !g->in_w || !g->in_b || !g->cb || !g->cbn || !g->cbn_sq || !g->out_w || !g->out_b || !g->codes || g->B <= 0 || g->T <= 0 || g->latent <= 0 ||
      g->cdim <= 0 || g->cdim > RVQ_MAXD || g->ncodes <= 0 || g->nq <= 0)
    return ptts_fail(PTTS_E_INVALID, "dh_rvq_encode: B=%d T=%d latent=%d cdim=%d codes=%d nq=%d", g->B, g->T, g->latent, g->cdim, g->ncodes, g->nq);
  hipLaunchKernelGGL(rvq_encode_kernel, dim3(g->T, g->B), dim3(256), (size_t)g->latent * 4, reinterpret_cast<hipStream_t>(stream), g->z, g->in_w, g->in_b, g->cb,
                     g->cbn, g->cbn_sq, g->out_w, g->out_b, g->codes, g->T, g->latent, g->cdim, g->ncodes, g->nq);
  return dh_launched("rvq_encode_kernel");
}

// the Snake probe: out[i] = snake_f<FAST>(x[i], alpha[i % C], inv[i % C]) with the [alpha | 1 / (alpha + 1e-9)] of inv_alpha_kernel
template <bool FAST>
__global__ void dh_snake_kernel(const float* __restrict__ x, const float* __restrict__ alpha, float* __restrict__ out, long long n, int C) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = snake_f<FAST>(x[i], alpha[i % C], alpha[C + i % C]);
}
DH_API int dh_snake(int fast, const float* x, float* alpha, float* out, long long n, int C, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!x || !alpha || !out || n <= 0 || C <= 0) return ptts_fail(PTTS_E_INVALID, "dh_snake: null or empty");
  dh_inv_alpha(alpha, C, st);
  const dim3 grid((unsigned)((n + 255) / 256)), blk(256);
  if (fast) hipLaunchKernelGGL(dh_snake_kernel<true>, grid, blk, 0, st, x, alpha, out, n, C);
  else hipLaunchKernelGGL(dh_snake_kernel<false>, grid, blk, 0, st, x, alpha, out, n, C);
  return dh_launched("dh_snake_kernel");
}
#endif  // DH_PART_MISC
