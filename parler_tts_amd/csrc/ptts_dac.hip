// DAC engine behind include/ptts.h. Replaces DACModel.decode (dac_wrapper/modeling_dac.py:106-142): quantizer.from_codes
// (:138) + the descript-audio-codec decoder (:139); and DACModel.encode (:33-104, voice prompts): model.preprocess (:64,
// done by the caller: right-pad to a hop multiple) + model.encode (:95) = encoder stack + residual VQ search.
//
// Design:
//   * activations are channels-last fp32 [b][t][c]: a B-operand fragment (16 consecutive channels of one frame and
//     tap) is 4 x 16 B per lane group, an output fragment (4 consecutive channels of one frame) is one float4 store;
//   * every Conv1d / ConvTranspose1d is an implicit GEMM  out[co][t] = sum_{tap,ci} W[co][tap][ci] * x[t + off(tap)][ci]
//     on v_mfma_f32_16x16x4_f32 (exact f32 = an fmaf chain, so the fp32 parity bar RMS <= 1e-4 holds by construction);
//     a stride-s transposed conv is s interleaved 2-tap phase convolutions;
//   * Snake is evaluated ONCE per element in the producer's epilogue (x + sin^2(ax)/(a+1e-9)), never in a consumer
//     prologue (7 taps x Cout/16 strips would recompute each sin dozens of times); bias, residual skip and the
//     next layer's Snake are fused into the same epilogue; weight-norm is folded by the caller at load;
//   * RVQ from_codes is a gather-sum over K precomputed [codebook_size][latent] tables (out_proj(codebook_i)+bias_i);
//   * encode: the encoder's stride-s Conv1d(k = 2s) is the same implicit GEMM with input frame t*s + tap - pad; the
//     residual VQ runs one workgroup per frame through all stages (in_proj, cosine nearest neighbour over the
//     L2-normalised codebook, straight-through expression p + (c - p), out_proj, residual update).
#include <map>
#include <set>
#include <string>
#include <vector>
#include <string.h>
#include <limits.h>

#include <algorithm>
#include <type_traits>

#include "ptts_common.h"
#include "../../include/ptts_dac_stream_voice.h"
#include "ptts_dac_kernels.h"
#include "ptts_dac_launch.h"

namespace {

struct ConvLayer {
  std::string name;        // descript module name, e.g. "decoder.model.1.block.1"
  std::string alpha_name;  // Snake applied to this conv's OUTPUT (the next layer's input activation), or ""
  int Cin, Cout, ksize, dil, stride;  // stride > 1 => transposed
  bool transposed;
  float *Wp = nullptr, *bias = nullptr, *alpha = nullptr;
  bool has_skip = false, write_raw = false;
  bool bf16 = false;       // bf16-operand mode (decoder layers of a PTTS_BF16 engine)
  int pad = -1;            // explicit padding (down-sampling convs, k3 final conv); -1: "same" padding (k-1)*dil/2
  DacConvShape shape() const { return DacConvShape{Cin, Cout, ksize, dil, stride, transposed ? 1 : 0, bf16 ? 1 : 0, pad}; }
};

}  // namespace

struct ptts_dac {
  ptts_dac_config cfg;
  hipStream_t own_stream = nullptr;
  std::vector<void*> allocs;
  std::vector<ConvLayer> convs;  // all MFMA convs in execution order
  float *out_w = nullptr, *out_b = nullptr;  // final Conv1d(C->1): [7][C], [1]
  int out_C = 0;
  float* table = nullptr;  // [K][codes][latent]
  std::vector<float*> cb, opw, opb;
  float *bufA0 = nullptr, *bufA1 = nullptr, *bufY = nullptr, *bufS = nullptr, *bufZ = nullptr;
  // encode side (cfg.encoder_dim > 0)
  std::vector<ConvLayer> enc_convs;             // MFMA convs of the encoder in execution order
  float *in0_w = nullptr, *in0_b = nullptr, *in0_alpha = nullptr;  // encoder.block.0: Conv1d(1 -> encoder_dim, k7) + Snake of the first unit
  float *ipw = nullptr, *ipb = nullptr;         // in_proj [K][cdim][latent], [K][cdim]
  float *cb_all = nullptr, *cbn = nullptr, *cbn_sq = nullptr, *opw_all = nullptr, *opb_all = nullptr;  // contiguous copies for the VQ search
  bool vq_ready = false;
  int* d_ktap = nullptr;
  std::set<std::string> loaded, required;
  bool table_ready = false;
  int hop = 1;
  // stream table (ptts_dac_stream_open): kept codes [slots][K][cap], counters [slots][4] = absorbed, kept, emitted, -; the plan of the pass in
  // flight [5][slots] = window length (the ragged `lens`), window start, skip and end in samples, slot. Host side: what the host knows without
  // reading the device - the raw frames absorbed (exact) and an upper bound of kept - emitted per slot.
  // Voice prompts (ptts_dac_stream_open_voice): the slots' prefixes [slots][K][st_pre_ld]; a slot's fourth counter is its prefix length,
  // negative when the prompt's frames are not emitted. Host side: the same per slot (st_voice, signed alike).
  int *st_tab = nullptr, *st_state = nullptr, *st_plan = nullptr, *st_pre = nullptr;
  int st_slots = 0, st_cap = 0, st_pre_ld = 0;
  std::vector<int> st_absorbed, st_ready_ub, st_voice;

  template <typename T> int alloc(T** p, size_t n) {
    void* v = nullptr;
    hipError_t e = hipMalloc(&v, n * sizeof(T) > 0 ? n * sizeof(T) : 16);
    if (e != hipSuccess) return ptts_fail(PTTS_E_HIP, "hipMalloc(%zu bytes) failed: %s", n * sizeof(T), hipGetErrorString(e));
    allocs.push_back(v);
    *p = reinterpret_cast<T*>(v);
    return PTTS_OK;
  }
};

extern "C" void ptts_dac_destroy(ptts_dac* d) {
  if (!d) return;
  PttsDeviceGuard _dg(d->cfg.device);
  hipDeviceSynchronize();
  for (void* p : d->allocs) hipFree(p);
  for (void* p : {(void*)d->st_tab, (void*)d->st_state, (void*)d->st_plan, (void*)d->st_pre}) if (p) hipFree(p);
  if (d->own_stream) hipStreamDestroy(d->own_stream);
  delete d;
}

extern "C" int ptts_dac_create(const ptts_dac_config* cfg, ptts_dac** out) {
  PTTS_CHECK(cfg && out, PTTS_E_INVALID, "null argument");
  const ptts_dac_config& c = *cfg;
  PTTS_CHECK(c.num_rates >= 1 && c.num_rates <= 8, PTTS_E_INVALID, "num_rates out of range");
  PTTS_CHECK(c.num_codebooks >= 1 && c.num_codebooks <= 32, PTTS_E_INVALID, "num_codebooks out of range");
  PTTS_CHECK(c.latent_dim % 16 == 0 && c.decoder_dim % (16 << c.num_rates) == 0, PTTS_E_UNSUPPORTED,
             "latent_dim and every decoder width must be multiples of 16");
  PTTS_CHECK(c.encoder_dim >= 0 && c.encoder_dim % 16 == 0 && c.codebook_dim <= RVQ_MAXD, PTTS_E_UNSUPPORTED,
             "encoder_dim must be 0 (decode only) or a multiple of 16, codebook_dim <= %d", RVQ_MAXD);
  PTTS_CHECK(c.compute_dtype == PTTS_F32 || c.compute_dtype == PTTS_BF16, PTTS_E_INVALID, "compute_dtype must be PTTS_F32 or PTTS_BF16");
  if (c.compute_dtype == PTTS_BF16)
    PTTS_CHECK(c.latent_dim % 32 == 0 && c.decoder_dim % (32 << c.num_rates) == 0, PTTS_E_UNSUPPORTED,
               "bf16-operand mode needs latent_dim and every decoder width to be multiples of 32");
  PTTS_CHECK(c.max_batch >= 1 && c.max_frames >= 1, PTTS_E_INVALID, "bad capacities");
  for (int i = 0; i < c.num_rates; ++i) PTTS_CHECK(c.rates[i] >= 2 && c.rates[i] <= 8 && c.rates[i] % 2 == 0, PTTS_E_UNSUPPORTED, "decoder rate %d unsupported (need an even stride in [2, 8])", c.rates[i]);
  PTTS_DEVICE(c.device);
  ptts_dac* d = new ptts_dac();
  d->cfg = c;
  int rc = PTTS_OK;
  auto fail = [&](int r) { ptts_dac_destroy(d); return r; };
  if (hipStreamCreateWithFlags(&d->own_stream, hipStreamNonBlocking) != hipSuccess) return fail(ptts_fail(PTTS_E_HIP, "hipStreamCreate failed"));
#define A(expr) if ((rc = (expr)) != PTTS_OK) return fail(rc)
  std::vector<ConvLayer>* target = &d->convs;
  auto add_conv = [&](const std::string& name, const std::string& alpha_name, int Cin, int Cout, int k, int dil, int stride, bool tr,
                      bool has_skip, bool write_raw) -> int {
    ConvLayer L;
    L.name = name; L.alpha_name = alpha_name; L.Cin = Cin; L.Cout = Cout; L.ksize = k; L.dil = dil; L.stride = stride; L.transposed = tr;
    L.has_skip = has_skip; L.write_raw = write_raw;
    L.bf16 = target == &d->convs && c.compute_dtype == PTTS_BF16;  // the encoder always runs the exact-f32 kernels
    const int ntaps = tr ? 2 : k, nphase = tr ? stride : 1;
    if (ntaps > 16) return ptts_fail(PTTS_E_UNSUPPORTED, "%s: kernel size %d unsupported", name.c_str(), k);
    PTTS_TRY(d->alloc(&L.Wp, (size_t)nphase * Cout * ntaps * Cin));
    PTTS_TRY(d->alloc(&L.bias, Cout));
    if (!alpha_name.empty()) PTTS_TRY(d->alloc(&L.alpha, 2 * (size_t)Cout));  // [alpha | 1 / (alpha + 1e-9)]
    d->required.insert(name + ".weight");
    d->required.insert(name + ".bias");
    if (!alpha_name.empty()) d->required.insert(alpha_name + ".alpha");
    target->push_back(L);
    return PTTS_OK;
  };
  char nm[128], an[128];
  int ch = c.decoder_dim;
  snprintf(an, sizeof an, "decoder.model.1.block.0");
  A(add_conv("decoder.model.0", an, c.latent_dim, ch, 7, 1, 1, false, false, false));
  int hop = 1;
  for (int bi = 0; bi < c.num_rates; ++bi) {
    const int cin = ch >> bi, cout = ch >> (bi + 1), s = c.rates[bi];
    hop *= s;
    snprintf(nm, sizeof nm, "decoder.model.%d.block.1", bi + 1);
    snprintf(an, sizeof an, "decoder.model.%d.block.2.block.0", bi + 1);
    A(add_conv(nm, an, cin, cout, 2 * s, 1, s, true, false, true));
    const int dils[3] = {1, 3, 9};
    for (int ri = 0; ri < 3; ++ri) {
      snprintf(nm, sizeof nm, "decoder.model.%d.block.%d.block.1", bi + 1, ri + 2);
      snprintf(an, sizeof an, "decoder.model.%d.block.%d.block.2", bi + 1, ri + 2);
      A(add_conv(nm, an, cout, cout, 7, dils[ri], 1, false, false, false));
      snprintf(nm, sizeof nm, "decoder.model.%d.block.%d.block.3", bi + 1, ri + 2);
      if (ri < 2) snprintf(an, sizeof an, "decoder.model.%d.block.%d.block.0", bi + 1, ri + 3);
      else if (bi + 1 < c.num_rates) snprintf(an, sizeof an, "decoder.model.%d.block.0", bi + 2);
      else snprintf(an, sizeof an, "decoder.model.%d", c.num_rates + 1);
      A(add_conv(nm, an, cout, cout, 1, 1, 1, false, true, ri < 2));
    }
  }
  d->hop = hop;
  d->out_C = ch >> c.num_rates;
  A(d->alloc(&d->out_w, (size_t)7 * d->out_C));
  A(d->alloc(&d->out_b, 1));
  snprintf(nm, sizeof nm, "decoder.model.%d", c.num_rates + 2);
  d->required.insert(std::string(nm) + ".weight");
  d->required.insert(std::string(nm) + ".bias");
  A(d->alloc(&d->table, (size_t)c.num_codebooks * c.codebook_size * c.latent_dim));
  d->cb.resize(c.num_codebooks); d->opw.resize(c.num_codebooks); d->opb.resize(c.num_codebooks);
  for (int i = 0; i < c.num_codebooks; ++i) {
    A(d->alloc(&d->cb[i], (size_t)c.codebook_size * c.codebook_dim));
    A(d->alloc(&d->opw[i], (size_t)c.latent_dim * c.codebook_dim));
    A(d->alloc(&d->opb[i], c.latent_dim));
    snprintf(nm, sizeof nm, "quantizer.quantizers.%d.", i);
    d->required.insert(std::string(nm) + "codebook.weight");
    d->required.insert(std::string(nm) + "out_proj.weight");
    d->required.insert(std::string(nm) + "out_proj.bias");
  }
  if (c.encoder_dim > 0) {  // encode side: descript Encoder, strides = the decoder's reversed
    target = &d->enc_convs;
    const int n = c.num_rates;
    int dim = c.encoder_dim;
    A(d->alloc(&d->in0_w, (size_t)dim * 7)); A(d->alloc(&d->in0_b, dim)); A(d->alloc(&d->in0_alpha, 2 * (size_t)dim));
    d->required.insert("encoder.block.0.weight"); d->required.insert("encoder.block.0.bias");
    d->required.insert("encoder.block.1.block.0.block.0.alpha");
    for (int bi = 0; bi < n; ++bi) {
      const int st = c.rates[n - 1 - bi];
      const int dils[3] = {1, 3, 9};
      for (int ri = 0; ri < 3; ++ri) {
        snprintf(nm, sizeof nm, "encoder.block.%d.block.%d.block.1", bi + 1, ri);
        snprintf(an, sizeof an, "encoder.block.%d.block.%d.block.2", bi + 1, ri);
        A(add_conv(nm, an, dim, dim, 7, dils[ri], 1, false, false, false));
        snprintf(nm, sizeof nm, "encoder.block.%d.block.%d.block.3", bi + 1, ri);
        if (ri < 2) snprintf(an, sizeof an, "encoder.block.%d.block.%d.block.0", bi + 1, ri + 1);
        else snprintf(an, sizeof an, "encoder.block.%d.block.3", bi + 1);
        A(add_conv(nm, an, dim, dim, 1, 1, 1, false, true, ri < 2));
      }
      snprintf(nm, sizeof nm, "encoder.block.%d.block.4", bi + 1);
      if (bi + 1 < n) snprintf(an, sizeof an, "encoder.block.%d.block.0.block.0", bi + 2);
      else snprintf(an, sizeof an, "encoder.block.%d", n + 1);
      A(add_conv(nm, an, dim, 2 * dim, 2 * st, 1, st, false, false, true));
      d->enc_convs.back().pad = (st + 1) / 2;
      dim *= 2;
    }
    snprintf(nm, sizeof nm, "encoder.block.%d", n + 2);
    A(add_conv(nm, "", dim, c.latent_dim, 3, 1, 1, false, false, true));
    const size_t K = c.num_codebooks;
    A(d->alloc(&d->ipw, K * c.codebook_dim * c.latent_dim)); A(d->alloc(&d->ipb, K * c.codebook_dim));
    A(d->alloc(&d->cb_all, K * c.codebook_size * c.codebook_dim)); A(d->alloc(&d->cbn, K * c.codebook_size * c.codebook_dim));
    A(d->alloc(&d->cbn_sq, K * c.codebook_size));
    A(d->alloc(&d->opw_all, K * c.latent_dim * c.codebook_dim)); A(d->alloc(&d->opb_all, K * c.latent_dim));
    for (int i = 0; i < c.num_codebooks; ++i) {
      snprintf(nm, sizeof nm, "quantizer.quantizers.%d.in_proj.", i);
      d->required.insert(std::string(nm) + "weight");
      d->required.insert(std::string(nm) + "bias");
    }
    target = &d->convs;
  }
  // activation buffers: max over layers of T_l * C_l
  size_t mx = (size_t)c.max_frames * std::max(c.latent_dim, c.decoder_dim);
  if (c.encoder_dim > 0) mx = std::max(mx, (size_t)c.max_frames * hop * c.encoder_dim);
  {
    size_t T = c.max_frames;
    for (int bi = 0; bi < c.num_rates; ++bi) { T *= c.rates[bi]; mx = std::max(mx, T * (size_t)(ch >> (bi + 1))); }
  }
  mx *= c.max_batch;
  A(d->alloc(&d->bufA0, mx)); A(d->alloc(&d->bufA1, mx)); A(d->alloc(&d->bufY, mx)); A(d->alloc(&d->bufS, mx));
  A(d->alloc(&d->bufZ, (size_t)c.max_batch * c.max_frames * c.latent_dim));
  A(d->alloc(&d->d_ktap, MAXTAPS * 8));
#undef A
  *out = d;
  return PTTS_OK;
}

extern "C" int ptts_dac_load_weight(ptts_dac* d, const char* name_c, const float* dev_ptr, const int64_t* shape, int32_t ndim, void* stream) {
  PTTS_CHECK(d && name_c && dev_ptr && shape, PTTS_E_INVALID, "null argument");
  PTTS_DEVICE(d->cfg.device);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);  // NULL = legacy default stream
  const ptts_dac_config& c = d->cfg;
  const std::string name(name_c);
  auto numel = [&]() { size_t n = 1; for (int i = 0; i < ndim; ++i) n *= (size_t)shape[i]; return n; };
  auto copy = [&](float* dst, size_t n) -> int {
    if (numel() != n) return ptts_fail(PTTS_E_INVALID, "%s: expected %zu elements, got %zu", name_c, n, numel());
    PTTS_HIP(hipMemcpyAsync(dst, dev_ptr, n * 4, hipMemcpyDeviceToDevice, st));
    d->loaded.insert(name);
    return PTTS_OK;
  };
  int qi = -1;
  char tail[64] = {0};
  if (sscanf(name_c, "quantizer.quantizers.%d.%63s", &qi, tail) == 2) {
    PTTS_CHECK(qi >= 0 && qi < c.num_codebooks, PTTS_E_INVALID, "%s: quantizer index out of range", name_c);
    d->table_ready = false;
    d->vq_ready = false;
    const std::string t(tail);
    if (t == "codebook.weight") return copy(d->cb[qi], (size_t)c.codebook_size * c.codebook_dim);
    if (t == "out_proj.weight") return copy(d->opw[qi], (size_t)c.latent_dim * c.codebook_dim);
    if (t == "out_proj.bias") return copy(d->opb[qi], c.latent_dim);
    if (t == "in_proj.weight") { d->vq_ready = false; return c.encoder_dim > 0 ? copy(d->ipw + (size_t)qi * c.codebook_dim * c.latent_dim, (size_t)c.codebook_dim * c.latent_dim) : PTTS_OK; }
    if (t == "in_proj.bias") return c.encoder_dim > 0 ? copy(d->ipb + (size_t)qi * c.codebook_dim, c.codebook_dim) : PTTS_OK;
    return ptts_fail(PTTS_E_INVALID, "unknown tensor name %s", name_c);
  }
  char fin[64];
  snprintf(fin, sizeof fin, "decoder.model.%d", c.num_rates + 2);
  if (name == std::string(fin) + ".weight") {  // [1][C][7] -> [7][C]
    PTTS_CHECK(ndim == 3 && shape[0] == 1 && shape[1] == d->out_C && shape[2] == 7, PTTS_E_INVALID, "%s: expected [1,%d,7]", name_c, d->out_C);
    // transpose on device via strided copies: 7 rows
    for (int k = 0; k < 7; ++k)
      PTTS_HIP(hipMemcpy2DAsync(d->out_w + (size_t)k * d->out_C, 4, dev_ptr + k, 7 * 4, 4, d->out_C, hipMemcpyDeviceToDevice, st));
    d->loaded.insert(name);
    return PTTS_OK;
  }
  if (name == std::string(fin) + ".bias") return copy(d->out_b, 1);
  if (c.encoder_dim > 0) {
    if (name == "encoder.block.0.weight") return copy(d->in0_w, (size_t)c.encoder_dim * 7);
    if (name == "encoder.block.0.bias") return copy(d->in0_b, c.encoder_dim);
    if (name == "encoder.block.1.block.0.block.0.alpha") {
      PTTS_TRY(copy(d->in0_alpha, c.encoder_dim));
      hipLaunchKernelGGL(inv_alpha_kernel, dim3((c.encoder_dim + 255) / 256), dim3(256), 0, st, d->in0_alpha, c.encoder_dim);
      return PTTS_OK;
    }
  }
  std::vector<ConvLayer*> all;
  for (ConvLayer& L : d->convs) all.push_back(&L);
  for (ConvLayer& L : d->enc_convs) all.push_back(&L);
  for (ConvLayer* Lp : all) {
    ConvLayer& L = *Lp;
    if (!L.alpha_name.empty() && name == L.alpha_name + ".alpha") {
      PTTS_TRY(copy(L.alpha, L.Cout));
      hipLaunchKernelGGL(inv_alpha_kernel, dim3((L.Cout + 255) / 256), dim3(256), 0, st, L.alpha, L.Cout);
      return PTTS_OK;
    }
    if (name == L.name + ".bias") return copy(L.bias, L.Cout);
    if (name == L.name + ".weight") {
      const int k = L.ksize;
      if (!L.transposed)  // torch Conv1d weight [Cout][Cin][k]
        PTTS_CHECK(ndim == 3 && shape[0] == L.Cout && shape[1] == L.Cin && shape[2] == k, PTTS_E_INVALID, "%s: expected [%d,%d,%d]", name_c, L.Cout, L.Cin, k);
      else  // torch ConvTranspose1d weight [Cin][Cout][2s]
        PTTS_CHECK(ndim == 3 && shape[0] == L.Cin && shape[1] == L.Cout && shape[2] == k, PTTS_E_INVALID, "%s: expected [%d,%d,%d]", name_c, L.Cin, L.Cout, k);
      const DacPackPlan pk = dac_pack_plan(L.shape());
      PTTS_HIP(hipMemcpyAsync(d->d_ktap, pk.ktap, sizeof pk.ktap, hipMemcpyHostToDevice, st));
      dac_pack_launch(L.shape(), pk, dev_ptr, L.Wp, d->d_ktap, st);
      PTTS_HIP(hipStreamSynchronize(st));  // d_ktap is reused by the next call
      d->loaded.insert(name);
      return PTTS_OK;
    }
  }
  if (name.rfind("encoder.", 0) == 0) return PTTS_OK;  // DAC encoder weights are not on the decode path
  return ptts_fail(PTTS_E_INVALID, "unknown tensor name %s", name_c);
}

extern "C" int ptts_dac_weights_ready(ptts_dac* d) {
  PTTS_CHECK(d, PTTS_E_INVALID, "null dac");
  std::string missing;
  int n = 0;
  for (const auto& r : d->required)
    if (!d->loaded.count(r)) { if (n++ < 8) missing += (missing.empty() ? "" : ", ") + r; }
  if (n) return ptts_fail(PTTS_E_MISSING, "%d tensors not loaded: %s%s", n, missing.c_str(), n > 8 ? ", ..." : "");
  return PTTS_OK;
}

static int run_conv(ptts_dac* d, const ConvLayer& L, const void* x, const float* skip, float* out_raw, void* out_act, int B, int Tin, hipStream_t st,
                    bool act_f32 = false, const int* lens = nullptr, int len_mul = 1) {
  ConvArgs a = {};
  a.act_f32 = act_f32 ? 1 : 0;
  a.lens = lens; a.len_mul = len_mul;
  a.x = x; a.Wp = L.Wp; a.bias = L.bias; a.skip = skip; a.out_raw = out_raw; a.out_act = out_act; a.alpha = L.alpha;
  a.B = B; a.Tin = Tin; a.Cin = L.Cin; a.Cout = L.Cout;
  dac_conv_geometry(L.shape(), B, Tin, a);
  return dac_conv_launch(dac_conv_plan(L.shape(), B, Tin), a, st);  // the size rules: ptts_dac_launch.h
}

// one residual unit (k7 dilated conv -> Snake -> k1 conv -> + skip -> Snake) in one launch; out_act must not be x's buffer
static bool resunit_fusable(const ConvLayer& c7, const ConvLayer& c1) {
  const char* ev = getenv("PTTS_DAC_NO_FUSE_RES");  // read per call: a test can switch it inside one process
  return dac_resunit_fusable(c7.shape(), c1.shape(), c7.alpha && c1.alpha, ev ? atoi(ev) : 0);
}
// PTTS_DAC_XIN=<mask> is read per call (a test switches it inside one process: every mask gives the same bits); the default: ptts_dac_launch.h
static bool resunit_xin_width(int C, long long frames) {
  const char* ev = getenv("PTTS_DAC_XIN");
  return dac_resunit_xin_width(C, frames, ev ? atoi(ev) : -1);
}
// `alpha_in` != null: an XIN unit - x is the fp32 stream (= skip) and alpha_in the [alpha | 1 / alpha] of the Snake in front of the unit; out_raw must
// then be a DIFFERENT buffer (neighbouring workgroups read x's halo rows). out_act may be null for a unit whose consumer is an XIN unit.
static int run_resunit(const ConvLayer& c7, const ConvLayer& c1, const void* x, const float* skip, float* out_raw, void* out_act, int B, int T,
                       hipStream_t st, bool act_f32, const int* lens = nullptr, int len_mul = 1, const float* alpha_in = nullptr) {
  ResArgs r = {};
  r.a.lens = lens; r.a.len_mul = len_mul;
  r.a.x = x; r.a.Wp = c7.Wp; r.a.bias = c7.bias; r.a.alpha = c7.alpha; r.a.dil = c7.dil; r.a.pad = (c7.ksize - 1) * c7.dil / 2;
  r.a.B = B; r.a.Tin = T; r.a.Tn = T; r.a.Cin = c7.Cin; r.a.Cout = c7.Cout; r.a.ntaps = 7; r.a.nphase = 1; r.a.stride = 1;
  r.Wp1 = c1.Wp; r.bias1 = c1.bias; r.alpha1 = c1.alpha; r.skip = skip; r.out_raw = out_raw; r.out_act = out_act; r.act_f32 = act_f32 ? 1 : 0;
  r.alpha_in = alpha_in;
  DacResPlan pl;
  PTTS_TRY(dac_resunit_plan(c7.Cout, B, T, out_raw != nullptr, act_f32, alpha_in != nullptr, out_act != nullptr, &pl));
  return dac_resunit_launch(pl, r, st);
}

// ---- streaming out of a continuous session (ptts_dac_stream_decode) ----------------------------------------------------------------
// Every slot of a session is at its own frame and the special-id filter keeps a SUBSEQUENCE of a request's frames, so the codec's window of a
// slot is counted in kept frames and lives in a per-slot table on the device. One pass = absorb + plan (one workgroup per listed row), a
// gather that reads each row's window out of the table, the unchanged convolution stack on the left-aligned windows (ragged: `lens`), the
// final convolution with a per-row emit range, and a zero fill of every row's tail.
namespace {

constexpr int STREAM_ROWS = 32;  // descriptors per absorb launch: they travel as kernel arguments (no staging buffer, nothing to synchronise)
struct StreamRowsArg {
  int r0, n;
  ptts_dac_stream_row row[STREAM_ROWS];
};
// the voice twin's own arguments (include/ptts_dac_stream_voice.h): the slots' prefixes [slots][K][pre_ld] and the cap of one pass's emit
struct StreamVoiceArg {
  const int* pre;
  int pre_ld, max_emit;
};
// compact_codes_kernel's ballot scan with an append offset and the (col0, delay) indexing of the raw id buffer; lane 0 then plans the row.
// VOICE (ptts_dac_stream_decode_capped, or a table opened with prefix storage): raw frame f of a slot whose fourth counter holds a prefix
// length T (negative: the prompt is not emitted) comes from the prefix for f < T; the kept frames among those count as emitted at once when
// the prompt is skipped; emit is capped and the window ends `halo` kept frames behind what is emitted. Compile-time: the plain instance keeps
// its code.
template <bool VOICE>
__global__ void __launch_bounds__(256) stream_absorb_kernel(StreamRowsArg ra, const long long* __restrict__ ids, long long ids_ld, int col0, int delay,
                                                            int K, int ncodes, int* __restrict__ tab, int cap, int* __restrict__ state, int halo,
                                                            int hop, int Tmax, long long wave_ld, int* __restrict__ p_lens, int* __restrict__ p_start,
                                                            int* __restrict__ p_skip, int* __restrict__ p_tend, int* __restrict__ p_slot,
                                                            int* __restrict__ out, StreamVoiceArg va) {
  __shared__ int s_wsum[4];
  __shared__ int s_base;
  __shared__ int s_psum[4];  // VOICE: kept prompt frames of the block, per wave
  __shared__ int s_pbase;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const ptts_dac_stream_row row = ra.row[blockIdx.x];
  const int r = ra.r0 + blockIdx.x;
  int* st = state + (size_t)row.slot * 4;
  const int absorbed = st[0], kept0 = st[1];
  int emitted = st[2];
  const long long* src = ids + (size_t)row.slot * K * ids_ld + col0;
  int* dst = tab + (size_t)row.slot * K * cap;
  // VOICE: the slot's prefix; a request that brings none has Tp == 0 and reads the id buffer alone
  const int Tp = VOICE ? abs(st[3]) : 0;
  const bool skip_prompt = VOICE && st[3] < 0;
  const int* pre = VOICE && va.pre ? va.pre + (size_t)row.slot * K * va.pre_ld : nullptr;
  auto raw = [&](int k, int f) -> long long {
    if constexpr (VOICE) { if (f < Tp) return pre[(size_t)k * va.pre_ld + f]; }
    return src[(size_t)k * ids_ld + f + k * delay];
  };
  if (tid == 0) {
    s_base = 0;
    if constexpr (VOICE) s_pbase = 0;
  }
  __syncthreads();
  for (int c0 = absorbed; c0 < row.complete; c0 += 256) {
    const int f = c0 + tid;
    int keep = 0;
    if (f < row.complete) {
      keep = 1;
      for (int k = 0; k < K; ++k) { const long long v = raw(k, f); if (v < 0 || v >= ncodes) keep = 0; }
    }
    const unsigned long long m = __ballot(keep);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_wsum[wave] = __popcll(m);
    if constexpr (VOICE) {
      const unsigned long long mp = __ballot(keep && f < Tp);
      if (lane == 0) s_psum[wave] = __popcll(mp);
    }
    __syncthreads();
    int off = kept0 + s_base;
    for (int w2 = 0; w2 < wave; ++w2) off += s_wsum[w2];
    if (keep && off + before < cap)
      for (int k = 0; k < K; ++k) dst[(size_t)k * cap + off + before] = (int)raw(k, f);
    __syncthreads();
    if (tid == 0) {
      s_base += s_wsum[0] + s_wsum[1] + s_wsum[2] + s_wsum[3];
      if constexpr (VOICE) s_pbase += s_psum[0] + s_psum[1] + s_psum[2] + s_psum[3];
    }
    __syncthreads();
  }
  if (tid != 0) return;
  const int kept = min(kept0 + s_base, cap);
  // a skipped prompt: its kept frames are the head of the table (the prompt is absorbed first) and leave as they come in, as left context only
  if (skip_prompt) emitted = min(emitted + s_pbase, kept);
  const int ready = kept - emitted;
  int emit = row.final ? ready : (ready - halo >= max(row.min_emit, 1) ? ready - halo : 0);
  if constexpr (VOICE) emit = min(emit, va.max_emit);
  const int w0 = max(0, emitted - halo);
  // the window's end: a capped emit leaves kept frames behind it, of which `halo` are its right context (uncapped: this is `kept`)
  const int w1 = VOICE ? (int)min((long long)kept, (long long)emitted + emit + halo) : kept;
  // the host sized the launch and the output rows from upper bounds of these: never true, and if it were, no store leaves its buffer
  if (emit < 0 || w1 - w0 > Tmax || (long long)emit * hop > wave_ld) emit = 0;
  p_lens[r] = emit > 0 ? w1 - w0 : 0;
  p_start[r] = w0;
  p_skip[r] = (emitted - w0) * hop;
  p_tend[r] = (emitted - w0 + emit) * hop;
  p_slot[r] = row.slot;
  out[2 * r] = emit;
  out[2 * r + 1] = kept;
  st[0] = row.complete;
  st[1] = kept;
  st[2] = emitted + emit;
}

// ptts_dac_stream_reset_voice: the slot's prefix int64 [K][T] -> int [K][pre_ld] (an id outside int's range becomes -1: the filter drops its
// frame either way), and the slot's fourth counter: T, negative when the prompt's frames are not to be emitted
__global__ void __launch_bounds__(256) stream_prefix_kernel(const long long* __restrict__ codes, int K, int T, int* __restrict__ pre, int pre_ld,
                                                            int* __restrict__ st, int emit_prompt) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < K * T) {
    const long long v = codes[i];
    pre[(size_t)(i / T) * pre_ld + i % T] = (v < 0 || v > 0x7fffffffll) ? -1 : (int)v;
  }
  if (i == 0) st[3] = emit_prompt ? T : -T;
}

// samples [hop * emit, wave_ld) of every row are zero (emit = out[2r], written by the absorb kernel of the same pass)
__global__ void stream_zero_tail_kernel(float* __restrict__ wave, long long wave_ld, const int* __restrict__ out, int hop) {
  const int r = blockIdx.y;
  const long long from = (long long)out[2 * r] * hop;
  for (long long i = (long long)blockIdx.x * 1024 + threadIdx.x; i < min(wave_ld, ((long long)blockIdx.x + 1) * 1024); i += 256)
    if (i >= from) wave[(size_t)r * wave_ld + i] = 0.f;
}

}  // namespace

// parity probe (ptts_dac_debug_decode_upto): the buffers holding a stage's outputs when the decode stops there
struct DacDebugTap { void* act; int act_is_bf16; float* raw; int rows, channels; };

// decode the window [t0, t0 + T) of codes rows with stride `ld`; samples [skip, hop*T) of the window go to wave_dev rows of out_ld
static int dac_decode_window(ptts_dac* d, const int64_t* codes_dev, long long ld, int t0, float* wave_dev, int skip, long long out_ld,
                             int32_t B, int32_t T, void* stream, int emit = -1, const int* lens = nullptr, int stop_stage = -1,
                             DacDebugTap* tap = nullptr, const StreamPlan* sp = nullptr) {
  PTTS_TRY(ptts_dac_weights_ready(d));
  const ptts_dac_config& c = d->cfg;
  PTTS_CHECK(B >= 1 && B <= c.max_batch, PTTS_E_CAPACITY, "batch %d exceeds dac max_batch %d", B, c.max_batch);
  PTTS_CHECK(T >= 1 && T <= c.max_frames, PTTS_E_CAPACITY, "frames %d exceed dac max_frames %d", T, c.max_frames);
  PTTS_DEVICE(c.device);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);  // NULL = legacy default stream
  if (!d->table_ready) {
    for (int i = 0; i < c.num_codebooks; ++i) {
      const size_t n = (size_t)c.codebook_size * c.latent_dim;
      hipLaunchKernelGGL(rvq_table_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d->cb[i], d->opw[i], d->opb[i],
                         d->table + (size_t)i * n, c.codebook_size, c.codebook_dim, c.latent_dim);
    }
    d->table_ready = true;
  }
  const bool bf = c.compute_dtype == PTTS_BF16;
  auto gather = [&](auto stream_pass, auto src) {  // streaming pass: row b's window comes out of its slot's kept codes; lens == sp->lens
    hipLaunchKernelGGL((rvq_gather_kernel<decltype(stream_pass)::value>), dim3(T, B), dim3(256), 0, st, src, (const float*)d->table, (void*)d->bufZ,
                       c.num_codebooks, T, c.codebook_size, c.latent_dim, bf ? 1 : 0, ld, t0, lens);
  };
  if (sp) gather(std::true_type{}, *sp);
  else gather(std::false_type{}, (const long long*)codes_dev);
  float *cur = d->bufA0, *other = d->bufA1;
  int Tcur = T, mul = 1;  // mul: rows per latent frame at the current layer (ragged decode: utterance b has lens[b] * mul valid rows)
  size_t li = 0;
  PTTS_TRY(run_conv(d, d->convs[li++], d->bufZ, nullptr, nullptr, cur, B, Tcur, st, false, lens, mul));
  int stage = 0;  // 0 = decoder.model.0; per block: the transposed conv, then its three residual units
  const bool dbg = stop_stage >= 0;
  auto stop_here = [&](float* raw, int ch, bool act_f32) {
    if (stage++ != stop_stage) return false;
    if (tap) { tap->act = cur; tap->act_is_bf16 = (bf && !act_f32) ? 1 : 0; tap->raw = raw; tap->rows = Tcur; tap->channels = ch; }
    return true;
  };
  if (stop_here(nullptr, d->convs[0].Cout, false)) return PTTS_OK;
  for (int bi = 0; bi < c.num_rates; ++bi) {
    const ConvLayer& up = d->convs[li++];
    // XIN block (round 6): all three units fused and this width enabled - the units read the fp32 stream (bufY / bufS in turns; bufS is otherwise only
    // the un-fused units' y) and evaluate the Snake in front of them on the way into LDS; nobody writes a bf16 activation but the block's last unit
    // (and the parity probe's stop stage, whose outputs the test reads). Same values, bit for bit.
    bool xin = up.alpha != nullptr && resunit_xin_width(up.Cout, (long long)B * T);
    for (int ri = 0; ri < 3 && xin; ++ri) xin = resunit_fusable(d->convs[li + 2 * ri], d->convs[li + 2 * ri + 1]);
    const bool up_act = !xin || (dbg && stage == stop_stage);
    PTTS_TRY(run_conv(d, up, cur, nullptr, d->bufY, up_act ? other : nullptr, B, Tcur, st, false, lens, mul));
    std::swap(cur, other);
    Tcur *= up.stride;
    mul *= up.stride;
    if (stop_here(d->bufY, up.Cout, false)) return PTTS_OK;
    float *s_in = d->bufY, *s_out = d->bufS;  // XIN: the stream before / after the next unit
    const float* alpha_in = up.alpha;
    for (int ri = 0; ri < 3; ++ri) {
      const ConvLayer& c7 = d->convs[li++];
      const ConvLayer& c1 = d->convs[li++];
      const bool last = bi + 1 == c.num_rates && ri == 2;  // feeds the final Conv1d(C -> 1): fp32 activations
      if (xin) {
        const bool want_raw = ri < 2 || dbg, want_act = ri == 2 || (dbg && stage == stop_stage);
        PTTS_TRY(run_resunit(c7, c1, s_in, s_in, want_raw ? s_out : nullptr, want_act ? other : nullptr, B, Tcur, st, last, lens, mul, alpha_in));
        if (want_act) std::swap(cur, other);
        if (want_raw) std::swap(s_in, s_out);
        alpha_in = c1.alpha;
        if (stop_here(s_in, c1.Cout, last)) return PTTS_OK;
        continue;
      }
      float* raw_out = (c1.write_raw || dbg) ? d->bufY : nullptr;  // the parity probe also wants the stream after a block's last unit (same arithmetic, one more store)
      if (resunit_fusable(c7, c1)) {  // both convs in one launch; the output goes to the OTHER activation buffer
        PTTS_TRY(run_resunit(c7, c1, cur, d->bufY, raw_out, other, B, Tcur, st, last, lens, mul));
        std::swap(cur, other);
      } else {
        PTTS_TRY(run_conv(d, c7, cur, nullptr, nullptr, d->bufS, B, Tcur, st, false, lens, mul));
        PTTS_TRY(run_conv(d, c1, d->bufS, d->bufY, raw_out, cur, B, Tcur, st, last, lens, mul));
      }
      if (stop_here(d->bufY, c1.Cout, last)) return PTTS_OK;
    }
  }
  auto conv_out = [&](auto rows, auto skip_of, auto t_end_of) {  // LDS-tiled at the 44.1 kHz width, otherwise the per-thread kernel
    constexpr bool ROWS = decltype(rows)::value;
    return dac_conv_out_launch<ROWS>(dac_conv_out_plan(d->out_C, B, Tcur), (const float*)cur, (const float*)d->out_w, (const float*)d->out_b, wave_dev, B, Tcur,
                                     d->out_C, skip_of, out_ld, t_end_of, lens, mul, st);
  };
  if (sp) PTTS_TRY(conv_out(std::true_type{}, sp->skip, sp->tend));  // per-row emit range
  else PTTS_TRY(conv_out(std::false_type{}, skip, emit < 0 ? Tcur : std::min(Tcur, skip + emit)));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ptts_fail(PTTS_E_HIP, "dac launch failed: %s", hipGetErrorString(e));
  return PTTS_OK;
}

extern "C" int ptts_dac_decode(ptts_dac* d, const int64_t* codes_dev, float* wave_dev, int32_t B, int32_t T, void* stream) {
  PTTS_CHECK(d && codes_dev && wave_dev, PTTS_E_INVALID, "null argument");
  return dac_decode_window(d, codes_dev, T, 0, wave_dev, 0, (long long)d->hop * T, B, T, stream);
}

// Ragged batch (generate()'s per-sample branch, modeling_parler_tts.py:3615-3647: every utterance keeps its own number of frames after
// the special-id filter; the reference decodes them one by one and zero-pads): ONE pass over codes [B][K][T] in which utterance b is
// decoded as exactly frames_dev[b] frames - rows beyond its length read as the convolutions' zero padding, tiles beyond it exit at once,
// its samples beyond hop * frames_dev[b] are zero (the buffer is cleared first). frames_dev: int32 [B] ON THE DEVICE (no host round trip
// between the filter and the codec), values clamped to [0, T].
extern "C" int ptts_dac_decode_ragged(ptts_dac* d, const int64_t* codes_dev, const int32_t* frames_dev, float* wave_dev, int32_t B, int32_t T,
                                      void* stream) {
  PTTS_CHECK(d && codes_dev && frames_dev && wave_dev, PTTS_E_INVALID, "null argument");
  PTTS_CHECK(B >= 1 && T >= 1, PTTS_E_INVALID, "bad batch / frames");
  {
    PTTS_DEVICE(d->cfg.device);
    PTTS_HIP(hipMemsetAsync(wave_dev, 0, (size_t)B * d->hop * T * sizeof(float), reinterpret_cast<hipStream_t>(stream)));
  }
  return dac_decode_window(d, codes_dev, T, 0, wave_dev, 0, (long long)d->hop * T, B, T, stream, -1, frames_dev);
}

// The filter in front of it (modeling_parler_tts.py:3627-3636): per utterance, drop every frame (column) in which ANY codebook holds an
// id >= codebook_size (or < 0), keep the others in order. codes_in / codes_out int64 [B][K][T] (may NOT alias), frames_out int32 [B].
// One workgroup per utterance: keep flags -> block-wide exclusive scan over the T columns -> scatter; columns past the kept count are
// filled with 0 (a valid id: the ragged decode never reads them).
__global__ void __launch_bounds__(256) compact_codes_kernel(const long long* __restrict__ in, long long* __restrict__ out, int* __restrict__ frames,
                                                            int K, int T, int ncodes) {
  __shared__ int s_wsum[4];
  __shared__ int s_base;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long* src = in + (size_t)b * K * T;
  long long* dst = out + (size_t)b * K * T;
  if (tid == 0) s_base = 0;
  __syncthreads();
  for (int c0 = 0; c0 < T; c0 += 256) {
    const int t = c0 + tid;
    int keep = 0;
    if (t < T) {
      keep = 1;
      for (int k = 0; k < K; ++k) { const long long v = src[(size_t)k * T + t]; if (v < 0 || v >= ncodes) keep = 0; }
    }
    // exclusive scan of `keep` over the 256 columns of this chunk: wave ballot + 4 wave totals
    const unsigned long long m = __ballot(keep);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_wsum[wave] = __popcll(m);
    __syncthreads();
    int off = s_base;
    for (int w2 = 0; w2 < wave; ++w2) off += s_wsum[w2];
    if (keep) for (int k = 0; k < K; ++k) dst[(size_t)k * T + off + before] = src[(size_t)k * T + t];
    __syncthreads();
    if (tid == 0) s_base += s_wsum[0] + s_wsum[1] + s_wsum[2] + s_wsum[3];
    __syncthreads();
  }
  const int n = s_base;
  for (int i = tid; i < (T - n) * K; i += 256) dst[(size_t)(i / (T - n)) * T + n + i % (T - n)] = 0;
  if (tid == 0) frames[b] = n;
}

extern "C" int ptts_dac_compact_codes(ptts_dac* d, const int64_t* codes_in_dev, int64_t* codes_out_dev, int32_t* frames_out_dev, int32_t B, int32_t T,
                                      void* stream) {
  PTTS_CHECK(d && codes_in_dev && codes_out_dev && frames_out_dev, PTTS_E_INVALID, "null argument");
  PTTS_CHECK(B >= 1 && T >= 1 && codes_in_dev != codes_out_dev, PTTS_E_INVALID, "bad batch / frames, or codes_out aliases codes_in");
  PTTS_DEVICE(d->cfg.device);
  hipLaunchKernelGGL(compact_codes_kernel, dim3(B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), (const long long*)codes_in_dev,
                     (long long*)codes_out_dev, (int*)frames_out_dev, d->cfg.num_codebooks, T, d->cfg.codebook_size);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ptts_fail(PTTS_E_HIP, "compact launch failed: %s", hipGetErrorString(e));
  return PTTS_OK;
}

// Streaming / chunked decode (parler_tts/streamer.py:66-131 re-decodes the WHOLE token cache every `play_steps`): samples of
// frames [first_frame, first_frame + n_frames) of codes [B][K][codes_ld], computed from the window that starts `halo` frames
// earlier (clamped at 0) and ends at first_frame + n_frames - exactly the samples a decode of frames [0, first_frame + n_frames)
// yields there whenever `halo` covers the decoder's one-sided receptive field (13 frames for strides 8, 8, 4, 2).
extern "C" int ptts_dac_decode_chunk(ptts_dac* d, const int64_t* codes_dev, int64_t codes_ld, int32_t first_frame, int32_t n_frames,
                                     int32_t halo, float* wave_dev, int64_t wave_ld, int32_t n_emit, int32_t B, void* stream) {
  PTTS_CHECK(d && codes_dev && wave_dev, PTTS_E_INVALID, "null argument");
  PTTS_CHECK(first_frame >= 0 && n_frames >= 1 && halo >= 0 && (int64_t)first_frame + n_frames <= codes_ld, PTTS_E_INVALID,
             "bad chunk [%d, %d) of %lld frames (halo %d)", first_frame, first_frame + n_frames, (long long)codes_ld, halo);
  if (n_emit <= 0 || n_emit > n_frames) n_emit = n_frames;
  if (wave_ld <= 0) wave_ld = (int64_t)d->hop * n_emit;
  PTTS_CHECK(wave_ld >= (int64_t)d->hop * n_emit, PTTS_E_INVALID, "wave_ld %lld < %d emitted frames", (long long)wave_ld, n_emit);
  const int w0 = first_frame > halo ? first_frame - halo : 0;
  return dac_decode_window(d, codes_dev, codes_ld, w0, wave_dev, (first_frame - w0) * d->hop, wave_ld, B, first_frame + n_frames - w0, stream,
                           n_emit * d->hop);
}

// ---- streaming out of a continuous session: include/ptts.h "streaming out of a continuous session" ----
// max_voice_frames > 0: + the slots' prefix storage (ptts_dac_stream_open_voice)
static int dac_stream_open(ptts_dac* d, int32_t slots, int32_t cap_frames, int32_t max_voice_frames, void* stream) {
  PTTS_CHECK(d, PTTS_E_INVALID, "null argument");
  PTTS_CHECK(slots >= 1 && slots <= d->cfg.max_batch, PTTS_E_CAPACITY, "stream slots %d exceed dac max_batch %d", slots, d->cfg.max_batch);
  PTTS_CHECK(cap_frames >= 1, PTTS_E_INVALID, "bad stream capacity %d", cap_frames);
  PTTS_CHECK(max_voice_frames >= 0, PTTS_E_INVALID, "bad max_voice_frames %d", max_voice_frames);
  PTTS_DEVICE(d->cfg.device);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (slots != d->st_slots || cap_frames != d->st_cap || max_voice_frames != d->st_pre_ld) {
    PTTS_HIP(hipStreamSynchronize(st));  // a pass in flight still reads the old table
    for (int** p : {&d->st_tab, &d->st_state, &d->st_plan, &d->st_pre}) { if (*p) hipFree(*p); *p = nullptr; }
    d->st_slots = d->st_cap = d->st_pre_ld = 0;
    PTTS_HIP(hipMalloc((void**)&d->st_tab, (size_t)slots * d->cfg.num_codebooks * cap_frames * sizeof(int)));
    PTTS_HIP(hipMalloc((void**)&d->st_state, (size_t)slots * 4 * sizeof(int)));
    PTTS_HIP(hipMalloc((void**)&d->st_plan, (size_t)slots * 5 * sizeof(int)));
    if (max_voice_frames > 0) PTTS_HIP(hipMalloc((void**)&d->st_pre, (size_t)slots * d->cfg.num_codebooks * max_voice_frames * sizeof(int)));
    d->st_slots = slots;
    d->st_cap = cap_frames;
    d->st_pre_ld = max_voice_frames;
  }
  PTTS_HIP(hipMemsetAsync(d->st_state, 0, (size_t)slots * 4 * sizeof(int), st));
  PTTS_HIP(hipMemsetAsync(d->st_plan, 0, (size_t)slots * 5 * sizeof(int), st));
  d->st_absorbed.assign(slots, 0);
  d->st_ready_ub.assign(slots, 0);
  d->st_voice.assign(slots, 0);
  return PTTS_OK;
}

extern "C" int ptts_dac_stream_open(ptts_dac* d, int32_t slots, int32_t cap_frames, void* stream) {
  return dac_stream_open(d, slots, cap_frames, 0, stream);
}

extern "C" int ptts_dac_stream_open_voice(ptts_dac* d, int32_t slots, int32_t cap_frames, int32_t max_voice_frames, void* stream) {
  return dac_stream_open(d, slots, cap_frames, max_voice_frames, stream);
}

extern "C" int ptts_dac_stream_reset(ptts_dac* d, int32_t slot, void* stream) {
  PTTS_CHECK(d, PTTS_E_INVALID, "null argument");
  PTTS_CHECK(d->st_slots > 0, PTTS_E_INVALID, "no stream table: call ptts_dac_stream_open first");
  PTTS_CHECK(slot >= 0 && slot < d->st_slots, PTTS_E_INVALID, "stream slot %d out of range [0, %d)", slot, d->st_slots);
  PTTS_DEVICE(d->cfg.device);
  PTTS_HIP(hipMemsetAsync(d->st_state + (size_t)slot * 4, 0, 4 * sizeof(int), reinterpret_cast<hipStream_t>(stream)));
  d->st_absorbed[slot] = d->st_ready_ub[slot] = d->st_voice[slot] = 0;
  return PTTS_OK;
}

extern "C" int ptts_dac_stream_reset_voice(ptts_dac* d, int32_t slot, const int64_t* codes_dev, int32_t T, int32_t emit_prompt, void* stream) {
  PTTS_CHECK(d, PTTS_E_INVALID, "null argument");
  PTTS_CHECK(d->st_slots > 0, PTTS_E_INVALID, "no stream table: call ptts_dac_stream_open first");
  PTTS_CHECK(slot >= 0 && slot < d->st_slots, PTTS_E_INVALID, "stream slot %d out of range [0, %d)", slot, d->st_slots);
  PTTS_CHECK(T >= 0, PTTS_E_INVALID, "bad voice prompt: %d frames", T);
  if (T == 0) return ptts_dac_stream_reset(d, slot, stream);
  PTTS_CHECK(d->st_pre, PTTS_E_INVALID, "the stream table has no prefix storage: open it with ptts_dac_stream_open_voice");
  PTTS_CHECK(T <= d->st_pre_ld, PTTS_E_INVALID, "voice prompt of %d frames, the stream table was opened for %d", T, d->st_pre_ld);
  PTTS_CHECK(codes_dev, PTTS_E_INVALID, "null voice prompt codes with %d frames", T);
  PTTS_TRY(ptts_dac_stream_reset(d, slot, stream));
  const int K = d->cfg.num_codebooks;
  PTTS_DEVICE(d->cfg.device);
  hipLaunchKernelGGL(stream_prefix_kernel, dim3((unsigned)(((size_t)K * T + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     (const long long*)codes_dev, K, T, d->st_pre + (size_t)slot * K * d->st_pre_ld, d->st_pre_ld, d->st_state + (size_t)slot * 4,
                     emit_prompt);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ptts_fail(PTTS_E_HIP, "stream prefix launch failed: %s", hipGetErrorString(e));
  d->st_voice[slot] = emit_prompt ? T : -T;
  return PTTS_OK;
}

// max_emit == INT_MAX: no cap (ptts_dac_stream_decode). The plain kernel instance runs iff there is neither a cap nor prefix storage.
static int dac_stream_decode(ptts_dac* d, const int64_t* ids_dev, int64_t ids_ld, int32_t col0, int32_t delay, const ptts_dac_stream_row* rows_host,
                             int32_t R, int32_t halo, float* wave_dev, int64_t wave_ld, int32_t* out_dev, void* stream, int32_t max_emit) {
  PTTS_CHECK(d && ids_dev && rows_host && wave_dev && out_dev, PTTS_E_INVALID, "null argument");
  PTTS_CHECK(d->st_slots > 0, PTTS_E_INVALID, "no stream table: call ptts_dac_stream_open first");
  PTTS_CHECK(max_emit >= 1, PTTS_E_INVALID, "bad stream pass: max_emit %d", max_emit);
  PTTS_TRY(ptts_dac_weights_ready(d));
  const ptts_dac_config& c = d->cfg;
  const int K = c.num_codebooks;
  PTTS_CHECK(R >= 1 && R <= d->st_slots, PTTS_E_INVALID, "bad stream pass: %d rows for %d slots", R, d->st_slots);
  PTTS_CHECK(halo >= 0 && col0 >= 0 && delay >= 0 && ids_ld >= 1 && wave_ld >= 1, PTTS_E_INVALID, "bad stream pass: halo %d, col0 %d, delay %d, ids_ld %lld, wave_ld %lld",
             halo, col0, delay, (long long)ids_ld, (long long)wave_ld);
  // validate every row and bound its window before anything is enqueued or counted
  int T = 0;
  long long emit_ub_max = 0;
  std::vector<char> seen(d->st_slots, 0);
  // the bound of ready once [absorbed, complete) is in: every raw frame may be kept, but those of a skipped prompt never become ready
  auto ready_bound = [&](const ptts_dac_stream_row& w) {
    const int v = d->st_voice[w.slot], a = d->st_absorbed[w.slot];
    return d->st_ready_ub[w.slot] + (v < 0 ? std::max(w.complete, -v) - std::max(a, -v) : w.complete - a);
  };
  for (int r = 0; r < R; ++r) {
    const ptts_dac_stream_row& w = rows_host[r];
    PTTS_CHECK(w.slot >= 0 && w.slot < d->st_slots, PTTS_E_INVALID, "bad stream row %d: slot %d out of range [0, %d)", r, w.slot, d->st_slots);
    PTTS_CHECK(!seen[w.slot], PTTS_E_INVALID, "bad stream row %d: slot %d listed twice", r, w.slot);
    seen[w.slot] = 1;
    PTTS_CHECK(w.complete >= d->st_absorbed[w.slot], PTTS_E_INVALID, "bad stream row %d: complete %d decreases (slot %d has absorbed %d raw frames)", r,
               w.complete, w.slot, d->st_absorbed[w.slot]);
    PTTS_CHECK(w.complete <= d->st_cap, PTTS_E_INVALID, "bad stream row %d: complete %d beyond the table's %d frames", r, w.complete, d->st_cap);
    PTTS_CHECK((long long)col0 + w.complete + (long long)(K - 1) * delay <= ids_ld || w.complete == d->st_absorbed[w.slot], PTTS_E_INVALID,
               "bad stream row %d: complete %d reads beyond ids_ld %lld (col0 %d, delay %d)", r, w.complete, (long long)ids_ld, col0, delay);
    const int ready_ub = ready_bound(w);
    const int emit_ub = std::min(w.final ? ready_ub : (ready_ub - halo >= std::max(w.min_emit, 1) ? ready_ub - halo : 0), max_emit);
    if (emit_ub > 0) {
      // the window holds kept frames only: never more than the raw frames; a capped emit has `halo` frames on either side
      T = std::max<long long>(T, std::min<long long>({(long long)halo + ready_ub, w.complete, 2ll * halo + max_emit}));
      emit_ub_max = std::max<long long>(emit_ub_max, emit_ub);
    }
  }
  PTTS_CHECK(T <= c.max_frames, PTTS_E_CAPACITY, "stream window of up to %d frames exceeds dac max_frames %d", T, c.max_frames);
  PTTS_CHECK(R <= c.max_batch, PTTS_E_CAPACITY, "batch %d exceeds dac max_batch %d", R, c.max_batch);
  PTTS_CHECK(wave_ld >= emit_ub_max * d->hop, PTTS_E_INVALID, "wave_ld %lld < %lld frames that may be emitted", (long long)wave_ld, emit_ub_max);
  PTTS_DEVICE(c.device);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int* pl = d->st_plan;
  const int S = d->st_slots;
  for (int r0 = 0; r0 < R; r0 += STREAM_ROWS) {
    StreamRowsArg ra;
    ra.r0 = r0;
    ra.n = std::min(STREAM_ROWS, R - r0);
    memset(ra.row, 0, sizeof ra.row);
    memcpy(ra.row, rows_host + r0, (size_t)ra.n * sizeof(ptts_dac_stream_row));
    auto absorb = [&](auto voice) {
      hipLaunchKernelGGL((stream_absorb_kernel<decltype(voice)::value>), dim3(ra.n), dim3(256), 0, st, ra, (const long long*)ids_dev, (long long)ids_ld,
                         col0, delay, K, c.codebook_size, d->st_tab, d->st_cap, d->st_state, halo, d->hop, T, (long long)wave_ld, pl, pl + S, pl + 2 * S,
                         pl + 3 * S, pl + 4 * S, (int*)out_dev, StreamVoiceArg{d->st_pre, d->st_pre_ld, max_emit});
    };
    if (d->st_pre || max_emit != INT_MAX) absorb(std::true_type{});
    else absorb(std::false_type{});
  }
  for (int r = 0; r < R; ++r) {
    const ptts_dac_stream_row& w = rows_host[r];
    const int before = ready_bound(w);
    // emitted: `halo` frames are left; not emitted: fewer than halo + min_emit were ready; flushed: none. A capped emit leaves ready - max_emit
    // (max_emit == INT_MAX: never the larger one)
    const int ub = std::max(w.final ? 0 : std::min(before, halo + std::max(w.min_emit, 1) - 1), before - max_emit);
    d->st_ready_ub[w.slot] = ub;
    d->st_absorbed[w.slot] = w.complete;
  }
  if (T > 0) {
    const StreamPlan sp{d->st_tab, pl, pl + S, pl + 2 * S, pl + 3 * S, pl + 4 * S, d->st_cap};
    PTTS_TRY(dac_decode_window(d, nullptr, 0, 0, wave_dev, 0, wave_ld, R, T, stream, -1, pl, -1, nullptr, &sp));
  }
  hipLaunchKernelGGL(stream_zero_tail_kernel, dim3((unsigned)((wave_ld + 1023) / 1024), (unsigned)R), dim3(256), 0, st, wave_dev, (long long)wave_ld,
                     (const int*)out_dev, d->hop);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ptts_fail(PTTS_E_HIP, "stream decode launch failed: %s", hipGetErrorString(e));
  return PTTS_OK;
}

extern "C" int ptts_dac_stream_decode(ptts_dac* d, const int64_t* ids_dev, int64_t ids_ld, int32_t col0, int32_t delay,
                                      const ptts_dac_stream_row* rows_host, int32_t R, int32_t halo, float* wave_dev, int64_t wave_ld,
                                      int32_t* out_dev, void* stream) {
  return dac_stream_decode(d, ids_dev, ids_ld, col0, delay, rows_host, R, halo, wave_dev, wave_ld, out_dev, stream, INT_MAX);
}

extern "C" int ptts_dac_stream_decode_capped(ptts_dac* d, const int64_t* ids_dev, int64_t ids_ld, int32_t col0, int32_t delay,
                                             const ptts_dac_stream_row* rows_host, int32_t R, int32_t halo, float* wave_dev, int64_t wave_ld,
                                             int32_t* out_dev, void* stream, int32_t max_emit) {
  return dac_stream_decode(d, ids_dev, ids_ld, col0, delay, rows_host, R, halo, wave_dev, wave_ld, out_dev, stream, max_emit);
}

// DACModel.encode (dac_wrapper/modeling_dac.py:33-104) for one chunk: wave_dev float32 [B][L] with L a multiple of the hop
// (the caller applies model.preprocess's right padding, :64) -> codes_dev int64 [B][nq][L / hop].
extern "C" int ptts_dac_encode(ptts_dac* d, const float* wave_dev, int64_t* codes_dev, int32_t B, int32_t L, int32_t n_quantizers, void* stream) {
  PTTS_CHECK(d && wave_dev && codes_dev, PTTS_E_INVALID, "null argument");
  const ptts_dac_config& c = d->cfg;
  PTTS_CHECK(c.encoder_dim > 0, PTTS_E_UNSUPPORTED, "this dac engine was created without the encoder (encoder_dim = 0)");
  PTTS_TRY(ptts_dac_weights_ready(d));
  PTTS_CHECK(B >= 1 && B <= c.max_batch, PTTS_E_CAPACITY, "batch %d exceeds dac max_batch %d", B, c.max_batch);
  PTTS_CHECK(L >= d->hop && L % d->hop == 0, PTTS_E_INVALID, "waveform length %d is not a positive multiple of the hop %d (apply preprocess padding)", L, d->hop);
  const int T = L / d->hop;
  PTTS_CHECK(T <= c.max_frames, PTTS_E_CAPACITY, "frames %d exceed dac max_frames %d", T, c.max_frames);
  const int nq = n_quantizers <= 0 || n_quantizers > c.num_codebooks ? c.num_codebooks : n_quantizers;
  PTTS_DEVICE(c.device);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!d->vq_ready) {  // contiguous [K][...] copies for the search kernel + the normalised codebooks
    for (int i = 0; i < c.num_codebooks; ++i) {
      const size_t ncb = (size_t)c.codebook_size * c.codebook_dim, nw = (size_t)c.latent_dim * c.codebook_dim;
      PTTS_HIP(hipMemcpyAsync(d->cb_all + i * ncb, d->cb[i], ncb * 4, hipMemcpyDeviceToDevice, st));
      PTTS_HIP(hipMemcpyAsync(d->opw_all + i * nw, d->opw[i], nw * 4, hipMemcpyDeviceToDevice, st));
      PTTS_HIP(hipMemcpyAsync(d->opb_all + (size_t)i * c.latent_dim, d->opb[i], (size_t)c.latent_dim * 4, hipMemcpyDeviceToDevice, st));
      hipLaunchKernelGGL(cb_normalize_kernel, dim3((c.codebook_size + 255) / 256), dim3(256), 0, st, d->cb_all + i * ncb, d->cbn + i * ncb,
                         d->cbn_sq + (size_t)i * c.codebook_size, c.codebook_size, c.codebook_dim);
    }
    d->vq_ready = true;
  }
  float *cur = d->bufA0, *other = d->bufA1;
  int Tcur = L;
  {
    const size_t n = (size_t)B * L * (c.encoder_dim / 4);
    hipLaunchKernelGGL(conv_in_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, wave_dev, d->in0_w, d->in0_b, d->in0_alpha, d->bufY, cur, B,
                       L, c.encoder_dim);
  }
  size_t li = 0;
  for (int bi = 0; bi < c.num_rates; ++bi) {
    for (int ri = 0; ri < 3; ++ri) {
      const ConvLayer& c7 = d->enc_convs[li++];
      PTTS_TRY(run_conv(d, c7, cur, nullptr, nullptr, d->bufS, B, Tcur, st));
      const ConvLayer& c1 = d->enc_convs[li++];
      PTTS_TRY(run_conv(d, c1, d->bufS, d->bufY, c1.write_raw ? d->bufY : nullptr, cur, B, Tcur, st));
    }
    const ConvLayer& down = d->enc_convs[li++];
    PTTS_TRY(run_conv(d, down, cur, nullptr, d->bufY, other, B, Tcur, st));
    std::swap(cur, other);
    Tcur = (Tcur + 2 * down.pad - down.ksize) / down.stride + 1;
  }
  PTTS_CHECK(Tcur == T, PTTS_E_INVALID, "encoder produced %d frames for %d expected", Tcur, T);
  PTTS_TRY(run_conv(d, d->enc_convs[li++], cur, nullptr, d->bufZ, nullptr, B, Tcur, st));
  hipLaunchKernelGGL(rvq_encode_kernel, dim3(T, B), dim3(256), (size_t)c.latent_dim * 4, st, d->bufZ, d->ipw, d->ipb, d->cb_all, d->cbn, d->cbn_sq,
                     d->opw_all, d->opb_all, (long long*)codes_dev, T, c.latent_dim, c.codebook_dim, c.codebook_size, nq);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ptts_fail(PTTS_E_HIP, "dac encode launch failed: %s", hipGetErrorString(e));
  return PTTS_OK;
}

// Debug / parity probe: ptts_dac_decode stopped after `stage` (0 = decoder.model.0; then per up-sampling block: its transposed conv, residual
// unit 1, 2, 3: 1 + 4 * num_rates stages in all). Hands out the engine's own buffers holding that stage's outputs (valid until the next call):
// act [B][rows][channels] = the Snake'd activation the next conv reads (bf16 bits if *act_is_bf16, else fp32), raw [B][rows][channels] fp32 =
// the residual stream (null for stage 0). tests/test_dac_stage_parity_gpu.py feeds stage s - 1's outputs to the oracle's restatement of stage s:
// every kernel is pinned on IDENTICAL inputs, free of the end-to-end amplification of bf16 rounding flips.
extern "C" int ptts_dac_debug_decode_upto(ptts_dac* d, const int64_t* codes_dev, int32_t B, int32_t T, int32_t stage, void* stream, void** act_dev,
                                          int32_t* act_is_bf16, float** raw_dev, int32_t* rows, int32_t* channels) {
  PTTS_CHECK(d && codes_dev && act_dev && act_is_bf16 && raw_dev && rows && channels, PTTS_E_INVALID, "null argument");
  PTTS_CHECK(stage >= 0 && stage < 1 + 4 * d->cfg.num_rates, PTTS_E_INVALID, "stage %d out of range [0, %d)", stage, 1 + 4 * d->cfg.num_rates);
  DacDebugTap tap = {};
  PTTS_TRY(dac_decode_window(d, codes_dev, T, 0, d->bufS /* unused: the decode stops before the final conv */, 0, (long long)d->hop * T, B, T, stream, -1, nullptr,
                             stage, &tap));
  *act_dev = tap.act; *act_is_bf16 = tap.act_is_bf16; *raw_dev = tap.raw; *rows = tap.rows; *channels = tap.channels;
  return PTTS_OK;
}

// Debug / parity probe: the latents z of the last ptts_dac_encode, channels-last fp32 [B][T][latent].
extern "C" int ptts_dac_debug_latents(ptts_dac* d, float** latents_dev) {
  PTTS_CHECK(d && latents_dev, PTTS_E_INVALID, "null argument");
  *latents_dev = d->bufZ;
  return PTTS_OK;
}
