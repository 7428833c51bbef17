// gemm_glds_kernel (round 6): the prefill-sized GEMM (> 256 activation rows: T5 on 32 descriptions x 64 tokens = 2048 rows, the prefill of 32
// utterances x 33 positions = 1056 rows) as an LDS ring filled by LDS-DMA (`global_load_lds_dwordx4`: global -> LDS without destination registers),
// NST stages deep, ONE raw s_barrier per stage and COUNTED vmcnt waits - loads stay in flight across the barriers. Round 5's gemm_tile_kernel staged
// global -> registers -> LDS two stages ahead and ran at 6-15 % of the bf16 MFMA peak (144-364 TFLOP/s, profiles/r05_prefill_kernels_bs32.txt): with
// K = 1024 a workgroup's whole MFMA work is shorter than one memory latency and the register ring cannot be deepened (VGPRs).
//   out[m][n] = sum_k W[n][k] x[m][k]     (modeling_parler_tts.py:3048-3097 description encoder, :1437-1439 prefill rows, :877-878 cross K/V)
// Operands (bf16 engine only; the fp32 parity engine keeps gemm_tile_kernel):
//   A = weights, packed at load in MFMA A-fragment order [N/16 strips][K/32 fragments][64 lanes][16 B]: one fragment = one contiguous 1 KiB = ONE
//       LDS-DMA wave-instruction, and the lane-linear LDS image (base + lane * 16) is exactly what the fragment's ds_read_b128 wants (conflict-free)
//   B = activations, row-major bf16 [M][K]: one wave-instruction brings 8 rows x 128 B (full cache lines: lanes 8 r .. 8 r + 7 read one line) into an
//       [8][8 x 16 B] image; the 16-byte piece a lane FETCHES is permuted within its line (piece = slot ^ row & 7: the swizzle sits on the SOURCE
//       address, the LDS-DMA destination is always lane-linear) and the fragment read applies the same XOR: the 16 lanes of every ds_read_b128 lane
//       group hit 16 different 16-byte slots of the 256-byte bank row (conflict-free; linear rows would be 4-way)
// Tile: BNS strips (16 weight rows each) x BMT row tiles (16 activation rows each) per workgroup, WN x WM waves of (BNS / WN) x (BMT / WM) MFMA tiles,
// BK = 64 per stage (2 fragments). Accumulation order over k is ascending whole fragments, no K split: bit-identical to gemm_tile_kernel /
// gemm_block_kernel (tests/test_gemm_kernels_gpu.py compares the three bitwise on random data). Epilogues: gemm_store_tile (store / residual / GELU /
// gated GELU / cross K/V scatter).
#pragma once
#include "ptts_lm_kernels.h"

namespace {

template <int N> __device__ __forceinline__ void ptts_wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// Kernel-argument preload (ptts_common.h; call 52): everything that addresses the wave's first LDS-DMA pieces arrives in SGPRs written by the command
// processor - W, x, K, M, the activation row stride, the tile order and the grid extents (gridDim is a hidden argument behind an s_load); the tail
// (epilogue operands) comes by s_load in the shadow of the first stage. The two pad slots keep the strip kernel's parameter layout.
#define GemmGldsHead_KHEAD(X)                                                                                                            \
  KDBG0(X)                                                                                                                               \
  KF(X, const void*, W)       /* weights in A-fragment order */                                                                          \
  KF(X, const void*, pad0_)                                                                                                              \
  KF(X, const float*, x)      /* activations, bf16 rows with row stride x_ld (consecutive rows: x_row_mul 1, x_row_off 0) */              \
  KF(X, float*, out) KF(X, int, K) KF(X, int, M) KF(X, int, x_ld)                                                                                           \
  KF(X, unsigned, tiles)      /* xcd_swz | tiles along N << 1 (11 bits) | tiles along M << 12 (20 bits): the grid; widths and rows checked \
                                 at engine creation */                                                                                    \
  KF(X, int, out_ld) KF(X, int, pad1_) KTAIL(X, GemmArgs)
struct GemmGldsHead {
  PTTS_KMEMBERS(GemmGldsHead)
  // the smallest tile is 64 x 64: the extents of any GEMM over N columns and `rows` rows fit the fields if these do
  static bool fits(long long N, long long rows) { return N / 64 <= 0x7ff && (rows + 63) / 64 <= 0xfffff; }
  static int pack(const GemmArgs& a, dim3 grid, GemmGldsHead& h) {
    if (a.x_row_mul != 1 || a.x_row_off != 0) return ptts_fail(PTTS_E_UNSUPPORTED, "gemm_glds: activation rows must be consecutive (x_row_mul %d, x_row_off %d)", a.x_row_mul, a.x_row_off);
    if (grid.x > 0x7ffu || grid.y > 0xfffffu) return ptts_fail(PTTS_E_UNSUPPORTED, "gemm_glds: %u x %u tiles above the 11- / 20-bit grid extents", grid.x, grid.y);
    h.W = a.W; h.pad0_ = nullptr; h.x = a.x; h.out = a.out; h.K = a.K; h.M = a.M; h.x_ld = a.x_ld;
    h.tiles = (a.xcd_swz ? 1u : 0u) | (grid.x << 1) | (grid.y << 12); h.out_ld = a.out_ld; h.pad1_ = 0;
    return PTTS_OK;
  }
  __device__ __forceinline__ void unpack(GemmArgs& a) const {
    a.W = W; a.x = x; a.out = out; a.K = K; a.M = M; a.out_ld = out_ld;
  }
  __device__ __forceinline__ int xcd_swz() const { return tiles & 1; }
  __device__ __forceinline__ int grid_n() const { return (tiles >> 1) & 0x7ff; }
  __device__ __forceinline__ int grid_m() const { return (int)(tiles >> 12); }
};
PTTS_KLAUNCH_VIA(GemmGldsHead, GemmArgs)

// RP = 1: every fragment read of a stage is issued before its first MFMA; RP = 0: reads and MFMAs one fragment at a time
template <int EPI, int BNS, int BMT, int WN, int WM, int NST, int RP = 0>
__global__ void __launch_bounds__(WN * WM * 64) gemm_glds_kernel(PTTS_KPARAMS(GemmGldsHead)) {
  PTTS_KJOIN_VIA(GemmGldsHead, GemmArgs, a)
  const int x_ld = h_.x_ld, xcd_swz = h_.xcd_swz(), grid_n = h_.grid_n(), grid_m = h_.grid_m();
  typedef bf16_t WT;
  constexpr int FPS = 2;  // fragments per stage: BK = 64
  constexpr int RB = FPS * 64, SPR = RB / 16, RPP = 1024 / RB;  // activation image: bytes per row, 16-byte slots per row, rows per 1 KiB piece
  constexpr int NW = WN * WM, NS = BNS / WN, MT = BMT / WM;
  constexpr int APC = BNS * FPS, BPC = BMT * FPS;           // 1 KiB pieces per stage: weights, activations
  // pieces per wave and stage (the first APW of them weight pieces). EVEN: every wave moves the same pieces per stage, weights first; otherwise
  // (tiles such as 176 weight rows: 22 + 32 pieces on 8 waves) piece p = wave + NW * i is a weight piece iff p < APC, decided per wave at run time, and a
  // wave without an i-th piece fetches its (i - 1)-th again (same source, same destination: the per-wave load count stays a compile-time constant)
  constexpr bool EVEN = APC % NW == 0 && BPC % NW == 0;
  constexpr int PPW = (APC + BPC + NW - 1) / NW, APW = APC / NW;
  static_assert(BNS % WN == 0 && BMT % WM == 0, "tile / wave split");
  static_assert((NST - 2) * PPW <= 63 && NST >= 2, "vmcnt is a 6-bit counter");
  constexpr int STAGE_B = (APC + BPC) * 1024;
  extern __shared__ __attribute__((aligned(1024))) char smem_raw[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), wn = wave % WN, wm = wave / WN;
  const int q = lane >> 4, j = lane & 15;
  if constexpr (EPI == EPI_KV) {  // the description's K/V of EVERY layer in one launch: blockIdx.z selects the layer's weights and caches
    if (a.kv_layers) { const KvLayer kl = a.kv_layers[blockIdx.z]; a.W = kl.W; a.kcache = kl.k; a.vcache = kl.v; }
  }
  int bx, by;
  xcd_tile_order(bx, by, xcd_swz, grid_n, grid_m);
  const int strip0 = bx * BNS, m0 = by * BMT * 16;
  const int nfrag = a.K >> 5, nstage = nfrag / FPS;        // host guarantees K % 64 == 0
  // this wave's pieces: piece p = wave + NW * i; p < APC: fragment p % FPS of strip p / FPS, else rows 8 (p - APC) .. + 7 of the row tile
  const char* src[PPW];
  int adv[PPW], pdst[PPW];  // !EVEN: bytes per stage the piece's source advances by, and its LDS slot
#pragma unroll
  for (int i = 0; i < PPW; ++i) {
    int p = wave + NW * i;
    if constexpr (!EVEN) { if (p >= APC + BPC) p -= NW; }
    const bool wpiece = EVEN ? i < APW : p < APC;
    adv[i] = wpiece ? FPS * 1024 : FPS * 64;
    pdst[i] = p * 1024;
    if (wpiece) {
      src[i] = reinterpret_cast<const char*>(a.W) + ((size_t)(strip0 + p / FPS) * nfrag + p % FPS) * 1024 + lane * 16;
    } else {
      const int rl = (p - APC) * RPP + lane / SPR;            // row of the tile; its image slot lane % SPR holds piece slot ^ (row & (SPR - 1))
      const int row = min(m0 + rl, a.M - 1);                  // clamped rows are computed and dropped
      src[i] = reinterpret_cast<const char*>(a.x) + (size_t)row * x_ld * sizeof(WT) + (((lane % SPR) ^ (rl & (SPR - 1))) << 4);  // x_row_mul 1, x_row_off 0 (launcher)
    }
  }
  auto issue = [&](int t, int buf) {
    char* dst = smem_raw + buf * STAGE_B + wave * 1024;
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
      if constexpr (EVEN)
        __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(src[i] + (size_t)t * (i < APW ? FPS * 1024 : FPS * 64)),
                                         (__attribute__((address_space(3))) void*)(dst + NW * i * 1024), 16, 0, 0);
      else
        __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(src[i] + (size_t)t * adv[i]),
                                         (__attribute__((address_space(3))) void*)(smem_raw + buf * STAGE_B + pdst[i]), 16, 0, 0);
    }
  };
  f32x4 acc[NS][MT];
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[s][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
  // per-lane read offsets: weights lane-linear; activations row j of the tile, piece (f * 4 + q) ^ (j & 7)
  const int a_off = wn * NS * FPS * 1024 + lane * 16;
  int b_off[FPS];
#pragma unroll
  for (int f = 0; f < FPS; ++f) b_off[f] = APC * 1024 + (wm * MT * 16 + j) * RB + (((f * 4 + q) ^ (j & (SPR - 1))) << 4);

#pragma unroll
  for (int t = 0; t < NST - 1; ++t)
    if (t < nstage) issue(t, t);
  int buf = 0;
  for (int t = 0; t < nstage; ++t) {
    // stage t has landed for this wave: loads of at most min(NST - 2, nstage - 1 - t) later stages may still be in flight
    const int later = nstage - 1 - t;
    if (later >= NST - 2) ptts_wait_vmcnt<(NST - 2) * PPW>();
    else if (NST > 3 && later == 1) ptts_wait_vmcnt<PPW>();
    else if (NST > 4 && later == 2) ptts_wait_vmcnt<2 * PPW>();
    else ptts_wait_vmcnt<0>();
    // ... and for every wave, and every wave is done reading buffer (t - 1) % NST (its fragments were consumed by MFMAs issued before this point)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (t + NST - 1 < nstage) issue(t + NST - 1, buf == 0 ? NST - 1 : buf - 1);
    const char* cur = smem_raw + buf * STAGE_B;
    if constexpr (RP == 1) {
      // every fragment read of the stage is issued before its first MFMA: one exposed LDS latency per stage instead of one per group of reads
      u32x4_t af[FPS][NS], bf[FPS][MT];
#pragma unroll
      for (int f = 0; f < FPS; ++f) {
#pragma unroll
        for (int s = 0; s < NS; ++s) af[f][s] = *reinterpret_cast<const u32x4_t*>(cur + a_off + (s * FPS + f) * 1024);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) bf[f][mt] = *reinterpret_cast<const u32x4_t*>(cur + b_off[f] + mt * 16 * RB);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int f = 0; f < FPS; ++f)
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) acc[s][mt] = mfma_step_v<WT>(af[f][s], bf[f][mt], acc[s][mt]);
    } else {
#pragma unroll
      for (int f = 0; f < FPS; ++f) {
        u32x4_t af[NS], bf[MT];
#pragma unroll
        for (int s = 0; s < NS; ++s) af[s] = *reinterpret_cast<const u32x4_t*>(cur + a_off + (s * FPS + f) * 1024);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) bf[mt] = *reinterpret_cast<const u32x4_t*>(cur + b_off[f] + mt * 16 * RB);
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) acc[s][mt] = mfma_step_v<WT>(af[s], bf[mt], acc[s][mt]);
      }
    }
    buf = buf + 1 == NST ? 0 : buf + 1;
  }
  if constexpr (EPI == EPI_RESID) {  // residual pieces requested before the first store (loads and stores retire in order on one counter)
    float4 res[NS][MT];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int m = min(m0 + (wm * MT + mt) * 16 + j, a.M - 1);
        res[s][mt] = *reinterpret_cast<const float4*>(a.out + (size_t)m * a.out_ld + (strip0 + wn * NS + s) * 16 + q * 4);
      }
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int m = m0 + (wm * MT + mt) * 16 + j;
        const f32x4 r = acc[s][mt];
        if (m < a.M)
          *reinterpret_cast<float4*>(a.out + (size_t)m * a.out_ld + (strip0 + wn * NS + s) * 16 + q * 4) =
              make_float4(res[s][mt].x + r[0], res[s][mt].y + r[1], res[s][mt].z + r[2], res[s][mt].w + r[3]);
      }
    return;
  }
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int m = m0 + (wm * MT + mt) * 16 + j;
      if (m < a.M) gemm_store_tile<WT, EPI>(a, m, (strip0 + wn * NS + s) * 16 + q * 4, acc[s][mt]);  // D[row = q*4 + r][col = j]
    }
}

template <int EPI, int BNS, int BMT, int WN, int WM, int NST, int RP = 0>
int launch_gemm_glds_inst(const GemmArgs& a, hipStream_t st) {
  constexpr size_t sh = (size_t)NST * (BNS + BMT) * 2 * 1024;  // BK = 64: two 1 KiB fragments per strip / row tile and stage
  static PttsPerDeviceOnce attr_once;
  const int attr_dev = PttsPerDeviceOnce::device();
  if (sh > 64 * 1024 && attr_once.need(attr_dev)) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_glds_kernel<EPI, BNS, BMT, WN, WM, NST, RP>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh);
    if (e != hipSuccess) return ptts_fail(PTTS_E_HIP, "hipFuncSetAttribute(max dynamic LDS) failed: %s", hipGetErrorString(e));
    attr_once.done(attr_dev);
  }
  const dim3 grid(a.N / (16 * BNS), (a.M + BMT * 16 - 1) / (BMT * 16), (EPI == EPI_KV && a.kv_layers) ? a.kv_nlayers : 1);
  GemmGldsHead h;
  PTTS_TRY(GemmGldsHead::pack(a, grid, h));
  ptts_klaunch(gemm_glds_kernel<EPI, BNS, BMT, WN, WM, NST, RP>, grid, dim3(WN * WM * 64), sh, st, h, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ptts_fail(PTTS_E_HIP, "gemm launch failed: %s", hipGetErrorString(e));
  return PTTS_OK;
}

// Tile policy, measured per shape on MI355X (tools/gemm_probe, profiles/r06_gemm_probe.txt; us per launch, fp32 outputs, weights from HBM):
//   narrow projections (N <= 1024: o, cross q / o, wo, fc2): 64 x 64 tiles, 3-stage ring - 272..512 workgroups, two per CU
//       2048 x 1024 x 1024 9.4 (r05 17.6)   2048 x 1024 x 2816 19.7 (41.0)   1056 x 1024 x 1024 8.3 (15.7)   1056 x 1024 x 4096 23.0 (53.0)
//   wide projections with >= 400 tiles of 128 x 128 (T5 wi, Large fc1): 128 x 128, 8 waves, 2-stage ring (64 KiB: two workgroups per CU)
//       2048 x 5632 x 1024 34.4 (73.0)   1056 x 6144 x 1536 28.7 (64.5)
//   the rest (q|k|v, fc1, cross K|V): 128 weight rows x 64 activation rows, 4 waves, 2-stage ring (48 KiB: three workgroups per CU)
//       2048 x 3072 x 1024 19.7 (41.6)   1056 x 3072 x 1024 14.5 (29.0)   1056 x 4096 x 1024 18.8 (34.5)   2048 x 2048 x 1024 15.2 (30.1)
// Deeper rings lose above one stage in flight wherever they cost a resident workgroup: every variant is bound by what ONE workgroup's
// dependent chain (barrier -> fragment reads -> MFMAs per stage) and its LDS-DMA issue rate sustain, so resident workgroups per CU beat
// pipeline depth; BK = 128 stages (half the barriers) lose for the same reason (twice the LDS per stage). -1 = shape not served.
// Round 6, calls 32-34 (profiles/r06_gemm_probe_call32.txt, _call34.txt): where tiles of ~1 / 256 of the output (or whole rounds of them) exist, fewer and
// larger workgroups beat two or three smaller resident ones - fewer L2 -> LDS bytes per flop: 2048 | 4096 | 8192 x 3072 x 1024 on 192 x 128 tiles (2-stage
// ring: two workgroups per CU) 19.2 | 31.3 | 61.0 us against 21.4 | 34.8 | 65.5, x 5632 on 176 x 256 tiles (one workgroup per CU; 22 + 32 pieces per stage
// on 8 waves: the uneven split) 29.5 | 60.9 | 111.2 against 34.8 | 62.5 | 118.9 (the vendor library at 2048 rows, graph-captured torch.matmul: 16.9 / 32.6,
// profiles/r06_vendor_gemm.txt). Only where the tile count fills whole rounds (>= 85 %): 1056 x 3072 on 192 x 128 tiles (144 of them) loses, 17.0 against 14.2.
// Deeper rings and a half-stage software pipeline lose on every shape (measured with probe builds; the code is in git history).
static inline bool glds_fills_rounds(int tiles, int slots) {
  const int rounds = (tiles + slots - 1) / slots;
  return tiles > 224 && (tiles <= 256 || tiles * 100 >= rounds * slots * 85);
}
template <int EPI>
int launch_gemm_glds(const GemmArgs& a, hipStream_t st) {
  if (a.K % 64 || a.N % 64 || a.x_ld % 8 || a.x_row_mul != 1 || a.x_row_off != 0) return -1;
  if constexpr (EPI == EPI_STORE) {
    if (a.N % 192 == 0 && glds_fills_rounds((a.N / 192) * ((a.M + 127) / 128), 512)) return launch_gemm_glds_inst<EPI, 12, 8, 4, 2, 2, 1>(a, st);
  }
  if constexpr (EPI == EPI_GATE_WT) {
    if (a.N % 176 == 0 && glds_fills_rounds((a.N / 176) * ((a.M + 255) / 256), 256)) return launch_gemm_glds_inst<EPI, 11, 16, 1, 8, 2, 1>(a, st);
  }
  if (a.N <= 1024 || a.N % 128) return launch_gemm_glds_inst<EPI, 4, 4, 2, 2, 3>(a, st);
  // (the description's K / V of every layer in ONE launch is kv_nlayers problems' worth of tiles: it fills the chip for many rounds like a large GEMM)
  const int tiles128 = (a.N / 128) * ((a.M + 127) / 128) * ((EPI == EPI_KV && a.kv_layers) ? a.kv_nlayers : 1);
  if (tiles128 >= 400) return launch_gemm_glds_inst<EPI, 8, 8, 4, 2, 2, 1>(a, st);
  return launch_gemm_glds_inst<EPI, 8, 4, 2, 2, 2, 1>(a, st);
}

}  // namespace
