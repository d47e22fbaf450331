// LDS-DMA (global_load_lds) MFMA GEMM for gfx950: the engine's mid-size GEMMs (M, N, K multiples of the tile).
//
// C[M,N] = A[M,K] * B[K,N] for the three operand layouts the transformer uses:
//   mode 0  A [M][K], B [N][K]          dX = dY W^T
//   mode 2  A [M][K], B [K][N]          forward, TL-layout weights (bf16 arena mirror)
//   mode 3  A [K][M], B [K][N]          weight gradients X^T dY (reduction over tokens)
// with the epilogue fused (bias / packed-QKV bias / fp32 residual add / bias+gelu_new with the pre-activation /
// fp32 accumulate into the gradient arena / fp32 store).
//
// Structure (cdna_hip_programming.md §5, "step-3" + T1/T2/T10):
// * 256 threads = 4 wave64 as 2x2; tile BM x BN x 64; each wave a (BM/2) x (BN/2) block of 16x16 fp32
//   accumulators fed by v_mfma_f32_16x16x32_bf16.
// * Operands are staged global -> LDS with 16-byte global_load_lds (no VGPR round trip, no ds_write pass) into
//   an NS-deep ring of LDS buffers: NS-1 K-tiles are in flight while the MFMAs consume one; each K-step waits
//   with a counted s_waitcnt vmcnt (never 0 in steady state) and one raw s_barrier, so the DMA spans barriers
//   (a __syncthreads() would drain it: "Pipelining across barriers").
// * LDS images are lane-linear per wave (what LDS-DMA requires) and XOR-swizzled through the *source* address:
//     k-contiguous [rows][64]:   16-B chunk c of row r lives at slot c ^ ((r >> 1) & 7)  -> ds_read_b128 fragment
//                                 reads of 16 rows hit 16 distinct bank groups (conflict-free);
//     k-major [64][cols]:         32-B block b of k-row r lives at b ^ f(r)  -> the 16 k-rows one
//                                 ds_read_b64_tr_b16 instruction touches spread over all 64 banks (2 passes, the minimum).
// * k-major operands (X^T dY, [K][N] weights) are transposed by the gfx950 LDS transpose read, so no operand is
//   ever re-laid-out in memory.
// * Bijective XCD-aware tile remap: the tiles of one XCD share A row panels in its L2.
// * Split-K (fp32 accumulate epilogue only): blockIdx.y takes a K range and adds its partial tile with fp32
//   atomics -- for the weight gradients, whose [d][N] outputs are too few tiles to fill 256 CUs.
// * Epilogue: accumulators -> LDS (fp32 tile) -> each thread owns 8 consecutive columns of a row: 16-B / 32-B
//   vector loads of bias / residual / accumulator and vector stores (the MFMA C layout would otherwise give
//   2-byte column-strided stores).
// * E_DGELU (mode 0, the MLP backward dpre = (dY W_out^T) * gelu_new'(pre)): reads the saved pre-activation in the
//   epilogue and, with ``csum``, also reduces the stored dpre tile over its rows in LDS into the b_in gradient
//   (one atomic per column per tile) -- the separate dgelu pass and the bias column-sum pass disappear.
#include "gemm_glds_body.h"
#include "gemm_tiles.h"

namespace {

template <int BM, int BN, int NS, bool AKM, bool BKM, int EPI, int NW, int BK = 64, int OCC = 1>
__global__ __launch_bounds__(NW * 64, OCC) void gemm_glds_kernel(G2Args p) {
  __shared__ __attribute__((aligned(16))) char smem[GldsSmem<BM, BN, NS, NW, BK, OCC>::BYTES];  // ONE LDS object
  gemm_glds_body<BM, BN, NS, AKM, BKM, EPI, NW, BK, OCC>(p, blockIdx.x, gridDim.x, blockIdx.y, gridDim.y, smem);
}

template <int BM, int BN, int NS, bool AKM, bool BKM, int EPI, int NW = 4, int BK = 64, int OCC = 1>
hipError_t launch(const G2Args& a, hipStream_t s) {
  const int tiles = (a.M / BM) * (a.N / BN);
  hipLaunchKernelGGL((gemm_glds_kernel<BM, BN, NS, AKM, BKM, EPI, NW, BK, OCC>), dim3(tiles, a.K / a.k_per_split),
                     dim3(NW * 64), 0, s, a);
  return hipGetLastError();
}

// one launch per row of IIT_GLDS_TILE_LIST (csrc/gemm_tiles.h)
template <bool AKM, bool BKM, int EPI>
hipError_t launch_tile(const G2Args& a, int tile, hipStream_t s) {
  switch (tile) {
#define X(ID, BM, BN, NS, NW, BK, OCC) \
  case ID: return launch<BM, BN, NS, AKM, BKM, EPI, NW, BK, OCC>(a, s);
    IIT_GLDS_TILE_LIST(X)
#undef X
    default: return hipErrorInvalidValue;  // unreachable: iit_gemm_glds_ok runs first
  }
}

// the (layout, epilogue) combinations instantiated for every tile: X(mode, A k-major, B k-major, epilogue)
#define IIT_GLDS_COMBO_LIST(X)                                                                                   \
  X(0, false, false, E_BF16) X(0, false, false, E_F32_ACC) X(0, false, false, E_F32_STORE)                       \
  X(0, false, false, E_DGELU) X(0, false, false, E_DGELU_ERF)                                                    \
  X(2, false, true, E_BF16) X(2, false, true, E_BF16_BIAS3) X(2, false, true, E_F32_RESID)                       \
  X(2, false, true, E_GELU) X(2, false, true, E_GELU_ERF) X(2, false, true, E_F32_ACC)                          \
  X(2, false, true, E_F32_STORE)                                                                                 \
  X(3, true, true, E_F32_ACC) X(3, true, true, E_F32_STORE)

constexpr bool combo_ok(int mode, int epi) {
#define X(MODE, AKM, BKM, EPI) \
  if (mode == (MODE) && epi == (EPI)) return true;
  IIT_GLDS_COMBO_LIST(X)
#undef X
  return false;
}

}  // namespace

// 1 when (shape, layout, epilogue, tile) is covered by the LDS-DMA kernel (caller falls back otherwise); tiles 40-42
// (gemm_tiles.h: the 256 x 256 kernels of gemm_8ph.hip / gemm_4w.hip) take no K split
#define IIT_8PH_TILE 40
#define IIT_4W_TILE 41
#define IIT_4W32_TILE 42
extern "C" int iit_gemm_8ph_ok(int M, int N, int K, int mode, int epi);
extern "C" int iit_gemm_8ph_run(const void* args, int mode, int epi, void* stream);
extern "C" int iit_gemm_4w_run(const void* args, int mode, int epi, int bk, void* stream);

IIT_EXPORT int iit_gemm_glds_ok(const void* A, const void* B, const void* C, const void* C2, const void* resid,
                                long lda, long ldb, long ldc, long ldc2, long ldr, int M, int N, int K, int mode,
                                int epi, int bias_cols, int tile, int splits, int reduce) {
  if (tile == IIT_8PH_TILE || tile == IIT_4W_TILE || tile == IIT_4W32_TILE) {  // 256 x 256 tiles, K % 64 == 0
    if (splits != 1 || reduce || !iit_gemm_8ph_ok(M, N, K, mode, epi)) return 0;
    if ((epi == E_DGELU || epi == E_DGELU_ERF) && !C2) return 0;
    if (lda % 8 || ldb % 8 || ldc % 8 || (C2 && ldc2 % 8) || (resid && ldr % 8)) return 0;
    if (((uintptr_t)A | (uintptr_t)B | (uintptr_t)C | (uintptr_t)C2 | (uintptr_t)resid) & 15) return 0;
    if (epi == E_BF16_BIAS3 && bias_cols % 8) return 0;
    return 1;
  }
  const TileRow* t = find_tile(kGldsRows, tile);
  if (!t) return 0;
  // tile 20 (192 x 192, 6 x 6 accumulators per wave) is offered for the weight gradients only: with a k-contiguous A
  // (modes 0 / 2) its kernels need more than 256 VGPRs, and hipcc parks the destinations of the asm-issued
  // ds_read_b128 fragment reads in AGPRs (v_accvgpr_write right after the issue, before the data has landed) and
  // reuses the registers -- one 16-row fragment per wave row came out wrong (tests/test_gemm_exact.py).  The mode-3
  // kernels hold no such copy and are exact.
  if (tile == 20 && mode != 3) return 0;
  // atomic split-K: fp32 accumulate only; reduction split-K (``reduce``): fp32 accumulate, store or residual add (the
  // last-arriving split runs the epilogue once on the summed tile)
  const bool split_epi = epi == E_F32_ACC || (reduce && (epi == E_F32_STORE || epi == E_F32_RESID));
  const int bk = t->bk;
  if (splits < 1 || (splits > 1 && (!split_epi || K % (bk * splits)))) return 0;
  if (reduce && splits < 2) return 0;
  if (!combo_ok(mode, epi)) return 0;
  const bool dg = epi == E_DGELU || epi == E_DGELU_ERF;
  if (dg && (mode != 0 || !C2)) return 0;
  if (M <= 0 || N <= 0 || K <= 0 || M % t->bm || N % t->bn || K % bk) return 0;
  if (lda % 8 || ldb % 8 || ldc % 8 || (C2 && ldc2 % 8) || (resid && ldr % 8)) return 0;
  const uintptr_t al = (uintptr_t)A | (uintptr_t)B | (uintptr_t)C | (uintptr_t)C2 | (uintptr_t)resid;
  if (al & 15) return 0;
  if (epi == E_BF16_BIAS3 && bias_cols % 8) return 0;
  return 1;
}

// the timeline probe of the NEXT iit_gemm_glds* launch from this host thread (scripts/gemm_timeline.py): a
// [workgroups][64] int64 device buffer, consumed by that launch
static thread_local long long* g_prof_buf = nullptr;
IIT_EXPORT void iit_gemm_glds_set_prof(void* buf) { g_prof_buf = (long long*)buf; }
// M-tiles per group of the XCD-local tile order for every later launch (0 = the default; the group experiment)
static int g_group_m = 0;
IIT_EXPORT void iit_gemm_glds_set_group_m(int gm) { g_group_m = gm; }

// the launch, with the epilogue store flavour (G2Args::store_mode) and, for the weight gradients (mode 3), the fused
// column sums of B (``bsum``, += atomically; nullable); ``gsq`` (fp32 store epilogue, nullable): += the sum of squares
// of the stored values, spread over 64 slots
IIT_EXPORT int iit_gemm_glds_sm(const void* A, const void* B, void* C, void* C2, const float* bias0,
                                const float* bias1, const float* bias2, const float* resid, long lda, long ldb, long ldc,
                                long ldc2, long ldr, int M, int N, int K, int mode, int epi, int bias_cols, int tile,
                                int splits, float* csum, float* ws, int* counters, int store_mode, float* bsum,
                                float* gsq, void* stream) {
  const int reduce = ws != nullptr;
  if (!iit_gemm_glds_ok(A, B, C, C2, resid, lda, ldb, ldc, ldc2, ldr, M, N, K, mode, epi, bias_cols, tile, splits,
                        reduce))
    return (int)hipErrorInvalidValue;
  if (reduce && !counters) return (int)hipErrorInvalidValue;
  G2Args a{};
  a.A = (const __bf16*)A; a.B = (const __bf16*)B; a.C = C; a.C2 = C2;
  a.bias0 = bias0; a.bias1 = bias1; a.bias2 = bias2; a.resid = resid;
  a.lda = lda; a.ldb = ldb; a.ldc = ldc; a.ldc2 = ldc2; a.ldr = ldr;
  a.M = M; a.N = N; a.K = K; a.bias_cols = bias_cols; a.k_per_split = K / splits;
  a.csum = (epi == E_DGELU || epi == E_DGELU_ERF) ? csum : nullptr;
  a.ws = reduce ? ws : nullptr;  // workspace >= splits * M * N floats, counters >= tiles ints (zero when idle)
  a.counters = reduce ? counters : nullptr;
  a.store_mode = store_mode;
  a.prof = g_prof_buf;
  g_prof_buf = nullptr;
  a.group_m = g_group_m;
  a.bsum = mode == 3 ? bsum : nullptr;
  a.gsq = epi == E_F32_STORE ? gsq : nullptr;
  hipStream_t s = (hipStream_t)stream;
  if (tile == IIT_8PH_TILE) return iit_gemm_8ph_run(&a, mode, epi, stream);
  if (tile == IIT_4W_TILE) return iit_gemm_4w_run(&a, mode, epi, 64, stream);
  if (tile == IIT_4W32_TILE) return iit_gemm_4w_run(&a, mode, epi, 32, stream);
#define X(MODE, AKM, BKM, EPI) \
  if (mode == (MODE) && epi == (EPI)) return (int)launch_tile<AKM, BKM, EPI>(a, tile, s);
  IIT_GLDS_COMBO_LIST(X)
#undef X
  return (int)hipErrorInvalidValue;
}

// The tile table of ``family`` (0 glds, 40-42 included; 1 edge; 2 dual dW; 3 dual dX; 4 conv; 5 conv weight
// gradient) from the lists of gemm_tiles.h: fills up to ``cap`` rows of 8 ints (TileRow) and returns the row count
// (0: no such family).  Host only; what iit_amd/ops/hip_kernels.py checks its tables against.
IIT_EXPORT int iit_tile_table(int family, TileRow* out, int cap) {
  const TileRow* rows = nullptr;
  int n = 0;
#define FAMILY(F, ROWS) \
  if (family == (F)) rows = ROWS, n = (int)(sizeof(ROWS) / sizeof(TileRow));
  FAMILY(0, kGldsRows)
  FAMILY(1, kEdgeRows)
  FAMILY(2, kDualWRows)
  FAMILY(3, kDualXRows)
  FAMILY(4, kConvRows)
  FAMILY(5, kConvWgRows)
#undef FAMILY
  for (int i = 0; i < n && i < cap; ++i) out[i] = rows[i];
  return n;
}
