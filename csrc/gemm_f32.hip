// Exact-fp32 MFMA GEMM for gfx950 (MI355X): C[M,N] = A * B (+ epilogue), fp32 operands, fp32 output.
//
// * Every product and sum goes through v_mfma_f32_16x16x4_f32 accumulators: the result of one K range is a k-ordered
//   fmaf chain starting from +0.  Nothing is rounded to bf16 and no product is split into bf16 terms.
// * 256-thread workgroups (4 wave64s as 2 x 2); each wave owns a (BM/2) x (BN/2) sub-tile of 16 x 16 accumulators:
//   4 independent ones for the 64 x 64 tile, 16 for the 128 x 128 tile (>= 2 cover the instruction's 40-cycle
//   dependent latency at its 32-cycle issue interval).
// * Layouts, as in gemm.hip: mode bit 1 = A stored [K][M] (else [M][K]), bit 2 = B stored [K][N] (else [N][K]).
// * K-tiles of 32 (64 x 64) / 16 (128 x 128: the same 36 KiB of LDS), register-staged float4 global loads into
//   double-buffered LDS, one barrier per K-tile.  Partial tiles are zero-filled while staging (a zero operand pair
//   leaves an fmaf chain unchanged) and guarded in the epilogue; nothing is read or written outside M x N x K.
// * LDS pitches.  A fragment read is one float per lane (ds_read_b32: 32 banks, the two 32-lane halves are served
//   separately): lane l reads row l & 15 at k = kb + (l >> 4), so one half reads 16 rows x 2 consecutive k.
//     k-contiguous image [row][BK + 2]: bank = (row * (BK + 2) + k) mod 32.  BK + 2 = 34 = 2 (mod 32) gives
//       2 row + k: 32 distinct banks; BK + 2 = 18 gives 18 row mod 32 = the 16 even banks, each once, + k.
//       (A pitch of 36 would put rows r and r + 8 on one bank: 36 * 8 = 0 mod 32.)  Rows are 8-byte aligned, so a
//       staged float4 is written as two 8-byte stores.
//     k-major image [k][rows + 16]: bank = (k * (rows + 16) + row) mod 32; rows + 16 = 16 (mod 32) for 64 and 128
//       rows: row + 16 (k & 1), 32 distinct banks.  Rows are 16-byte aligned: one 16-byte store per float4.
// * Deterministic split-K: split s reduces the K range [s * kps, (s + 1) * kps), kps a multiple of the K-tile, and
//   stores its partial tile (zeros for an empty range) into ws[s][M][N]; a second kernel on the same stream sums
//   the partials in split order and applies the epilogue.  No atomics, tickets or fences: the kernel boundary orders.
// * Epilogues, evaluated in the written order: EPI_F32_STORE C = acc (+ bias[n]); EPI_F32_RESID
//   C = (acc (+ bias[n])) + resid[m][n]; EPI_F32_ACC C = C + acc.  Two activation epilogues work with an auxiliary
//   fp32 matrix aux[M][ldx]: EPI_GELU pre = acc (+ bias[n]), aux = pre, C = gelu_new(pre) (the MLP's W_in forward,
//   the pre-activation stored in the same pass); EPI_DGELU C = acc * gelu_new'(aux) (dpre out of dY W_out^T; no bias).
//   gelu_new_f / gelu_new_grad_f of common.h (the sigmoid form).
// * Workgroup order: the bijective XCD remap of gemm.hip, so the tiles one XCD works on are consecutive (they share
//   A row panels in that XCD's L2).  It changes which workgroup computes a tile, never what it computes.
#include "gemm_f32_body.h"  // F32Tile, the XCD remap, the split-order sum

namespace {

// the Epi values of gemm.hip
enum : int { F32_EPI_RESID = 2, F32_EPI_GELU = 3, F32_EPI_DGELU = 4, F32_EPI_ACC = 5, F32_EPI_STORE = 7 };

struct F32Args {
  const float* A;
  const float* B;
  float* C;
  const float* bias;
  const float* resid;
  float* ws;
  float* aux;
  long lda, ldb, ldc, ldr, ldx;
  int M, N, K;
  int k_per_split;
  int splits;
  int epi;
};

__device__ __forceinline__ void epilogue_f32(const F32Args& p, int row, int col, float v) {
  float* dst = p.C + (long)row * p.ldc + col;
  if (p.epi == F32_EPI_ACC) {
    *dst = *dst + v;
    return;
  }
  if (p.epi == F32_EPI_DGELU) {
    *dst = v * gelu_new_grad_f(p.aux[(long)row * p.ldx + col]);
    return;
  }
  if (p.bias) v = v + p.bias[col];
  if (p.epi == F32_EPI_RESID) v = v + p.resid[(long)row * p.ldr + col];
  if (p.epi == F32_EPI_GELU) {
    p.aux[(long)row * p.ldx + col] = v;
    v = gelu_new_f(v);
  }
  *dst = v;
}

template <int BM, int BN, int BK, bool AKM, bool BKM>
__global__ __launch_bounds__(256) void gemm_f32_kernel(F32Args p) {
  constexpr int WM = BM / 2, WN = BN / 2;
  constexpr int TM = WM / 16, TN = WN / 16;
  using LA = F32Tile<AKM, BM, BK>;
  using LB = F32Tile<BKM, BN, BK>;
  constexpr int STAGE = LA::ELEMS + LB::ELEMS;
  __shared__ __attribute__((aligned(16))) float smem[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int tiles_n = (p.N + BN - 1) / BN, tiles_m = (p.M + BM - 1) / BM;
  const int t = xcd_remap_f32(blockIdx.x, tiles_n * tiles_m);
  const int m0 = (t / tiles_n) * BM, n0 = (t % tiles_n) * BN;
  const int split = blockIdx.y;
  const int kbeg = min(p.K, split * p.k_per_split);
  const int kend = min(p.K, kbeg + p.k_per_split);
  const int ntiles = (kend - kbeg + BK - 1) / BK;  // 0 for an empty trailing split: the partial tile is zeros

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  LA la;
  LB lb;
#define SA(buf) (smem + (buf) * STAGE)
#define SB(buf) (smem + (buf) * STAGE + LA::ELEMS)
  if (ntiles > 0) {
    la.load(p.A, p.lda, m0, p.M, kbeg, kend, tid);
    lb.load(p.B, p.ldb, n0, p.N, kbeg, kend, tid);
    la.store(SA(0), tid);
    lb.store(SB(0), tid);
  }
  __syncthreads();
  int cur = 0;
  for (int kt = 0; kt < ntiles; ++kt) {
    const bool more = kt + 1 < ntiles;
    if (more) {
      la.load(p.A, p.lda, m0, p.M, kbeg + (kt + 1) * BK, kend, tid);
      lb.load(p.B, p.ldb, n0, p.N, kbeg + (kt + 1) * BK, kend, tid);
    }
#pragma unroll
    for (int kb = 0; kb < BK; kb += 4) {
      float a[TM], b[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) a[i] = LA::frag(SA(cur), wm * WM + i * 16, kb, lane);
#pragma unroll
      for (int j = 0; j < TN; ++j) b[j] = LB::frag(SB(cur), wn * WN + j * 16, kb, lane);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    if (more) {
      la.store(SA(cur ^ 1), tid);
      lb.store(SB(cur ^ 1), tid);
    }
    __syncthreads();
    cur ^= 1;
  }
#undef SA
#undef SB

  // C/D map of the 16 x 16 forms: column = lane & 15, row = 4 (lane >> 4) + register
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col = n0 + wn * WN + j * 16 + (lane & 15);
      if (col >= p.N) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wm * WM + i * 16 + 4 * (lane >> 4) + r;
        if (row >= p.M) continue;
        if (p.splits > 1) p.ws[((long)split * p.M + row) * p.N + col] = acc[i][j][r];
        else epilogue_f32(p, row, col, acc[i][j][r]);
      }
    }
  }
}

// sums the partial tiles ws[s][M][N] in split order, then the epilogue; one element per thread
__global__ __launch_bounds__(256) void gemm_f32_reduce_kernel(F32Args p) {
  const long total = (long)p.M * p.N;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  epilogue_f32(p, (int)(idx / p.N), (int)(idx % p.N), f32_split_sum(p.ws, p.splits, total, idx));
}

template <int BM, int BN, int BK>
hipError_t launch_mode(const F32Args& a, int mode, hipStream_t s) {
  dim3 grid(cdiv(a.M, BM) * cdiv(a.N, BN), a.splits);
  switch (mode) {
    case 0: hipLaunchKernelGGL((gemm_f32_kernel<BM, BN, BK, false, false>), grid, dim3(256), 0, s, a); break;
    case 1: hipLaunchKernelGGL((gemm_f32_kernel<BM, BN, BK, true, false>), grid, dim3(256), 0, s, a); break;
    case 2: hipLaunchKernelGGL((gemm_f32_kernel<BM, BN, BK, false, true>), grid, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL((gemm_f32_kernel<BM, BN, BK, true, true>), grid, dim3(256), 0, s, a); break;
  }
  return hipGetLastError();
}

}  // namespace

// tile ids: 0 = 64 x 64 (K-tile 32), 1 = 128 x 128 (K-tile 16).
// 1 when the kernel covers the problem: fp32 operands whose base pointers are 16-byte aligned (A, B, C, the
// residual, the auxiliary matrix and the split workspace; the bias is read one float at a time and needs 4) and
// whose leading dimensions are multiples of 4 elements and cover their rows.  ``aux`` [M][ldx] is required by
// EPI_GELU (written) and EPI_DGELU (read) and ignored by the other epilogues.
IIT_EXPORT int iit_gemm_f32_aux_ok(const void* A, const void* B, const void* C, const void* bias, const void* resid,
                                   const void* aux, const void* ws, long lda, long ldb, long ldc, long ldr, long ldx,
                                   int M, int N, int K, int mode, int epi, int tile, int splits) {
  if (!A || !B || !C || M < 1 || N < 1 || K < 1) return 0;
  if (mode < 0 || mode > 3 || tile < 0 || tile > 1 || splits < 1 || splits > 64) return 0;
  if (epi != F32_EPI_STORE && epi != F32_EPI_RESID && epi != F32_EPI_ACC && epi != F32_EPI_GELU &&
      epi != F32_EPI_DGELU)
    return 0;
  if (!aligned16(A) || !aligned16(B) || !aligned16(C) || ((uintptr_t)bias & 3)) return 0;
  if ((lda & 3) || (ldb & 3) || (ldc & 3)) return 0;
  if (lda < ((mode & 1) ? M : K) || ldb < ((mode & 2) ? N : K) || ldc < N) return 0;
  if (epi == F32_EPI_RESID && (!resid || !aligned16(resid) || (ldr & 3) || ldr < N)) return 0;
  if ((epi == F32_EPI_ACC || epi == F32_EPI_DGELU) && bias) return 0;
  if ((epi == F32_EPI_GELU || epi == F32_EPI_DGELU) && (!aux || !aligned16(aux) || (ldx & 3) || ldx < N)) return 0;
  if (splits > 1 && (!ws || !aligned16(ws))) return 0;
  return 1;
}

// launches on ``stream``; no host synchronisation, no allocation.  ``ws``: splits * M * N floats when splits > 1.
IIT_EXPORT int iit_gemm_f32_aux(const void* A, const void* B, void* C, const float* bias, const float* resid,
                                void* aux, void* ws, long lda, long ldb, long ldc, long ldr, long ldx, int M, int N,
                                int K, int mode, int epi, int tile, int splits, void* stream) {
  if (!iit_gemm_f32_aux_ok(A, B, C, bias, resid, aux, ws, lda, ldb, ldc, ldr, ldx, M, N, K, mode, epi, tile, splits))
    return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  F32Args a;
  a.A = (const float*)A; a.B = (const float*)B; a.C = (float*)C;
  a.bias = bias; a.resid = resid; a.ws = (float*)ws; a.aux = (float*)aux;
  a.lda = lda; a.ldb = ldb; a.ldc = ldc; a.ldr = ldr; a.ldx = ldx;
  a.M = M; a.N = N; a.K = K;
  a.splits = splits; a.epi = epi;
  const int bk = tile == 1 ? 16 : 32;
  a.k_per_split = cdiv(cdiv(K, splits), bk) * bk;
  hipError_t rc = tile == 1 ? launch_mode<128, 128, 16>(a, mode, s) : launch_mode<64, 64, 32>(a, mode, s);
  if (rc != hipSuccess || splits == 1) return (int)rc;
  hipLaunchKernelGGL(gemm_f32_reduce_kernel, dim3(cdiv((long)M * N, 256)), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}

// the three epilogues without an auxiliary matrix: the exports above with ``aux`` = null
IIT_EXPORT int iit_gemm_f32_ok(const void* A, const void* B, const void* C, const void* bias, const void* resid,
                               const void* ws, long lda, long ldb, long ldc, long ldr, int M, int N, int K, int mode,
                               int epi, int tile, int splits) {
  if (epi != F32_EPI_STORE && epi != F32_EPI_RESID && epi != F32_EPI_ACC) return 0;
  return iit_gemm_f32_aux_ok(A, B, C, bias, resid, nullptr, ws, lda, ldb, ldc, ldr, 0, M, N, K, mode, epi, tile,
                             splits);
}

IIT_EXPORT int iit_gemm_f32(const void* A, const void* B, void* C, const float* bias, const float* resid, void* ws,
                            long lda, long ldb, long ldc, long ldr, int M, int N, int K, int mode, int epi, int tile,
                            int splits, void* stream) {
  if (epi != F32_EPI_STORE && epi != F32_EPI_RESID && epi != F32_EPI_ACC) return (int)hipErrorInvalidValue;
  return iit_gemm_f32_aux(A, B, C, bias, resid, nullptr, ws, lda, ldb, ldc, ldr, 0, M, N, K, mode, epi, tile, splits,
                          stream);
}
