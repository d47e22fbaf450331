// The LDS-DMA MFMA GEMM (csrc/gemm_glds.hip, csrc/gemm_glds_body.h) for a ragged N: problems whose B is k-major
// ([K][N]: the forward from TL-layout weights, mode 2, and the weight gradients X^T dY, mode 3) and whose N is not a
// multiple of the tile -- the vocabulary-sized unembed GEMMs (N = 50257) -- in ONE launch, instead of a tile-aligned
// bulk plus a narrow tail on the older register-staged kernel.
//
// The edge is a compile-time variant of the shared body (EDGE = true), instantiated here only; the instantiations of
// gemm_glds.hip / gemm_dual.hip that carry the layer GEMMs are untouched.  What changes in the last N-tile:
//   * B granules (8 columns, 16 B) that start at or beyond column N are read from a 16-B zero page instead of the
//     operand (the same redirect the convolution's taps use), so nothing is read past an operand row's pad8(N)
//     columns -- in particular nothing past the last row; the granule that straddles N brings in the row's pad
//     columns [N, pad8(N)), whose contents (anything, NaN included) reach only output columns >= N;
//   * output columns >= N are never stored, and never enter ``bsum`` (column sums of B) or ``gsq`` (sum of squares
//     of the stored values); ``bias0`` is not read at or beyond N.
// M and K stay multiples of the tile; one K split.  iit_gemm_edge_plan exposes the edge arithmetic to the host.
#include "gemm_glds_body.h"
#include "gemm_tiles.h"

namespace {

__device__ __attribute__((aligned(16))) unsigned int g_edge_zero[4];  // the zero page (zero-initialised)

// k-major B [K][N] staged as OperandStager<true, R, NW, BK> does, except that a DMA whose 8-column granule starts at
// or beyond column N (edge_redirect) reads the zero page.  ``oob`` holds one bit per DMA instruction of this lane.
template <int R, int NW, int BK>
struct EdgeBStager {
  using Base = OperandStager<true, R, NW, BK, false>;
  static constexpr int NP = Base::NP, PR = Base::PR;
  static constexpr int SN = Stager<true, PR, NW, BK, false>::N;  // DMA instructions per panel
  static constexpr int N = Base::N;
  static_assert(NP * SN <= 32, "one bit per DMA instruction");
  Base st;
  unsigned oob;

  __device__ __forceinline__ void init(const G2Args& p, int n0, int kbeg, int wave, int lane) {
    st.init(p.B, p.ldb, n0, kbeg, wave, lane);
    // the granule column of every DMA, as Stager<true, ...>::init lays it out
    constexpr int CH = PR / 8, KRI = 64 / CH;
    oob = 0;
#pragma unroll
    for (int q = 0; q < NP; ++q)
#pragma unroll
      for (int i = 0; i < SN; ++i) {
        const int kr = (i * NW + wave) * KRI + lane / CH;
        const int ch = lane % CH;
        const int col = (((ch >> 1) ^ kmaj_swz<PR>(kr)) << 4) + ((ch & 1) << 3);
        if (edge_redirect(n0 + q * PR + col, p.N)) oob |= 1u << (q * SN + i);
      }
  }

  __device__ __forceinline__ void stage(int kt, char* img) const {
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      const long k = kt * st.st[q].kstep;
#pragma unroll
      for (int i = 0; i < SN; ++i) {
        const __bf16* src = (oob >> (q * SN + i)) & 1 ? (const __bf16*)g_edge_zero : st.st[q].ptr[i] + k;
        glds16(src, img + q * PR * BK * 2 + st.st[q].off[i]);
      }
    }
  }
};

template <int BM, int BN, int NS, bool AKM, int EPI, int NW, int OCC>
__global__ __launch_bounds__(NW * 64, OCC) void gemm_glds_edge_kernel(G2Args p) {
  __shared__ __attribute__((aligned(16))) char smem[GldsSmem<BM, BN, NS, NW, 64, OCC>::BYTES];
  gemm_glds_body<BM, BN, NS, AKM, true, EPI, NW, 64, OCC, false, void, EdgeBStager<BN, NW, 64>, true>(
      p, blockIdx.x, gridDim.x, 0, 1, smem);
}

template <int BM, int BN, int NS, bool AKM, int EPI, int NW = 4, int OCC = 1>
hipError_t launch(const G2Args& a, hipStream_t s) {
  const int tiles = (a.M / BM) * ((a.N + BN - 1) / BN);
  hipLaunchKernelGGL((gemm_glds_edge_kernel<BM, BN, NS, AKM, EPI, NW, OCC>), dim3(tiles), dim3(NW * 64), 0, s, a);
  return hipGetLastError();
}

// one launch per row of IIT_EDGE_TILE_LIST (csrc/gemm_tiles.h): the edge-capable tiles, under the tile ids (and with
// the ring depths / occupancy, asserted there) they have in gemm_glds.hip
template <bool AKM, int EPI>
hipError_t launch_tile(const G2Args& a, int tile, hipStream_t s) {
  switch (tile) {
#define X(ID, BM, BN, NS, NW, OCC) \
  case ID: return launch<BM, BN, NS, AKM, EPI, NW, OCC>(a, s);
    IIT_EDGE_TILE_LIST(X)
#undef X
    default: return hipErrorInvalidValue;
  }
}

// the (layout, epilogue) combinations instantiated for every tile: X(mode, A k-major, epilogue)
#define IIT_EDGE_COMBO_LIST(X) \
  X(2, false, E_BF16) X(2, false, E_F32_STORE) X(2, false, E_F32_ACC) X(3, true, E_F32_ACC) X(3, true, E_F32_STORE)

constexpr bool combo_ok(int mode, int epi) {
#define X(MODE, AKM, EPI) \
  if (mode == (MODE) && epi == (EPI)) return true;
  IIT_EDGE_COMBO_LIST(X)
#undef X
  return false;
}

inline long pad8l(long n) { return (n + 7) / 8 * 8; }

}  // namespace

// The N edge of a k-major operand / an output of ``rows`` rows, N columns and row stride ``ld`` (elements of
// ``elem`` bytes) under edge tile ``tile``, by walking every 8-column granule of every row of the launch's N-tiles
// with the predicates the kernels use (pure host arithmetic).  out6 = {N-tiles, granules per row read from (or
// stored to) the operand, granules per row redirected to the zero page (or skipped), columns of the straddling
// granule that are valid (0: none straddles), one past the last byte touched, one past the operand's last valid
// byte ((rows - 1) * ld + pad8(N) elements)}.
IIT_EXPORT int iit_gemm_edge_plan(int rows, int N, long ld, int elem, int tile, long* out6) {
  const TileRow* t = find_tile(kEdgeRows, tile);
  if (!t || rows <= 0 || N <= 0 || ld < pad8l(N) || (elem != 2 && elem != 4)) return (int)hipErrorInvalidValue;
  const int tiles_n = (N + t->bn - 1) / t->bn;
  long used = 0, redirected = 0, straddle = 0, last = 0;
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < tiles_n * t->bn; c += 8) {
      if (edge_redirect(c, N)) {
        redirected += r == 0;
        continue;
      }
      used += r == 0;
      const int nv = edge_valid(c, N);
      if (nv < 8) straddle = nv;
      const long end = ((long)r * ld + c + 8) * elem;  // a read takes the whole granule, pad columns included
      if (end > last) last = end;
    }
  out6[0] = tiles_n; out6[1] = used; out6[2] = redirected; out6[3] = straddle; out6[4] = last;
  out6[5] = ((long)(rows - 1) * ld + pad8l(N)) * elem;
  return 0;
}

// 1 when (shape, layout, epilogue, tile) is covered by the edge variant: mode 2 (bf16 / fp32 store / fp32 accumulate)
// or mode 3 (fp32 store / accumulate), N any positive number, M and K tile multiples, rows of B and C at least
// pad8(N) long
IIT_EXPORT int iit_gemm_glds_edge_ok(const void* A, const void* B, const void* C, const void* bias0, long lda,
                                     long ldb, long ldc, int M, int N, int K, int mode, int epi, int tile) {
  const TileRow* t = find_tile(kEdgeRows, tile);
  if (!t || !combo_ok(mode, epi)) return 0;
  if (M <= 0 || N <= 0 || K <= 0 || M % t->bm || K % t->bk) return 0;
  if (lda % 8 || ldb % 8 || ldc % 8 || ldb < pad8l(N) || ldc < pad8l(N)) return 0;
  if (((uintptr_t)A | (uintptr_t)B | (uintptr_t)C | (uintptr_t)bias0) & 15) return 0;
  return 1;
}

// arguments as iit_gemm_glds_sm (csrc/gemm_glds.hip); ``bias0`` needs N readable floats, ``bsum`` N writable ones
IIT_EXPORT int iit_gemm_glds_edge(const void* A, const void* B, void* C, const float* bias0, long lda, long ldb,
                                  long ldc, int M, int N, int K, int mode, int epi, int tile, int store_mode,
                                  float* bsum, float* gsq, int group_m, void* stream) {
  if (!iit_gemm_glds_edge_ok(A, B, C, bias0, lda, ldb, ldc, M, N, K, mode, epi, tile)) return (int)hipErrorInvalidValue;
  G2Args a{};
  a.A = (const __bf16*)A; a.B = (const __bf16*)B; a.C = C;
  a.bias0 = epi == E_F32_ACC ? nullptr : bias0;
  a.lda = lda; a.ldb = ldb; a.ldc = ldc;
  a.M = M; a.N = N; a.K = K; a.k_per_split = K;
  a.store_mode = store_mode;
  a.group_m = group_m;
  a.bsum = mode == 3 ? bsum : nullptr;
  a.gsq = epi == E_F32_STORE ? gsq : nullptr;
  hipStream_t s = (hipStream_t)stream;
#define X(MODE, AKM, EPI) \
  if (mode == (MODE) && epi == (EPI)) return (int)launch_tile<AKM, EPI>(a, tile, s);
  IIT_EDGE_COMBO_LIST(X)
#undef X
  return (int)hipErrorInvalidValue;
}
