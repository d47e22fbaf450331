// Building blocks of the exact-fp32 MFMA GEMMs.  gemm_f32.hip's header comment derives the pitches and states the
// arithmetic contract.
// * Used by both gemm_f32.hip and conv_f32.hip: the LDS operand images (F32Tile), the XCD remap, the split-order sum
//   of the partial tiles (f32_split_sum) and aligned16.
// * Used by conv_f32.hip ONLY: the double-buffered K loop (f32_main_loop) and the walk over a workgroup's outputs
//   (f32_for_each_out).  gemm_f32.hip keeps its own copy of both inside gemm_f32_kernel: routing that kernel through
//   the functions below changed its register allocation (one instantiation 51 -> 52 VGPRs), and its code was to stay
//   as it was.  A change to the loop here does NOT change gemm_f32.hip's loop, and the other way round; keep the two
//   in step by hand.
// f32_main_loop knows nothing about where an operand element comes from -- a "stager" supplies it:
//   struct Stager { void load(int k0, int kend, int tid);     // K-tile [k0, k0 + BK) of the operand -> registers,
//                                                             //   zeros past kend and past the operand's rows
//                   void store(float* lds, int tid) const; }; // registers -> the F32Tile image at ``lds``
#pragma once
#include "common.h"

namespace {

template <bool KMAJ, int ROWS, int BK>
struct F32Tile {
  static constexpr int PITCH = KMAJ ? ROWS + 16 : BK + 2;
  static constexpr int ELEMS = KMAJ ? BK * PITCH : ROWS * PITCH;
  static constexpr int PER_THREAD = ROWS * BK / 4 / 256;  // float4 chunks per thread
  static_assert(ROWS * BK / 4 % 256 == 0, "tile must split into whole float4 chunks per thread");
  float4 r[PER_THREAD];

  // chunk c of the tile: 4 consecutive elements along the operand's contiguous dimension
  static __device__ __forceinline__ void where(int c, int& row, int& k) {
    if (KMAJ) {
      k = c / (ROWS / 4);
      row = (c % (ROWS / 4)) * 4;
    } else {
      row = c / (BK / 4);
      k = (c % (BK / 4)) * 4;
    }
  }

  __device__ __forceinline__ void load(const float* base, long ld, int row0, int nrows, int k0, int kend, int tid) {
#pragma unroll
    for (int i = 0; i < PER_THREAD; ++i) {
      int row, k;
      where(tid + i * 256, row, k);
      row += row0;
      k += k0;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row < nrows && k < kend) {
        const long off = KMAJ ? (long)k * ld + row : (long)row * ld + k;
        const int n = KMAJ ? nrows - row : kend - k;  // valid elements of this chunk
        if (n >= 4) {
          v = *(const float4*)(base + off);
        } else {
          v.x = base[off];
          if (n > 1) v.y = base[off + 1];
          if (n > 2) v.z = base[off + 2];
        }
      }
      r[i] = v;
    }
  }

  __device__ __forceinline__ void store(float* lds, int tid) const {
#pragma unroll
    for (int i = 0; i < PER_THREAD; ++i) {
      int row, k;
      where(tid + i * 256, row, k);
      if (KMAJ) {
        *(float4*)(lds + k * PITCH + row) = r[i];
      } else {
        float* d = lds + row * PITCH + k;
        *(float2*)d = make_float2(r[i].x, r[i].y);
        *(float2*)(d + 2) = make_float2(r[i].z, r[i].w);
      }
    }
  }

  // 16x16x4 operand fragment: lane l gets X[row0 + (l & 15)][kb + (l >> 4)]
  static __device__ __forceinline__ float frag(const float* lds, int row0, int kb, int lane) {
    if (KMAJ) return lds[(kb + (lane >> 4)) * PITCH + row0 + (lane & 15)];
    return lds[(row0 + (lane & 15)) * PITCH + kb + (lane >> 4)];
  }
};

__device__ __forceinline__ int xcd_remap_f32(int bid, int nwg) {
  const int xcd = bid % 8;
  const int q = nwg / 8, r = nwg % 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + bid / 8;
}

// floats of LDS a BM x BN workgroup needs for the images LA and LB, double-buffered
template <class LA, class LB>
constexpr int f32_smem_elems() { return 2 * (LA::ELEMS + LB::ELEMS); }

// acc += A[BM rows][kbeg, kend) * B[BN rows][kbeg, kend) for this wave's (BM/2) x (BN/2) sub-tile: register-staged
// loads into double-buffered LDS, one barrier per K-tile.  An empty range leaves acc alone.
template <int BM, int BN, int BK, class LA, class LB, class SA, class SB>
__device__ __forceinline__ void f32_main_loop(float* smem, SA& la, SB& lb, int kbeg, int kend, int tid,
                                              f32x4 (&acc)[BM / 32][BN / 32]) {
  constexpr int WM = BM / 2, WN = BN / 2;
  constexpr int TM = WM / 16, TN = WN / 16;
  constexpr int STAGE = LA::ELEMS + LB::ELEMS;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int ntiles = (kend - kbeg + BK - 1) / BK;  // 0 for an empty trailing split: the partial tile is zeros
#define SA_(buf) (smem + (buf) * STAGE)
#define SB_(buf) (smem + (buf) * STAGE + LA::ELEMS)
  if (ntiles > 0) {
    la.load(kbeg, kend, tid);
    lb.load(kbeg, kend, tid);
    la.store(SA_(0), tid);
    lb.store(SB_(0), tid);
  }
  __syncthreads();
  int cur = 0;
  for (int kt = 0; kt < ntiles; ++kt) {
    const bool more = kt + 1 < ntiles;
    if (more) {
      la.load(kbeg + (kt + 1) * BK, kend, tid);
      lb.load(kbeg + (kt + 1) * BK, kend, tid);
    }
#pragma unroll
    for (int kb = 0; kb < BK; kb += 4) {
      float a[TM], b[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) a[i] = LA::frag(SA_(cur), wm * WM + i * 16, kb, lane);
#pragma unroll
      for (int j = 0; j < TN; ++j) b[j] = LB::frag(SB_(cur), wn * WN + j * 16, kb, lane);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    if (more) {
      la.store(SA_(cur ^ 1), tid);
      lb.store(SB_(cur ^ 1), tid);
    }
    __syncthreads();
    cur ^= 1;
  }
#undef SA_
#undef SB_
}

// f(row, col, value) for every accumulator element of this wave inside M x N.
// C/D map of the 16 x 16 forms: column = lane & 15, row = 4 (lane >> 4) + register
template <int BM, int BN, class F>
__device__ __forceinline__ void f32_for_each_out(const f32x4 (&acc)[BM / 32][BN / 32], int m0, int n0, int M, int N,
                                                 int tid, F f) {
  constexpr int WM = BM / 2, WN = BN / 2;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
#pragma unroll
  for (int i = 0; i < WM / 16; ++i) {
#pragma unroll
    for (int j = 0; j < WN / 16; ++j) {
      const int col = n0 + wn * WN + j * 16 + (lane & 15);
      if (col >= N) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wm * WM + i * 16 + 4 * (lane >> 4) + r;
        if (row >= M) continue;
        f(row, col, acc[i][j][r]);
      }
    }
  }
}

// element idx of the partial tiles ws[splits][total], added in split order
__device__ __forceinline__ float f32_split_sum(const float* ws, int splits, long total, long idx) {
  float v = ws[idx];
  for (int s = 1; s < splits; ++s) v = v + ws[s * total + idx];
  return v;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace
