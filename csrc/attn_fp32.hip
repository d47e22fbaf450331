// Exact-fp32 attention for gfx950 (MI355X), forward and backward, 1 <= S <= 64, 1 <= dh <= 64.
//
// * q, k, v, dO, z, dq, dk, dv are fp32 [B][S][H][dh]; every tensor has its own element strides for batch, position
//   and head and a unit last stride.  lse is [B][H][S] contiguous.  Nothing is rounded to bf16: operands, P and dS
//   stay fp32 and every product runs on v_mfma_f32_16x16x4_f32 (a k-ordered fmaf chain from +0, see gemm_f32.hip).
// * One wave owns a (batch, head); a workgroup holds 1..4 waves, as many as fit 160 KiB of LDS
//   (iit_attn_f32_waves).  The waves share nothing; they run the same loop bounds (S, dh and causal are uniform), so
//   every barrier is reached by all of them, and a wave past the last (batch, head) computes on zeros and touches
//   no memory.
// * Per wave the operands sit in LDS as [Sp][Dp + 2] images, Sp = S rounded up to 16 and Dp = dh rounded up to 16,
//   zero-filled past S and dh (a zero pair leaves an fmaf chain unchanged).  A tensor whose base is 16-byte aligned
//   and whose strides and dh are multiples of 4 is read and written with 16-byte accesses; any other one element
//   at a time (a head of dh = 20 inside a packed row whose pitch is a multiple of 4 still takes the vector path; a
//   base offset by one float takes the scalar one).  Nothing is read or written past S or dh.
// * Score tiles are 16 x 16 accumulators: lane l holds column (key) l & 15 and rows (queries) 4 (l >> 4) + r.  The
//   scaled, masked scores go to a per-wave [Sp][Sp + 2] LDS table; every later product reads P / dS from there as an
//   MFMA operand in whichever orientation it needs (z^T = V^T P^T, dV^T = dO^T P, dK^T = Q^T dS, dQ^T = K^T dS^T), so
//   each output tile has its feature index on the registers and is stored 4 consecutive floats per lane.
// * Softmax is two-pass over the row's tiles: row max m of the scaled scores in natural units, p = exp2((s - m)
//   log2 e) (a masked or padded key gets exactly 0), the sum in key-tile order then a 16-lane butterfly,
//   lse = m + ln 2 * log2(sum), z = (P V) / sum.  A sum of exactly 1 gives lse = m bit for bit.
// * The backward recomputes P = exp2((s - lse) log2 e), forms D = rowsum(P o dP) (z is not needed) and
//   dS = P (dP - D) scale.  A causal product skips the key tiles above the diagonal.
// * No atomics; every sum has one fixed order, so results are bit-identical from run to run.
// * The paired forward (iit_attn_f32_fwd_pair) is the forward over 2B batches, rows [0, B) base and [B, 2B) source,
//   with an interchange splice of z in the store: a SpliceSpec (splice_spec.h) over the base shape [B][S][H][dh]
//   selects the elements of a base row that the source wave of the same (batch, head) stores, and the base wave
//   stores the others; the two never write the same element.  The masked backward (iit_attn_f32_bwd_masked) stages
//   the selected elements of dO as +0.  Both are the plain kernels' second template instantiation; the plain
//   instantiation takes an empty trailing argument and compiles to the same instructions as without it.
#include "common.h"
#include "splice_spec.h"

namespace {

constexpr size_t kAttnF32LdsMax = 160 * 1024;
constexpr float kLog2e = 1.4426950408889634f, kLn2 = 0.6931471805599453f;

struct Str3 {
  long b, s, h;
};

struct AttnF32Args {
  const float *q, *k, *v, *dout, *lse_in;
  float *z, *lse, *dq, *dk, *dv;
  Str3 sq, sk, sv, sdo, sz, sdq, sdk, sdv;
  int B, S, H, dh;
  float scale;
  int causal;
  int waves;
};

// the trailing kernel argument: the spec of the paired forward / masked backward, nothing for the plain kernels
template <bool WITH>
struct SpecArg {
  SpliceSpec sp;
};
template <>
struct SpecArg<false> {};

inline int up16(int n) { return (n + 15) / 16 * 16; }

// floats of LDS one wave needs: 3 (forward) or 4 (backward) operand images, one or two score tables, the forward's
// row of reciprocal sums
inline size_t wave_floats(int S, int dh, bool backward) {
  const size_t Sp = up16(S), DP = up16(dh) + 2, PS = Sp + 2;
  return backward ? 4 * Sp * DP + 2 * Sp * PS : 3 * Sp * DP + Sp * PS + Sp;
}

inline int waves_for(int S, int dh, bool backward) {
  const size_t per = wave_floats(S, dh, backward) * sizeof(float);
  const size_t fit = kAttnF32LdsMax / per;
  return fit >= 4 ? 4 : (int)fit;
}

__device__ __forceinline__ bool vec4_ok(const void* p, const Str3& s, int dh) {
  return (((uintptr_t)p & 15) == 0) && (((s.b | s.s | s.h) & 3) == 0) && ((dh & 3) == 0);
}

// the [Sp][Dp] zero-padded image of one head's [S][dh] rows, pitch Dp + 2 (rows 8-byte aligned: a staged float4 is
// two 8-byte stores)
__device__ __forceinline__ void stage(const float* base, long ss, bool vec, bool active, int S, int dh, int Sp, int Dp,
                                      float* lds, int lane) {
  const int per_row = Dp >> 2, DP = Dp + 2;
  for (int c = lane; c < Sp * per_row; c += 64) {
    const int row = c / per_row, col = (c % per_row) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (active && row < S && col < dh) {
      const float* p = base + (long)row * ss + col;
      const int n = dh - col;
      if (vec) {
        v = *(const float4*)p;
      } else {
        v.x = p[0];
        if (n > 1) v.y = p[1];
        if (n > 2) v.z = p[2];
        if (n > 3) v.w = p[3];
      }
    }
    float* d = lds + row * DP + col;
    *(float2*)d = make_float2(v.x, v.y);
    *(float2*)(d + 2) = make_float2(v.z, v.w);
  }
}

// out[row][d .. d + 3] = v, guarded by dh
__device__ __forceinline__ void store4(float* base, long ss, bool vec, int row, int d, int dh, f32x4 v) {
  if (d >= dh) return;
  float* p = base + (long)row * ss + d;
  if (vec) {
    *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (d + r < dh) p[r] = v[r];
  }
}

// bit r set iff element (c0, c1, c2, d + r) is selected, for the chunk's elements below dh: dimensions 0..2 once per
// chunk, dimension 3 per element
__device__ __forceinline__ int sel4(const SpliceSpec& sp, int c0, int c1, int c2, int d, int dh) {
  if (!(in_ranges(sp, 0, c0) && in_ranges(sp, 1, c1) && in_ranges(sp, 2, c2))) return 0;
  int bits = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (d + r < dh && in_ranges(sp, 3, d + r)) bits |= 1 << r;
  return bits;
}

// store4 of the elements whose bit is set: a whole chunk as one 16-byte store on the vector path, a partial one
// element by element, none at all for bits == 0
__device__ __forceinline__ void store4_bits(float* base, long ss, bool vec, int row, int d, int dh, f32x4 v, int bits) {
  if (d >= dh || bits == 0) return;
  float* p = base + (long)row * ss + d;
  if (vec && bits == 15) {
    *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (d + r < dh && ((bits >> r) & 1)) p[r] = v[r];
  }
}

// stage() of one head's dO rows with the selected elements replaced by +0 (a selection, never a product: a NaN
// there does not reach LDS); a wholly selected chunk is not loaded
__device__ __forceinline__ void stage_masked(const float* base, long ss, bool vec, bool active, int S, int dh, int Sp,
                                             int Dp, float* lds, int lane, const SpliceSpec& sp, int b, int h) {
  const int per_row = Dp >> 2, DP = Dp + 2;
  for (int c = lane; c < Sp * per_row; c += 64) {
    const int row = c / per_row, col = (c % per_row) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (active && row < S && col < dh) {
      const float* p = base + (long)row * ss + col;
      const int n = dh - col;
      const int sel = sel4(sp, b, row, h, col, dh);
      if (vec) {
        if (sel != 15) v = *(const float4*)p;
      } else {
        if (!(sel & 1)) v.x = p[0];
        if (n > 1 && !(sel & 2)) v.y = p[1];
        if (n > 2 && !(sel & 4)) v.z = p[2];
        if (n > 3 && !(sel & 8)) v.w = p[3];
      }
      v.x = (sel & 1) ? 0.f : v.x;
      v.y = (sel & 2) ? 0.f : v.y;
      v.z = (sel & 4) ? 0.f : v.z;
      v.w = (sel & 8) ? 0.f : v.w;
    }
    float* d = lds + row * DP + col;
    *(float2*)d = make_float2(v.x, v.y);
    *(float2*)(d + 2) = make_float2(v.z, v.w);
  }
}

// butterfly over the 16 lanes that hold one score row; every lane ends with the same bits
__device__ __forceinline__ float row_max16(float v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float row_sum16(float v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v = v + __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// PAIR: rows [0, B) of the 2B batches are base and rows [B, 2B) source; ``sp`` selects, over the base shape
// [B][S][H][dh], the elements of a base row's z that the source wave of the same (batch - B, head) writes instead of
// the base wave (disjoint elements: no ordering between the two waves is needed)
template <bool PAIR>
__global__ __launch_bounds__(256) void attn_f32_fwd_kernel(AttnF32Args p, SpecArg<PAIR> x) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int S = p.S, dh = p.dh;
  const int Sp = (S + 15) & ~15, Dp = (dh + 15) & ~15, D4 = (dh + 3) & ~3;
  const int DP = Dp + 2, PS = Sp + 2;
  const long bh = (long)blockIdx.x * p.waves + wave;
  const bool active = bh < (long)p.B * p.H;
  const long b = active ? bh / p.H : 0, h = active ? bh % p.H : 0;

  float* Qs = sm + (size_t)wave * (3 * Sp * DP + Sp * PS + Sp);
  float* Ks = Qs + Sp * DP;
  float* Vs = Ks + Sp * DP;
  float* Ps = Vs + Sp * DP;
  float* Ls = Ps + Sp * PS;

  const float* q = p.q + b * p.sq.b + h * p.sq.h;
  const float* k = p.k + b * p.sk.b + h * p.sk.h;
  const float* v = p.v + b * p.sv.b + h * p.sv.h;
  float* z = p.z + b * p.sz.b + h * p.sz.h;
  stage(q, p.sq.s, vec4_ok(p.q, p.sq, dh), active, S, dh, Sp, Dp, Qs, lane);
  stage(k, p.sk.s, vec4_ok(p.k, p.sk, dh), active, S, dh, Sp, Dp, Ks, lane);
  stage(v, p.sv.s, vec4_ok(p.v, p.sv, dh), active, S, dh, Sp, Dp, Vs, lane);
  __syncthreads();

  const int nt = Sp >> 4;
  for (int ti = 0; ti < nt; ++ti) {
    const int jt_end = p.causal ? ti + 1 : nt;
    float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int tj = 0; tj < jt_end; ++tj) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      const float* qa = Qs + (ti * 16 + c) * DP + g;
      const float* kb_ = Ks + (tj * 16 + c) * DP + g;
      for (int kb = 0; kb < D4; kb += 4) acc = mfma4(qa[kb], kb_[kb], acc);
      const int j = tj * 16 + c;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = ti * 16 + 4 * g + r;
        const bool ok = j < S && (!p.causal || j <= i);
        const float s = ok ? acc[r] * p.scale : -INFINITY;
        m[r] = fmaxf(m[r], s);
        Ps[i * PS + j] = s;
      }
    }
    float sum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) m[r] = row_max16(m[r]);  // finite: key 0 is allowed for every query
    for (int tj = 0; tj < jt_end; ++tj) {
      const int j = tj * 16 + c;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = ti * 16 + 4 * g + r;
        const float s = Ps[i * PS + j];  // this lane's own store
        const float e = s == -INFINITY ? 0.f : __builtin_amdgcn_exp2f((s - m[r]) * kLog2e);
        sum[r] = sum[r] + e;
        Ps[i * PS + j] = e;
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = ti * 16 + 4 * g + r;
      const float tot = row_sum16(sum[r]);  // >= 1: the row's top key contributes exp2(0)
      if (c == 0) {
        Ls[i] = 1.0f / tot;
        if (active && i < S) p.lse[bh * S + i] = m[r] + __builtin_amdgcn_logf(tot) * kLn2;
      }
    }
  }
  __syncthreads();

  // z^T[d][i] = sum_j V[j][d] P[i][j]: lane -> query i = ti * 16 + c, features d = td * 16 + 4 g + r
  const bool vz = vec4_ok(p.z, p.sz, dh);
  for (int ti = 0; ti < nt; ++ti) {
    const int kend = p.causal ? (ti + 1) * 16 : Sp;
    const int i = ti * 16 + c;
    const float inv = Ls[i];
    const float* pb = Ps + i * PS + g;
    for (int td = 0; td * 16 < dh; ++td) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      const float* va = Vs + g * DP + td * 16 + c;
      for (int kb = 0; kb < kend; kb += 4) acc = mfma4(va[kb * DP], pb[kb], acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = acc[r] * inv;
      if constexpr (!PAIR) {
        if (active && i < S) store4(z, p.sz.s, vz, i, td * 16 + 4 * g, dh, acc);
      } else if (active && i < S) {
        const int d = td * 16 + 4 * g;
        const int nb = p.B >> 1;
        const bool source = b >= nb;
        const int sel = sel4(x.sp, (int)(source ? b - nb : b), i, (int)h, d, dh);  // per valid element of the chunk
        if (source) {
          store4(z, p.sz.s, vz, i, d, dh, acc);
          store4_bits(z - (long)nb * p.sz.b, p.sz.s, vz, i, d, dh, acc, sel);
        } else {
          store4_bits(z, p.sz.s, vz, i, d, dh, acc, ~sel & 15);
        }
      }
    }
  }
}

// MASKED: the elements of dO that ``sp`` selects (over [B][S][H][dh]) are staged as +0
template <bool MASKED>
__global__ __launch_bounds__(256) void attn_f32_bwd_kernel(AttnF32Args p, SpecArg<MASKED> x) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int S = p.S, dh = p.dh;
  const int Sp = (S + 15) & ~15, Dp = (dh + 15) & ~15, D4 = (dh + 3) & ~3;
  const int DP = Dp + 2, PS = Sp + 2;
  const long bh = (long)blockIdx.x * p.waves + wave;
  const bool active = bh < (long)p.B * p.H;
  const long b = active ? bh / p.H : 0, h = active ? bh % p.H : 0;

  float* Qs = sm + (size_t)wave * (4 * Sp * DP + 2 * Sp * PS);
  float* Ks = Qs + Sp * DP;
  float* Vs = Ks + Sp * DP;
  float* Os = Vs + Sp * DP;
  float* Ps = Os + Sp * DP;
  float* Ds = Ps + Sp * PS;

  stage(p.q + b * p.sq.b + h * p.sq.h, p.sq.s, vec4_ok(p.q, p.sq, dh), active, S, dh, Sp, Dp, Qs, lane);
  stage(p.k + b * p.sk.b + h * p.sk.h, p.sk.s, vec4_ok(p.k, p.sk, dh), active, S, dh, Sp, Dp, Ks, lane);
  stage(p.v + b * p.sv.b + h * p.sv.h, p.sv.s, vec4_ok(p.v, p.sv, dh), active, S, dh, Sp, Dp, Vs, lane);
  if constexpr (MASKED)
    stage_masked(p.dout + b * p.sdo.b + h * p.sdo.h, p.sdo.s, vec4_ok(p.dout, p.sdo, dh), active, S, dh, Sp, Dp, Os,
                 lane, x.sp, (int)b, (int)h);
  else
    stage(p.dout + b * p.sdo.b + h * p.sdo.h, p.sdo.s, vec4_ok(p.dout, p.sdo, dh), active, S, dh, Sp, Dp, Os, lane);
  __syncthreads();

  const int nt = Sp >> 4;
  for (int ti = 0; ti < nt; ++ti) {
    const int jt_end = p.causal ? ti + 1 : nt;
    float lse[4], dsum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = ti * 16 + 4 * g + r;
      lse[r] = (active && i < S) ? p.lse_in[bh * S + i] : 0.f;  // a padded query: zero scores, P = 1, dO = 0
    }
    for (int tj = 0; tj < jt_end; ++tj) {
      f32x4 as = {0.f, 0.f, 0.f, 0.f}, ap = {0.f, 0.f, 0.f, 0.f};
      const int io = (ti * 16 + c) * DP + g, jo = (tj * 16 + c) * DP + g;
      for (int kb = 0; kb < D4; kb += 4) {
        as = mfma4(Qs[io + kb], Ks[jo + kb], as);
        ap = mfma4(Os[io + kb], Vs[jo + kb], ap);
      }
      const int j = tj * 16 + c;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = ti * 16 + 4 * g + r;
        const bool ok = j < S && (!p.causal || j <= i);
        const float pr = ok ? __builtin_amdgcn_exp2f((as[r] * p.scale - lse[r]) * kLog2e) : 0.f;
        dsum[r] = dsum[r] + pr * ap[r];
        Ps[i * PS + j] = pr;
        Ds[i * PS + j] = ap[r];
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) dsum[r] = row_sum16(dsum[r]);
    for (int tj = 0; tj < jt_end; ++tj) {
      const int j = tj * 16 + c;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = (ti * 16 + 4 * g + r) * PS + j;  // this lane's own stores
        Ds[o] = Ps[o] * (Ds[o] - dsum[r]) * p.scale;
      }
    }
  }
  __syncthreads();

  float* dq = p.dq + b * p.sdq.b + h * p.sdq.h;
  float* dk = p.dk + b * p.sdk.b + h * p.sdk.h;
  float* dv = p.dv + b * p.sdv.b + h * p.sdv.h;
  const bool vq = vec4_ok(p.dq, p.sdq, dh), vk = vec4_ok(p.dk, p.sdk, dh), vv = vec4_ok(p.dv, p.sdv, dh);
  // dV^T[d][j] = sum_i dO[i][d] P[i][j] and dK^T[d][j] = sum_i Q[i][d] dS[i][j]: lane -> key j = tj * 16 + c,
  // features d = td * 16 + 4 g + r; causal: queries below the key tile's first row see none of its keys
  for (int tj = 0; tj < nt; ++tj) {
    const int kbeg = p.causal ? tj * 16 : 0;
    const int j = tj * 16 + c;
    for (int td = 0; td * 16 < dh; ++td) {
      f32x4 av = {0.f, 0.f, 0.f, 0.f}, ak = {0.f, 0.f, 0.f, 0.f};
      const int xo = g * DP + td * 16 + c, po = g * PS + j;
      for (int kb = kbeg; kb < Sp; kb += 4) {
        av = mfma4(Os[xo + kb * DP], Ps[po + kb * PS], av);
        ak = mfma4(Qs[xo + kb * DP], Ds[po + kb * PS], ak);
      }
      if (active && j < S) {
        store4(dv, p.sdv.s, vv, j, td * 16 + 4 * g, dh, av);
        store4(dk, p.sdk.s, vk, j, td * 16 + 4 * g, dh, ak);
      }
    }
  }
  // dQ^T[d][i] = sum_j K[j][d] dS[i][j]: lane -> query i = ti * 16 + c
  for (int ti = 0; ti < nt; ++ti) {
    const int kend = p.causal ? (ti + 1) * 16 : Sp;
    const int i = ti * 16 + c;
    for (int td = 0; td * 16 < dh; ++td) {
      f32x4 aq = {0.f, 0.f, 0.f, 0.f};
      const int xo = g * DP + td * 16 + c, so = i * PS + g;
      for (int kb = 0; kb < kend; kb += 4) aq = mfma4(Ks[xo + kb * DP], Ds[so + kb], aq);
      if (active && i < S) store4(dq, p.sdq.s, vq, i, td * 16 + 4 * g, dh, aq);
    }
  }
}

inline bool aligned4(const void* p) { return p && ((uintptr_t)p & 3) == 0; }

inline bool shape_ok(int B, int S, int H, int dh) {
  return B >= 1 && H >= 1 && S >= 1 && S <= 64 && dh >= 1 && dh <= 64 && (long)B * H <= 0x7fffffffL;
}

}  // namespace

// bytes of dynamic LDS one wave of the forward / backward kernel needs at (S, dh); 0 outside the supported range
IIT_EXPORT int iit_attn_f32_lds(int S, int dh, int backward) {
  if (!shape_ok(1, S, 1, dh)) return 0;
  return (int)(wave_floats(S, dh, backward != 0) * sizeof(float));
}

// waves (= (batch, head) pairs) per workgroup: as many as fit 160 KiB, at most 4; 0 outside the supported range
IIT_EXPORT int iit_attn_f32_waves(int S, int dh, int backward) {
  if (!shape_ok(1, S, 1, dh)) return 0;
  return waves_for(S, dh, backward != 0);
}

// 1 when the kernels take the problem: 1 <= S, dh <= 64 and four non-null, 4-byte aligned fp32 operands (the strides
// are free: unit last stride is the ABI, everything else is handled by the scalar path)
IIT_EXPORT int iit_attn_f32_ok(const void* q, const void* k, const void* v, const void* o, int B, int S, int H,
                               int dh) {
  if (!shape_ok(B, S, H, dh)) return 0;
  if (!aligned4(q) || !aligned4(k) || !aligned4(v) || !aligned4(o)) return 0;
  return waves_for(S, dh, true) >= 1 ? 1 : 0;
}

// strides: 3 longs (batch, position, head; in elements) per tensor, in the order q, k, v, z
IIT_EXPORT int iit_attn_f32_fwd(const void* q, const void* k, const void* v, void* z, void* lse, const long* strides,
                                int B, int S, int H, int dh, float scale, int causal, void* stream) {
  if (!strides || !aligned4(lse) || !iit_attn_f32_ok(q, k, v, z, B, S, H, dh)) return (int)hipErrorInvalidValue;
  AttnF32Args a = {};
  a.q = (const float*)q; a.k = (const float*)k; a.v = (const float*)v;
  a.z = (float*)z; a.lse = (float*)lse;
  const Str3* s = (const Str3*)strides;
  a.sq = s[0]; a.sk = s[1]; a.sv = s[2]; a.sz = s[3];
  a.B = B; a.S = S; a.H = H; a.dh = dh;
  a.scale = scale; a.causal = causal;
  a.waves = waves_for(S, dh, false);
  const size_t lds = a.waves * wave_floats(S, dh, false) * sizeof(float);
  hipLaunchKernelGGL(attn_f32_fwd_kernel<false>, dim3(cdiv((long)B * H, a.waves)), dim3(64 * a.waves), lds,
                     (hipStream_t)stream, a, SpecArg<false>{});
  return (int)hipGetLastError();
}

// strides: 3 longs per tensor, in the order q, k, v, dO, dq, dk, dv
IIT_EXPORT int iit_attn_f32_bwd(const void* q, const void* k, const void* v, const void* dout, const void* lse,
                                void* dq, void* dk, void* dv, const long* strides, int B, int S, int H, int dh,
                                float scale, int causal, void* stream) {
  if (!strides || !aligned4(lse) || !aligned4(dq) || !aligned4(dk) || !aligned4(dv) ||
      !iit_attn_f32_ok(q, k, v, dout, B, S, H, dh))
    return (int)hipErrorInvalidValue;
  AttnF32Args a = {};
  a.q = (const float*)q; a.k = (const float*)k; a.v = (const float*)v;
  a.dout = (const float*)dout; a.lse_in = (const float*)lse;
  a.dq = (float*)dq; a.dk = (float*)dk; a.dv = (float*)dv;
  const Str3* s = (const Str3*)strides;
  a.sq = s[0]; a.sk = s[1]; a.sv = s[2]; a.sdo = s[3]; a.sdq = s[4]; a.sdk = s[5]; a.sdv = s[6];
  a.B = B; a.S = S; a.H = H; a.dh = dh;
  a.scale = scale; a.causal = causal;
  a.waves = waves_for(S, dh, true);
  const size_t lds = a.waves * wave_floats(S, dh, true) * sizeof(float);
  hipLaunchKernelGGL(attn_f32_bwd_kernel<false>, dim3(cdiv((long)B * H, a.waves)), dim3(64 * a.waves), lds,
                     (hipStream_t)stream, a, SpecArg<false>{});
  return (int)hipGetLastError();
}

namespace {

// the spec must describe exactly the base shape
inline bool spec_ok(const void* spec, int B, int S, int H, int dh) {
  if (!spec) return false;
  const SpliceSpec* sp = (const SpliceSpec*)spec;
  if (sp->shape[0] != B || sp->shape[1] != S || sp->shape[2] != H || sp->shape[3] != dh) return false;
  for (int d = 0; d < 4; ++d)
    if (sp->nr[d] < 0 || sp->nr[d] > 8) return false;
  return true;
}

}  // namespace

// iit_attn_f32_fwd over B2 = 2B batches, rows [0, B) base and [B, 2B) source, with an interchange splice of z in
// the store: ``spec`` (host pointer to one SpliceSpec over the base shape [B][S][H][dh], copied into the kernel
// arguments; ``sstride`` is not read) selects the elements of a base row that take the source row's value.  Every
// wave computes and writes its lse as the plain kernel does.  strides: as iit_attn_f32_fwd.
IIT_EXPORT int iit_attn_f32_fwd_pair(const void* q, const void* k, const void* v, void* z, void* lse,
                                     const long* strides, int B2, int S, int H, int dh, float scale, int causal,
                                     const void* spec, void* stream) {
  if (!strides || !aligned4(lse) || !iit_attn_f32_ok(q, k, v, z, B2, S, H, dh) || (B2 & 1) ||
      !spec_ok(spec, B2 / 2, S, H, dh))
    return (int)hipErrorInvalidValue;
  AttnF32Args a = {};
  a.q = (const float*)q; a.k = (const float*)k; a.v = (const float*)v;
  a.z = (float*)z; a.lse = (float*)lse;
  const Str3* s = (const Str3*)strides;
  a.sq = s[0]; a.sk = s[1]; a.sv = s[2]; a.sz = s[3];
  a.B = B2; a.S = S; a.H = H; a.dh = dh;
  a.scale = scale; a.causal = causal;
  a.waves = waves_for(S, dh, false);
  const size_t lds = a.waves * wave_floats(S, dh, false) * sizeof(float);
  const SpecArg<true> sp = {*(const SpliceSpec*)spec};
  hipLaunchKernelGGL(attn_f32_fwd_kernel<true>, dim3(cdiv((long)B2 * H, a.waves)), dim3(64 * a.waves), lds,
                     (hipStream_t)stream, a, sp);
  return (int)hipGetLastError();
}

// iit_attn_f32_bwd with the spec-selected elements of dO ([B][S][H][dh]) taken as +0: the backward of the base rows
// of iit_attn_f32_fwd_pair.  strides: as iit_attn_f32_bwd.
IIT_EXPORT int iit_attn_f32_bwd_masked(const void* q, const void* k, const void* v, const void* dout,
                                       const void* lse, void* dq, void* dk, void* dv, const long* strides, int B,
                                       int S, int H, int dh, float scale, int causal, const void* spec,
                                       void* stream) {
  if (!strides || !aligned4(lse) || !aligned4(dq) || !aligned4(dk) || !aligned4(dv) ||
      !iit_attn_f32_ok(q, k, v, dout, B, S, H, dh) || !spec_ok(spec, B, S, H, dh))
    return (int)hipErrorInvalidValue;
  AttnF32Args a = {};
  a.q = (const float*)q; a.k = (const float*)k; a.v = (const float*)v;
  a.dout = (const float*)dout; a.lse_in = (const float*)lse;
  a.dq = (float*)dq; a.dk = (float*)dk; a.dv = (float*)dv;
  const Str3* s = (const Str3*)strides;
  a.sq = s[0]; a.sk = s[1]; a.sv = s[2]; a.sdo = s[3]; a.sdq = s[4]; a.sdk = s[5]; a.sdv = s[6];
  a.B = B; a.S = S; a.H = H; a.dh = dh;
  a.scale = scale; a.causal = causal;
  a.waves = waves_for(S, dh, true);
  const size_t lds = a.waves * wave_floats(S, dh, true) * sizeof(float);
  const SpecArg<true> sp = {*(const SpliceSpec*)spec};
  hipLaunchKernelGGL(attn_f32_bwd_kernel<true>, dim3(cdiv((long)B * H, a.waves)), dim3(64 * a.waves), lds,
                     (hipStream_t)stream, a, sp);
  return (int)hipGetLastError();
}
