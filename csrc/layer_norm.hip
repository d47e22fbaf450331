// Layer norm (LN / LNPre) for gfx950: one wave per row, fp32 statistics, wave64-native.
//
//  ln_fwd_kernel<W, N>                 y = (x - mean) * rstd (* w + b) in bf16, optional fp32 twin, row select
//  ln_bwd_kernel<W, N, DY_F32, XH16>   dx for one row per wave (+ dres, accumulate, bf16 copy)
//  ln_bwd_part_kernel<N, DY_F32, R>    dx for R rows per wave with the affine-gradient partials fused
//  ln_dwdb_kernel / ln_dwdb_vec_kernel / ln_part_reduce_kernel   affine gradients dw / db
//
// A lane owns N "lane elements" of W floats (column group lane + 64 i): W = 4 is the vector layout (16-B fp32 /
// 8-B bf16 accesses; needs d % 4 == 0 and aligned rows, ln_vec), W = 1 covers any d <= 4096 and any alignment.
// The row arithmetic is written once over Pack<W> and shared by both widths.
#include "common.h"
#include "prefetch.h"
#include <initializer_list>
#include <stdlib.h>
#include <type_traits>

// ============================================================================ lane elements
// W floats of one lane: loads, stores, the two horizontal sums, and the arithmetic as per-float formulas --
// map(f, a, b, ..) applies f to each float of the operands in turn
template <int W>
struct Pack;

template <>
struct Pack<4> {
  float4 v;
  static __device__ __forceinline__ Pack splat(float s) { return {make_float4(s, s, s, s)}; }
  // element i (in units of W floats) of an fp32 / bf16 row
  static __device__ __forceinline__ Pack load(const float* p, long i) { return {((const float4*)p)[i]}; }
  static __device__ __forceinline__ Pack load(const __bf16* p, long i) {
    const bf16x4 t = ((const bf16x4*)p)[i];
    return {make_float4(bf2f(t[0]), bf2f(t[1]), bf2f(t[2]), bf2f(t[3]))};
  }
  template <class F, class... P>
  static __device__ __forceinline__ Pack map(F f, const P&... a) {
    return {make_float4(f(a.v.x...), f(a.v.y...), f(a.v.z...), f(a.v.w...))};
  }
  // keeps the association (x + y) + (z + w)
  __device__ __forceinline__ float hsum() const { return (v.x + v.y) + (v.z + v.w); }
  // Sum of the products in the same association.  Each pair becomes a multiply and an fma, and which product is
  // the rounded one is the compiler's choice (PIN = 0).  For the N = 1 kernels that choice follows how the SLP
  // vectoriser happens to pair the floats, so it is written out there to keep their results what they have always
  // been: PIN = 1 rounds y y' and w w' (backward), PIN = 2 rounds x x' and z z' (forward).
  template <int PIN>
  static __device__ __forceinline__ float dot(const Pack& a, const Pack& b) {
    if constexpr (PIN == 1)
      return __builtin_fmaf(a.v.x, b.v.x, a.v.y * b.v.y) + __builtin_fmaf(a.v.z, b.v.z, a.v.w * b.v.w);
    else if constexpr (PIN == 2)
      return __builtin_fmaf(a.v.y, b.v.y, a.v.x * b.v.x) + __builtin_fmaf(a.v.w, b.v.w, a.v.z * b.v.z);
    else
      return (a.v.x * b.v.x + a.v.y * b.v.y) + (a.v.z * b.v.z + a.v.w * b.v.w);
  }
  __device__ __forceinline__ void store(float* p, long i) const { ((float4*)p)[i] = v; }
  // stores the bf16 rounding and returns it widened again
  __device__ __forceinline__ Pack store_bf16(__bf16* p, long i) const {
    const bf16x4 t = {f2bf(v.x), f2bf(v.y), f2bf(v.z), f2bf(v.w)};
    ((bf16x4*)p)[i] = t;
    return {make_float4(bf2f(t[0]), bf2f(t[1]), bf2f(t[2]), bf2f(t[3]))};
  }
};

template <>
struct Pack<1> {
  float v;
  static __device__ __forceinline__ Pack splat(float s) { return {s}; }
  static __device__ __forceinline__ Pack load(const float* p, long i) { return {p[i]}; }
  static __device__ __forceinline__ Pack load(const __bf16* p, long i) { return {bf2f(p[i])}; }
  template <class F, class... P>
  static __device__ __forceinline__ Pack map(F f, const P&... a) { return {f(a.v...)}; }
  __device__ __forceinline__ float hsum() const { return v; }
  template <int PIN>
  static __device__ __forceinline__ float dot(const Pack& a, const Pack& b) { return a.v * b.v; }
  __device__ __forceinline__ void store(float* p, long i) const { p[i] = v; }
  __device__ __forceinline__ Pack store_bf16(__bf16* p, long i) const {
    const __bf16 t = f2bf(v);
    p[i] = t;
    return {bf2f(t)};
  }
};

__device__ __forceinline__ float ln_add(float a, float b) { return a + b; }
__device__ __forceinline__ float ln_mul(float a, float b) { return a * b; }

template <int W, bool F32>
__device__ __forceinline__ Pack<W> ln_load(const void* p, long i) {
  if constexpr (F32) return Pack<W>::load((const float*)p, i);
  else return Pack<W>::load((const __bf16*)p, i);
}

// Row select: the interchange splice of whole positions of an LN output inside the LN kernel itself (a paired
// source+base forward, iit_amd/models/bert.py forward_paired: MQNLI's ``hook_normalized_resid_post`` position
// sites).  Rows [0, Tb) are the base rows, [Tb, 2 Tb) the source rows at the same (batch, position); a base row
// whose position s has bit s of ``mask`` set normalises the SOURCE row instead (out[idx] = src[idx] for whole
// rows), and in the backward the same base rows get no gradient (the spliced slice is a constant).  mask == 0:
// plain LN.
struct RowSel {
  unsigned long long mask;
  int S;
  int Tb;
};

__device__ __forceinline__ bool sel_hit(const RowSel& sel, int row) {
  return sel.mask != 0ull && row < sel.Tb && ((sel.mask >> (row % sel.S)) & 1ull);
}

// ============================================================================ forward
// ``y32`` (nullable, W = 4 only): the fp32 twin of the rounded output (a post-norm block's residual operand: no
// separate cast pass).
// ``pf``: the first pf.wgs workgroups of the grid do no row work: they read the weights of the GEMMs that follow this
// norm (the block's bf16 mirrors, HBM-cold after the optimizer pass) into the caches and leave (csrc/prefetch.h); at
// the front of the grid, so their HBM latency runs under the row work.  The row blocks follow them.
template <int W, int N>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                     const float* __restrict__ b, __bf16* __restrict__ y,
                                                     float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                     int T, int d, float eps, RowSel sel, float* __restrict__ y32,
                                                     Prefetch pf) {
  using P = Pack<W>;
  if ((int)blockIdx.x < pf.wgs) {  // uniform over the block
    prefetch_part(pf, blockIdx.x);
    return;
  }
  const int row = (blockIdx.x - pf.wgs) * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= T) return;
  const int dn = d / W;
  const long xat = (long)(sel_hit(sel, row) ? row + sel.Tb : row) * dn, yat = (long)row * dn;
  P v[N];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int c = lane + i * 64;
    v[i] = c < dn ? P::load(x, xat + c) : P::splat(0.f);
    s += v[i].hsum();
  }
  const float mu = wave_sum(s) / d;
  float s2 = 0.f;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int c = lane + i * 64;
    // (the same sums either way: a select for W = 1 and a branch for W = 4 is what keeps every instantiation's
    // occupancy, profiles/ln_refactor_resources.txt)
    if (W == 1 || c < dn) {
      v[i] = c < dn ? P::map([&](float a) { return a - mu; }, v[i]) : P::splat(0.f);
      s2 += P::template dot<N == 1 ? 2 : 0>(v[i], v[i]);
    }
  }
  const float rstd = rsqrtf(wave_sum(s2) / d + eps);
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int c = lane + i * 64;
    if (c < dn) {
      P o = P::map([&](float z) { return z * rstd; }, v[i]);
      if (w) o = P::map([](float a, float ww, float bb) { return a * ww + bb; }, o, P::load(w, c), P::load(b, c));
      [[maybe_unused]] const P r = o.store_bf16(y, yat + c);
      if constexpr (W == 4)
        if (y32) r.store(y32, yat + c);
    }
  }
  if (lane == 0) {
    mean_out[row] = mu;
    rstd_out[row] = rstd;
  }
}

// ============================================================================ backward
// dx = rstd * (g - mean(g) - xhat * mean(g * xhat)) (+ dres),  g = dy * w.
// ``dres`` (nullable) is the residual stream's skip-connection gradient: fusing it here saves autograd's
// separate gradient-sum pass over the fp32 residual.  ``dx16`` (nullable) receives a bf16 copy of dx: the
// next backward GEMMs (W_O / W_out dX and dW) read bf16, so the cast rides along with this pass.
//
// One row from its loaded operands: ``g`` = dy * w and ``xh`` = xhat, both zero outside the row; ``at`` = row * dn +
// lane.
template <int W, int N>
__device__ __forceinline__ void ln_bwd_row(const Pack<W> (&g)[N], const Pack<W> (&xh)[N], float rs, long at, int lane,
                                           int dn, int d, float* dx, const float* dres, __bf16* dx16, int accumulate) {
  using P = Pack<W>;
  float sg = 0.f, sgx = 0.f;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    sg += g[i].hsum();
    sgx += P::template dot<N == 1 ? 1 : 0>(g[i], xh[i]);
  }
  sg = wave_sum(sg) / d;
  sgx = wave_sum(sgx) / d;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int c = lane + i * 64;
    if (c < dn) {
      P o = P::map([&](float a, float h) { return rs * (a - sg - h * sgx); }, g[i], xh[i]);
      if (dres) o = P::map(ln_add, o, P::load(dres, at + i * 64));
      if (accumulate) o = P::map(ln_add, o, P::load(dx, at + i * 64));
      o.store(dx, at + i * 64);
      if (dx16) o.store_bf16(dx16, at + i * 64);
    }
  }
}

// One row per wave.  The affine gradients dw/db are NOT done here (see ln_dwdb_kernel: per-block partial sums,
// few atomics).  XH16: ``x`` is the forward's bf16 output xhat of a norm without affine parameters (LNPre): 2 bytes
// per element instead of the fp32 input, and no mean.  A spliced row (row select) loads nothing: its output came
// from the source row, so dx = dres only.
template <int W, int N, bool DY_F32, bool XH16>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const void* __restrict__ dy_, const void* __restrict__ x,
                                                     const float* __restrict__ mean, const float* __restrict__ rstd,
                                                     const float* __restrict__ w, float* __restrict__ dx,
                                                     const float* __restrict__ dres, __bf16* __restrict__ dx16,
                                                     int T, int d, int accumulate, RowSel sel) {
  using P = Pack<W>;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= T) return;
  const int dn = d / W;
  const long at = (long)row * dn + lane;
  const bool dead = sel_hit(sel, row);
  const float mu = XH16 ? 0.f : mean[row], rs = rstd[row];
  P g[N], xh[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int c = lane + i * 64;
    g[i] = xh[i] = P::splat(0.f);
    if (c < dn && !dead) {
      g[i] = ln_load<W, DY_F32>(dy_, at + i * 64);
      if constexpr (XH16) xh[i] = ln_load<W, false>(x, at + i * 64);
      else xh[i] = P::map([&](float a) { return (a - mu) * rs; }, ln_load<W, true>(x, at + i * 64));
      if (w) g[i] = P::map(ln_mul, g[i], P::load(w, c));
    }
  }
  ln_bwd_row<W, N>(g, xh, rs, at, lane, dn, d, dx, dres, dx16, accumulate);
}

// ln_bwd_kernel (vector layout) with the affine gradients fused: each wave takes R rows (row = block * 4R + 4 r +
// wave), so a lane keeps the same columns for all of them and sums dy * xhat and dy in registers; the block's 4
// waves meet in LDS and write ONE partial row pair (dw part, db part) to ``part[block][2 d]`` with plain stores -- no
// atomics here (the separate ln_dwdb kernels re-read dy and x and did one memory-side fp32 atomic per column per
// 32 rows: ~17 us for [3840][768], profiles/mqnli_step_breakdown_r5.txt).  ln_part_reduce_kernel sums the partials.
// R = rows per wave (the block covers 4 R rows): IIT_LN_PART_R = 1 / 2 / 4, default 1 -- the MQNLI (BERT-base)
// step measured 11.93-11.96 ms at R = 1, 12.03-12.04 at 2 and 12.38-12.40 at 4 (interleaved, one box;
// profiles/mqnli_native_r6.txt): more, shorter blocks beat the smaller partial array
static int ln_part_r() {
  static const int r = [] {
    const char* e = getenv("IIT_LN_PART_R");
    const int v = e ? atoi(e) : 1;
    return (v == 2 || v == 4) ? v : 1;
  }();
  return r;
}
template <int N, bool DY_F32, int R>
__global__ __launch_bounds__(256) void ln_bwd_part_kernel(const void* __restrict__ dy_, const float* __restrict__ x,
                                                          const float* __restrict__ mean,
                                                          const float* __restrict__ rstd, const float* __restrict__ w,
                                                          float* __restrict__ dx, const float* __restrict__ dres,
                                                          __bf16* __restrict__ dx16, float* __restrict__ part, int T,
                                                          int d, int accumulate, RowSel sel,
                                                          const float* __restrict__ dy2) {
  using P = Pack<4>;
  __shared__ P red[2][4][64 * N];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int dn = d >> 2;
  P pw[N], pb[N], ww[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int c = lane + i * 64;
    pw[i] = pb[i] = P::splat(0.f);
    ww[i] = (w && c < dn) ? P::load(w, c) : P::splat(1.f);
  }
  // every row's operands are loaded before the first is used: the R rows' memory latency overlaps
  P dyv[R][N], xvv[R][N];
  float muv[R], rsv[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int row = blockIdx.x * 4 * R + 4 * r + wave;
    const long at = (long)row * dn + lane;
    const bool live = row < T && !sel_hit(sel, row);
    muv[r] = row < T ? mean[row] : 0.f;
    rsv[r] = row < T ? rstd[row] : 0.f;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int c = lane + i * 64;
      dyv[r][i] = xvv[r][i] = P::splat(0.f);
      if (c < dn && live) {
        dyv[r][i] = ln_load<4, DY_F32>(dy_, at + i * 64);
        // the fp32 twin output's gradient (LayerNormTwinFn): dy = dy + dy2
        if (dy2) dyv[r][i] = P::map(ln_add, dyv[r][i], P::load(dy2, at + i * 64));
        xvv[r][i] = P::load(x, at + i * 64);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int row = blockIdx.x * 4 * R + 4 * r + wave;
    if (row >= T) break;
    const bool dead = sel_hit(sel, row);
    P g[N], xh[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const float mu = muv[r], rs = rsv[r];
      xh[i] = dead ? P::splat(0.f) : P::map([&](float a) { return (a - mu) * rs; }, xvv[r][i]);
      // affine partials from the raw dy (dw += dy * xhat, db += dy), then g = dy * w
      pw[i] = P::map([](float s, float a, float h) { return s + a * h; }, pw[i], dyv[r][i], xh[i]);
      pb[i] = P::map(ln_add, pb[i], dyv[r][i]);
      g[i] = P::map(ln_mul, dyv[r][i], ww[i]);
    }
    ln_bwd_row<4, N>(g, xh, rsv[r], (long)row * dn + lane, lane, dn, d, dx, dres, dx16, accumulate);
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    red[0][wave][lane + i * 64] = pw[i];
    red[1][wave][lane + i * 64] = pb[i];
  }
  __syncthreads();
  // 256 threads write the block's 2 x dn partial elements
  for (int k = threadIdx.x; k < 2 * dn; k += 256) {
    const int which = k >= dn, c = which ? k - dn : k;
    const P ab = P::map(ln_add, red[which][0][c], red[which][1][c]);
    const P ef = P::map(ln_add, red[which][2][c], red[which][3][c]);
    P::map(ln_add, ab, ef).store(part, (long)blockIdx.x * 2 * dn + k);
  }
}

// ============================================================================ affine gradients
// dw[c] += sum_t dy[t][c] * xhat[t][c], db[c] += sum_t dy[t][c].
// Block = 64 columns x 256 rows (4 waves x 64 rows), LDS combine, one atomic per column per block.
template <bool DY_F32>
__global__ __launch_bounds__(256) void ln_dwdb_kernel(const void* __restrict__ dy_, const float* __restrict__ x,
                                                      const float* __restrict__ mean, const float* __restrict__ rstd,
                                                      float* __restrict__ dw, float* __restrict__ db, int T, int d,
                                                      RowSel sel) {
  __shared__ float pw[4][64], pb[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), wv = threadIdx.x >> 6;
  const int t0 = blockIdx.y * 256;
  float sw = 0.f, sb = 0.f;
  if (c < d)
    for (int i = 0; i < 64; ++i) {
      const int t = t0 + wv * 64 + i;
      if (t >= T) break;
      if (sel_hit(sel, t)) continue;
      const float dy = DY_F32 ? ((const float*)dy_)[(long)t * d + c] : bf2f(((const __bf16*)dy_)[(long)t * d + c]);
      sw += dy * (x[(long)t * d + c] - mean[t]) * rstd[t];
      sb += dy;
    }
  pw[wv][threadIdx.x & 63] = sw;
  pb[wv][threadIdx.x & 63] = sb;
  __syncthreads();
  if (wv == 0 && c < d) {
    const int l = threadIdx.x;
    atomicAdd(dw + c, pw[0][l] + pw[1][l] + pw[2][l] + pw[3][l]);
    atomicAdd(db + c, pb[0][l] + pb[1][l] + pb[2][l] + pb[3][l]);
  }
}

// Vectorised affine gradients (d % 4 == 0, 16-B aligned rows): a wave covers 256 columns as float4 lanes, the block's 4
// waves take interleaved rows of a 32-row chunk with all 8 rows' loads issued before the first use, and the waves meet
// in LDS for one atomic per column per block.  ~700 blocks at T = 7680 (the 64-column kernel above ran 180-360
// blocks of 64 serial dependent loads per thread: 29 us for [7680][768], profiles/mqnli_step_breakdown_r4.txt).
constexpr int LN_DWDB_ROWS = 32;
template <bool DY_F32>
__global__ __launch_bounds__(256) void ln_dwdb_vec_kernel(const void* __restrict__ dy_, const float* __restrict__ x,
                                                          const float* __restrict__ mean,
                                                          const float* __restrict__ rstd, float* __restrict__ dw,
                                                          float* __restrict__ db, int T, int d, RowSel sel) {
  __shared__ float4 pw[4][64], pb[4][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int d4 = d >> 2;
  const int c4 = blockIdx.x * 64 + lane;
  const int r0 = blockIdx.y * LN_DWDB_ROWS;
  float4 sw = make_float4(0.f, 0.f, 0.f, 0.f), sb = sw;
  if (c4 < d4) {
    constexpr int R = LN_DWDB_ROWS / 4;
    float4 g[R], xv[R];
    float mu[R], rs[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int t = r0 + wv + 4 * i;
      const bool live = t < T && !sel_hit(sel, t);
      g[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      xv[i] = g[i];
      mu[i] = 0.f;
      rs[i] = 0.f;
      if (live) {
        if (DY_F32) {
          g[i] = ((const float4*)dy_)[(long)t * d4 + c4];
        } else {
          const bf16x4 b = ((const bf16x4*)dy_)[(long)t * d4 + c4];
          g[i] = make_float4(bf2f(b[0]), bf2f(b[1]), bf2f(b[2]), bf2f(b[3]));
        }
        xv[i] = ((const float4*)x)[(long)t * d4 + c4];
        mu[i] = mean[t];
        rs[i] = rstd[t];
      }
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
      sw.x += g[i].x * (xv[i].x - mu[i]) * rs[i];
      sw.y += g[i].y * (xv[i].y - mu[i]) * rs[i];
      sw.z += g[i].z * (xv[i].z - mu[i]) * rs[i];
      sw.w += g[i].w * (xv[i].w - mu[i]) * rs[i];
      sb.x += g[i].x; sb.y += g[i].y; sb.z += g[i].z; sb.w += g[i].w;
    }
  }
  pw[wv][lane] = sw;
  pb[wv][lane] = sb;
  __syncthreads();
  if (wv == 0 && c4 < d4) {
    const float4 a = pw[0][lane], b = pw[1][lane], c = pw[2][lane], e = pw[3][lane];
    const float4 p = pb[0][lane], q = pb[1][lane], r = pb[2][lane], u = pb[3][lane];
    float* w4 = dw + 4 * c4;
    float* b4 = db + 4 * c4;
    atomicAdd(w4 + 0, (a.x + b.x) + (c.x + e.x));
    atomicAdd(w4 + 1, (a.y + b.y) + (c.y + e.y));
    atomicAdd(w4 + 2, (a.z + b.z) + (c.z + e.z));
    atomicAdd(w4 + 3, (a.w + b.w) + (c.w + e.w));
    atomicAdd(b4 + 0, (p.x + q.x) + (r.x + u.x));
    atomicAdd(b4 + 1, (p.y + q.y) + (r.y + u.y));
    atomicAdd(b4 + 2, (p.z + q.z) + (r.z + u.z));
    atomicAdd(b4 + 3, (p.w + q.w) + (r.w + u.w));
  }
}

// dw[c] += sum_b part[b][c], db[c] += sum_b part[b][d + c]: thread = one float4 column of the 2 d, blockIdx.y = one of
// G groups of partial rows; one fp32 atomic per element per group (G <= 32)
__global__ __launch_bounds__(256) void ln_part_reduce_kernel(const float* __restrict__ part, int nblk, int d,
                                                             float* __restrict__ dw, float* __restrict__ db) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  const int d4 = d >> 2;
  if (k >= 2 * d4) return;
  const int G = gridDim.y;
  const int per = (nblk + G - 1) / G, b0 = blockIdx.y * per, b1 = min(nblk, b0 + per);
  if (b1 <= b0) return;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  int b = b0;
  for (; b + 4 <= b1; b += 4) {  // four independent loads in flight
    const float4 v0 = ((const float4*)(part + (long)b * 2 * d))[k];
    const float4 v1 = ((const float4*)(part + (long)(b + 1) * 2 * d))[k];
    const float4 v2 = ((const float4*)(part + (long)(b + 2) * 2 * d))[k];
    const float4 v3 = ((const float4*)(part + (long)(b + 3) * 2 * d))[k];
    s.x += (v0.x + v1.x) + (v2.x + v3.x);
    s.y += (v0.y + v1.y) + (v2.y + v3.y);
    s.z += (v0.z + v1.z) + (v2.z + v3.z);
    s.w += (v0.w + v1.w) + (v2.w + v3.w);
  }
  for (; b < b1; ++b) {
    const float4 v = ((const float4*)(part + (long)b * 2 * d))[k];
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  float* dst = k < d4 ? dw + 4 * k : db + 4 * (k - d4);
  atomicAdd(dst + 0, s.x);
  atomicAdd(dst + 1, s.y);
  atomicAdd(dst + 2, s.z);
  atomicAdd(dst + 3, s.w);
}

// ============================================================================ launch
// A row pointer with the alignment the vector layout needs of it: 16 B for fp32 rows, 8 B for bf16 rows
struct LnPtr {
  const void* p;
  unsigned align;
};
static inline LnPtr f32_rows(const void* p) { return {p, 16}; }
static inline LnPtr bf16_rows(const void* p) { return {p, 8}; }

// the vector layout (W = 4) applies: d % 4 == 0 and every given pointer aligned (a null pointer is no operand)
static bool ln_vec(int d, std::initializer_list<LnPtr> ptrs) {
  if (d % 4) return false;
  for (const LnPtr& q : ptrs)
    if (((uintptr_t)q.p) & (q.align - 1)) return false;
  return true;
}

// f(W, N) as integral constants for a row of d <= 4096 floats: N = 1, 2, 3, 4, 6, 8, 12, 16 float4 per lane on the
// vector layout, else 4, 16, 32, 64 floats per lane
template <int V>
using ln_int = std::integral_constant<int, V>;
template <class F>
static void ln_dispatch(bool vec, int d, F&& f) {
  const int n = vec ? (d / 4 + 63) / 64 : (d + 63) / 64;
  if (vec) {
    const ln_int<4> W;
    if (n <= 1) f(W, ln_int<1>{}); else if (n <= 2) f(W, ln_int<2>{}); else if (n <= 3) f(W, ln_int<3>{});
    else if (n <= 4) f(W, ln_int<4>{}); else if (n <= 6) f(W, ln_int<6>{}); else if (n <= 8) f(W, ln_int<8>{});
    else if (n <= 12) f(W, ln_int<12>{}); else f(W, ln_int<16>{});
  } else {
    const ln_int<1> W;
    if (n <= 4) f(W, ln_int<4>{}); else if (n <= 16) f(W, ln_int<16>{}); else if (n <= 32) f(W, ln_int<32>{});
    else f(W, ln_int<64>{});
  }
}

// f(std::bool_constant<b>)
template <class F>
static void ln_flag(bool b, F&& f) {
  if (b) f(std::true_type{}); else f(std::false_type{});
}

// ``y32`` (nullable): also writes fp32(y); vector layout only, refused (nothing launched) elsewhere.  ``pos_mask``
// (RowSel): base rows [0, Tb) at positions with their bit set normalise the source row row + Tb.
// ``pf0`` / ``pf1`` (nullable, ``pf*_bytes`` long; whole 4-B words are read) are read into the caches by ``pf_wgs``
// (<= 1024) extra workgroups in front of the row blocks: the weights of the GEMMs that follow.  Without a range or
// with pf_wgs <= 0 the grid is the row blocks alone.
IIT_EXPORT int iit_ln_fwd_pf(const float* x, const float* w, const float* b, void* y, float* y32, float* mean,
                             float* rstd, int T, int d, float eps, unsigned long long pos_mask, int S, int Tb,
                             const void* pf0, long pf0_bytes, const void* pf1, long pf1_bytes, int pf_wgs,
                             void* stream) {
  if (pos_mask && (S <= 0 || S > 64 || 2 * (long)Tb > T)) return (int)hipErrorInvalidValue;
  const bool vec = ln_vec(d, {f32_rows(x), bf16_rows(y), f32_rows(y32), f32_rows(w), f32_rows(b)});
  if (d > 4096 || (y32 && !vec)) return (int)hipErrorInvalidValue;
  const RowSel sel{pos_mask, S > 0 ? S : 1, Tb};
  Prefetch pf{{(const char*)pf0, (const char*)pf1}, {pf0 ? pf0_bytes & ~3L : 0, pf1 ? pf1_bytes & ~3L : 0}, 0};
  if (((uintptr_t)pf0 | (uintptr_t)pf1) & 3) return (int)hipErrorInvalidValue;
  if ((pf.bytes[0] > 0 || pf.bytes[1] > 0) && pf_wgs > 0) pf.wgs = pf_wgs < 1024 ? pf_wgs : 1024;
  ln_dispatch(vec, d, [&](auto W, auto N) {
    hipLaunchKernelGGL((ln_fwd_kernel<W, N>), dim3(pf.wgs + (T + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, w, b,
                       (__bf16*)y, mean, rstd, T, d, eps, sel, y32, pf);
  });
  return hipGetLastError();
}

IIT_EXPORT int iit_ln_fwd(const float* x, const float* w, const float* b, void* y, float* y32, float* mean,
                          float* rstd, int T, int d, float eps, unsigned long long pos_mask, int S, int Tb,
                          void* stream) {
  return iit_ln_fwd_pf(x, w, b, y, y32, mean, rstd, T, d, eps, pos_mask, S, Tb, nullptr, 0, nullptr, 0, 0, stream);
}

// rows per block of the fused affine-gradient backward (the caller sizes ``part`` as blocks x 2 d floats)
IIT_EXPORT int iit_ln_bwd_part_rows() { return 4 * ln_part_r(); }

// Backward over T rows.  ``x_is_xhat16``: ``x`` is the forward's bf16 output of a norm without affine parameters
// (vector layout only, no w / dw / db).  ``pos_mask``: rows at masked positions get dx = dres only and add nothing to
// dw / db.  With ``part`` (ceil(T / iit_ln_bwd_part_rows()) x 2 d floats of scratch) and d <= 1024 on the vector
// layout, dw / db are fused into the dx pass (ln_bwd_part_kernel + ln_part_reduce_kernel); otherwise the dx kernel
// is followed by a dwdb kernel.  ``dy2`` (nullable, fp32 [T, d]) is added to dy by the fused pass only: refused
// elsewhere (the caller sums first).
IIT_EXPORT int iit_ln_bwd(const void* dy, int dy_f32, const void* x, int x_is_xhat16, const float* mean,
                          const float* rstd, const float* w, float* dx, const float* dres, void* dx16, float* dw,
                          float* db, float* part, const float* dy2, int T, int d, int accumulate,
                          unsigned long long pos_mask, int S, void* stream) {
  if (d > 4096 || (pos_mask && (S <= 0 || S > 64))) return (int)hipErrorInvalidValue;
  const LnPtr dyp = dy_f32 ? f32_rows(dy) : bf16_rows(dy), xp = x_is_xhat16 ? bf16_rows(x) : f32_rows(x);
  const bool vec = ln_vec(d, {dyp, xp, f32_rows(dx), f32_rows(dres), f32_rows(w), bf16_rows(dx16)});
  const bool fused = vec && !x_is_xhat16 && part && dw && db && d <= 1024 &&
                     ln_vec(d, {f32_rows(dw), f32_rows(db), f32_rows(part), f32_rows(dy2)});
  if ((dy2 && !fused) || (x_is_xhat16 && (!vec || w || dw || db))) return (int)hipErrorInvalidValue;
  const RowSel sel{pos_mask, S > 0 ? S : 1, T};
  hipStream_t s = (hipStream_t)stream;
  __bf16* d16 = (__bf16*)dx16;
  const float* xf = (const float*)x;
  if (fused && T > 0) {
    const int R = ln_part_r(), nblk = (T + 4 * R - 1) / (4 * R);
    bool launched = false;  // the fused kernel exists for N <= 4 only (d <= 1024, part of ``fused``)
    ln_dispatch(true, d, [&](auto W, auto N) {
      if constexpr (W == 4 && N <= 4)
        ln_flag(dy_f32, [&](auto F32) {
          launched = true;
          auto launch = [&](auto RR) {
            hipLaunchKernelGGL((ln_bwd_part_kernel<N, F32, RR>), dim3(nblk), dim3(256), 0, s, dy, xf, mean, rstd, w, dx,
                               dres, d16, part, T, d, accumulate, sel, dy2);
          };
          if (R == 1) launch(ln_int<1>{});
          else if (R == 4) launch(ln_int<4>{});
          else launch(ln_int<2>{});
        });
    });
    if (!launched) return (int)hipErrorInvalidValue;
    static const int gcap = [] {  // IIT_LN_REDUCE_G: most groups of partial rows (default 32)
      const char* e = getenv("IIT_LN_REDUCE_G");
      const int v = e ? atoi(e) : 32;
      return v >= 1 && v <= 1024 ? v : 32;
    }();
    const int G = max(1, min(gcap, nblk / 8));  // >= ~8 partial rows per thread
    hipLaunchKernelGGL(ln_part_reduce_kernel, dim3((2 * (d / 4) + 255) / 256, G), dim3(256), 0, s, part, nblk, d, dw, db);
    return hipGetLastError();
  }
  dim3 grid((T + 3) / 4), block(256);
  ln_dispatch(vec, d, [&](auto W, auto N) {
    ln_flag(dy_f32, [&](auto F32) {
      ln_flag(x_is_xhat16, [&](auto XH16) {
        if constexpr (W == 4 || !XH16)
          hipLaunchKernelGGL((ln_bwd_kernel<W, N, F32, XH16>), grid, block, 0, s, dy, x, mean, rstd, w, dx, dres, d16, T,
                             d, accumulate, sel);
      });
    });
  });
  if (dw) {
    if (ln_vec(d, {dyp, xp, f32_rows(dw), f32_rows(db)})) {
      dim3 g2((d / 4 + 63) / 64, (T + LN_DWDB_ROWS - 1) / LN_DWDB_ROWS);
      ln_flag(dy_f32, [&](auto F32) {
        hipLaunchKernelGGL(ln_dwdb_vec_kernel<F32>, g2, block, 0, s, dy, xf, mean, rstd, dw, db, T, d, sel);
      });
    } else {
      dim3 g2((d + 63) / 64, (T + 255) / 256);
      ln_flag(dy_f32, [&](auto F32) {
        hipLaunchKernelGGL(ln_dwdb_kernel<F32>, g2, block, 0, s, dy, xf, mean, rstd, dw, db, T, d, sel);
      });
    }
  }
  return hipGetLastError();
}
