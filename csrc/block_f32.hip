// The fp32 glue of a GPT-2-family block for gfx950 (MI355X): LayerNorm forward / backward on fp32 rows and the
// gelu_new derivative, for the ``hip32n`` backend.  Nothing is rounded to bf16, nothing is an atomic, every sum has
// one fixed order, so the results are bit-identical run to run and between eager launches and a graph replay.
//
// * LayerNorm forward: one wave64 per row, four rows per 256-thread block.  Three passes over the row (the second
//   and third hit the cache): sum -> mean = sum / d; the centred sum of squares q = sum fma(c, c, q), c = x - mean
//   -> rstd = 1 / sqrt(q / d + eps); y = (x - mean) * rstd, with w and b y = fma(y, w, b).
//   A lane adds its own elements in index order (lane, lane + 64, ...; the four floats of a float4 in order), then
//   the 64 lanes meet in the xor butterfly of wave_sum: one order for a given (d, layout).
// * LayerNorm backward: a block covers LN_PART_ROWS rows.  Phase 1, wave per row: xhat = (x - mean) * rstd,
//   g = dy * w (dy without w), s1 = sum g, s2 = sum fma(g, xhat, s2), m1 = s1 / d, m2 = s2 / d,
//   dx = rstd * fma(-xhat, m2, g - m1).  Phase 2 (dw / db asked for), thread per column: the block's rows in row
//   order, pw = fma(dy, xhat, pw), pb = pb + dy, stored to part[block][2][d].  A second kernel adds the partials of
//   a column in block order and stores dw / db; the kernel boundary is the only ordering device.
// * Layouts: float4 lanes when d % 4 == 0 and every base and row pitch is 16-byte aligned, else one float per lane.
//   Both compute each row sum in their own fixed order.  Phase 2 and the partial sums are one float per thread.
// * dgelu: dpre = dpost * gelu_new'(pre) over n contiguous floats; float4 with a scalar tail when the three bases
//   are 16-byte aligned, else one float per thread.
#include "common.h"

namespace {

constexpr int LN_MAX_D = 4096;
constexpr int LN_PART_ROWS = 32;  // rows per block of the backward (8 per wave)

__device__ __forceinline__ float add4(float acc, float4 v) { return (((acc + v.x) + v.y) + v.z) + v.w; }

template <bool VEC>
__global__ __launch_bounds__(256) void ln_f32_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ b, float* __restrict__ y,
                                                         float* __restrict__ mean, float* __restrict__ rstd, int T,
                                                         int d, long ldx, long ldy, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= T) return;
  const float* xr = x + (long)row * ldx;
  float* yr = y + (long)row * ldy;
  const int n = VEC ? d >> 2 : d;  // items per row

  float s = 0.f;
  for (int i = lane; i < n; i += 64) {
    if (VEC) s = add4(s, ((const float4*)xr)[i]);
    else s = s + xr[i];
  }
  const float mu = wave_sum(s) / (float)d;

  float q = 0.f;
  for (int i = lane; i < n; i += 64) {
    if (VEC) {
      const float4 v = ((const float4*)xr)[i];
      float c = v.x - mu; q = __builtin_fmaf(c, c, q);
      c = v.y - mu; q = __builtin_fmaf(c, c, q);
      c = v.z - mu; q = __builtin_fmaf(c, c, q);
      c = v.w - mu; q = __builtin_fmaf(c, c, q);
    } else {
      const float c = xr[i] - mu;
      q = __builtin_fmaf(c, c, q);
    }
  }
  const float rs = 1.f / sqrtf(wave_sum(q) / (float)d + eps);

  for (int i = lane; i < n; i += 64) {
    if (VEC) {
      const float4 v = ((const float4*)xr)[i];
      float4 o = make_float4((v.x - mu) * rs, (v.y - mu) * rs, (v.z - mu) * rs, (v.w - mu) * rs);
      if (w) {
        const float4 wv = ((const float4*)w)[i], bv = ((const float4*)b)[i];
        o.x = __builtin_fmaf(o.x, wv.x, bv.x);
        o.y = __builtin_fmaf(o.y, wv.y, bv.y);
        o.z = __builtin_fmaf(o.z, wv.z, bv.z);
        o.w = __builtin_fmaf(o.w, wv.w, bv.w);
      }
      ((float4*)yr)[i] = o;
    } else {
      float o = (xr[i] - mu) * rs;
      if (w) o = __builtin_fmaf(o, w[i], b[i]);
      yr[i] = o;
    }
  }
  if (lane == 0) {
    mean[row] = mu;
    rstd[row] = rs;
  }
}

struct LnBwdArgs {
  const float* dy;
  const float* x;
  const float* mean;
  const float* rstd;
  const float* w;
  float* dx;
  float* part;
  float* dw;
  float* db;
  long ldx, lddy, lddx;
  int T, d, nblocks;
};

template <bool VEC>
__global__ __launch_bounds__(256) void ln_f32_bwd_kernel(LnBwdArgs p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row0 = blockIdx.x * LN_PART_ROWS;
  const int rows = min(LN_PART_ROWS, p.T - row0);
  const int d = p.d;
  const int n = VEC ? d >> 2 : d;
  const float* w = p.w;

  for (int r = wave; r < rows; r += 4) {
    const int row = row0 + r;
    const float* xr = p.x + (long)row * p.ldx;
    const float* gr = p.dy + (long)row * p.lddy;
    float* dr = p.dx + (long)row * p.lddx;
    const float mu = p.mean[row], rs = p.rstd[row];
    float s1 = 0.f, s2 = 0.f;
    for (int i = lane; i < n; i += 64) {
      if (VEC) {
        const float4 xv = ((const float4*)xr)[i];
        float4 g = ((const float4*)gr)[i];
        if (w) {
          const float4 wv = ((const float4*)w)[i];
          g.x = g.x * wv.x; g.y = g.y * wv.y; g.z = g.z * wv.z; g.w = g.w * wv.w;
        }
        s1 = add4(s1, g);
        s2 = __builtin_fmaf(g.x, (xv.x - mu) * rs, s2);
        s2 = __builtin_fmaf(g.y, (xv.y - mu) * rs, s2);
        s2 = __builtin_fmaf(g.z, (xv.z - mu) * rs, s2);
        s2 = __builtin_fmaf(g.w, (xv.w - mu) * rs, s2);
      } else {
        float g = gr[i];
        if (w) g = g * w[i];
        s1 = s1 + g;
        s2 = __builtin_fmaf(g, (xr[i] - mu) * rs, s2);
      }
    }
    const float m1 = wave_sum(s1) / (float)d;
    const float m2 = wave_sum(s2) / (float)d;
    for (int i = lane; i < n; i += 64) {
      if (VEC) {
        const float4 xv = ((const float4*)xr)[i];
        float4 g = ((const float4*)gr)[i];
        if (w) {
          const float4 wv = ((const float4*)w)[i];
          g.x = g.x * wv.x; g.y = g.y * wv.y; g.z = g.z * wv.z; g.w = g.w * wv.w;
        }
        float4 o;
        o.x = rs * __builtin_fmaf(-((xv.x - mu) * rs), m2, g.x - m1);
        o.y = rs * __builtin_fmaf(-((xv.y - mu) * rs), m2, g.y - m1);
        o.z = rs * __builtin_fmaf(-((xv.z - mu) * rs), m2, g.z - m1);
        o.w = rs * __builtin_fmaf(-((xv.w - mu) * rs), m2, g.w - m1);
        ((float4*)dr)[i] = o;
      } else {
        float g = gr[i];
        if (w) g = g * w[i];
        dr[i] = rs * __builtin_fmaf(-((xr[i] - mu) * rs), m2, g - m1);
      }
    }
  }

  if (!p.dw) return;
  // phase 2 reads only the kernel's inputs, so it needs no barrier after phase 1
  float* pw = p.part + (long)blockIdx.x * 2 * d;
  float* pb = pw + d;
  for (int j = threadIdx.x; j < d; j += 256) {
    float aw = 0.f, ab = 0.f;
    for (int r = 0; r < rows; ++r) {
      const int row = row0 + r;
      const float g = p.dy[(long)row * p.lddy + j];
      const float xh = (p.x[(long)row * p.ldx + j] - p.mean[row]) * p.rstd[row];
      aw = __builtin_fmaf(g, xh, aw);
      ab = ab + g;
    }
    pw[j] = aw;
    pb[j] = ab;
  }
}

// dw[j] / db[j] = the partials of column j added in block order (a plain store)
__global__ __launch_bounds__(256) void ln_f32_bwd_sum_kernel(LnBwdArgs p) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= p.d) return;
  float aw = p.part[j], ab = p.part[p.d + j];
  for (int k = 1; k < p.nblocks; ++k) {
    aw = aw + p.part[(long)k * 2 * p.d + j];
    ab = ab + p.part[(long)k * 2 * p.d + p.d + j];
  }
  p.dw[j] = aw;
  p.db[j] = ab;
}

// items [0, n4) are float4s, items [n4, n4 + tail) the scalar tail; without VEC every item is one float
template <bool VEC>
__global__ __launch_bounds__(256) void dgelu_f32_kernel(const float* __restrict__ dpost, const float* __restrict__ pre,
                                                        float* __restrict__ dpre, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (VEC) {
    const long n4 = n >> 2;
    if (i < n4) {
      const float4 g = ((const float4*)dpost)[i], x = ((const float4*)pre)[i];
      ((float4*)dpre)[i] = make_float4(g.x * gelu_new_grad_f(x.x), g.y * gelu_new_grad_f(x.y),
                                       g.z * gelu_new_grad_f(x.z), g.w * gelu_new_grad_f(x.w));
      return;
    }
    const long e = 4 * n4 + (i - n4);
    if (e < n) dpre[e] = dpost[e] * gelu_new_grad_f(pre[e]);
  } else if (i < n) {
    dpre[i] = dpost[i] * gelu_new_grad_f(pre[i]);
  }
}

inline bool al4(const void* p) { return ((uintptr_t)p & 3) == 0; }
inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

// rows of one block of iit_ln_f32_bwd: ``part`` holds cdiv(T, rows) * 2 * d floats
IIT_EXPORT int iit_ln_f32_part_rows() { return LN_PART_ROWS; }

// fp32 rows x [T][ldx], y [T][ldy] (any 4-byte aligned base, pitches >= d), w and b [d] both or neither,
// mean / rstd [T]; 1 <= d <= 4096, T >= 1
IIT_EXPORT int iit_ln_f32_fwd_ok(const void* x, const void* w, const void* b, const void* y, const void* mean,
                                 const void* rstd, int T, int d, long ldx, long ldy) {
  if (!x || !y || !mean || !rstd || (w == nullptr) != (b == nullptr)) return 0;
  if (!al4(x) || !al4(w) || !al4(b) || !al4(y) || !al4(mean) || !al4(rstd)) return 0;
  if (T < 1 || d < 1 || d > LN_MAX_D || ldx < d || ldy < d) return 0;
  return 1;
}

IIT_EXPORT int iit_ln_f32_fwd(const float* x, const float* w, const float* b, float* y, float* mean, float* rstd,
                              int T, int d, long ldx, long ldy, float eps, void* stream) {
  if (!iit_ln_f32_fwd_ok(x, w, b, y, mean, rstd, T, d, ldx, ldy)) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const bool vec = d % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && al16(x) && al16(y) && al16(w) && al16(b);
  const dim3 grid(cdiv(T, 4)), block(256);
  if (vec) hipLaunchKernelGGL(ln_f32_fwd_kernel<true>, grid, block, 0, s, x, w, b, y, mean, rstd, T, d, ldx, ldy, eps);
  else hipLaunchKernelGGL(ln_f32_fwd_kernel<false>, grid, block, 0, s, x, w, b, y, mean, rstd, T, d, ldx, ldy, eps);
  return (int)hipGetLastError();
}

// dy [T][lddy], x [T][ldx], dx [T][lddx], mean / rstd [T], w [d] or null (LNPre); dw and db [d] both or neither
// (they need w, and ``part``: cdiv(T, iit_ln_f32_part_rows()) * 2 * d floats)
IIT_EXPORT int iit_ln_f32_bwd_ok(const void* dy, const void* x, const void* mean, const void* rstd, const void* w,
                                 const void* dx, const void* part, const void* dw, const void* db, int T, int d,
                                 long ldx, long lddy, long lddx) {
  if (!dy || !x || !mean || !rstd || !dx || (dw == nullptr) != (db == nullptr)) return 0;
  if (dw && (!w || !part)) return 0;
  if (!al4(dy) || !al4(x) || !al4(mean) || !al4(rstd) || !al4(w) || !al4(dx) || !al4(part) || !al4(dw) || !al4(db))
    return 0;
  if (T < 1 || d < 1 || d > LN_MAX_D || ldx < d || lddy < d || lddx < d) return 0;
  return 1;
}

IIT_EXPORT int iit_ln_f32_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* w,
                              float* dx, float* part, float* dw, float* db, int T, int d, long ldx, long lddy,
                              long lddx, void* stream) {
  if (!iit_ln_f32_bwd_ok(dy, x, mean, rstd, w, dx, part, dw, db, T, d, ldx, lddy, lddx))
    return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  LnBwdArgs a;
  a.dy = dy; a.x = x; a.mean = mean; a.rstd = rstd; a.w = w;
  a.dx = dx; a.part = part; a.dw = dw; a.db = db;
  a.ldx = ldx; a.lddy = lddy; a.lddx = lddx;
  a.T = T; a.d = d; a.nblocks = cdiv(T, LN_PART_ROWS);
  const bool vec = d % 4 == 0 && ldx % 4 == 0 && lddy % 4 == 0 && lddx % 4 == 0 && al16(dy) && al16(x) && al16(dx) &&
                   al16(w);
  if (vec) hipLaunchKernelGGL(ln_f32_bwd_kernel<true>, dim3(a.nblocks), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(ln_f32_bwd_kernel<false>, dim3(a.nblocks), dim3(256), 0, s, a);
  hipError_t rc = hipGetLastError();
  if (rc != hipSuccess || !dw) return (int)rc;
  hipLaunchKernelGGL(ln_f32_bwd_sum_kernel, dim3(cdiv(d, 256)), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}

// n >= 1 contiguous floats per operand, any 4-byte aligned bases
IIT_EXPORT int iit_dgelu_f32_ok(const void* dpost, const void* pre, const void* dpre, long n) {
  if (!dpost || !pre || !dpre || !al4(dpost) || !al4(pre) || !al4(dpre)) return 0;
  if (n < 1 || n > (1L << 38)) return 0;
  return 1;
}

IIT_EXPORT int iit_dgelu_f32(const float* dpost, const float* pre, float* dpre, long n, void* stream) {
  if (!iit_dgelu_f32_ok(dpost, pre, dpre, n)) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  if (al16(dpost) && al16(pre) && al16(dpre))
    hipLaunchKernelGGL(dgelu_f32_kernel<true>, dim3(cdiv((n >> 2) + (n & 3), 256)), dim3(256), 0, s, dpost, pre, dpre,
                       n);
  else hipLaunchKernelGGL(dgelu_f32_kernel<false>, dim3(cdiv(n, 256)), dim3(256), 0, s, dpost, pre, dpre, n);
  return (int)hipGetLastError();
}
