// Exact-fp32 implicit-GEMM convolutions for gfx950 (MI355X): forward, input gradient and weight gradient of a dense
// NHWC fp32 convolution on gemm_f32.hip's tile images and a copy of its main loop (gemm_f32_body.h), one or both
// operands gathered.
//
//   x [N][H][W][Cin]    w [Cout][k][k][Cin] (the memory of a channels-last [Cout, Cin, k, k] parameter)
//   y [N][OH][OW][Cout] OH = (H + 2 pad - k) / s + 1, OW likewise
//   square kernel 1 <= k <= 7, stride 1 or 2, 0 <= pad < k, no dilation, groups or bias, any N, H, W, Cin, Cout >= 1.
//
// * forward (pass 0): Y [P = N OH OW][Cout] = im2col(x) W^T, reduction index kk = (kh k + kw) Cin + ci.  A row p =
//   (n, oh, ow) reads pixel (n, oh s - pad + kh, ow s - pad + kw), zeros outside the image; B is w as stored.
// * input gradient (pass 1): dX [N H W][Cin], reduction index (kh k + kw) Cout + co.  A is gathered from dY at
//   ((h + pad - kh) / s, (w + pad - kw) / s), zero where a division is not exact or the result is out of range; B is
//   the forward weight read in place (element (tap, co, ci) at co k k Cin + tap Cin + ci).  Every element of dX is
//   written: pixels no forward window reads get +0.
// * weight gradient (pass 2): dW [Cout][k k Cin], reduced over the P output pixels in ascending order; A = dY
//   (k-major, [P][Cout]), B = the im2col columns gathered k-major from x.
// * Arithmetic: the contract of gemm_f32.hip.  Nothing is rounded below fp32; each output of one K range is a single
//   ascending fmaf chain from +0; padding and inexact taps enter as zero operands; split-K is the same scheme
//   (ws[splits][M][N], partials added in split order by a second kernel; no atomics, tickets or fences), so results
//   are bit-identical run to run and between eager and graph replay.
// * Gather: register-staged loads into the F32Tile LDS images.  float4 chunks when the channel counts the pass reads
//   along (Cin forward; Cin and Cout for the gradients) are multiples of 4 and both operand bases are 16-byte
//   aligned -- a chunk then never straddles a tap -- else one float per element (the stem's Cin = 3).  What a thread
//   keeps across K-tiles is decomposed once before the main loop: the row -> (n, oh, ow) split for forward and input
//   gradient, the column -> (tap, ci) split for the weight gradient.
// * Nothing is read or written outside the three tensors and the workspace: every load is guarded by its own range
//   test and every store by row < M, col < N.
#include "gemm_f32_body.h"

namespace {

struct ConvGeom {
  int N, H, W, Cin, OH, OW, Cout, k, s, pad;
};

struct ConvF32Args {
  const float* a;  // forward: x; input gradient: dy; weight gradient: dy
  const float* b;  // forward: w; input gradient: w;  weight gradient: x
  float* out;      // [M][N] dense
  float* ws;       // [splits][M][N] when splits > 1
  ConvGeom g;
  int M, Nn, K;
  int k_per_split, splits;
};

// ---------------------------------------------------------------------------- operand sources
// A source names one operand element by a part a thread keeps across K-tiles (``Fixed``: a row of the LDS image)
// and a part that moves with k (``Var``).  ``addr`` is the element's address, or null for a zero operand.
struct Pix {  // an output pixel of the forward: its image's first pixel index (-1: no such row) and window origin
  int pix0, ih0, iw0;
};
struct Tap {  // a reduction index of the forward: (kh, kw, channel); c = -1: no such column
  int kh, kw, c;
};

struct Im2col {
  const float* x;
  int H, W, C, k, s, pad, OH, OW, P, K;
  __device__ __forceinline__ Pix pix(int p) const {
    if (p >= P) return Pix{-1, 0, 0};
    const int n = p / (OH * OW), r = p - n * (OH * OW);
    const int oh = r / OW, ow = r - oh * OW;
    return Pix{n * H * W, oh * s - pad, ow * s - pad};
  }
  __device__ __forceinline__ Tap tap(int kk) const {
    if (kk >= K) return Tap{0, 0, -1};
    const int t = kk / C, kh = t / k;
    return Tap{kh, t - kh * k, kk - t * C};
  }
  __device__ __forceinline__ void next(Tap& t) const {
    if (++t.c == C) {
      t.c = 0;
      if (++t.kw == k) {
        t.kw = 0;
        ++t.kh;
      }
    }
  }
  __device__ __forceinline__ const float* addr(const Pix& p, const Tap& t) const {
    const int ih = p.ih0 + t.kh, iw = p.iw0 + t.kw;
    if (p.pix0 < 0 || t.c < 0 || ih < 0 || ih >= H || iw < 0 || iw >= W) return nullptr;
    return x + (long)(p.pix0 + ih * W + iw) * C + t.c;
  }
};

struct ImRows : Im2col {  // forward A: row = output pixel, k = (tap, ci)
  using Fixed = Pix;
  using Var = Tap;
  __device__ __forceinline__ Fixed fix(int row) const { return pix(row); }
  __device__ __forceinline__ Var var(int kk) const { return tap(kk); }
  __device__ __forceinline__ void step(Var& v) const { next(v); }
  __device__ __forceinline__ const float* at(const Fixed& f, const Var& v) const { return addr(f, v); }
};

struct ImCols : Im2col {  // weight-gradient B: row = (tap, ci) column, k = output pixel
  using Fixed = Tap;
  using Var = Pix;
  __device__ __forceinline__ Fixed fix(int row) const { return tap(row); }
  __device__ __forceinline__ Var var(int p) const { return pix(p); }
  __device__ __forceinline__ void step(Var&) const {}
  __device__ __forceinline__ const float* at(const Fixed& f, const Var& v) const { return addr(v, f); }
};

struct DyRows {  // input-gradient A: row = input pixel (n, h, w), k = (tap, co)
  const float* dy;
  int H, W, C, k, s, pad, OH, OW, rows, K;  // C = Cout
  struct Fixed {
    int pix0, hp, wp;  // n OH OW (-1: no such row), h + pad, w + pad
  };
  using Var = Tap;
  __device__ __forceinline__ Fixed fix(int m) const {
    if (m >= rows) return Fixed{-1, 0, 0};
    const int n = m / (H * W), r = m - n * (H * W);
    const int h = r / W, w = r - h * W;
    return Fixed{n * OH * OW, h + pad, w + pad};
  }
  __device__ __forceinline__ Var var(int kk) const {
    const int t = kk / C, kh = t / k;
    return Tap{kh, t - kh * k, kk - t * C};
  }
  __device__ __forceinline__ void step(Var& t) const {
    if (++t.c == C) {
      t.c = 0;
      if (++t.kw == k) {
        t.kw = 0;
        ++t.kh;
      }
    }
  }
  __device__ __forceinline__ const float* at(const Fixed& f, const Var& t) const {
    const int th = f.hp - t.kh, tw = f.wp - t.kw;
    if (f.pix0 < 0 || th < 0 || tw < 0 || ((th | tw) & (s - 1))) return nullptr;  // s is 1 or 2
    const int oh = th >> (s - 1), ow = tw >> (s - 1);
    if (oh >= OH || ow >= OW) return nullptr;
    return dy + (long)(f.pix0 + oh * OW + ow) * C + t.c;
  }
};

struct WRows {  // forward B: w [Cout][K] as stored; row = co, k = kk
  const float* w;
  int rows, K;
  using Fixed = long;  // co K, -1: no such row
  using Var = int;
  __device__ __forceinline__ Fixed fix(int co) const { return co < rows ? (long)co * K : -1; }
  __device__ __forceinline__ Var var(int kk) const { return kk; }
  __device__ __forceinline__ void step(Var& v) const { ++v; }
  __device__ __forceinline__ const float* at(const Fixed& f, const Var& v) const { return f < 0 ? nullptr : w + f + v; }
};

struct WTaps {  // input-gradient B: the forward weight in place; row = ci, k = (tap, co)
  const float* w;
  int Cin, Cout, KC;  // KC = k k Cin
  using Fixed = int;  // ci, -1: no such row
  using Var = long;   // co k k Cin + tap Cin
  __device__ __forceinline__ Fixed fix(int ci) const { return ci < Cin ? ci : -1; }
  __device__ __forceinline__ Var var(int kk) const {
    const int t = kk / Cout, co = kk - t * Cout;
    return (long)co * KC + (long)t * Cin;
  }
  __device__ __forceinline__ void step(Var&) const {}
  __device__ __forceinline__ const float* at(const Fixed& f, const Var& v) const { return f < 0 ? nullptr : w + v + f; }
};

struct DyCols {  // weight-gradient A: dy [P][Cout] k-major; row = co, k = output pixel
  const float* dy;
  int Cout;
  using Fixed = int;  // co, -1: no such row
  using Var = long;   // p Cout
  __device__ __forceinline__ Fixed fix(int co) const { return co < Cout ? co : -1; }
  __device__ __forceinline__ Var var(int p) const { return (long)p * Cout; }
  __device__ __forceinline__ void step(Var&) const {}
  __device__ __forceinline__ const float* at(const Fixed& f, const Var& v) const { return f < 0 ? nullptr : dy + v + f; }
};

// ---------------------------------------------------------------------------- the gathering stager
// Fills the registers of an F32Tile from a source.  A thread's chunks share their k offset (k-contiguous image: one
// row per chunk) or their four rows (k-major image), so the fixed parts are decomposed once in ``init``.
template <class Src, bool KMAJ, int ROWS, int BK, bool VEC>
struct F32Gather {
  using Tile = F32Tile<KMAJ, ROWS, BK>;
  static constexpr int NFIX = KMAJ ? (VEC ? 1 : 4) : Tile::PER_THREAD;
  static_assert(256 % (ROWS / 4) == 0 && 256 % (BK / 4) == 0, "a thread's chunks must share a row group / k offset");
  Tile t;
  Src src;
  typename Src::Fixed fx[NFIX];

  __device__ __forceinline__ void init(const Src& s, int row0, int tid) {
    src = s;
#pragma unroll
    for (int i = 0; i < NFIX; ++i) {
      int row, k;
      Tile::where(KMAJ ? tid : tid + i * 256, row, k);
      fx[i] = src.fix(row0 + row + (KMAJ ? i : 0));
    }
  }

  __device__ __forceinline__ void load(int k0, int kend, int tid) {
#pragma unroll
    for (int i = 0; i < Tile::PER_THREAD; ++i) {
      int row, k;
      Tile::where(tid + i * 256, row, k);
      k += k0;
      float e[4] = {0.f, 0.f, 0.f, 0.f};
      if (k < kend) {
        typename Src::Var v = src.var(k);
        if (VEC) {  // 4 | channels and 4 | k (or 4 | row): the chunk is inside one tap and one image row
          const float* p = src.at(fx[KMAJ ? 0 : i], v);
          if (p) {
            const float4 q = *(const float4*)p;
            e[0] = q.x; e[1] = q.y; e[2] = q.z; e[3] = q.w;
          }
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (KMAJ || k + j < kend) {
              const float* p = src.at(fx[KMAJ ? j : i], v);
              if (p) e[j] = *p;
            }
            if (!KMAJ) src.step(v);
          }
        }
      }
      t.r[i] = make_float4(e[0], e[1], e[2], e[3]);
    }
  }

  __device__ __forceinline__ void store(float* lds, int tid) const { t.store(lds, tid); }
};

// ---------------------------------------------------------------------------- the passes
template <int PASS>
struct ConvPass;

template <>
struct ConvPass<0> {  // forward
  using SrcA = ImRows;
  using SrcB = WRows;
  static constexpr bool AKM = false, BKM = false;
  static __device__ __forceinline__ SrcA a(const ConvF32Args& p) {
    const ConvGeom& g = p.g;
    return SrcA{{p.a, g.H, g.W, g.Cin, g.k, g.s, g.pad, g.OH, g.OW, p.M, p.K}};
  }
  static __device__ __forceinline__ SrcB b(const ConvF32Args& p) { return SrcB{p.b, p.Nn, p.K}; }
};

template <>
struct ConvPass<1> {  // input gradient
  using SrcA = DyRows;
  using SrcB = WTaps;
  static constexpr bool AKM = false, BKM = true;
  static __device__ __forceinline__ SrcA a(const ConvF32Args& p) {
    const ConvGeom& g = p.g;
    return SrcA{p.a, g.H, g.W, g.Cout, g.k, g.s, g.pad, g.OH, g.OW, p.M, p.K};
  }
  static __device__ __forceinline__ SrcB b(const ConvF32Args& p) {
    return SrcB{p.b, p.g.Cin, p.g.Cout, p.g.k * p.g.k * p.g.Cin};
  }
};

template <>
struct ConvPass<2> {  // weight gradient
  using SrcA = DyCols;
  using SrcB = ImCols;
  static constexpr bool AKM = true, BKM = true;
  static __device__ __forceinline__ SrcA a(const ConvF32Args& p) { return SrcA{p.a, p.g.Cout}; }
  static __device__ __forceinline__ SrcB b(const ConvF32Args& p) {
    const ConvGeom& g = p.g;
    return SrcB{{p.b, g.H, g.W, g.Cin, g.k, g.s, g.pad, g.OH, g.OW, p.K, p.Nn}};
  }
};

template <int BM, int BN, int BK, int PASS, bool VEC>
__global__ __launch_bounds__(256) void conv_f32_kernel(ConvF32Args p) {
  using CP = ConvPass<PASS>;
  using GA = F32Gather<typename CP::SrcA, CP::AKM, BM, BK, VEC>;
  using GB = F32Gather<typename CP::SrcB, CP::BKM, BN, BK, VEC>;
  using LA = typename GA::Tile;
  using LB = typename GB::Tile;
  __shared__ __attribute__((aligned(16))) float smem[f32_smem_elems<LA, LB>()];

  const int tid = threadIdx.x;
  const int tiles_n = (p.Nn + BN - 1) / BN, tiles_m = (p.M + BM - 1) / BM;
  const int t = xcd_remap_f32(blockIdx.x, tiles_n * tiles_m);
  const int m0 = (t / tiles_n) * BM, n0 = (t % tiles_n) * BN;
  const int split = blockIdx.y;
  const long kb = (long)split * p.k_per_split;
  const int kbeg = kb < p.K ? (int)kb : p.K;
  const int kend = kb + p.k_per_split < p.K ? (int)(kb + p.k_per_split) : p.K;

  f32x4 acc[BM / 32][BN / 32];
#pragma unroll
  for (int i = 0; i < BM / 32; ++i)
#pragma unroll
    for (int j = 0; j < BN / 32; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  GA ga;
  GB gb;
  ga.init(CP::a(p), m0, tid);
  gb.init(CP::b(p), n0, tid);
  f32_main_loop<BM, BN, BK, LA, LB>(smem, ga, gb, kbeg, kend, tid, acc);

  float* dst = p.splits > 1 ? p.ws + (long)split * p.M * p.Nn : p.out;
  const int ld = p.Nn;
  f32_for_each_out<BM, BN>(acc, m0, n0, p.M, p.Nn, tid,
                           [dst, ld](int row, int col, float v) { dst[(long)row * ld + col] = v; });
}

// sums the partial tiles ws[s][M][N] in split order; one element per thread
__global__ __launch_bounds__(256) void conv_f32_reduce_kernel(ConvF32Args p) {
  const long total = (long)p.M * p.Nn;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  p.out[idx] = f32_split_sum(p.ws, p.splits, total, idx);
}

template <int BM, int BN, int BK, int PASS>
hipError_t launch_vec(const ConvF32Args& a, bool vec, hipStream_t s) {
  dim3 grid(cdiv(a.M, BM) * cdiv(a.Nn, BN), a.splits);
  if (vec) hipLaunchKernelGGL((conv_f32_kernel<BM, BN, BK, PASS, true>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((conv_f32_kernel<BM, BN, BK, PASS, false>), grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

template <int BM, int BN, int BK>
hipError_t launch_pass(const ConvF32Args& a, int pass, bool vec, hipStream_t s) {
  switch (pass) {
    case 0: return launch_vec<BM, BN, BK, 0>(a, vec, s);
    case 1: return launch_vec<BM, BN, BK, 1>(a, vec, s);
    default: return launch_vec<BM, BN, BK, 2>(a, vec, s);
  }
}

constexpr long INT_LIMIT = 2147483647L;

// the product of the extents, or -1 once it leaves int
inline long extent(std::initializer_list<int> dims) {
  long v = 1;
  for (int d : dims) {
    v *= d;
    if (v > INT_LIMIT) return -1;
  }
  return v;
}

void gemm_extents(int pass, const ConvGeom& g, int& M, int& N, int& K);

bool geometry_ok(int pass, const ConvGeom& g, int tile, int splits) {
  if (pass < 0 || pass > 2 || tile < 0 || tile > 1 || splits < 1 || splits > 64) return false;
  if (g.N < 1 || g.H < 1 || g.W < 1 || g.Cin < 1 || g.Cout < 1) return false;
  if (g.k < 1 || g.k > 7 || (g.s != 1 && g.s != 2) || g.pad < 0 || g.pad >= g.k) return false;
  if ((long)g.H + 2 * g.pad < g.k || (long)g.W + 2 * g.pad < g.k) return false;
  if (g.OH != (g.H + 2 * g.pad - g.k) / g.s + 1 || g.OW != (g.W + 2 * g.pad - g.k) / g.s + 1) return false;
  if (extent({g.N, g.H, g.W, g.Cin}) < 0 || extent({g.N, g.OH, g.OW, g.Cout}) < 0 ||
      extent({g.Cout, g.k, g.k, g.Cin}) < 0 || extent({g.k, g.k, g.Cout}) < 0)
    return false;
  // a tile-rounded row, column or k index stays inside int as well
  int M, Nn, K;
  gemm_extents(pass, g, M, Nn, K);
  return M <= INT_LIMIT - 128 && Nn <= INT_LIMIT - 128 && K <= INT_LIMIT - 128;
}

// M, N, K of the pass's GEMM
void gemm_extents(int pass, const ConvGeom& g, int& M, int& N, int& K) {
  if (pass == 0) {
    M = g.N * g.OH * g.OW; N = g.Cout; K = g.k * g.k * g.Cin;
  } else if (pass == 1) {
    M = g.N * g.H * g.W; N = g.Cin; K = g.k * g.k * g.Cout;
  } else {
    M = g.Cout; N = g.k * g.k * g.Cin; K = g.N * g.OH * g.OW;
  }
}

// the channel counts the pass reads along allow float4 chunks (the launch also needs 16-byte aligned bases)
bool vector_geometry(int pass, const ConvGeom& g) {
  return g.Cin % 4 == 0 && (pass == 0 || g.Cout % 4 == 0);
}

int launch_conv(int pass, const void* a, const void* b, void* out, void* ws, const ConvGeom& g, int tile, int splits,
                void* stream) {
  hipStream_t s = (hipStream_t)stream;
  ConvF32Args p;
  p.a = (const float*)a; p.b = (const float*)b; p.out = (float*)out; p.ws = (float*)ws;
  p.g = g;
  gemm_extents(pass, g, p.M, p.Nn, p.K);
  p.splits = splits;
  const int bk = tile == 1 ? 16 : 32;
  p.k_per_split = cdiv(cdiv(p.K, splits), bk) * bk;
  const bool vec = vector_geometry(pass, g) && aligned16(a) && aligned16(b);
  hipError_t rc = tile == 1 ? launch_pass<128, 128, 16>(p, pass, vec, s) : launch_pass<64, 64, 32>(p, pass, vec, s);
  if (rc != hipSuccess || splits == 1) return (int)rc;
  hipLaunchKernelGGL(conv_f32_reduce_kernel, dim3(cdiv((long)p.M * p.Nn, 256)), dim3(256), 0, s, p);
  return (int)hipGetLastError();
}

}  // namespace

// tile ids: 0 = 64 x 64 (K-tile 32), 1 = 128 x 128 (K-tile 16).  pass: 0 forward, 1 input gradient, 2 weight
// gradient; x, w, y are the tensors of those shapes whichever of them the pass writes.
// 1 when the kernels cover the problem: non-null 4-byte aligned pointers, a geometry of the list in this file's
// header with OH, OW as its formula gives them, a tile in {0, 1}, 1..64 splits with -- when splits > 1 -- a 16-byte
// aligned workspace, and no tensor extent (nor the workgroup grid's) beyond int.
IIT_EXPORT int iit_conv_f32_ok(int pass, const void* x, const void* w, const void* y, const void* ws, int N, int H,
                               int W, int Cin, int OH, int OW, int Cout, int k, int s, int pad, int tile, int splits) {
  if (!x || !w || !y || ((uintptr_t)x & 3) || ((uintptr_t)w & 3) || ((uintptr_t)y & 3)) return 0;
  if (!geometry_ok(pass, ConvGeom{N, H, W, Cin, OH, OW, Cout, k, s, pad}, tile, splits)) return 0;
  if (splits > 1 && (!ws || !aligned16(ws))) return 0;
  return 1;
}

// pure host: out = {M, N, K, k_per_split, grid.x, vector-path flag} of the launch the pass would make (the flag from
// the geometry; a launch also needs 16-byte aligned operand bases to take the float4 path).  0 on success.
IIT_EXPORT int iit_conv_f32_plan(int pass, int N, int H, int W, int Cin, int OH, int OW, int Cout, int k, int s,
                                 int pad, int tile, int splits, int* out) {
  const ConvGeom g{N, H, W, Cin, OH, OW, Cout, k, s, pad};
  if (!out || !geometry_ok(pass, g, tile, splits)) return (int)hipErrorInvalidValue;
  int M, Nn, K;
  gemm_extents(pass, g, M, Nn, K);
  const int bk = tile == 1 ? 16 : 32, bm = tile == 1 ? 128 : 64;
  out[0] = M; out[1] = Nn; out[2] = K;
  out[3] = cdiv(cdiv(K, splits), bk) * bk;
  out[4] = cdiv(M, bm) * cdiv(Nn, bm);
  out[5] = vector_geometry(pass, g) ? 1 : 0;
  return 0;
}

// each launches on ``stream``; no host synchronisation, no allocation.  ``ws``: splits * M * N floats of the pass's
// GEMM (iit_conv_f32_plan) when splits > 1.
IIT_EXPORT int iit_conv_f32_fwd(const void* x, const void* w, void* y, void* ws, int N, int H, int W, int Cin, int OH,
                                int OW, int Cout, int k, int s, int pad, int tile, int splits, void* stream) {
  if (!iit_conv_f32_ok(0, x, w, y, ws, N, H, W, Cin, OH, OW, Cout, k, s, pad, tile, splits))
    return (int)hipErrorInvalidValue;
  return launch_conv(0, x, w, y, ws, ConvGeom{N, H, W, Cin, OH, OW, Cout, k, s, pad}, tile, splits, stream);
}

IIT_EXPORT int iit_conv_f32_dgrad(const void* dy, const void* w, void* dx, void* ws, int N, int H, int W, int Cin,
                                  int OH, int OW, int Cout, int k, int s, int pad, int tile, int splits,
                                  void* stream) {
  if (!iit_conv_f32_ok(1, dx, w, dy, ws, N, H, W, Cin, OH, OW, Cout, k, s, pad, tile, splits))
    return (int)hipErrorInvalidValue;
  return launch_conv(1, dy, w, dx, ws, ConvGeom{N, H, W, Cin, OH, OW, Cout, k, s, pad}, tile, splits, stream);
}

IIT_EXPORT int iit_conv_f32_wgrad(const void* x, const void* dy, void* dw, void* ws, int N, int H, int W, int Cin,
                                  int OH, int OW, int Cout, int k, int s, int pad, int tile, int splits,
                                  void* stream) {
  if (!iit_conv_f32_ok(2, x, dw, dy, ws, N, H, W, Cin, OH, OW, Cout, k, s, pad, tile, splits))
    return (int)hipErrorInvalidValue;
  return launch_conv(2, dy, x, dw, ws, ConvGeom{N, H, W, Cin, OH, OW, Cout, k, s, pad}, tile, splits, stream);
}
