"""Helpers shared by the exact-fp32 convolution tests (tests/test_conv_f32_kernel.py and tests/test_conv_f32_ops.py on
the GPU, tests/test_conv_f32_ref.py on the CPU): shapes, float64 references written as the kernels' index arithmetic,
operand families, comparators and the wrong convolutions a comparator must flag.

A shape is ``(N, H, W, Cin, Cout, k, s, pad)``; tensors are dense NHWC: ``x [N][H][W][Cin]``, ``w [Cout][k][k][Cin]``,
``dy [N][OH][OW][Cout]``.  Every pass is the product ``A [M][K] @ B [K][N]`` of two matrices gathered by index
arithmetic (:func:`gemm_operands`), and its ``[M][N]`` result is the pass's dense output: ``y``, ``dx`` or ``dw``.

The exact families reuse the ranges of tests/gemm_f32_util.py, the wide operand always on the side a reduction sees
at most once per index so that every partial sum stays below 2^24 (:func:`worst_sum`, asserted per shape and pass in
:func:`tensors`):

* ``F1``: |a| <= 3, |b| <= 2 -- indexing mistakes.
* ``F2``: |a| <= 4095, |b| <= 3 -- 12-bit operands bf16 cannot hold.
* ``F3``: sparse wide -- the operand that is not gathered by window (``w`` for forward and input gradient, ``dy`` for
  the weight gradient) has at most 3 nonzeros per reduction, each below 2^22; the other is in {-1, 0, 1} -- 22-bit
  operands a bf16 hi + lo split cannot hold.

``REAL`` (standard normal) is compared with ``|got - ref| <= gamma(K, splits) mag``: ``gemm_f32_util.gamma``, ``K`` the
pass's reduction length, ``mag`` the same convolution of absolute values in float64.
"""
import functools

import torch

import gemm_exact_util as U
import gemm_f32_util as F

FWD, DGRAD, WGRAD = 0, 1, 2
PASSES = (FWD, DGRAD, WGRAD)
F1, F2, F3, REAL = F.F1, F.F2, F.F3, F.REAL
EXACT = (F1, F2, F3)
FAMILIES = EXACT + (REAL,)
TILES = {0: (64, 64, 32), 1: (128, 128, 16)}  # tile id -> (BM, BN, BK)

# (N, H, W, Cin, Cout, k, s, pad) -> what it exercises
SHAPES = {
    (2, 5, 7, 8, 12, 3, 1, 1): "non-square input, partial M and N tiles, vector path",
    (2, 6, 6, 4, 8, 3, 2, 1): "stride 2, even extents",
    (1, 7, 5, 4, 4, 3, 2, 1): "stride 2, odd extents",
    (2, 6, 6, 8, 16, 1, 2, 0): "the downsample: rows of dX no window reads",
    (1, 7, 7, 8, 8, 1, 2, 0): "the downsample, odd extents",
    (2, 12, 12, 3, 8, 7, 2, 3): "the stem: scalar path, Cin = 3, K = 147",
    (3, 1, 1, 8, 8, 3, 1, 1): "layer 4 at 1 x 1: only the centre tap is in range",
    (2, 9, 9, 12, 72, 3, 1, 1): "3 x 2 tiles of 64; K-tiles that straddle taps",
    (2, 9, 9, 6, 10, 3, 1, 1): "Cin % 4 != 0, scalar path",
}
SPLIT_SHAPE = (2, 9, 9, 12, 72, 3, 1, 1)


def out_hw(shape):
    N, H, W, Cin, Cout, k, s, pad = shape
    return (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1


def geom(shape):
    """The geometry tuple of ``hip_kernels``: (N, H, W, Cin, OH, OW, Cout, k, s, pad)."""
    N, H, W, Cin, Cout, k, s, pad = shape
    OH, OW = out_hw(shape)
    return (N, H, W, Cin, OH, OW, Cout, k, s, pad)


def mnk(pass_, shape):
    """(M, N, K) of the pass's GEMM."""
    N, H, W, Cin, Cout, k, s, pad = shape
    OH, OW = out_hw(shape)
    if pass_ == FWD:
        return N * OH * OW, Cout, k * k * Cin
    if pass_ == DGRAD:
        return N * H * W, Cin, k * k * Cout
    return Cout, k * k * Cin, N * OH * OW


def vector_path(pass_, shape):
    N, H, W, Cin, Cout, k, s, pad = shape
    return Cin % 4 == 0 and (pass_ == FWD or Cout % 4 == 0)


# ------------------------------------------------------------------------------ gathers, as the kernels index
def im2col(x, k, s, pad, *, gather_pad=None, swap=False):
    """``[N OH OW][k k C]``: row (n, oh, ow), column (kh k + kw) C + c = x[n, oh s - pad + kh, ow s - pad + kw, c],
    zero outside the image.  ``gather_pad`` (an off-by-one pad) and ``swap`` (kh and kw exchanged in the address)
    make the wrong kernels of the CPU test; the output extent is always the true one."""
    N, H, W, C = x.shape
    OH, OW = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    gp = pad if gather_pad is None else gather_pad
    cols = x.new_zeros(N, OH, OW, k, k, C)
    oh, ow = torch.arange(OH), torch.arange(OW)
    for kh in range(k):
        for kw in range(k):
            a, b = (kw, kh) if swap else (kh, kw)
            ih, iw = oh * s - gp + a, ow * s - gp + b
            ok = ((ih >= 0) & (ih < H))[:, None] & ((iw >= 0) & (iw < W))[None, :]
            g = x[:, ih.clamp(0, H - 1)][:, :, iw.clamp(0, W - 1)]
            cols[:, :, :, kh, kw] = torch.where(ok[None, :, :, None], g, torch.zeros_like(g))
    return cols.reshape(N * OH * OW, k * k * C)


def dy_gather(dy, H, W, k, s, pad, *, no_div=False):
    """``[N H W][k k Cout]``: row (n, h, w), column (kh k + kw) Cout + co = dy[n, (h + pad - kh) / s,
    (w + pad - kw) / s, co], zero where a division is not exact or the result is out of range.  ``no_div`` drops the
    divisibility test (a wrong kernel)."""
    N, OH, OW, Co = dy.shape
    out = dy.new_zeros(N, H, W, k, k, Co)
    h, w = torch.arange(H), torch.arange(W)
    for kh in range(k):
        for kw in range(k):
            th, tw = h + pad - kh, w + pad - kw
            okh = (th >= 0) & (th // s < OH) & ((th % s == 0) | no_div)
            okw = (tw >= 0) & (tw // s < OW) & ((tw % s == 0) | no_div)
            g = dy[:, (th // s).clamp(0, OH - 1)][:, :, (tw // s).clamp(0, OW - 1)]
            ok = okh[:, None] & okw[None, :]
            out[:, :, :, kh, kw] = torch.where(ok[None, :, :, None], g, torch.zeros_like(g))
    return out.reshape(N * H * W, k * k * Co)


def weight_taps(w):
    """``[k k Cout][Cin]``: row tap Cout + co, column ci = w[co, kh, kw, ci] (the forward weight read in place)."""
    Cout, k, _, Cin = w.shape
    return w.permute(1, 2, 0, 3).reshape(k * k * Cout, Cin)


def gemm_operands(pass_, shape, x, w, dy, **wrong):
    """``(A [M][K], B [K][N])`` of the pass in the dtype of the tensors; ``wrong``: the keywords of :func:`im2col` /
    :func:`dy_gather`."""
    N, H, W, Cin, Cout, k, s, pad = shape
    if pass_ == FWD:
        return im2col(x, k, s, pad, **wrong), w.reshape(Cout, -1).t()
    if pass_ == DGRAD:
        return dy_gather(dy, H, W, k, s, pad, **wrong), weight_taps(w)
    return dy.reshape(-1, Cout).t(), im2col(x, k, s, pad, **wrong)


def reference(pass_, shape, x, w, dy):
    """float64 value and magnitude sum (the same pass on absolute values) of the pass, ``[M][N]``."""
    a, b = gemm_operands(pass_, shape, x.double(), w.double(), dy.double())
    return a @ b, a.abs() @ b.abs()


def chain_f32(a, b, splits=1, bk=32):
    """fp32 emulation of the stated chain: per split an ascending sum from +0 over its K range (each product rounded,
    then added: two roundings where the fmaf has one), the splits added in order."""
    K = a.shape[1]
    kps = -(-(-(-K // splits)) // bk) * bk
    total = None
    for s in range(splits):
        acc = torch.zeros(a.shape[0], b.shape[1], dtype=torch.float32)
        for kk in range(min(K, s * kps), min(K, (s + 1) * kps)):
            acc = acc + a[:, kk, None] * b[None, kk, :]
        total = acc if total is None else total + acc
    return total


# ------------------------------------------------------------------------------ operand families
def worst_sum(family, pass_, shape):
    """Largest |value| a partial or final sum of the pass can reach on ``family``."""
    K = mnk(pass_, shape)[2]
    if family == F1:
        return U.A_MAX * U.B_MAX * K
    if family == F2:
        return F.F2_A * F.F2_B * K
    return F.F3_WIDE * min(F.F3_NNZ, K)


def _ints(shape, bound, g):
    return torch.randint(-bound, bound + 1, shape, generator=g).float()


def _sparse(shape, g):
    """Integers below 2^22 in magnitude, at most ``F3_NNZ`` nonzeros for each index of the first dimension."""
    n = 1
    for d in shape[1:]:
        n *= d
    return F._sparse_wide(shape[0], n, g).reshape(shape)


@functools.lru_cache(maxsize=None)
def tensors(family, pass_, shape, seed=0):
    """``(x, w, dy)`` NHWC fp32 on the CPU for one pass; the tensor the pass does not read is zeros."""
    N, H, W, Cin, Cout, k, s, pad = shape
    OH, OW = out_hw(shape)
    g = torch.Generator().manual_seed(1000 * seed + 10 * (hash(shape) % 97) + pass_)
    xs, ws, ys = (N, H, W, Cin), (Cout, k, k, Cin), (N, OH, OW, Cout)
    if family in EXACT:
        assert worst_sum(family, pass_, shape) < F.LIMIT, (family, pass_, shape)
    x, w, dy = torch.zeros(xs), torch.zeros(ws), torch.zeros(ys)
    if family == REAL:
        x, w, dy = (torch.randn(t, generator=g) for t in (xs, ws, ys))
    elif family in (F1, F2):
        wide, small = (U.A_MAX, U.B_MAX) if family == F1 else (F.F2_A, F.F2_B)
        if pass_ == FWD:
            x, w = _ints(xs, wide, g), _ints(ws, small, g)
        elif pass_ == DGRAD:
            dy, w = _ints(ys, wide, g), _ints(ws, small, g)
        else:
            dy, x = _ints(ys, wide, g), _ints(xs, small, g)
    elif pass_ == FWD:  # F3: at most 3 wide weights per output channel
        x, w = _ints(xs, 1, g), _sparse(ws, g)
    elif pass_ == DGRAD:  # at most 3 wide weights per input channel
        dy, w = _ints(ys, 1, g), _sparse((Cin, Cout, k, k), g).permute(1, 2, 3, 0).contiguous()
    else:  # at most 3 wide output gradients per output channel
        x, dy = _ints(xs, 1, g), _sparse((Cout, N, OH, OW), g).permute(1, 2, 3, 0).contiguous()
    return x, w, dy


@functools.lru_cache(maxsize=None)
def expected(family, pass_, shape, seed=0):
    """``(ref, mag)`` of :func:`tensors`' data, computed once."""
    return reference(pass_, shape, *tensors(family, pass_, shape, seed))


# ------------------------------------------------------------------------------ comparators
def bad(family, got, ref, mag, K, splits=1):
    """Elements of ``got [M][N]`` (fp32) the family's comparator rejects: bitwise for the exact families, the
    ``gamma(K, splits) mag`` bound for ``REAL``."""
    if family in EXACT:
        return U.bad_f32(got, ref)
    return F.bad_real(got, ref, mag, K, splits)
