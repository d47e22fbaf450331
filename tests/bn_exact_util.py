"""Helpers shared by the exact tests of csrc/bn_nhwc.hip: the fused BatchNorm (+ residual) (+ ReLU) forward and
backward on channels-last bf16 / fp32 rows, both statistics reductions, splice-on-read, the tile-record finalize of
``iit_bn_fwd_tiles`` and the 3x3 / stride-2 max pool (tests/test_bn_exact.py and tests/test_maxpool_exact.py on the
GPU, tests/test_bn_exact_ref.py on the CPU).  Conventions are those of tests/kern_exact_util.py: float64 references of
the same fp32 / bf16 inputs, comparators that return the mask of bad elements (NaN and the buffer sentinel count as
bad), ``E`` = 2^-24, ``U`` = 2^-8, every bound times ``SLACK``.  Activations are handled as rows ``[M, C]`` (M = N H W,
the channels-last memory order); every reference runs on the device of its inputs.

Reduction plan (:func:`bn_plan`, a mirror of ``grid_for``): ``G = C / 8`` threads share a row, ``rpi = 256 / G`` rows
per workgroup pass, ``grid = min(2048, ceil(ceil(M / rpi) / rows))`` workgroups; the thread of the first row adds
``rpt = ceil(M / (grid rpi))`` rows.  One channel's additions on the longest path: ``n = rpt + rpi + ceil(grid / 8) +
8`` (the thread, the LDS combine, the atomics of one of the 8 slots, the slots) with the atomic reduction and ``n = rpt
+ rpi + ceil(grid / 64) + 6`` with the two-level one (a lane's share of the partials, six butterfly levels).

Forward statistics, rounding by rounding after the kernel's pivot algorithm (``p = x'[0][c]``, ``d = x' - p``):

* ``d``: one rounding, ``E |d|``.  ``S1 = sum d`` at depth n: ``tol_S1 = n E sum |d|`` (n - 1 additions and d's own).
  ``S2 = sum fma(d, d, .)``: d's rounding enters squared (2 E), every fma rounds once, all terms are non-negative:
  ``tol_S2 = (n + 2) E sum d^2``.
* ``dm = S1 / M`` (M < 2^24 is exact): ``tol_dm = tol_S1 / M + E |dm|``;  ``mean = p + dm``:
  ``tol_mean = tol_dm + E |mean|``.
* ``var = max(S2 / M - dm^2, 0)``: the division (E msq), the square (E dm^2; none when contracted to an fma -- the
  uncontracted form is the larger bound, so both pass), the subtraction (E var) and dm's error:
  ``tol_var = tol_S2 / M + E msq + (2 |dm| + tol_dm) tol_dm + E dm^2 + E var``, ``msq = E[d^2]``.
* ``rstd = rsqrt(var + eps)``: the addition (E), halved with tol_var by the inverse square root, and the hardware
  rsqrt of 1 ulp = 2 E: ``rel_rstd = (tol_var / (var + eps) + E) / 2 + 2 E``.
* The variance bound therefore carries ``(E[d^2] + dm^2) / var`` = ``1 + 2 (mean - p)^2 / var``: a pivot k standard
  deviations from the mean costs ``(n + 3)(1 + 2 k^2) E / 2`` on rstd.  The ``pivot_outlier`` family tests k = 8 (129
  times the bound of a central pivot); beyond that the pivot algorithm cancels like ``E[x^2] - mean^2`` does.  That is a
  property of the design (the first row is the pivot, whatever it holds), recorded here and not changed; the inputs
  stop at 8.
* ``exact`` family (integers, ``M (2 lim)^2 < 2^24``, :func:`exact_lim`): d, S1 and S2 are exact integers in any
  order, ``tol_S1 = tol_S2 = 0`` and only the finalize roundings remain -- a lost or doubled row is a gross error.
* running statistics: ``unb = var M / (M - 1)`` (two roundings; ``var`` itself at M = 1),
  ``r' = (1 - momentum) r + momentum v``: ``tol = 2 E |(1 - momentum) r| + E |momentum v| + momentum tol_v + E |r'|``
  (``1 - momentum`` and its product, the second product, the sum).  ``num_batches_tracked``: exactly + 1.
* ``y`` end to end against the float64 statistics (not the kernel's ``save``): ``sc = w rstd``
  (``tol_sc = |w| rstd rel_rstd + E |sc|``), ``sh = b - mean sc`` (``E |mean sc|`` absolute, which the ``offset`` family
  makes 1000 times the output, and ``E |sh|``), the fma (``E |v|``), the residual add (``E |v + res|``), the ReLU
  (exact), the bf16 store (``U |y|``).  The errors of sc and mean enter as ``|x - mean| tol_sc + |sc| tol_mean``
  (``x sc' + (b - mean' sc') = (x - mean') sc' + b``).
* eval mode: ``save = (rmean, rsqrt(rvar + eps))``, the mean bitwise and rstd within 2 E relative; ``y`` as above with
  ``tol_mean = 0`` and ``rel_rstd = 2.5 E``; running statistics and ``num_batches_tracked`` bit-unchanged.

Backward.  The reference takes the kernel's ``save`` and saved ``y`` as exact inputs (as the LN backward reference
takes mean and rstd):

* ``dz = dy (y > 0)`` (``dy`` without a saved y); ``dres`` bitwise ``dz`` (a masked element is +0).
* ``coef[0:C] = sum dz``: bitwise in the ``exact`` family, else ``(n + 3) E sum |dz|``;
  ``coef[C:2C] = sum dz xhat``: ``(n + 6) E sum |dz xhat|`` (xhat = (x' - mean) rstd: two roundings, the fma).
* ``dw = dw0 + coef[C:]``, ``db = db0 + coef[:C]``: one more rounding each (``E |dw|``); ``db`` bitwise in the ``exact``
  family when ``db0`` is an integer too.  Null ``dw`` / ``db``: nothing to check.
* training: ``dx = k1 (dz - k2 - xhat k3)``, ``k1 = w rstd``, ``k2 = coef0 fl(1 / M)``, ``k3 = coef1 fl(1 / M)``:
  ``tol_k2 = tol_coef0 / M + 2 E |k2|`` (k3 alike), ``tol_dx = |k1| (tol_k2 + |xhat| tol_k3 + 3 E |xhat k3| +
  E |dz - k2| + E |core|) + 2 E |dx|`` (+ ``U |dx|`` for bf16).  Eval: ``dx = k1 dz``, ``2 E |dx|`` (+ ``U |dx|``).
* spliced elements of ``dx``: exactly +0 (bit pattern).

Tile records (``iit_bn_fwd_tiles``): :func:`tile_records` cuts ``[T R, C]`` into ``(p_t, S1_t, S2_t)`` in float64
rounded to fp32; :func:`tile_ref` combines given fp32 records, taken as exact inputs, in float64 around ``P = p_0``:
``a_t = S1_t + R d_t``, ``q_t = S2_t + d_t (R d_t + 2 S1_t)``, ``d_t = p_t - P``.  ``bn_tile_finalize_kernel`` adds
``nt = ceil(T / 256)`` terms per thread and 8 tree levels: ``tol_S1 = (nt + 9) E sum |a_t| + R E sum |d_t|`` (d's
rounding times R, the fma), ``tol_S2 = (nt + 9) E sum q_t + sum (3 E |d_t (R d_t + 2 S1_t)| + R E d_t^2)`` (the
inner fma, the product, the add, d's rounding through ``dq / dd = (R d + 2 S1) + R d``), then the finalize as above.

Max pool: ``y`` and the tap byte (``kh 3 + kw`` of the full 3x3 window) from ``torch.nn.functional.max_pool2d(...,
return_indices=True)`` on the CPU (:func:`pool_ref_torch`), and from an independent tap scan written from the rule
"first tap in scan order wins, a NaN is taken" (:func:`pool_ref_scan`), both bitwise (any NaN equals any NaN).  The
backward (:func:`pool_bwd_emul`) adds the contributing ``dy`` in ascending ``(kh, kw)`` order in fp32 and rounds once
to the output type: bitwise; an element no window chose is +0.

Measured on an MI355X (the figures per quantity are in the docstring of tests/test_bn_exact.py): no quantity exceeded
its bound; the largest ratios, 0.99, are the bf16 store of ``y`` / ``dx`` and the single rounding of ``p + dm`` where
the sums are exact.

Kernel instantiations of csrc/bn_nhwc.hip and a passing case that runs each (GPU modules):

=========================================  =====================================================================
bn_stats_kernel<false, bf16 / float>       test_bn_exact.py::test_bn_stats[*-bf16-* / *-f32-*], training cases
bn_stats_kernel<true, bf16 / float>        test_bn_exact.py::test_bn_splice[*-bf16-* / *-f32-*], training
bn_finalize_kernel<false, bf16 / float>    test_bn_stats[*-two], training cases
bn_finalize_kernel<true, bf16 / float>     test_bn_splice[*-two], training
bn_apply_kernel<false, bf16 / float>       test_bn_stats (training and eval), test_bn_tiles (bf16)
bn_apply_kernel<true, bf16 / float>        test_bn_splice (training and eval)
bn_bwd_stats_kernel<false, bf16 / float>   test_bn_stats (every case: training and eval)
bn_bwd_stats_kernel<true, bf16 / float>    test_bn_splice
bn_bwd_finalize_kernel                     test_bn_stats[*-two], test_bn_splice[*-two]
bn_bwd_apply_kernel<false, bf16 / float>   test_bn_stats
bn_bwd_apply_kernel<true, bf16 / float>    test_bn_splice (training: hit from load_x; eval: its own branch)
bn_tile_finalize_kernel                    test_bn_exact.py::test_bn_tiles (T = 1 ... 1000)
maxpool3s2_fwd_kernel<bf16 / float>        test_maxpool_exact.py::test_maxpool_fwd_bwd
maxpool3s2_bwd_kernel<bf16 / float>        test_maxpool_exact.py::test_maxpool_fwd_bwd, test_maxpool_bwd_hand_built
IIT_BN_ROWS = 0 / IIT_BN_GRID grid sizing   test_launch_variants.py only (fifth variant, test_bn_stats*)
=========================================  =====================================================================
"""
import math
import os

import torch

from kern_exact_util import E, SLACK, U, bad_bits, bad_bound, filled, gen  # noqa: F401  (re-exported)

F32, BF16 = torch.float32, torch.bfloat16
TPB = 256
BN_SLOTS = 8
BN_EPS = 1e-5
BN_C = [8, 16, 64, 512, 2048]
X_FAMILIES = ["random", "offset", "pivot_outlier", "lowvar", "exact"]
DY_FAMILIES = ["random", "exact"]


def f32(v: float) -> float:
    return float(torch.tensor(v, dtype=F32))


# ================================================================================================ the plan
def _atoi(s: str) -> int:
    """C ``atoi``: optional blanks and sign, then the leading digits (0 without any)."""
    s = s.lstrip(" \t\n\r\f\v")
    sign = 1
    if s[:1] in ("+", "-"):
        sign = -1 if s[0] == "-" else 1
        s = s[1:]
    n = 0
    for ch in s:
        if not ("0" <= ch <= "9"):
            break
        n = 10 * n + ord(ch) - 48
    return sign * n


def env_int(name: str, dflt: int, lo: int, hi: int) -> int:
    """``env_int`` of csrc/bn_nhwc.hip: the variable if it lies in [lo, hi], else the default."""
    e = os.environ.get(name)
    r = _atoi(e) if e is not None else dflt
    return r if lo <= r <= hi else dflt


def rpi_of(C: int) -> int:
    return TPB // (C // 8)


def bn_plan(M: int, C: int, rows=None, target=None) -> dict:
    """``grid_for`` and the addition depths of one channel.  ``rows`` / ``target`` default to ``IIT_BN_ROWS`` (8) and
    ``IIT_BN_GRID`` (1024) with the kernel's clamping."""
    rows = env_int("IIT_BN_ROWS", 8, 0, 256) if rows is None else rows
    target = env_int("IIT_BN_GRID", 1024, 64, 2048) if target is None else target
    assert C >= 8 and C % 8 == 0 and TPB % (C // 8) == 0 and M > 0
    G = C // 8
    rpi = TPB // G
    want = (M + rpi - 1) // rpi
    if rows == 0:
        rows = (want + target - 1) // target
    rows = max(rows, 1)
    grid = min(max((want + rows - 1) // rows, 1), 2048)
    rpt = (M + grid * rpi - 1) // (grid * rpi)
    return {"G": G, "rpi": rpi, "grid": grid, "rpt": rpt,
            "atomic": rpt + rpi + (grid + BN_SLOTS - 1) // BN_SLOTS + BN_SLOTS,
            "two": rpt + rpi + (grid + 63) // 64 + 6}


def bn_rows(C: int):
    """The row counts of the GPU module: idle thread groups, a full group, a second workgroup holding one row, nine
    workgroups (slot 0 used twice) and seventeen."""
    R = rpi_of(C)
    return sorted({m for m in (1, R - 1, R, R + 1, 8 * R + 1, 64 * R + 3, 136 * R - 5) if m >= 1})


# ================================================================================================ operands
def exact_lim(M: int, cap: int = 64) -> int:
    """Largest ``lim <= cap`` with ``M (2 lim)^2 < 2^24``: integers in [-lim, lim] keep the sums of ``x - p`` and
    ``(x - p)^2`` over M rows (and of M integers ``|dy| <= lim``) exact in fp32 in any order."""
    lim = min(cap, int(math.isqrt((2 ** 24 - 1) // (4 * M))))
    assert lim >= 1 and M * (2 * lim) ** 2 < 2 ** 24, (M, lim)
    return lim


def bn_x(family: str, M: int, C: int, dtype, seed: int, lim: int = 0) -> torch.Tensor:
    """Activation rows [M, C] of one operand family (``offset``: fp32 only in the statistics tests; its bf16 form, means
    of 36 to 44, feeds the tile records, whose kernel is bf16 only)."""
    g = gen(seed)
    if family == "exact":
        lim = lim or exact_lim(M)
        assert M * (2 * lim) ** 2 < 2 ** 24 and lim <= 256
        return torch.randint(-lim, lim + 1, (M, C), generator=g).to(dtype)
    if family == "offset":
        mean = 900.0 + 200.0 * torch.rand(C, generator=g)
        if dtype == BF16:  # (the tile records only: 36 to 44, where bf16 still resolves a quarter)
            mean = 36.0 + 0.04 * (mean - 900.0)
        std = 0.5 + torch.rand(C, generator=g)
        return (mean + std * torch.randn(M, C, generator=g)).to(dtype)
    if family == "lowvar":  # a channel constant times (1 + k ulp), |k| <= 3; the last channel exactly constant
        c = (torch.randint(1, 9, (C,), generator=g).double() / 4) * torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0)
        ulp = 2.0 ** -23 if dtype == F32 else 2.0 ** -7
        k = torch.randint(-3, 4, (M, C), generator=g).double()
        k[:, C - 1] = 0
        return (c * (1 + k * ulp)).to(dtype)
    x = 0.3 + 1.5 * torch.randn(M, C, generator=g)
    if family == "pivot_outlier":
        x[0] = 0.3 + 8 * 1.5 * torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0)
    else:
        assert family == "random", family
    return x.to(dtype)


def bn_dy(family: str, M: int, C: int, dtype, seed: int) -> torch.Tensor:
    g = gen(seed + 7000)
    if family == "exact":
        lim = exact_lim(M)
        return torch.randint(-lim, lim + 1, (M, C), generator=g).to(dtype)
    return torch.randn(M, C, generator=g).to(dtype)


def bn_params(C: int, seed: int, exact: bool = False) -> dict:
    """w, b, the running statistics and the gradient prefills (integers for ``exact``)."""
    g = gen(seed + 500)
    out = {"w": (1.0 + 0.5 * torch.randn(C, generator=g)).float(), "b": (0.5 * torch.randn(C, generator=g)).float(),
           "rm": (0.4 * torch.rand(C, generator=g) - 0.2).float(),
           "rv": (0.5 + 1.5 * torch.rand(C, generator=g)).float(),
           "dw0": torch.randn(C, generator=g).float(), "db0": torch.randn(C, generator=g).float()}
    if exact:
        out["db0"] = torch.randint(-9, 10, (C,), generator=g).float()
    return out


# ================================================================================================ splice specs
def spec_dims(shape, ranges, strides):
    """The ``dims`` of an ``iit_amd.ops.splice.PatchSpec`` built by hand: per dimension (size, [(lo, hi), ...],
    source stride in elements)."""
    assert len(shape) == len(ranges) == len(strides) == 4
    for n, runs in zip(shape, ranges):
        assert 1 <= len(runs) <= 8 and all(0 <= lo < hi <= n for lo, hi in runs)
    return [(int(n), [(int(a), int(b)) for a, b in r], int(s)) for n, r, s in zip(shape, ranges, strides)]


def splice_mask(shape, ranges) -> torch.Tensor:
    """bool [N, C, H, W] by plain indexing: the product of the per-dimension unions of ranges."""
    m = torch.ones(shape, dtype=torch.bool)
    for d, (n, runs) in enumerate(zip(shape, ranges)):
        sel = torch.zeros(n, dtype=torch.bool)
        for lo, hi in runs:
            sel[lo:hi] = True
        view = [1, 1, 1, 1]
        view[d] = n
        m = m & sel.view(view)
    return m


def splice_source(shape, layout: str, dtype, seed: int):
    """(storage tensor to hand to the kernel, logical [N, C, H, W] view of it, element strides).  ``nchw``
    contiguous, ``cl`` channels-last, ``bcast`` one [C, H, W] image for every batch element (stride 0)."""
    N, C, H, W = shape
    g = gen(seed + 900)
    if layout == "bcast":
        st = (5.0 + torch.randn(1, C, H, W, generator=g)).to(dtype)
        return st, st.expand(N, C, H, W), (0, H * W, W, 1)
    if layout == "cl":
        st = (5.0 + torch.randn(N, H, W, C, generator=g)).to(dtype)
        return st, st.permute(0, 3, 1, 2), (H * W * C, 1, W * C, C)
    assert layout == "nchw"
    st = (5.0 + torch.randn(N, C, H, W, generator=g)).to(dtype)
    return st, st, (C * H * W, H * W, W, 1)


def rows_of(t4: torch.Tensor) -> torch.Tensor:
    """[N, C, H, W] -> rows [N H W, C] (a copy)."""
    N, C, H, W = t4.shape
    return t4.permute(0, 2, 3, 1).reshape(N * H * W, C).clone()


SPLICE_CASES = [
    # name, (N, C, H, W), ranges per dimension, source layout; row 0 = (n, h, w) = (0, 0, 0) is the pivot row
    ("pivot_out_nchw", (3, 16, 5, 4), [[(1, 3)], [(3, 13)], [(0, 2), (3, 5)], [(0, 1), (2, 3)]], "nchw"),
    ("pivot_in_cl", (3, 16, 5, 4), [[(0, 1), (2, 3)], [(1, 4), (5, 6), (9, 15)], [(0, 3)], [(0, 2)]], "cl"),
    ("pivot_in_bcast", (2, 64, 3, 3), [[(0, 2)], [(3, 13), (20, 21), (41, 63)], [(0, 1), (2, 3)], [(0, 3)]], "bcast"),
    ("pivot_out_three", (2, 64, 3, 3), [[(1, 2)], [(3, 13), (20, 21)], [(1, 3)], [(0, 1), (1, 2), (2, 3)]], "nchw"),
]


def hull8(runs):
    """The defect of a ``hit`` computed per channel group: every channel range widened to its 8-aligned hull."""
    return [(lo // 8 * 8, (hi + 7) // 8 * 8) for lo, hi in runs]


# ================================================================================================ forward
def _finalize(p, s1, tol_s1, s2, tol_s2, M: int, eps: float) -> dict:
    """mean / var / rstd from the pivot sums with their bounds (see the module docstring)."""
    dm = s1 / M
    mean = p + dm
    msq = s2 / M
    var = (msq - dm * dm).clamp(min=0.0)
    tol_dm = tol_s1 / M + E * dm.abs()
    tol_mean = tol_dm + E * mean.abs()
    tol_var = tol_s2 / M + E * msq + (2 * dm.abs() + tol_dm) * tol_dm + E * dm * dm + E * var
    ve = var + eps
    rel_rstd = (tol_var / ve + E) / 2 + 2 * E
    return {"mean": mean, "var": var, "rstd": ve.rsqrt(), "tol_mean": tol_mean, "tol_var": tol_var,
            "rel_rstd": rel_rstd}


def _running(fin: dict, rm0, rv0, M: int, mom: float) -> dict:
    a = 1.0 - mom
    k = M / (M - 1) if M > 1 else 1.0
    unb = fin["var"] * k
    tol_unb = fin["tol_var"] * k + (2 * E * unb if M > 1 else 0.0)
    rm = a * rm0.double() + mom * fin["mean"]
    rv = a * rv0.double() + mom * unb
    tol = lambda r0, v, tv, r1: (2 * E * (a * r0.double()).abs() + E * (mom * v).abs() + mom * tv  # noqa: E731
                                 + E * r1.abs()) * SLACK
    return {"rm": rm, "rv": rv, "tol_rm": tol(rm0, fin["mean"], fin["tol_mean"], rm),
            "tol_rv": tol(rv0, unb, tol_unb, rv)}


def _apply(out: dict, xd, res, w, b, mean, tol_mean, rstd, rel_rstd, relu: bool, dtype) -> None:
    wd, bd = w.double(), b.double()
    sc = wd * rstd
    tol_sc = wd.abs() * rstd * rel_rstd + E * sc.abs()
    sh = bd - mean * sc
    v = (xd - mean) * sc + bd
    tol = (xd - mean).abs() * tol_sc + sc.abs() * tol_mean + E * (mean * sc).abs() + E * sh.abs() + E * v.abs()
    if res is not None:
        v = v + res.double()
        tol = tol + E * v.abs()
    y = v.clamp(min=0.0) if relu else v
    if dtype == BF16:
        tol = tol + U * y.abs()
    out.update(y=y, tol_y=tol * SLACK)


def bn_fwd_ref(xp, res, w, b, rm0, rv0, nbt0, *, eps: float, mom: float, relu: bool, training: bool, depth: int,
               exact: bool = False) -> dict:
    """Float64 forward of rows ``xp`` [M, C] (the spliced activation x', bf16 or fp32) with its bounds.  ``depth``:
    :func:`bn_plan`'s additions per channel; ``exact``: the integer family (the sums carry no error)."""
    xd = xp.double()
    M = xd.shape[0]
    eps, mom = f32(eps), f32(mom)
    out = {}
    if training:
        p = xd[0]
        d = xd - p
        s1, s2 = d.sum(0), (d * d).sum(0)
        if exact:
            assert float(d.abs().sum(0).max()) < 2 ** 24 and float(s2.max()) < 2 ** 24
            t1, t2 = torch.zeros_like(s1), torch.zeros_like(s2)
        else:
            t1, t2 = depth * E * d.abs().sum(0), (depth + 2) * E * s2
        fin = _finalize(p, s1, t1, s2, t2, M, eps)
        out.update(_running(fin, rm0, rv0, M, mom))
        out.update(mean=fin["mean"], rstd=fin["rstd"], tol_mean=fin["tol_mean"] * SLACK,
                   tol_rstd=fin["rstd"] * fin["rel_rstd"] * SLACK, nbt=None if nbt0 is None else nbt0 + 1)
        _apply(out, xd, res, w, b, fin["mean"], fin["tol_mean"], fin["rstd"], fin["rel_rstd"], relu, xp.dtype)
    else:
        mean = rm0.double()
        rstd = (rv0.double() + eps).rsqrt()
        zero = torch.zeros_like(mean)
        out.update(mean=mean, rstd=rstd, tol_mean=zero, tol_rstd=2 * E * rstd * SLACK, rm=mean, rv=rv0.double(),
                   tol_rm=zero, tol_rv=zero, nbt=nbt0)
        _apply(out, xd, res, w, b, mean, zero, rstd, 2.5 * E, relu, xp.dtype)
    return out


def bn_fwd_check(got: dict, ref: dict) -> dict:
    """Masks of bad elements of ``save`` (mean, rstd), the running statistics and y; ``got["nbt"]`` an int or None."""
    C = ref["mean"].numel()
    out = {"mean": bad_bound(got["save"][:C], ref["mean"], ref["tol_mean"]),
           "rstd": bad_bound(got["save"][C:], ref["rstd"], ref["tol_rstd"]),
           "rm": bad_bound(got["rm"], ref["rm"], ref["tol_rm"]), "rv": bad_bound(got["rv"], ref["rv"], ref["tol_rv"]),
           "y": bad_bound(got["y"], ref["y"], ref["tol_y"])}
    if ref["nbt"] is not None:
        out["nbt"] = torch.tensor([got["nbt"] != ref["nbt"]])
    return out


def worst(got: torch.Tensor, ref: torch.Tensor, tol: torch.Tensor) -> float:
    """Largest ``|got - ref| / tol`` over the elements with a non-zero bound (the recorded measurement)."""
    err = (got.double() - ref).abs()
    live = tol > 0
    return float((err[live] / tol[live]).max()) if bool(live.any()) else 0.0


def _osum(v: torch.Tensor, order: str) -> torch.Tensor:
    """fp32 column sums of ``v`` [M, C] in a deliberately bad order: rows last to first, or pairwise."""
    if order == "rev":
        s = torch.zeros(v.shape[1], dtype=F32)
        for t in range(v.shape[0] - 1, -1, -1):
            s = s + v[t]
        return s
    assert order == "pair"
    while v.shape[0] > 1:
        if v.shape[0] % 2:
            v = torch.cat([v, torch.zeros(1, v.shape[1], dtype=F32)])
        v = v[0::2] + v[1::2]
    return v[0].clone()


def _fma(a, b, c) -> torch.Tensor:
    """fp32 ``fma(a, b, c)``: the product of two fp32 values is exact in float64."""
    return (a.double() * b.double() + c.double()).float()


def _finalize_emul(p, s, q, M: int, eps, mom, rm0, rv0, bug: str = ""):
    F = lambda a: torch.tensor(a, dtype=F32)  # noqa: E731
    Mf = F(float(M))
    dm = s / Mf
    mean = p + dm
    var = (q / Mf - dm * dm).clamp(min=0.0)
    rstd = torch.rsqrt(var + F(eps))
    unb = var * Mf / F(float(M - 1)) if M > 1 and bug != "biased_running" else var
    m = F(mom)
    a, c = (m, 1.0 - m) if bug == "momentum_swapped" else (1.0 - m, m)
    return mean, rstd, a * rm0 + c * mean, a * rv0 + c * unb


def bn_fwd_emul(x, xp, res, w, b, rm0, rv0, nbt0, *, eps: float, mom: float, relu: bool, training: bool, order: str,
                bug: str = "") -> dict:
    """fp32 torch emulation of the forward kernels' own expressions on rows ``xp`` (= x' ; ``x`` the unspliced rows),
    the sums in ``order``.  ``bug``: ``drop_last`` (the statistics miss the last row, whose y keeps the sentinel),
    ``row_twice`` (row 1 counted twice), ``naive_var`` (E[x^2] - mean^2), ``pivot_unspliced`` (the sums around
    x'[0], the finalize around x[0]), ``biased_running``, ``momentum_swapped``, ``relu_first``."""
    xf = xp.float()
    M, C = xf.shape
    if training:
        p = xf[0]
        rows = xf[:M - 1] if bug == "drop_last" else (torch.cat([xf, xf[1:2]]) if bug == "row_twice" else xf)
        if bug == "naive_var":
            s, q = _osum(rows, order), _osum(rows * rows, order)
            p = torch.zeros(C)
        else:
            d = rows - p
            s, q = _osum(d, order), _osum(d * d, order)
        pf = x.float()[0] if bug == "pivot_unspliced" else p
        mean, rstd, rm, rv = _finalize_emul(pf, s, q, M, eps, mom, rm0, rv0, bug)
        nbt = None if nbt0 is None else nbt0 + 1
    else:
        mean, rstd, rm, rv, nbt = rm0, torch.rsqrt(rv0 + torch.tensor(eps, dtype=F32)), rm0, rv0, nbt0
    sc = w * rstd
    sh = b - mean * sc
    v = _fma(xf, sc, sh)
    if bug == "relu_first":
        v = v.clamp(min=0.0)
    if res is not None:
        v = v + res.float()
    if relu and bug != "relu_first":
        v = v.clamp(min=0.0)
    y = v.to(xp.dtype)
    if bug == "drop_last":
        y[M - 1] = filled((C,), xp.dtype)
    return {"save": torch.cat([mean, rstd]), "rm": rm, "rv": rv, "nbt": nbt, "y": y}


# ================================================================================================ backward
def bn_bwd_ref(dy, y, xp, hit, save, w, dw0, db0, *, training: bool, depth: int, exact: bool = False) -> dict:
    """Float64 backward.  ``y``: the kernel's saved output (None without ReLU), ``save``: the kernel's fp32 (mean,
    rstd), both exact inputs; ``xp`` the rows of x', ``hit`` (bool [M, C] or None) its spliced elements; ``dw0`` /
    ``db0`` the prefills (None: a null pointer).  ``exact``: integer ``dy`` (``sum dz`` carries no error)."""
    dt = dy.dtype
    dyd = dy.double()
    M, C = dyd.shape
    dz = dyd if y is None else torch.where(y.double() > 0, dyd, torch.zeros_like(dyd))
    mean, rstd = save[:C].double(), save[C:].double()
    xhat = (xp.double() - mean) * rstd
    c0, c1 = dz.sum(0), (dz * xhat).sum(0)
    a0, a1 = dz.abs().sum(0), (dz * xhat).abs().sum(0)
    if exact:
        assert float(a0.max()) < 2 ** 24
    tol_c0 = torch.zeros_like(c0) if exact else (depth + 3) * E * a0
    tol_c1 = (depth + 6) * E * a1
    out = {"dz": dz.to(dt), "coef": torch.cat([c0, c1]), "tol_coef": torch.cat([tol_c0, tol_c1]) * SLACK}
    if dw0 is not None:
        out.update(dw=dw0.double() + c1, db=db0.double() + c0)
        out.update(tol_dw=(tol_c1 + E * out["dw"].abs()) * SLACK)
        out.update(tol_db=torch.zeros_like(c0) if exact else (tol_c0 + E * out["db"].abs()) * SLACK)
    k1 = w.double() * rstd
    if training:
        k2, k3 = c0 / M, c1 / M
        tk2, tk3 = tol_c0 / M + 2 * E * k2.abs(), tol_c1 / M + 2 * E * k3.abs()
        core = dz - k2 - xhat * k3
        dx = k1 * core
        tol = k1.abs() * (tk2 + xhat.abs() * tk3 + 3 * E * (xhat * k3).abs() + E * (dz - k2).abs() + E * core.abs()) \
            + 2 * E * dx.abs()
    else:
        dx = k1 * dz
        tol = 2 * E * dx.abs()
    if dt == BF16:
        tol = tol + U * dx.abs()
    if hit is not None:
        dx = torch.where(hit, torch.zeros_like(dx), dx)
        tol = torch.where(hit, torch.zeros_like(tol), tol)
    out.update(dx=dx, tol_dx=tol * SLACK, hit=hit)
    return out


def bn_bwd_check(got: dict, ref: dict) -> dict:
    """coef, dw / db (when given), dx within their bounds; dres bitwise dz; spliced elements of dx exactly +0."""
    out = {"coef": bad_bound(got["coef"], ref["coef"], ref["tol_coef"]),
           "dx": bad_bound(got["dx"], ref["dx"], ref["tol_dx"])}
    if "dw" in ref:
        out["dw"] = bad_bound(got["dw"], ref["dw"], ref["tol_dw"])
        out["db"] = bad_bound(got["db"], ref["db"], ref["tol_db"])
    if got.get("dres") is not None:
        out["dres"] = bad_bits(got["dres"], ref["dz"])
    if ref["hit"] is not None:
        out["dx_spliced"] = bad_bits(got["dx"], torch.zeros_like(got["dx"])) & ref["hit"]
    return out


def bn_bwd_emul(dy, y, xp, hit, save, w, dw0, db0, *, training: bool, order: str, bug: str = "") -> dict:
    """fp32 emulation of the backward kernels.  ``bug``: ``mask_sign_dy`` (dz from dy > 0), ``splice_kept`` (a
    spliced element keeps its gradient), ``dw_stored`` (dw = coef instead of dw0 + coef)."""
    dt = dy.dtype
    d = dy.float()
    M, C = d.shape
    if bug == "mask_sign_dy":
        d = torch.where(d > 0, d, torch.zeros(()))
    elif y is not None:
        d = torch.where(y.float() > 0, d, torch.zeros(()))
    mean, rstd = save[:C], save[C:]
    xh = (xp.float() - mean) * rstd
    c0, c1 = _osum(d, order), _osum(d * xh, order)
    out = {"coef": torch.cat([c0, c1]), "dres": d.to(dt)}
    if dw0 is not None:
        out.update(dw=c1.clone() if bug == "dw_stored" else dw0 + c1, db=db0 + c0)
    k1 = w * rstd
    if training:
        inv = torch.tensor(1.0, dtype=F32) / torch.tensor(float(M), dtype=F32)
        dx = k1 * (d - c0 * inv - xh * (c1 * inv))
    else:
        dx = k1 * d
    if hit is not None and bug != "splice_kept":
        dx = torch.where(hit, torch.zeros(()), dx)
    out["dx"] = dx.to(dt)
    return out


# ================================================================================================ tile records
def tile_records(x: torch.Tensor, T: int, R: int) -> torch.Tensor:
    """fp32 [3, C, T]: per row tile t of ``x`` [T R, C] the pivot (its first row), ``sum (v - p_t)`` and
    ``sum (v - p_t)^2``, computed in float64 and rounded to fp32 -- the layout of ``cstat``."""
    M, C = x.shape
    assert M == T * R
    v = x.double().view(T, R, C)
    p = v[:, 0, :]
    d = v - p[:, None, :]
    return torch.stack([p.t(), d.sum(1).t(), (d * d).sum(1).t()]).float().contiguous()


def tile_ref(cstat, T: int, R: int, rm0, rv0, nbt0, *, eps: float, mom: float, wrong: str = "") -> dict:
    """Float64 combine of the given fp32 records (exact inputs) around ``P = p_0`` with the bound of
    ``bn_tile_finalize_kernel``'s own arithmetic; returns the statistics part of :func:`bn_fwd_ref`'s result plus the
    raw ``fin`` for :func:`tile_apply`.  ``wrong``: ``no_cross`` (without ``2 d_t S1_t``), ``r_is_t`` (R taken as
    the tile count)."""
    rec = cstat.double().view(3, -1, T)
    C = rec.shape[1]
    M = T * R
    eps, mom = f32(eps), f32(mom)
    pv, s1, s2 = rec[0], rec[1], rec[2]
    P = pv[:, :1]
    d = pv - P
    fr = float(T if wrong == "r_is_t" else R)
    a = s1 + fr * d
    inner = fr * d + (0.0 if wrong == "no_cross" else 2.0) * s1
    q = s2 + d * inner
    nt = (T + 255) // 256 + 8
    t1 = (nt + 1) * E * a.abs().sum(1) + fr * E * d.abs().sum(1)
    t2 = (nt + 1) * E * q.abs().sum(1) + (3 * E * (d * inner).abs() + fr * E * d * d).sum(1)
    fin = _finalize(P[:, 0], a.sum(1), t1, q.sum(1), t2, M, eps)
    out = dict(_running(fin, rm0, rv0, M, mom))
    out.update(mean=fin["mean"], rstd=fin["rstd"], tol_mean=fin["tol_mean"] * SLACK,
               tol_rstd=fin["rstd"] * fin["rel_rstd"] * SLACK, nbt=None if nbt0 is None else nbt0 + 1, fin=fin)
    assert C == out["mean"].numel()
    return out


def tile_apply(ref: dict, x, res, w, b, relu: bool) -> dict:
    """Adds ``y`` / ``tol_y`` of rows ``x`` under the statistics of :func:`tile_ref`."""
    fin = ref["fin"]
    _apply(ref, x.double(), res, w, b, fin["mean"], fin["tol_mean"], fin["rstd"], fin["rel_rstd"], relu, x.dtype)
    return ref


def tile_emul(cstat, T: int, R: int, rm0, rv0, *, eps: float, mom: float, order: str) -> dict:
    """fp32 emulation of ``bn_tile_finalize_kernel`` with the tiles added in ``order``."""
    rec = cstat.view(3, -1, T)
    pv, s1, s2 = rec[0], rec[1], rec[2]
    P = pv[:, :1]
    d = pv - P
    fr = torch.tensor(float(R), dtype=F32)
    a = fr * d + s1
    q = s2 + d * (fr * d + 2.0 * s1)
    mean, rstd, rm, rv = _finalize_emul(P[:, 0], _osum(a.t().contiguous(), order), _osum(q.t().contiguous(), order),
                                        T * R, eps, mom, rm0, rv0)
    return {"save": torch.cat([mean, rstd]), "rm": rm, "rv": rv}


# ================================================================================================ max pool
POOL_SHAPES = [(1, 8, 1, 1), (2, 8, 2, 3), (1, 16, 5, 4), (3, 24, 7, 7), (2, 64, 12, 9)]
POOL_FAMILIES = ["random", "ties", "specials"]
NAN, INF = float("nan"), float("inf")


def pool_out(H: int, W: int):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def pool_x(family: str, shape, dtype, seed: int) -> torch.Tensor:
    """[N, C, H, W] (NCHW, contiguous).  ``ties``: integers -3 .. 3 with both zeros.  ``specials``: NaN, +-inf, whole
    windows of -inf (the first image's top-left 3 x 3 and one whole channel), a NaN followed by a larger finite
    value."""
    g = gen(seed)
    N, C, H, W = shape
    if family == "ties":
        x = torch.randint(-3, 4, shape, generator=g).float()
        neg = torch.rand(shape, generator=g) < 0.5
        return torch.where((x == 0) & neg, torch.tensor(-0.0), x).to(dtype)
    x = torch.randn(shape, generator=g)
    if family == "specials":
        r = torch.rand(shape, generator=g)
        x = torch.where(r < 0.08, torch.tensor(NAN), x)
        x = torch.where((r >= 0.08) & (r < 0.16), torch.tensor(INF), x)
        x = torch.where((r >= 0.16) & (r < 0.30), torch.tensor(-INF), x)
        x[0, :, :3, :3] = -INF
        x[:, C - 1] = -INF
        if H * W >= 2:  # channel 1: a NaN, then the largest finite value of the tensor in the next tap
            x[:, 1, 0, 0] = NAN
            x[:, 1, 1 // W, 1 % W] = 100.0
    else:
        assert family == "random", family
    return x.to(dtype)


def pool_ref_torch(x: torch.Tensor):
    """(y [N, C, OH, OW] in x's dtype, tap uint8) from torch's CPU max pool of the fp32 image of ``x``."""
    N, C, H, W = x.shape
    y, flat = torch.nn.functional.max_pool2d(x.float().cpu().contiguous(), 3, 2, 1, return_indices=True)
    OH, OW = y.shape[2:]
    ih, iw = flat // W, flat % W
    kh = ih - (2 * torch.arange(OH).view(1, 1, OH, 1) - 1)
    kw = iw - (2 * torch.arange(OW).view(1, 1, 1, OW) - 1)
    assert bool(((kh >= 0) & (kh < 3) & (kw >= 0) & (kw < 3)).all())
    return y.to(x.dtype), (kh * 3 + kw).to(torch.uint8)


def pool_ref_scan(x: torch.Tensor, rule: str = ""):
    """The same from the rule alone: scan the taps (kh, kw) in row-major order, skip those outside the image; the
    first valid tap is taken, then every tap that is larger or a NaN.  ``rule`` (the defects): ``last_tie`` (>=),
    ``clipped_numbering`` (the tap numbered among the valid taps of the window), ``skip_nan`` (a NaN never taken)."""
    xf = x.float().cpu()
    N, C, H, W = xf.shape
    OH, OW = pool_out(H, W)
    best = torch.full((N, C, OH, OW), -INF)
    arg = torch.zeros((N, C, OH, OW), dtype=torch.int64)
    seen = torch.zeros((1, 1, OH, OW), dtype=torch.int64)
    pad = torch.full((N, C, H + 2, W + 2), -INF)
    pad[:, :, 1:H + 1, 1:W + 1] = xf
    for kh in range(3):
        for kw in range(3):
            ih = 2 * torch.arange(OH).view(1, 1, OH, 1) - 1 + kh
            iw = 2 * torch.arange(OW).view(1, 1, 1, OW) - 1 + kw
            valid = (ih >= 0) & (ih < H) & (iw >= 0) & (iw < W)
            f = pad[:, :, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2]
            take = (f >= best) if rule == "last_tie" else (f > best)
            if rule != "skip_nan":
                take = take | torch.isnan(f)
            take = valid & ((seen == 0) | take)
            best = torch.where(take, f, best)
            num = seen.expand_as(arg) if rule == "clipped_numbering" else torch.full_like(arg, kh * 3 + kw)
            arg = torch.where(take, num, arg)
            seen = seen + valid.long()
    return best.to(x.dtype), arg.to(torch.uint8)


def bad_pool_y(got: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """Bitwise, any NaN equal to any NaN (the sentinel is no NaN)."""
    both = torch.isnan(got.float()) & torch.isnan(ref.float())
    return bad_bits(got, ref) & ~both


def pool_bwd_emul(dy: torch.Tensor, tap: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """[N, C, H, W] in dy's dtype: every input element adds, in fp32 from +0 and in ascending (kh, kw) order, the
    ``dy`` of the windows whose byte names it; one rounding to the output type."""
    N, C, OH, OW = dy.shape
    acc = torch.zeros(N, C, H + 2, W + 2, dtype=F32)
    d = dy.float().cpu()
    t = tap.cpu()
    for kh in range(3):
        for kw in range(3):
            view = acc[:, :, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2]
            view.copy_(torch.where(t == kh * 3 + kw, view + d, view))
    return acc[:, :, 1:H + 1, 1:W + 1].to(dy.dtype).contiguous()
