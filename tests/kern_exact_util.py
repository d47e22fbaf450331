"""Helpers shared by the exact tests of the layer-norm kernels of csrc/layer_norm.hip and the cross-entropy and fused-Adam
kernels of csrc/kernels.hip
(tests/test_ln_exact.py, tests/test_ce_exact.py and tests/test_adam_exact.py on the GPU, tests/test_kern_exact_ref.py
on the CPU): float64 references of the same fp32 / bf16 inputs, element-wise bounds built from reference quantities
alone, operand families, and the perturbations the comparators must flag.

A comparator returns the boolean mask of elements outside their bound (NaN and the buffer sentinel count as bad); a
test passes only with no such element.  ``E`` = 2^-24 is the unit roundoff of fp32, ``U`` = 2^-8 that of bf16; every
bound is multiplied by ``SLACK`` = 1 + 2^-8 for the second-order terms.

Layer norm (one wave per row; a lane adds its <= 4 ceil(d / 256) columns serially, six shuffle levels join the lanes:
``depth(d) = 4 ceil(d / 256) + 6`` additions on the longest path):

* ``tol_mean = depth E mean|x| + E |mean|``
* ``rel_rstd = ((depth + 5) / 2 + 2) E + tol_mean^2 / (2 (var + eps))`` -- the centring and squaring (3 roundings), the
  sum, the division and ``+ eps`` (2), halved by the inverse square root, then the hardware rsqrt (1 ulp = 2 E); the
  error of the mean enters the variance only squared.  At d = 4096 this is 39.5 E = 2.4e-6 relative, fifty times
  below the 1.2e-4 of a variance divided by d - 1.
* ``tol_y = U |y| + |w| (rstd tol_mean + |xhat| (rel_rstd + 2 E)) + 2 E (|xhat w| + |y|)``
* backward (``mean`` / ``rstd`` are inputs: the reference takes the fp32 values the kernel is given as exact), with
  ``g = dy w``, ``c1 = mean(g)``, ``c2 = mean(g xhat)``:
  ``tol_c1 = (depth + 2) E mean|g|``, ``tol_c2 = (depth + 5) E mean|g xhat|``,
  ``tol_dx = rstd (tol_c1 + |xhat| tol_c2 + 6 E (|g| + |c1| + |xhat c2|)) + E (|core| + |core + dres| + |dx|)`` -- one
  term per rounding point: g (and dy + dy2), the two row means, the combination, dres, the accumulate add.
* ``tol_dw = (T + 4) E (sum_t |dy xhat| + |dw0|)``, ``tol_db = (T + 4) E (sum_t |dy| + |db0|)``: T - 1 additions in
  any order (LDS combine, partial rows, atomics), three roundings of xhat and the product, the add into the prefill.

Cross-entropy:

* ``lse``: ``|lse - ref| <= 2^-18 max(1, |ref|)`` (the bound of tests/attn_exact_util.py); ``loss``: that plus
  ``E (|lse| + |loss|)`` for the stored fp32 lse and the subtraction.
* gradient, fed the fp32 rounding of the reference lse, ``a = x - lse``, ``p = exp(a)``:
  ``|g - ref| <= scale p (C1 2^-23 + C2 2^-24 |a|) + 3 E |ref| + scale 2^-126`` with C1 = 2, C2 = 3.  ``__expf`` is one
  product by log2(e) and one hardware exp2: the subtraction (E |a|), the product (E |a|) and the constant (its fp32
  rounding, <= E / 2 relative) move the exponent by 2.5 E |a| -> C2 = 3; the hardware exp2 is good to 1 ulp = 2^-23,
  taken twice -> C1 = 2.  ``3 E |ref|`` covers ``p - onehot`` and the two products by the scales (for every column but
  the label it only raises C1 by 1.5; at the label |ref| = scale (1 - p) is not small when p is).  ``scale 2^-126``: a
  denormal probability may be flushed.  bf16 outputs add ``U |ref|``.  Columns at -inf must be exactly zero.

Fused Adam (one step from a given state, float64 with the fp32-rounded hyper-parameters):

* clip coefficient: the squares are non-negative, so the fp32 sum is within ``NSQ E`` = 40 E relative (3 inside a
  float4, <= 5 per thread, 6 + 2 to the block, 16 + 6 over the partials, the squares), the sqrt halves it, then the
  sqrt, ``+ 1e-6`` and the division round: ``rel_coef = 23 E`` when the coefficient is below 1, 0 when it is 1.
* ``gr = g coef + wd p``, ``tol_gr = |g coef| (rel_coef + E) + 2 E |wd p| + E |gr|``
* ``tol_m = (1 - b1) tol_gr + E (|b1 m| + |(1 - b1) gr| + |m'|)`` (three roundings), the same for v with
  ``2 |gr| tol_gr`` and two products, plus 2^-125 where ``gr^2`` can be denormal (the tiny-gradient family).
* bias corrections ``1 - b^t``: ``powf`` is within ``POW_K`` ulps of b^t, so ``r(b, t) = (POW_K 2^-23 b^t + E) /
  (1 - b^t)`` for t > 1 and 0 at t = 1 (``powf(b, 1) = b`` and ``1 - b`` are exact).
* ``tol_p`` follows ``p - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps)`` rounding by rounding (see :func:`adam_ref`).

``POW_K`` = 1.02: twice the worst error measured on an MI355X, 0.508 ulps (beta = 0.9, t = 3).  The measurement goes
through the kernel itself: with b2 = 0, eps = 0, lr = 1 and g = 1 from a zero state the step stores
``p' = -fl(fl(1 / bc1) (1 - b1))``, and the fp32 candidates for ``powf(b1, t)`` that reproduce p' bit for bit are
unique for beta = 0.9 at t = 1, 2, 3 and for beta = 0.999 at t = 1, 2, 3, 10, 100, 1000 (errors 0, -0.24, 0.51 and 0,
0.22, -0.31, 0.05, 0.15, -0.13 ulps); at beta = 0.9, t = 10 three neighbours match (smallest error 0.09 ulps), and
from beta^t < 1e-4 on (t = 100 .. 10000) the power is below the resolution of ``1 - beta^t`` and cannot matter.  (The
bounds started from 4 before the measurement.)

Kernel instantiations of csrc/layer_norm.hip (``ln_*``; W = 4 the vector layout, W = 1 the fallback) and
csrc/kernels.hip, and a passing case that runs each (GPU modules):

=========================================  =====================================================================
ln_fwd_kernel<4, 1,2,3,4,6,8,12,16>        test_ln_exact.py::test_ln_fwd, d = 4 / 252 / 256 ... 4096 (both ends)
ln_fwd_kernel<4, *> with y32               test_ln_exact.py::test_ln_fwd (twin checked in every vector case)
ln_fwd_kernel<1, 4,16,32,64>               test_ln_fwd, d = 1..255 / 257..1023 / 1025..2047 / 2049..4095, offset view
ln_bwd_kernel<4, 1..16, f32 / bf16>        test_ln_bwd[plain], same vector d; <4, *, *, XH16> test_ln_bwd_xh16
ln_bwd_kernel<1, 4,16,32,64, f32 / bf16>   test_ln_bwd[plain], scalar d and the offset view
ln_bwd_part_kernel<1..4, *, R = 1>         test_ln_bwd[fused], d <= 1024; test_ln_bwd_long (T = 149, 1021)
ln_bwd_part_kernel<*, *, R = 2 / 4>        test_launch_variants.py only (IIT_LN_PART_R)
ln_part_reduce_kernel                      test_ln_bwd_long: G = 4 (T = 149: 4-wide loop + rest), G = 32 (T = 1021)
ln_dwdb_vec_kernel<f32 / bf16>             test_ln_dwdb_vec (IIT_LN_FUSED_DWDB=0, and d > 1024)
ln_dwdb_kernel<f32 / bf16>                 test_ln_dwdb_scalar (d = 130, T = 257) and scalar d of test_ln_bwd
row select (RowSel) of all of the above    test_ln_row_select, S = 3 / 64
ce_fwd_kernel                              test_ce_exact.py::test_ce_fwd
ce_bwd_kernel<float> (+ out16), <__bf16>   test_ce_exact.py::test_ce_bwd
ce_bwd16_kernel<true / false>              test_ce_exact.py::test_ce_bwd (aligned dense / every other stride)
sumsq_span_kernel                          test_adam_exact.py::test_adam_step (clip or nan guard)
adam_span_kernel<true, 4>                  test_adam_exact.py, every case
adam_span_kernel<false, 4>, <true, 1 / 2>  test_launch_variants.py only (IIT_ADAM_NT, IIT_ADAM_UNROLL)
adam_span_kernel<false, 1 / 2>             not run by any test
=========================================  =====================================================================
"""
import math

import torch

from gemm_exact_util import BF16_FILL, bad_bits  # noqa: F401  (re-exported)

E = 2.0 ** -24
U = 2.0 ** -8
SLACK = 1.0 + 2.0 ** -8
LSE_TOL = 2.0 ** -18
NAN = float("nan")
NINF = float("-inf")
POW_K = 1.02
CE_C1, CE_C2 = 2.0, 3.0
NSQ = 40


def bad_bound(got: torch.Tensor, ref: torch.Tensor, tol: torch.Tensor) -> torch.Tensor:
    """Elements with ``|got - ref| > tol`` (NaN and the buffer sentinel count as bad)."""
    assert got.shape == ref.shape == tol.shape, (got.shape, ref.shape, tol.shape)
    return ~((got.double() - ref).abs() <= tol)


def norm_ratio(got: torch.Tensor, ref: torch.Tensor) -> float:
    """The criterion of tests/test_hip_kernels.py: ||got - ref|| / ||ref||."""
    return ((got.double() - ref.double()).norm() / ref.double().norm()).item()


def filled(shape, dtype, device="cpu") -> torch.Tensor:
    """Output buffer prefilled with NaN (fp32) / the sentinel (bf16) / -7 (integers)."""
    if dtype == torch.float32:
        return torch.full(shape, NAN, dtype=dtype, device=device)
    if dtype == torch.bfloat16:
        return torch.full(shape, BF16_FILL, dtype=dtype, device=device)
    return torch.full(shape, -7, dtype=dtype, device=device)


def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


# ================================================================================================ layer norm
LN_D_VEC = [4, 252, 256, 260, 512, 516, 768, 772, 1024, 1028, 1536, 1540, 2048, 2052, 3072, 3076, 4096]
LN_D_SCALAR = [1, 2, 3, 66, 255, 257, 1023, 1025, 2047, 2049, 4095]
LN_T = [1, 3, 5, 9]
LN_FAMILIES = ["random", "offset", "lowvar", "balanced"]
LN_EPS = 1e-5


def ln_depth(d: int) -> int:
    return 4 * ((d + 255) // 256) + 6


def ln_inputs(family: str, T: int, d: int, seed: int, affine: bool = True):
    """fp32 ``x`` [T, d], ``w``, ``b`` (None without affine) of one operand family.  ``balanced`` returns rows of
    ``m -+ a`` (d even; an odd d gets the random family) with w = 1, b = 0."""
    g = gen(seed)
    w = b = None
    if affine:
        w = (1.0 + 0.5 * torch.randn(d, generator=g)).float()
        b = (0.5 * torch.randn(d, generator=g)).float()
    if family == "balanced" and d % 2 == 0:
        m = torch.randint(-3, 4, (T, 1), generator=g).double()
        a = 2.0 ** torch.randint(-2, 3, (T, 1), generator=g).double()
        sign = torch.where(torch.arange(d) % 2 == 0, -1.0, 1.0).double()
        if d >= 8:  # not a period-2 pattern: a column swap or a dropped column shows
            sign[:d // 2] = -1.0
            sign[d // 2:] = 1.0
            sign[1], sign[d - 2] = 1.0, -1.0
        x = (m + a * sign).float()
        if affine:
            w, b = torch.ones(d), torch.zeros(d)
        return x, w, b
    if family == "offset":
        x = 1000.0 + torch.randn(T, d, generator=g)
    elif family == "lowvar":
        x = torch.randint(-3, 4, (T, 1), generator=g).float() + 1e-3 * torch.randn(T, d, generator=g)
    else:
        x = 3.0 * torch.randn(T, d, generator=g) + 1.0
    return x.float(), w, b


def ln_fwd_ref(x, w, b, eps: float, wrong: str = "") -> dict:
    """Float64 layer norm of fp32 ``x`` [T, d] with its bounds.  ``wrong`` computes a perturbed result instead."""
    x = x.double()
    T, d = x.shape
    xs = x
    if wrong == "stats_pad4":  # statistics over 4 ceil(d / 4) columns (zeros appended)
        xs = torch.cat([x, x.new_zeros(T, (-d) % 4)], 1)
    elif wrong == "stats_drop_last":
        xs = x[:, :d - 1]
    n = xs.shape[1]
    mean = xs.sum(1, keepdim=True) / n
    var = ((xs - mean) ** 2).sum(1, keepdim=True) / (n - 1 if wrong == "var_dm1" else n)
    rstd = 1.0 / torch.sqrt(var) + eps if wrong == "eps_after" else 1.0 / torch.sqrt(var + eps)
    xhat = (x - mean) * rstd
    y = xhat
    if w is not None:
        y = xhat * w.double() + (0.0 if wrong == "no_bias" else b.double())
    if wrong == "swap_groups" and d >= 8:
        y = y.clone()
        y[:, 0:4], y[:, 4:8] = y[:, 4:8].clone(), y[:, 0:4].clone()
    if wrong == "last_row_missing":
        y = y.clone()
        y[T - 1] = BF16_FILL
    out = {"mean": mean[:, 0], "rstd": rstd[:, 0], "y": y, "xhat": xhat}
    if wrong:
        return out
    dep = ln_depth(d)
    tol_mean = dep * E * x.abs().mean(1, keepdim=True) + E * mean.abs()
    rel_rstd = ((dep + 5) / 2 + 2) * E + tol_mean ** 2 / (2 * (var + eps))
    aw = 1.0 if w is None else w.double().abs()
    tol_y = U * y.abs() + aw * (rstd * tol_mean + xhat.abs() * (rel_rstd + 2 * E)) + 2 * E * ((xhat * aw).abs() + y.abs())
    out.update(tol_mean=tol_mean[:, 0] * SLACK, tol_rstd=(rstd * rel_rstd)[:, 0] * SLACK, tol_y=tol_y * SLACK)
    return out


def ln_fwd_check(got: dict, ref: dict) -> dict:
    """Masks of bad elements of y (bf16), mean and rstd."""
    return {"y": bad_bound(got["y"], ref["y"], ref["tol_y"]),
            "mean": bad_bound(got["mean"], ref["mean"], ref["tol_mean"]),
            "rstd": bad_bound(got["rstd"], ref["rstd"], ref["tol_rstd"])}


def bad_balanced(y: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """Balanced family with w = 1, b = 0: every |y| of a row is the same bf16 value, not zero, with the sign of
    ``x - median``."""
    yd = y.double()
    mid = (x.double().max(1, keepdim=True).values + x.double().min(1, keepdim=True).values) / 2
    same = yd.abs() == yd[:, :1].abs()
    return ~(same & (yd != 0) & (torch.sign(yd) == torch.sign(x.double() - mid)))


def ln_bwd_inputs(T: int, d: int, seed: int, bf16_dy: bool):
    g = gen(seed + 1000)
    dy = torch.randn(T, d, generator=g).float()
    if bf16_dy:
        dy = dy.bfloat16()
    return {"dy": dy, "dres": torch.randn(T, d, generator=g).float(), "dy2": torch.randn(T, d, generator=g).float(),
            "dx0": torch.randn(T, d, generator=g).float(), "dw0": torch.randn(d, generator=g).float(),
            "db0": torch.randn(d, generator=g).float()}


def ln_bwd_ref(dy, x, mean, rstd, w, dres=None, dx0=None, dy2=None, dw0=None, db0=None, dead=None, xh16=False,
               wrong: str = "") -> dict:
    """Float64 layer-norm backward.  ``mean`` / ``rstd`` are the fp32 tensors the kernel is given (exact inputs);
    ``xh16``: ``x`` is the bf16 xhat itself.  ``dead`` (bool [T]): row-select rows -- dx = dres (or 0), nothing added
    to dw / db.  ``dx0`` the accumulate prefill, ``dw0`` / ``db0`` the prefill of the affine gradients."""
    dyt = dy.double() + (0.0 if dy2 is None else dy2.double())
    T, d = dyt.shape
    rs = rstd.double().view(T, 1)
    xhat = x.double() if xh16 else (x.double() - mean.double().view(T, 1)) * rs
    live = torch.ones(T, 1, dtype=torch.float64) if dead is None else (~dead).double().view(T, 1)
    g = dyt if w is None else dyt * w.double()
    c1 = g.mean(1, keepdim=True)
    c2 = (g * xhat).mean(1, keepdim=True)
    core = rs * (g - (0.0 if wrong == "no_mean_g" else c1) - xhat * c2) * live
    r = 0.0 if dres is None else dres.double()
    a0 = 0.0 if dx0 is None else dx0.double()
    dx = core + r + a0
    wl = torch.ones_like(live) if wrong == "dead_in_dw" else live
    dw = (dyt * xhat * wl).sum(0) + (0.0 if dw0 is None else dw0.double())
    db = (dyt * wl).sum(0) + (0.0 if db0 is None else db0.double())
    if wrong == "last_row_missing":
        dx = dx.clone()
        dx[T - 1] = NAN
    out = {"dx": dx, "dw": dw, "db": db}
    if wrong:
        return out
    dep = ln_depth(d)
    tol_c1 = (dep + 2) * E * g.abs().mean(1, keepdim=True)
    tol_c2 = (dep + 5) * E * (g * xhat).abs().mean(1, keepdim=True)
    tol_dx = rs * (tol_c1 + xhat.abs() * tol_c2 + 6 * E * (g.abs() + c1.abs() + (xhat * c2).abs())) * live \
        + E * (core.abs() + (core + r).abs() + dx.abs())
    kT = (T + 4) * E
    out.update(tol_dx=tol_dx * SLACK,
               tol_dw=kT * ((dyt * xhat * live).abs().sum(0) + (0.0 if dw0 is None else dw0.double().abs())) * SLACK,
               tol_db=kT * ((dyt * live).abs().sum(0) + (0.0 if db0 is None else db0.double().abs())) * SLACK)
    return out


def _lane_sum(v: torch.Tensor, rev: bool) -> torch.Tensor:
    """fp32 row sums of ``v`` [T, n] in the shape of the kernels' reduction but another order: column c belongs to
    lane c % 64, a lane adds its columns one by one (last first with ``rev``), the 64 lanes meet in a tree (halves
    first, or neighbours first with ``rev``)."""
    T, n = v.shape
    per = (n + 63) // 64
    pad = torch.zeros(T, per * 64, dtype=torch.float32)
    pad[:, :n] = v
    lanes = pad.view(T, per, 64)
    acc = torch.zeros(T, 64, dtype=torch.float32)
    for i in (range(per - 1, -1, -1) if rev else range(per)):
        acc = acc + lanes[:, i]
    while acc.shape[1] > 1:
        h = acc.shape[1] // 2
        acc = (acc[:, 0::2] + acc[:, 1::2]) if rev else (acc[:, :h] + acc[:, h:])
    return acc


def ln_fwd_emul(x, w, b, eps: float, rev: bool) -> dict:
    """fp32 emulation of the forward (two-pass variance, bf16 output)."""
    x = x.float()
    d = x.shape[1]
    mu = _lane_sum(x, rev) / d
    z = x - mu
    rstd = torch.rsqrt(_lane_sum(z * z, rev) / d + torch.tensor(eps, dtype=torch.float32))
    o = z * rstd
    if w is not None:
        o = o * w + b
    return {"y": o.bfloat16(), "mean": mu[:, 0], "rstd": rstd[:, 0]}


def ln_bwd_emul(dy, x, mean, rstd, w, rev: bool, dres=None, dx0=None, dy2=None, dw0=None, db0=None, xh16=False) -> dict:
    """fp32 emulation of the backward; dw / db add the rows one by one (last first with ``rev``)."""
    dyt = dy.float() if dy2 is None else dy.float() + dy2
    T, d = dyt.shape
    rs = rstd.view(T, 1)
    xh = x.float() if xh16 else (x - mean.view(T, 1)) * rs
    g = dyt if w is None else dyt * w
    c1 = _lane_sum(g, rev) / d
    c2 = _lane_sum(g * xh, rev) / d
    o = rs * (g - c1 - xh * c2)
    if dres is not None:
        o = o + dres
    if dx0 is not None:
        o = dx0 + o
    dw = torch.zeros(d) if dw0 is None else dw0.clone()
    db = torch.zeros(d) if db0 is None else db0.clone()
    sw, sb = torch.zeros(d), torch.zeros(d)
    for t in (range(T - 1, -1, -1) if rev else range(T)):
        sw = sw + dyt[t] * xh[t]
        sb = sb + dyt[t]
    return {"dx": o, "dw": dw + sw, "db": db + sb}


def ln_bwd_check(got: dict, ref: dict) -> dict:
    out = {"dx": bad_bound(got["dx"], ref["dx"], ref["tol_dx"])}
    if got.get("dw") is not None:
        out["dw"] = bad_bound(got["dw"], ref["dw"], ref["tol_dw"])
        out["db"] = bad_bound(got["db"], ref["db"], ref["tol_db"])
    return out


def sel_dead(T: int, S: int, mask: int) -> torch.Tensor:
    """bool [T]: base rows whose position (row % S) has its bit set in ``mask``."""
    return torch.tensor([bool((mask >> (r % S)) & 1) for r in range(T)])


# ================================================================================================ cross-entropy
CE_V = [1, 3, 7, 8, 9, 255, 257, 1023, 1025, 4097, 8200]
CE_R = [1, 3, 8]
CE_FAMILIES = ["random", "offset", "equal", "ties", "masked_block", "masked_scatter"]
CE_LAYOUTS = ["dense", "plus3", "pad8", "offset1"]


def pad8(V: int) -> int:
    return (V + 7) // 8 * 8


def ce_label_columns(V: int):
    """The label placements: 0, V - 1, the vector/scalar seam 4 (V / 4) and the column before it."""
    seam = 4 * (V // 4)
    return sorted({0, V - 1, min(seam, V - 1), max(seam - 1, 0)})


def ce_tie_columns(V: int):
    """Columns that repeat the maximum: around a float4, a thread's 4 * 1024 stride, a wave (4 * 64) and the seam."""
    seam = 4 * (V // 4)
    cand = [3, 4, 255, 256, 4095, 4096, seam - 1, seam, V - 1]
    return sorted({c for c in cand if 0 <= c < V})


def ce_inputs(family: str, R: int, V: int, seed: int):
    """fp32 logits [R, V], labels [R] (int64), ``want_amax`` (None: the reference argmax)."""
    g = gen(seed)
    x = (4.0 * torch.randn(R, V, generator=g)).float()
    cols = ce_label_columns(V)
    labels = torch.tensor([cols[r % len(cols)] for r in range(R)], dtype=torch.int64)
    if family == "offset":
        x = (x + 1e4).float()
    elif family == "equal":
        x = torch.full((R, V), 2.5) + torch.arange(R).float().view(R, 1)
    elif family == "ties":
        x = x.clamp(max=6.0)
        tc = ce_tie_columns(V)
        for r in range(R):  # row r starts the run of maxima at its r-th tie column
            x[r, tc[r % len(tc):]] = 9.0
    elif family in ("masked_block", "masked_scatter"):
        if family == "masked_block":
            dead = torch.zeros(V, dtype=torch.bool)
            dead[V // 4:V // 4 + V // 2] = True
        else:
            dead = torch.arange(V) % 3 == 1
            dead[4::4096] = dead[5::4096] = dead[6::4096] = dead[7::4096] = True  # the whole share of thread 1
        dead[labels] = False
        if bool(dead.all()):
            dead[:] = False
        x[:, dead] = NINF
    return x, labels


def ce_ref(x, labels, gs: float, inv_rows: float, wrong: str = "") -> dict:
    """Float64 cross-entropy forward and gradient of fp32 logits [R, V].  ``gs`` / ``inv_rows`` are rounded to fp32 as
    the kernel's arguments are.  The gradient is that of the fp32 rounding of the reference lse (``lse32``)."""
    x = x.double()
    R, V = x.shape
    gs = float(torch.tensor(gs, dtype=torch.float32))
    inv = float(torch.tensor(inv_rows, dtype=torch.float32))
    xl = x[:, :V - 1] if wrong == "lse_drop_last" and V > 1 else x
    if wrong == "lse_reads_pad":
        xl = torch.cat([x, x.new_full((R, 1), NAN)], 1)
    lse = torch.logsumexp(xl, 1)
    mx = x.max(1, keepdim=True).values
    idx = torch.arange(V).expand(R, V)
    if wrong == "tie_highest":
        amax = torch.where(x == mx, idx, torch.full_like(idx, -1)).max(1).values
    else:
        amax = torch.where(x == mx, idx, torch.full_like(idx, V)).min(1).values
    xlab = x.gather(1, labels.view(R, 1))[:, 0]
    loss = lse - xlab
    lse32 = lse.float()
    a = x - lse32.double().view(R, 1)
    p = torch.exp(a)
    lab = (labels + 1) % V if wrong == "onehot_shift" else labels
    onehot = (idx == lab.view(R, 1)).double()
    scale = abs(gs) * (1.0 if wrong == "no_inv_rows" else inv)
    grad = (p - onehot) * gs * (1.0 if wrong == "no_inv_rows" else inv)
    out = {"lse": lse, "loss": loss, "amax": amax, "lse32": lse32, "grad": grad}
    if wrong:
        return out
    tol_lse = LSE_TOL * lse.abs().clamp(min=1.0)
    fin = torch.isfinite(a)
    tol_g = scale * p * (CE_C1 * 2 * E + CE_C2 * E * torch.where(fin, a.abs(), torch.zeros_like(a))) \
        + 3 * E * grad.abs() + scale * 2.0 ** -126
    tol_g = torch.where(fin, tol_g * SLACK, torch.zeros_like(tol_g))  # columns at -inf: exactly zero
    out.update(tol_lse=tol_lse, tol_loss=tol_lse + E * (lse.abs() + loss.abs()) * SLACK, tol_grad=tol_g,
               tol_grad16=(tol_g + U * grad.abs()) * (1 + U))
    return out


def ce_fwd_emul(x, labels, rev: bool) -> dict:
    """fp32 emulation: max, then the exponentials added one by one (last first with ``rev``)."""
    x = x.float()
    R, V = x.shape
    m = x.max(1).values
    s = torch.zeros(R)
    for j in (range(V - 1, -1, -1) if rev else range(V)):
        s = s + torch.exp(x[:, j] - m)
    lse = m + torch.log(s)
    amax = torch.where(x == m.view(R, 1), torch.arange(V).expand(R, V), torch.full((R, V), V)).min(1).values
    return {"lse": lse, "loss": lse - x.gather(1, labels.view(R, 1))[:, 0], "amax": amax}


def ce_bwd_emul(x, labels, lse32, gs: float, inv_rows: float) -> torch.Tensor:
    x = x.float()
    R, V = x.shape
    p = torch.exp(x - lse32.view(R, 1))
    onehot = (torch.arange(V).expand(R, V) == labels.view(R, 1)).float()
    return (p - onehot) * torch.tensor(gs, dtype=torch.float32) * torch.tensor(inv_rows, dtype=torch.float32)


def ce_fwd_check(got: dict, ref: dict) -> dict:
    out = {}
    if got.get("lse") is not None:
        out["lse"] = bad_bound(got["lse"], ref["lse"], ref["tol_lse"])
    if got.get("loss") is not None:
        out["loss"] = bad_bound(got["loss"], ref["loss"], ref["tol_loss"])
    if got.get("amax") is not None:
        out["amax"] = got["amax"].long() != ref["amax"]
    return out


def ce_out(R: int, ld_out: int, dtype, device="cpu", spare: int = 16):
    """Prefilled flat gradient buffer of R rows of stride ``ld_out`` plus ``spare`` elements, and a copy of it."""
    buf = filled((R * ld_out + spare,), dtype, device)
    return buf, buf.clone()


def ce_grad_check(buf: torch.Tensor, prefill: torch.Tensor, ref: dict, R: int, V: int, ld_out: int) -> dict:
    """``buf`` flat (see :func:`ce_out`): columns [0, V) of every row within the bound, the pad columns [V, ld_out)
    exactly zero, everything past the last row untouched."""
    key = "tol_grad16" if buf.dtype == torch.bfloat16 else "tol_grad"
    rows = buf[:R * ld_out].view(R, ld_out)
    return {"grad": bad_bound(rows[:, :V], ref["grad"], ref[key]),
            "pad": bad_bits(rows[:, V:], torch.zeros_like(rows[:, V:])),
            "beyond": bad_bits(buf[R * ld_out:], prefill[R * ld_out:])}


def ce_layout(x: torch.Tensor, layout: str):
    """(logits view [R, V] inside a NaN-filled buffer, ld): dense, ld = V + 3, ld = pad8(V) + 8, base offset by one
    float (dense rows)."""
    R, V = x.shape
    ld = {"dense": V, "plus3": V + 3, "pad8": pad8(V) + 8, "offset1": V}[layout]
    off = 1 if layout == "offset1" else 0
    flat = torch.full((off + R * ld + 4,), NAN, dtype=torch.float32, device=x.device)
    view = flat[off:off + R * ld].view(R, ld)[:, :V]
    view.copy_(x)
    return view, ld


# ================================================================================================ fused Adam
ADAM_T = [1, 2, 3, 10, 10000]
ADAM_RUNS = [1, 255, 256, 257, 1023, 1024, 1025]  # live-row runs of the restricted embedding, in float4 groups
ADAM_HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)


def adam_model():
    """Tiny ModuleDict: an embedding of one float4 per row whose live rows (see :func:`adam_live_rows`) cut the arena
    into spans of ADAM_RUNS float4 groups (1025 = 1024 + 1), and a Linear whose weight (21) and bias (3) are no
    multiple of 4."""
    torch.manual_seed(0)
    rows = sum(ADAM_RUNS) + len(ADAM_RUNS)
    return torch.nn.ModuleDict({"emb": torch.nn.Embedding(rows, 4), "lin": torch.nn.Linear(7, 3)})


def adam_live_rows() -> torch.Tensor:
    live, r = [], 0
    for n in ADAM_RUNS:
        live += list(range(r, r + n))
        r += n + 1  # one dead row after every run
    return torch.tensor(live)


def f32(v: float) -> float:
    return float(torch.tensor(v, dtype=torch.float32))


def adam_masks(flat, restricted: bool = True):
    """(param, active) bool [numel] of a FlatParams arena: elements that belong to a parameter (the rest is the
    padding between slots), and elements inside the optimizer's spans (everything but the restricted rows)."""
    param = torch.zeros(flat.numel, dtype=torch.bool)
    for p in flat.params:
        o = flat.offset_of(p)
        param[o:o + p.numel()] = True
    active = torch.ones(flat.numel, dtype=torch.bool)
    if restricted:
        for a, b in flat.inactive_ranges():
            active[a:b] = False
    return param, active


def adam_state(family: str, n: int, active: torch.Tensor, seed: int, param=None) -> dict:
    """fp32 p, g, m, v [n]: g, m, v hold values on ``active`` parameter elements and zero elsewhere (a restricted row
    never receives gradient); p holds a value on every parameter element and zero in the padding."""
    gn = gen(seed)
    p = torch.randn(n, generator=gn).float()
    if param is not None:
        p = torch.where(param, p, torch.zeros(()))
        active = active & param
    s = 1e-12 if family == "tiny" else 1.0
    g = (s * torch.randn(n, generator=gn)).float()
    m = (0.3 * s * torch.randn(n, generator=gn)).float()
    v = (0.1 * s * s * torch.rand(n, generator=gn)).float()
    if family in ("inf", "nan"):
        g[int(active.nonzero()[len(active.nonzero()) // 2])] = float(family)
    z = torch.zeros(())
    return {"p": p, "g": torch.where(active, g, z), "m": torch.where(active, m, z), "v": torch.where(active, v, z)}


def adam_ref(p, g, m, v, t: int, *, lr, b1, b2, eps, wd=0.0, clip=None, active=None, wrong: str = "") -> dict:
    """One float64 Adam step (torch semantics) from the given fp32 state with fp32-rounded hyper-parameters; the
    global norm runs over ``active`` elements.  Returns p, m, v, the bf16 mirror and their bounds."""
    p0, g, m, v = (a.double() for a in (p, g, m, v))
    lr, b1, b2, eps, wd = (f32(a) for a in (lr, b1, b2, eps, wd))
    act = torch.ones_like(p0, dtype=torch.bool) if active is None else active
    ssq = (g[act] ** 2).sum()
    coef, rel_coef = 1.0, 0.0
    if clip:
        c = f32(clip) / ((ssq if wrong == "coef_sq" else torch.sqrt(ssq)) + f32(1e-6))
        if wrong == "coef_sq" or float(c) < 1.0:
            coef, rel_coef = float(c), (NSQ / 2 + 3) * E
    if wrong == "t_off":
        t = t + 1
    gc = g * coef
    gr = (g + wd * p0) * coef if wrong == "decay_unclipped" else gc + wd * p0
    m1 = b1 * m + (1 - b1) * gr
    v1 = b2 * v + (1 - b2) * gr * gr
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    bc2s = bc2 if wrong == "bc2_no_sqrt" else math.sqrt(bc2)
    stepsz = lr / bc1
    den = torch.sqrt(v1 / bc2 + eps) if wrong == "eps_in_sqrt" else torch.sqrt(v1) / bc2s + eps
    upd = stepsz * m1 / den
    p1 = p0 - upd
    out = {"p": torch.where(act, p1, p0), "m": torch.where(act, m1, m), "v": torch.where(act, v1, v)}
    out["mirror"] = (p0 if wrong == "mirror_early" else out["p"]).float().bfloat16()
    if wrong:
        return out
    r1 = 0.0 if t == 1 else (POW_K * 2 * E * b1 ** t + E) / bc1
    r2 = 0.0 if t == 1 else (POW_K * 2 * E * b2 ** t + E) / bc2
    tol_gr = gc.abs() * (rel_coef + E) + 2 * E * (wd * p0).abs() + E * gr.abs()
    tol_m = (1 - b1) * tol_gr + E * ((b1 * m).abs() + ((1 - b1) * gr).abs() + m1.abs())
    tol_v = (1 - b2) * 2 * gr.abs() * tol_gr + E * ((b2 * v).abs() + 2 * (1 - b2) * gr * gr + v1.abs())
    tol_v = tol_v + torch.where(gr != 0, 2.0 ** -125, 0.0)  # gr^2 of the tiny family may be denormal (flushed or not)
    sq = torch.sqrt(v1)
    d_sq = tol_v / (2 * sq).clamp(min=1e-300) + E * sq
    q = sq / bc2s
    d_den = d_sq / bc2s + q * (r2 / 2 + 2 * E) + E * den
    d_upd = upd.abs() * (r1 + 3 * E + d_den / den) + stepsz * tol_m / den
    tol_p = d_upd + E * p1.abs()
    zero = torch.zeros_like(p0)
    out.update(tol_p=torch.where(act, tol_p * SLACK, zero), tol_m=torch.where(act, tol_m * SLACK, zero),
               tol_v=torch.where(act, tol_v * SLACK, zero))
    return out


def adam_emul(p, g, m, v, t: int, *, lr, b1, b2, eps, wd=0.0, clip=None, active=None, rev=False) -> dict:
    """fp32 emulation of the fused step (the squares added one by one, last first with ``rev``)."""
    F = lambda a: torch.tensor(a, dtype=torch.float32)  # noqa: E731
    lr, b1, b2, eps, wd = F(lr), F(b1), F(b2), F(eps), F(wd)
    act = torch.ones_like(p, dtype=torch.bool) if active is None else active
    coef = F(1.0)
    if clip:
        sq = (g[act] * g[act]).view(-1, 4)  # one float4 group per thread pass, groups then joined in fp64-free fp32
        part = (sq[:, 0] + sq[:, 1]) + (sq[:, 2] + sq[:, 3])
        part = part.flip(0) if rev else part
        blocks = part.split(256)
        s = F(0.0)
        for blk in blocks:
            s = s + _lane_sum(blk.view(1, -1), rev)[0, 0]
        coef = torch.minimum(F(1.0), F(clip) / (torch.sqrt(s) + F(1e-6)))
    gr = g * coef
    if float(wd) != 0.0:
        gr = gr + wd * p
    m1 = b1 * m + (1 - b1) * gr
    v1 = b2 * v + (1 - b2) * gr * gr
    tt = F(float(t))
    bc1 = 1 - torch.pow(b1, tt)
    bc2s = torch.sqrt(1 - torch.pow(b2, tt))
    p1 = p - (lr / bc1) * m1 / (torch.sqrt(v1) / bc2s + eps)
    out = {"p": torch.where(act, p1, p), "m": torch.where(act, m1, m), "v": torch.where(act, v1, v)}
    out["mirror"] = out["p"].bfloat16()
    return out


def adam_check(got: dict, ref: dict, active: torch.Tensor) -> dict:
    """p, m, v within their bounds on the active elements and bit-identical (tolerance 0) elsewhere; the mirror
    bitwise the bf16 rounding of the kernel's own p on the active elements."""
    out = {k: bad_bound(got[k], ref[k], ref["tol_" + k]) for k in ("p", "m", "v")}
    out["mirror"] = bad_bits(got["mirror"], got["p"].bfloat16()) & active
    return out
