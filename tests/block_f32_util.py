"""Helpers shared by the tests of the fp32 block kernels: the ``EPI_GELU`` / ``EPI_DGELU`` epilogues of
csrc/gemm_f32.hip and the LayerNorm and dgelu kernels of csrc/block_f32.hip (tests/test_block_f32_kernel.py on the GPU,
tests/test_block_f32_ref.py on the CPU).  Conventions are those of tests/kern_exact_util.py and tests/misc_exact_util.py:
float64 references of the same fp32 inputs, comparators that return the mask of bad elements (NaN counts as bad),
``E`` = 2^-24 (half an fp32 ulp, one rounding to nearest), ``TINY`` = 2^-126, every bound times ``SLACK``.

gelu_new, fp32 in and out (``gelu_new_f`` / ``gelu_new_grad_f`` of csrc/common.h).  The analysis is that of
``misc_exact_util.gelu_ref`` (it holds for any fp32 input, not only bf16 values): ``rel_s``, the relative error of
``s = rcp(1 + exp2(-m))``, and the flushed-denormal terms are taken from there unchanged.  Its bf16 store term
``U |ref|`` is replaced by an fp32 one, ``E |ref|`` (the store itself does not round; the term is kept as a margin
for the product ``x * s``, which the base bound already counts once):

* forward ``tol = E |ref| + |ref| (rel_s + E) + |x| min(s, TINY) + TINY``, i.e. ``gelu_ref``'s bound with U -> E.
* derivative ``dtol`` unchanged (it is the bound of the fp32 derivative itself); a product ``g * gelu'(x)`` stored
  in fp32: ``tol = |g| dtol + E |ref| + TINY``.  ``|x| <= 2^40``, the limit misc_exact_util records.

LayerNorm forward on rows of ``d`` floats.  ``n = ln_depth(d) = 4 ceil(d / 256) + 6`` bounds the additions one
element passes through in either layout (float4: 4 ceil(d / 256) serial additions per lane; one float per lane:
ceil(d / 64) <= that; 6 butterfly levels):

* ``mean = sum / d``: n additions and the division, ``tol_mean = (n + 1) E sum|x| / d``.  Call it ``dm``.
* the centred sum of squares uses the computed mean: ``sum (x - mean')^2 / d = var + (mean' - mean)^2`` exactly, every
  term non-negative.  ``c = x - mean'`` rounds once (twice in the square: 2 E), ``fma(c, c, q)`` once per addition
  (n E), the division (E): ``|var' - var| <= (var + dm^2) (n + 3) E + dm^2``; ``+ eps`` rounds once more:
  ``a_ve = (var + dm^2) (n + 3) E + dm^2 + E (var + eps)``, ``rel = a_ve / (var + eps)``.
* ``rstd = 1 / sqrt(var + eps)``: ``(v (1 + r))^-1/2`` moves by at most ``0.5 r / (1 - r)`` relative; the square root
  and the division are within 1 ulp = 2 E each whatever sequence the compiler emits:
  ``tol_rstd = rstd (0.5 rel / (1 - rel) + 4 E)``.
* ``xhat' = (x - mean') * rstd'``: the subtraction carries ``dm`` and one rounding, the product one more:
  ``e_xh = rstd (dm + E |c|) + |xhat| (tol_rstd / rstd + E)``; ``y = fma(xhat', w, b)`` rounds once:
  ``tol_y = |w| e_xh + E |y|`` (LNPre: ``e_xh``), ``+ TINY``.

LayerNorm backward; ``mean`` and ``rstd`` are the fp32 values the kernel is handed (exact inputs):

* ``xhat' = (x - mean) * rstd`` 2 E relative, ``g' = dy * w`` E relative (0 without w).
* ``m1 = sum g / d``: ``tol_m1 = (n + 2) E sum|g| / d``; ``m2 = sum fma(g, xhat, .) / d``: terms 3 E, chain n E,
  division E: ``tol_m2 = (n + 4) E sum|g xhat| / d``.
* ``inner = fma(-xhat, m2, g - m1)``: ``g - m1`` carries E |g|, tol_m1 and its rounding E (|g| + |m1|); the product
  ``|xhat| tol_m2 + 2 E |xhat m2|``; the fma's rounding E (|g| + |m1| + |xhat m2|):
  ``tol_inner = E (3 |g| + 2 |m1| + 3 |xhat m2|) + tol_m1 + |xhat| tol_m2``; ``dx = rstd * inner`` rounds once:
  ``tol_dx = rstd tol_inner + E |dx| + TINY``.
* ``dw = sum_rows dy xhat``: a block adds its R = ``PART_ROWS`` rows one by one (fma), the second kernel the
  ``ceil(T / R)`` partials one by one: ``N = min(T, R) + ceil(T / R)`` additions, terms 2 E:
  ``tol_dw = (N + 2) E sum|dy xhat|``, ``tol_db = N E sum|dy|``, ``+ TINY``.

The emulations evaluate the kernels' own expressions in fp32 torch on the CPU in the kernels' order: a lane adds its
items in index order, the 64 lanes meet in the xor butterfly (32, 16, ..., 1), partials are added in block order.
"""
import torch

import misc_exact_util as M
from kern_exact_util import E, SLACK, U, bad_bits, bad_bound, gen, ln_depth  # noqa: F401

F32 = torch.float32
TINY = 2.0 ** -126
PART_ROWS = 32  # iit_ln_f32_part_rows(): asserted against the library on the GPU
LN_D = [1, 3, 64, 68, 260, 768, 1023, 4096]
LN_T = [1, 5, 9]
LN_EPS = 1e-5
DGELU_N = [1, 7, 4096 + 3]


# ================================================================================================ gelu_new in fp32
def gelu_inputs(n: int, seed: int) -> torch.Tensor:
    """``n`` fp32 pre-activations: spread over [-12, 12], with +-2^20, +-2^40, +-0 and a denormal among the first."""
    x = (torch.rand(n, generator=gen(seed), dtype=torch.float64) * 24.0 - 12.0).float()
    special = torch.tensor([2.0 ** 20, -2.0 ** 20, 2.0 ** 40, -2.0 ** 40, 0.0, -0.0, 2.0 ** -130, -12.0, 12.0], dtype=F32)
    k = min(n, special.numel())
    x[:k] = special[:k]
    return x


def gelu_ref(x: torch.Tensor) -> dict:
    """float64 gelu_new and derivative of fp32 ``x`` with the fp32 bounds: ``y``, ``tol``, ``dy``, ``dtol``."""
    r = M.gelu_ref(x, "new")
    ay = r["y"].abs()
    tol = r["tol"] / SLACK - U * ay + E * ay  # the bf16 store term replaced by an fp32 one
    return {"y": r["y"], "tol": tol * SLACK, "dy": r["dy"], "dtol": r["dtol"]}


def dgelu_ref(g: torch.Tensor, x: torch.Tensor) -> dict:
    """float64 ``g * gelu_new'(x)`` and its bound ``|g| dtol + E |ref| + TINY``."""
    r = gelu_ref(x)
    y = g.double() * r["dy"]
    return {"y": y, "tol": (g.double().abs() * r["dtol"] + E * y.abs() + TINY) * SLACK}


def _f(v: float) -> torch.Tensor:
    return torch.tensor(v, dtype=F32)


def _sig2u(x: torch.Tensor, x2: torch.Tensor) -> torch.Tensor:
    m = x * (_f(0.10294324) * x2 + _f(2.3022082))
    return 1.0 / (1.0 + torch.exp2(-m))


def gelu_emul(x: torch.Tensor) -> torch.Tensor:
    """fp32 emulation of ``gelu_new_f``."""
    x = x.float()
    return x * _sig2u(x, x * x)


def dgelu_emul(g: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """fp32 emulation of ``g * gelu_new_grad_f(x)``."""
    x = x.float()
    x2 = x * x
    s = _sig2u(x, x2)
    du = _f(0.21406445) * x2 + _f(1.5957691)
    return g.float() * ((x * du) * (s - s * s) + s)


# ================================================================================================ LayerNorm
LN_FAMILIES = ["random", "offset", "equal"]


def ln_inputs(family: str, T: int, d: int, seed: int, affine: bool):
    """fp32 ``x [T][d]``, ``w``, ``b`` (None without affine).  ``offset``: row 0 sits at 2^12 (the centred second
    pass); ``equal``: row 0 is one value repeated (variance 0, eps alone)."""
    g = gen(seed)
    x = torch.randn(T, d, generator=g).float()
    if family == "offset":
        x[0] = x[0] + 4096.0
    elif family == "equal":
        x[0] = 1.375
    w = b = None
    if affine:
        w = (1.0 + 0.5 * torch.randn(d, generator=g)).float()
        b = (0.5 * torch.randn(d, generator=g)).float()
    return x, w, b


def ln_fwd_ref(x, w, b, eps: float) -> dict:
    x = x.double()
    T, d = x.shape
    n = ln_depth(d)
    mean = x.mean(1)
    dm = (n + 1) * E * x.abs().sum(1) / d
    c = x - mean[:, None]
    var = (c * c).mean(1)
    ve = var + eps
    a_ve = (var + dm * dm) * (n + 3) * E + dm * dm + E * ve
    rel = a_ve / ve
    rstd = ve.rsqrt()
    tol_rstd = rstd * (0.5 * rel / (1 - rel) + 4 * E)
    xhat = c * rstd[:, None]
    e_xh = rstd[:, None] * (dm[:, None] + E * c.abs()) + xhat.abs() * (tol_rstd / rstd + E)[:, None]
    if w is None:
        y, tol_y = xhat, e_xh
    else:
        y = xhat * w.double() + b.double()
        tol_y = w.double().abs() * e_xh + E * y.abs()
    return {"mean": mean, "rstd": rstd, "y": y, "tol_mean": dm * SLACK + TINY, "tol_rstd": tol_rstd * SLACK,
            "tol_y": tol_y * SLACK + TINY}


def ln_bwd_ref(dy, x, mean, rstd, w) -> dict:
    dy, x = dy.double(), x.double()
    T, d = x.shape
    n = ln_depth(d)
    rs = rstd.double()[:, None]
    xhat = (x - mean.double()[:, None]) * rs
    g = dy if w is None else dy * w.double()
    m1 = g.mean(1, keepdim=True)
    m2 = (g * xhat).mean(1, keepdim=True)
    tol_m1 = (n + 2) * E * g.abs().sum(1, keepdim=True) / d
    tol_m2 = (n + 4) * E * (g * xhat).abs().sum(1, keepdim=True) / d
    dx = rs * (g - m1 - xhat * m2)
    xm = (xhat * m2).abs()
    tol_inner = E * (3 * g.abs() + 2 * m1.abs() + 3 * xm) + tol_m1 + xhat.abs() * tol_m2
    N = min(T, PART_ROWS) + -(-T // PART_ROWS)
    return {"dx": dx, "tol_dx": (rs * tol_inner + E * dx.abs()) * SLACK + TINY,
            "dw": (dy * xhat).sum(0), "tol_dw": (N + 2) * E * (dy * xhat).abs().sum(0) * SLACK + TINY,
            "db": dy.sum(0), "tol_db": N * E * dy.abs().sum(0) * SLACK + TINY}


def _wave_sum(v: torch.Tensor, vec: bool) -> torch.Tensor:
    """fp32 row sums of ``v [T][n]`` in the kernels' order.  One float per lane: element i belongs to lane i % 64;
    float4: element i belongs to lane (i // 4) % 64; a lane adds its elements in index order starting from 0, then the
    xor butterfly."""
    T, n = v.shape
    group = 4 if vec else 1
    per = -(-n // (64 * group))
    pad = torch.zeros(T, per * 64 * group, dtype=F32)
    pad[:, :n] = v
    lanes = pad.view(T, per, 64, group)
    acc = torch.zeros(T, 64, dtype=F32)
    for i in range(per):
        for k in range(group):
            acc = acc + lanes[:, i, :, k]
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, idx ^ o]
    return acc[:, 0]


def ln_fwd_emul(x, w, b, eps: float, vec: bool) -> dict:
    x = x.float()
    d = x.shape[1]
    mu = _wave_sum(x, vec) / _f(float(d))
    c = x - mu[:, None]
    rs = 1.0 / torch.sqrt(_wave_sum(c * c, vec) / _f(float(d)) + _f(eps))
    y = c * rs[:, None]
    if w is not None:
        y = y * w + b
    return {"mean": mu, "rstd": rs, "y": y}


def ln_bwd_emul(dy, x, mean, rstd, w, vec: bool) -> dict:
    dy, x = dy.float(), x.float()
    T, d = x.shape
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy if w is None else dy * w
    m1 = _wave_sum(g, vec) / _f(float(d))
    m2 = _wave_sum(g * xh, vec) / _f(float(d))
    dx = rstd[:, None] * ((g - m1[:, None]) - xh * m2[:, None])
    dw = db = None
    for r0 in range(0, T, PART_ROWS):
        pw, pb = torch.zeros(d, dtype=F32), torch.zeros(d, dtype=F32)
        for r in range(r0, min(T, r0 + PART_ROWS)):
            pw = pw + dy[r] * xh[r]
            pb = pb + dy[r]
        dw, db = (pw, pb) if dw is None else (dw + pw, db + pb)
    return {"dx": dx, "dw": dw, "db": db}


def ln_fwd_check(got: dict, ref: dict) -> dict:
    return {k: bad_bound(got[k], ref[k], ref["tol_" + k]) for k in ("y", "mean", "rstd")}


def ln_bwd_check(got: dict, ref: dict, affine: bool) -> dict:
    return {k: bad_bound(got[k], ref[k], ref["tol_" + k]) for k in (("dx", "dw", "db") if affine else ("dx",))}


def selector_case(T: int, d: int, seed: int):
    """An integer case every kernel expression evaluates exactly (``eps = 0``): rows ``m + a sgn`` with as many +1 as
    -1 (d even), m a small integer and a a power of two, so mean = m, var = a^2, rstd = 1 / a and xhat = sgn; w powers
    of two, b and dy small integers.  With d a power of two the backward's two row means are exact as well.  Returns
    ``x, w, b, dy`` and the exact results (built from m, a and sgn, not recomputed from x)."""
    assert d % 2 == 0
    g = gen(seed)
    sgn = torch.ones(T, d)
    for r in range(T):
        sgn[r, torch.randperm(d, generator=g)[:d // 2]] = -1.0
    m = torch.randint(-8, 9, (T, 1), generator=g).float()
    pow2 = torch.tensor([0.25, 0.5, 1.0, 2.0, 4.0])
    a = pow2[torch.randint(0, 5, (T, 1), generator=g)]
    x = m + a * sgn
    w = pow2[torch.randint(0, 5, (d,), generator=g)] * (1.0 - 2.0 * torch.randint(0, 2, (d,), generator=g))
    b = torch.randint(-4, 5, (d,), generator=g).float()
    dy = torch.randint(-3, 4, (T, d), generator=g).float()
    sd, wd, gd = sgn.double(), w.double(), dy.double() * w.double()
    ref = {"mean": m[:, 0], "rstd": 1.0 / a[:, 0], "y": (sd * wd + b.double()).float(), "dw": (dy.double() * sd).sum(0).float(),
           "db": dy.double().sum(0).float(),
           "dx": ((gd - gd.mean(1, keepdim=True) - sd * (gd * sd).mean(1, keepdim=True)) / a.double()).float()}
    return x.float(), w.float(), b, dy, ref


def strided_rows(x: torch.Tensor, ld: int, offset: int, device) -> torch.Tensor:
    """``x [T][d]`` as a view of a NaN-filled buffer with row pitch ``ld`` starting ``offset`` floats into it."""
    T, d = x.shape
    buf = torch.full((offset + T * ld,), float("nan"), dtype=F32, device=device)
    view = buf[offset:].view(T, ld)[:, :d]
    view.copy_(x)
    return view
