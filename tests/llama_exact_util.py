"""Helpers shared by the exact tests of the Llama-family kernels of csrc/llama_ops.hip: RMSNorm forward / backward and
its two weight-gradient kernels, the two rotary kernels, SwiGLU forward / backward, and the producer-side splice
kernels ``swiglu_splice_*`` / ``embed_splice_*`` (tests/test_rms_exact.py, tests/test_rotary_exact.py,
tests/test_swiglu_exact.py and tests/test_llama_splice_exact.py on the GPU, tests/test_llama_exact_ref.py on the CPU).
Conventions are those of tests/kern_exact_util.py and tests/misc_exact_util.py: float64 references of the same bf16 /
fp32 inputs, comparators that return the mask of bad elements (NaN and the buffer sentinel count as bad), ``E`` = 2^-24,
``U`` = 2^-8, every bound times ``SLACK``.  ``v_exp_f32``, ``v_rcp_f32`` and ``v_rsq_f32`` are taken as 1 ulp = 2 E
each, ``__expf`` as a product by log2(e) plus the hardware exp2; a denormal intermediate or result may be flushed (the
``2^-126`` terms).

RMSNorm (one wave per row; a lane adds the 8 squares of each of its ceil(d / 512) chunks serially, six shuffle levels
join the lanes: ``depth(d) = 8 ceil(d / 512) + 6`` additions on the longest path):

* forward, ``r = rsqrt(mean(x^2) + eps)``: every term is non-negative, so the sum is good to (depth + 1) E relative (the
  squares and the additions); ``/ d`` and ``+ eps`` add one each, the inverse square root halves the lot, the hardware
  rsqrt adds 1 ulp: ``rel_r = ((depth + 1) + 2) / 2 E + 2 E``.  ``rstd_out`` is held to ``rel_r |ref|``;
  ``tol_y = |y| (U + rel_r + 2 E)`` (the products by r and by w, the bf16 store), with ``w`` given or null.
* backward (``rstd`` is an input: the reference takes the fp32 values the kernel is given), ``g = dy w``, ``xh = x r``,
  ``s = mean(g xh)``: each term carries the roundings of g, xh and their product, the sum ``depth`` additions, then
  ``/ d``: ``tol_s = (depth + 3) E mean|g xh| + E |s|``.  ``core = r (g - xh s)`` rounding by rounding:
  ``tol_dx = r (|xh| tol_s + 2 E |xh s| + E |g| + E |g - xh s|) + E |core| [+ E |core + dres|] + ST |dx|`` -- the error
  of s, the rounding of xh and of the product ``xh s``, the rounding of g, the subtraction, the product by r, the
  ``dres`` add where there is one, and the store: ST = U for a bf16 ``x`` (dx has x's type), E for fp32.
* ``dw`` (``rms_dw_vec_kernel`` and, under ``IIT_LLAMA_VEC=0``, ``rms_dw_kernel``): an order-free sum over T,
  ``tol = (T + 4) E (sum_t |dy x rstd| + |dw0|)`` as ``tol_dw`` of the layer norm.  The ``exact`` family has integer
  ``dy`` and ``x`` (|.| <= 64), ``rstd`` in {1, 2, 4} per row and an integer prefill, so every partial sum is an
  integer below 2^24 (``int_operand`` checks (T + 1) 64 * 4 * 64) and the result is the float64 sum bit for bit.

Rotary, arbitrary tables ``cos`` / ``sin`` [n_ctx, rd] (pairs (i0, i1) = (j, j + rd / 2) or (2j, 2j + 1); ``sign`` = -1
for the inverse): ``out[i0] = x[i0] cos[i0] - sign x[i1] sin[i0]``, ``out[i1] = x[i1] cos[i1] + sign x[i0] sin[i1]``,
``tol = U |ref| + E (|x cos| + |x sin| + |ref|)`` -- two products, the addition (an fma only removes a rounding), the
bf16 store; the product by ``sign`` is exact.  Features from ``rd`` on are compared bit for bit.  The tables of the
tests hold different values in every entry (the model's tables repeat each angle for both elements of a pair, which
hides a read at the partner's index) and NaN in every row outside [offset, offset + S).  ``exact`` family: integer x
with |x| <= 32 and table entries from {0, +-1, +-1/2, +-1/4}: every result is a multiple of 1/4 of magnitude <= 64,
exact in bf16, compared bitwise.

SwiGLU, ``s = 1 / (1 + exp(-g))``: the exponent ``-g log2(e)`` carries the product and the constant (1.5 E |g|), the
hardware exp2 2 E; an error of ``q = exp(-g)`` moves s by (1 - s) of it; ``1 + q`` and the rcp add E + 2 E:
``rel_s = (1 - s) (1.5 |g| + 2) E + 3 E``; ``fl = min(s, 2^-126)`` (a denormal s may be flushed).

* ``post = g s u``: ``U |ref| + |ref| (rel_s + 2 E) + |g u| fl + 2^-126``; ``dup = dv g s``: the same with ``|dv g|``.
* ``dgate = dv u s h``, ``h = 1 + g (1 - s)``: ``ds = s rel_s + fl``, ``tol_h = |g| (ds + 2 E (1 - s)) + E |h|``,
  ``tol = |dv u| (ds |h| + s tol_h) + (3 E + U) |ref| + 2^-126``.  The absolute term ``|dv u| s tol_h`` keeps the bound
  honest where h cancels (``silu'`` has its zero at g = -1.278).
* Inputs: every finite bf16 ``g`` with |g| <= 2^40 (42754 values; beyond, ``dv * g`` overflows in the kernel's order, as
  recorded for GELU in tests/misc_exact_util.py), ``u`` and ``dv`` normal.

Splice kernels (spec from ``patch_spec`` of an ``Ix`` index over [B, S, d], d % 8 == 0; the reference mask is built by
torch indexing, not from the range table): ``swiglu_splice_fwd`` -- selected elements are ``src`` bit for bit, the
others within the SwiGLU bound; ``swiglu_splice_bwd`` -- selected ``dgate`` / ``dup`` are == 0; ``embed_splice_fwd`` --
``W16[tok]`` or ``src`` bit for bit; ``embed_splice_bwd`` -- an order-free sum per (token, column) over the rows of that
token that are not spliced: ``exact`` bitwise, ``random`` within ``tol_sum`` with n the number of such rows, n = 0 and
the ``ldg - d`` gap keep the prefill's bits.

Worst ``|got - ref| / bound``, fp32 emulations on the CPU (tests/test_llama_exact_ref.py) / kernels on an MI355X:
RMSNorm y 0.991 / 0.992, rstd 0.154 / 0.178, dx 0.992 / 0.992, dw 0.368 / 0.36; rotary 0.992 / 0.990 (vector) and 0.984
(per-pair); SwiGLU post 0.986 / 0.984, dup 0.990 / 0.990, dgate 0.986 / 0.991; embedding splice gradient -- / 0.264.
Wall time of the GPU modules: test_rms_exact.py 4.4 s (256 cases), test_rotary_exact.py 3.6 s (46),
test_swiglu_exact.py 4.0 s (12), test_llama_splice_exact.py 2.6 s (98), each including about 3 s of start-up.

Kernel instantiations of csrc/llama_ops.hip and a passing case that runs each:

=============================================  =================================================================
rms_fwd_kernel<1 / 2 / 4 / 8 / 16>             test_rms_exact.py::test_rms_fwd, d = 8, 512 / 520, 1024 / 1032, 2048 /
                                               2056, 4096 / 4104, 8192; x bf16 and fp32, w given and null
rms_bwd_kernel<1 / 2 / 4 / 8 / 16>             test_rms_exact.py::test_rms_bwd, the same d; dres given and null
rms_dw_vec_kernel                              test_rms_exact.py::test_rms_dw (both families, x bf16 and fp32)
rms_dw_kernel (IIT_LLAMA_VEC=0)                test_launch_variants.py only (fourth variant, test_rms_dw)
rotary_vec_kernel, halves / adjacent           test_rotary_exact.py::test_rotary[vec-*] (both families, both directions)
rotary_kernel by shape                         test_rotary_exact.py::test_rotary[scalar-*]
rotary_kernel by fallback (view, strides)      test_rotary_exact.py::test_rotary_views[offset1 / stride_odd]
rotary_kernel at vector shapes                 test_launch_variants.py only (IIT_LLAMA_VEC=0, all of test_rotary_exact)
swiglu_fwd_kernel, swiglu_bwd_kernel           test_swiglu_exact.py::test_swiglu_sweep, test_swiglu_sizes
swiglu_splice_fwd_kernel / _bwd_kernel         test_llama_splice_exact.py::test_swiglu_splice
embed_splice_fwd_kernel                        test_llama_splice_exact.py::test_embed_splice_fwd
embed_splice_bwd_kernel<__bf16>, <float>       test_llama_splice_exact.py::test_embed_splice_bwd[bf16 / f32]
=============================================  =================================================================
"""
import math

import torch

from misc_exact_util import (BF16, BF16_FILL, E, F32, FAMILIES, NAN, SLACK, TINY, U, all_bf16, bad_bits,  # noqa: F401
                             bad_bound, bad_sum, filled, gen, int_operand, strided, tol_sum)

LOG2E = 1.4426950408889634


def f32c(v: float) -> torch.Tensor:
    return torch.tensor(v, dtype=F32)


def worst(got: torch.Tensor, ref: torch.Tensor, tol: torch.Tensor) -> float:
    """Largest ``|got - ref| / tol`` (0 / 0 counts as 0, NaN as inf): the figure the docstrings record."""
    err = (got.double() - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / tol)
    return float(torch.nan_to_num(r, nan=float("inf")).max()) if r.numel() else 0.0


def count(bad: dict) -> dict:
    return {n: int(m.sum()) for n, m in bad.items() if int(m.sum())}


# ================================================================================================ RMSNorm
RMS_D = [8, 512, 520, 1024, 1032, 2048, 2056, 4096, 4104, 8192]
RMS_T = [1, 3, 5, 9]
RMS_FAMILIES = ["random", "balanced", "tiny", "large"]
RMS_EPS = 1e-5
RMS_DW_T = [1, 63, 64, 65, 129]
RMS_DW_D = [8, 56, 64, 72, 248, 256, 264, 520]  # 56 / 64 / 72: the 64-column block of the scalar rms_dw_kernel


def rms_vb(d: int) -> int:
    """The ``VB`` template argument iit_rms_fwd / iit_rms_bwd_res pick for ``d``."""
    vb = (d + 511) // 512
    return next(v for v in (1, 2, 4, 8, 16) if vb <= v)


def rms_depth(d: int) -> int:
    return 8 * ((d + 511) // 512) + 6


def rms_inputs(family: str, T: int, d: int, seed: int, x_dtype, affine: bool = True):
    """``x`` [T, d] in ``x_dtype`` and fp32 ``w`` (None without affine).  ``balanced``: rows of ``+- a`` (a power of
    two per row) in a sign pattern of no period, w = 1 -- every |y| of a row is then one value, and a swapped or
    dropped column shows; ``tiny``: ``mean(x^2)`` of the order of eps; ``large``: |x| ~ 2^40."""
    g = gen(seed)
    w = (1.0 + 0.5 * torch.randn(d, generator=g)).float() if affine else None
    if family == "balanced":
        a = 2.0 ** torch.randint(-2, 3, (T, 1), generator=g).double()
        sign = torch.ones(d, dtype=torch.float64)
        sign[:d // 2] = -1.0
        sign[1], sign[d - 2] = 1.0, -1.0
        x = a * sign
        w = torch.ones(d) if affine else None
    elif family == "tiny":
        x = math.sqrt(RMS_EPS) * torch.randn(T, d, generator=g)
    elif family == "large":
        x = 2.0 ** 40 * torch.randn(T, d, generator=g)
    else:
        x = 3.0 * torch.randn(T, d, generator=g) + 1.0
    return x.to(x_dtype), w


def rms_fwd_ref(x, w, eps: float, wrong: str = "") -> dict:
    """Float64 RMSNorm of ``x`` [T, d] (bf16 or fp32) with its bounds; ``eps`` rounded to fp32 as the kernel's
    argument is.  ``wrong``: ``mean_dm8`` (the mean runs over the first d - 8 columns), ``no_eps``, ``w_shift8``
    (w read 8 columns further on)."""
    x = x.double()
    T, d = x.shape
    eps = float(f32c(eps))
    xs = x[:, :d - 8] if wrong == "mean_dm8" else x
    ms = (xs * xs).sum(1, keepdim=True) / xs.shape[1]
    r = 1.0 / torch.sqrt(ms + (0.0 if wrong == "no_eps" else eps))
    y = x * r
    if w is not None:
        y = y * (w.double().roll(-8) if wrong == "w_shift8" else w.double())
    out = {"y": y, "rstd": r[:, 0]}
    if wrong:
        return out
    rel_r = ((rms_depth(d) + 1) + 2) / 2 * E + 2 * E
    out.update(tol_rstd=rel_r * r[:, 0] * SLACK, tol_y=y.abs() * (U + rel_r + 2 * E) * SLACK)
    return out


def rms_fwd_check(got: dict, ref: dict) -> dict:
    return {"y": bad_bound(got["y"], ref["y"], ref["tol_y"]),
            "rstd": bad_bound(got["rstd"], ref["rstd"], ref["tol_rstd"])}


def bad_rms_balanced(y: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """Balanced family with w = 1 (or null): every |y| of a row is the same bf16 value, not zero, with x's sign."""
    yd = y.double()
    return ~((yd.abs() == yd[:, :1].abs()) & (yd != 0) & (torch.sign(yd) == torch.sign(x.double())))


def rms_bwd_inputs(family: str, T: int, d: int, seed: int, x_dtype):
    """bf16 ``dy``, ``dres`` in x's type, fp32 ``dw0``; ``exact``: integers (see the module docstring)."""
    g = gen(seed + 1000)
    if family == "exact":
        terms = (T + 1) * 64 * 4
        return {"dy": int_operand((T, d), BF16, seed + 1, terms, 64),
                "dres": torch.randint(-8, 9, (T, d), generator=g).to(x_dtype),
                "dw0": int_operand((d,), F32, seed + 2, terms, 64)}
    return {"dy": torch.randn(T, d, generator=g).bfloat16(), "dres": torch.randn(T, d, generator=g).to(x_dtype),
            "dw0": torch.randn(d, generator=g).float()}


def rms_exact_x(T: int, d: int, seed: int, x_dtype):
    """``exact`` family of the dw kernels: integer x (|x| <= 64) and rstd in {1, 2, 4} per row."""
    x = int_operand((T, d), x_dtype, seed, (T + 1) * 64 * 4, 64)
    rstd = 2.0 ** torch.randint(0, 3, (T,), generator=gen(seed + 7)).float()
    return x, rstd


def rms_bwd_ref(dy, x, rstd, w, dres=None, dw0=None, wrong: str = "") -> dict:
    """Float64 RMSNorm backward; ``rstd`` is the fp32 tensor the kernel is given.  ``wrong``: ``neighbour_rstd`` (row
    t takes rstd[t ^ 1]), ``w_shift8``, ``s_not_div_d``, ``no_dres``, ``dw_drop_row`` (the last row is not added)."""
    dyd, x32 = dy.double(), x.dtype == F32
    x = x.double()
    T, d = x.shape
    r = rstd.double().view(T, 1)
    if wrong == "neighbour_rstd":
        r = r[[min(t ^ 1, T - 1) for t in range(T)]]
    g = dyd
    if w is not None:
        g = dyd * (w.double().roll(-8) if wrong == "w_shift8" else w.double())
    xh = x * r
    s = (g * xh).sum(1, keepdim=True) / (1 if wrong == "s_not_div_d" else d)
    core = r * (g - xh * s)
    res = None if dres is None or wrong == "no_dres" else dres.double()
    dx = core if res is None else core + res
    terms = dyd * x * r
    if wrong == "dw_drop_row":
        terms = terms[:T - 1]
    dw = terms.sum(0) + (0.0 if dw0 is None else dw0.double())
    out = {"dx": dx, "dw": dw}
    if wrong:
        return out
    tol_s = (rms_depth(d) + 3) * E * (g * xh).abs().mean(1, keepdim=True) + E * s.abs()
    tol_dx = r * (xh.abs() * tol_s + 2 * E * (xh * s).abs() + E * g.abs() + E * (g - xh * s).abs()) + E * core.abs()
    if res is not None:
        tol_dx = tol_dx + E * dx.abs()
    tol_dx = tol_dx + (E if x32 else U) * dx.abs()
    tol_dw = (T + 4) * E * (terms.abs().sum(0) + (0.0 if dw0 is None else dw0.double().abs()))
    out.update(tol_dx=tol_dx * SLACK, tol_dw=tol_dw * SLACK)
    return out


def _rms_lane_sum(v: torch.Tensor, rev: bool) -> torch.Tensor:
    """fp32 row sums [T, 1] in the shape of the kernels' reduction (lane = (column / 8) % 64; a lane adds its columns
    one by one, the lanes meet in a tree) -- first to last and halves first, or, with ``rev``, a deliberately
    different order: last to first and neighbours first."""
    T, n = v.shape
    chunks = (n + 511) // 512
    pad = torch.zeros(T, chunks * 512, dtype=F32)
    pad[:, :n] = v
    lanes = pad.view(T, chunks, 64, 8).permute(0, 2, 1, 3).reshape(T, 64, chunks * 8)
    acc = torch.zeros(T, 64, dtype=F32)
    for i in (range(chunks * 8 - 1, -1, -1) if rev else range(chunks * 8)):
        acc = acc + lanes[:, :, i]
    while acc.shape[1] > 1:
        h = acc.shape[1] // 2
        acc = (acc[:, 0::2] + acc[:, 1::2]) if rev else (acc[:, :h] + acc[:, h:])
    return acc


def rms_fwd_emul(x, w, eps: float, rev: bool) -> dict:
    x = x.float()
    d = x.shape[1]
    r = torch.rsqrt(_rms_lane_sum(x * x, rev) / d + f32c(eps))
    o = x * r
    if w is not None:
        o = o * w
    return {"y": o.bfloat16(), "rstd": r[:, 0]}


def rms_bwd_emul(dy, x, rstd, w, rev: bool, dres=None, dw0=None) -> dict:
    """fp32 emulation of the backward; dw adds the rows one by one (last first with ``rev``)."""
    xt = x.dtype
    dy, x = dy.float(), x.float()
    T, d = x.shape
    r = rstd.view(T, 1)
    g = dy if w is None else dy * w
    xh = x * r
    s = _rms_lane_sum(g * xh, rev) / d
    o = r * (g - xh * s)
    if dres is not None:
        o = o + dres.float()
    dw = torch.zeros(d)
    for t in (range(T - 1, -1, -1) if rev else range(T)):
        dw = dw + dy[t] * x[t] * rstd[t]
    return {"dx": o.to(xt), "dw": dw if dw0 is None else dw0 + dw}


# ================================================================================================ rotary
ROT_B, ROT_S, ROT_H = 2, 5, 3
ROT_OFFSETS = [0, 3]
# (D, rd), each with both pairings; :func:`rotary_vec_ok` tells which kernel a contiguous aligned x takes: the vector
# kernel for halves at (128, 128), (128, 64), (16, 16), (24, 16) and for adjacent pairs at those and (8, 8), (32, 24);
# the per-pair kernel for the rest ((3, 2): an odd pass-through)
ROT_SHAPES = [(128, 128), (128, 64), (16, 16), (24, 16), (8, 8), (32, 24), (3, 2), (2, 2)]


def rotary_vec_ok(D: int, rd: int, adjacent: bool) -> bool:
    """The shape part of iit_rotary's choice of the vector kernel."""
    return D % 8 == 0 and (rd % 8 == 0 if adjacent else rd % 16 == 0)


def rotary_inputs(family: str, B: int, S: int, H: int, D: int, rd: int, offset: int, seed: int):
    """bf16 ``x`` [B, S, H, D] and fp32 ``cos`` / ``sin`` [offset + S, rd]: every entry its own value (``random``) or
    drawn from {0, +-1, +-1/2, +-1/4} (``exact``, integer x); rows before ``offset`` are NaN."""
    g = gen(seed)
    n_ctx = offset + S
    if family == "exact":
        x = torch.randint(-32, 33, (B, S, H, D), generator=g).bfloat16()
        vals = torch.tensor([0.0, 1.0, -1.0, 0.5, -0.5, 0.25, -0.25])
        cos = vals[torch.randint(0, 7, (n_ctx, rd), generator=g)]
        sin = vals[torch.randint(0, 7, (n_ctx, rd), generator=g)]
    else:
        x = (2.0 * torch.randn(B, S, H, D, generator=g)).bfloat16()
        cos = (2.0 * torch.rand(n_ctx, rd, generator=g) - 1.0).float()
        sin = (2.0 * torch.rand(n_ctx, rd, generator=g) - 1.0).float()
    cos[:offset] = NAN
    sin[:offset] = NAN
    return x, cos.contiguous(), sin.contiguous()


def rotary_pairs(rd: int, adjacent: bool):
    j = torch.arange(rd // 2)
    return (2 * j, 2 * j + 1) if adjacent else (j, j + rd // 2)


def rotary_ref(x, cos, sin, rd: int, offset: int, adjacent: bool, inverse: bool, wrong: str = "") -> dict:
    """Float64 rotary of bf16 ``x`` [B, S, H, D] over arbitrary tables, with its bound (0 on the pass-through
    features).  ``wrong``: ``table_i1`` (element i0 reads the tables at i1), ``no_offset``, ``swap_pairing``,
    ``no_sign`` (the inverse rotates forward), ``no_pass`` (the pass-through features keep the buffer's prefill)."""
    B, S, H, D = x.shape
    xd = x.double()
    off = 0 if wrong == "no_offset" else offset
    c = cos[off:off + S].double().view(1, S, 1, rd)
    s = sin[off:off + S].double().view(1, S, 1, rd)
    i0, i1 = rotary_pairs(rd, adjacent != (wrong == "swap_pairing"))
    t0 = i1 if wrong == "table_i1" else i0
    sign = -1.0 if inverse and wrong != "no_sign" else 1.0
    a, b = xd[..., i0], xd[..., i1]
    out = xd.clone()
    out[..., i0] = a * c[..., t0] - (b * s[..., t0]) * sign
    out[..., i1] = b * c[..., i1] + (a * s[..., i1]) * sign
    if wrong == "no_pass":
        out[..., rd:] = BF16_FILL
    res = {"out": out}
    if wrong:
        return res
    mag = torch.zeros_like(xd)
    mag[..., i0] = (a * c[..., i0]).abs() + (b * s[..., i0]).abs()
    mag[..., i1] = (b * c[..., i1]).abs() + (a * s[..., i1]).abs()
    tol = U * out.abs() + E * (mag + out.abs())
    tol[..., rd:] = 0.0
    res["tol"] = tol * SLACK
    return res


def rotary_check(got, x, ref: dict, rd: int, family: str) -> dict:
    """Rotated features within the bound (``exact``: the bf16 image of the float64 result bit for bit); pass-through
    features bit for bit."""
    rot = bad_bits(got[..., :rd], ref["out"][..., :rd].bfloat16()) if family == "exact" else \
        bad_bound(got[..., :rd], ref["out"][..., :rd], ref["tol"][..., :rd])
    return {"rot": rot, "pass": bad_bits(got[..., rd:], x[..., rd:])}


def rotary_emul(x, cos, sin, rd: int, offset: int, adjacent: bool, inverse: bool, other: bool = False):
    """fp32 emulation (bf16 result): the kernel's ``a c - b s sign`` with every product rounded, or (``other``) the
    sum taken the other way round, ``-(b s sign) + a c``, through a float64 product rounded once (an fma)."""
    B, S, H, D = x.shape
    xf = x.float()
    c, s = cos[offset:offset + S].view(1, S, 1, rd), sin[offset:offset + S].view(1, S, 1, rd)
    i0, i1 = rotary_pairs(rd, adjacent)
    sign = -1.0 if inverse else 1.0
    a, b = xf[..., i0], xf[..., i1]
    out = xf.clone()
    if other:
        out[..., i0] = (-(b * s[..., i0] * sign).double() + a.double() * c[..., i0].double()).float()
        out[..., i1] = ((a * s[..., i1] * sign).double() + b.double() * c[..., i1].double()).float()
    else:
        out[..., i0] = a * c[..., i0] - b * s[..., i0] * sign
        out[..., i1] = b * c[..., i1] + a * s[..., i1] * sign
    return out.bfloat16()


# ================================================================================================ SwiGLU
SW_SIZES = [8, 2040, 2048, 2056, 8184, 8192, 8200, 3 * 8192 + 2056]  # SW_U = 4 chunks of 256 x 8 per block
SW_SWEEP_N = 4 * 43008  # the padded sweep four times over: see swiglu_sweep


def swiglu_sweep() -> torch.Tensor:
    """bf16 gate [SW_SWEEP_N]: every finite bf16 value with |g| <= 2^40 (42754), padded with normal values to
    43008 = 21 * 2048 elements, then repeated four times: element e belongs to chunk slot (e / 2048) % 4 of its
    block and every copy starts 21 slots after the one before, so each of the ``SW_U`` = 4 slots sees every value."""
    v = all_bf16()
    base = torch.cat([v, (2.0 * torch.randn(43008 - v.numel(), generator=gen(40))).bfloat16()])
    return base.repeat(4)


def swiglu_ref(g, u, dv=None, wrong: str = "") -> dict:
    """Float64 SwiGLU forward (and backward with ``dv``) of bf16 operands with the bounds of the bf16 results.
    ``wrong``: ``term_1pct`` (``h = 1 + 1.01 g (1 - s)``), ``s_bf16`` (s rounded to bf16 before the products),
    ``swap`` (dgate and dup exchanged)."""
    g, u = g.double(), u.double()
    s = 1.0 / (1.0 + torch.exp(-g))
    s1 = 1.0 / (1.0 + torch.exp(g))  # 1 - s without the cancellation
    if wrong == "s_bf16":
        s, s1 = s.float().bfloat16().double(), s1.float().bfloat16().double()
    post = g * s * u
    out = {"post": post}
    ag = g.abs()
    rel_s = torch.where(s1 > 0, s1 * (1.5 * ag + 2), torch.zeros_like(g)) * E + 3 * E
    fl = torch.minimum(s, torch.full_like(s, TINY))
    if not wrong:
        out["tol_post"] = (U * post.abs() + post.abs() * (rel_s + 2 * E) + (g * u).abs() * fl + TINY) * SLACK
    if dv is None:
        return out
    dv = dv.double()
    gs1 = torch.where(s1 > 0, g * s1, torch.zeros_like(g))
    h = 1.0 + (1.01 if wrong == "term_1pct" else 1.0) * gs1
    dup = dv * g * s
    dgate = dv * u * s * h
    if wrong == "swap":
        dup, dgate = dgate, dup
    out.update(dup=dup, dgate=dgate)
    if wrong:
        return out
    ds = s * rel_s + fl
    tol_h = ag * (ds + 2 * E * s1) + E * h.abs()
    out["tol_dup"] = (U * dup.abs() + dup.abs() * (rel_s + 2 * E) + (dv * g).abs() * fl + TINY) * SLACK
    out["tol_dgate"] = ((dv * u).abs() * (ds * h.abs() + s * tol_h) + (3 * E + U) * dgate.abs() + TINY) * SLACK
    return out


def swiglu_check(got: dict, ref: dict) -> dict:
    return {k: bad_bound(got[k], ref[k], ref["tol_" + k]) for k in ("post", "dup", "dgate") if k in got}


def swiglu_emul(g, u, dv=None, other: bool = False) -> dict:
    """fp32 emulation in the kernel's operation order (``__expf`` as exp2 of the product by log2(e)), or (``other``)
    with ``exp`` itself and the products associated the other way round."""
    g, u = g.float(), u.float()
    q = torch.exp(-g) if other else torch.exp2(-g * f32c(LOG2E))
    s = 1.0 / (1.0 + q)
    out = {"post": (g * (s * u) if other else g * s * u).bfloat16()}
    if dv is not None:
        dv = dv.float()
        h = 1.0 + g * (1.0 - s)
        out["dup"] = (dv * (g * s) if other else dv * g * s).bfloat16()
        out["dgate"] = ((dv * u) * (s * h) if other else dv * u * s * h).bfloat16()
    return out


# ================================================================================================ splice kernels
SPL_B, SPL_S, SPL_D = 2, 17, 16


def splice_indices() -> dict:
    """``Ix`` indices over [SPL_B, SPL_S, SPL_D]: name -> index."""
    from iit_amd.core.index import Ix
    return {"one_pos": Ix[:, 3], "three_runs": Ix[:, [0, 2, 3, 4, 9]], "eight_runs": Ix[:, [0, 2, 4, 6, 8, 10, 13, 16]],
            "inner_3_13": Ix[:, -1, 3:13], "inner_two_runs": Ix[1, 2:9, [0, 1, 2, 3, 4, 9, 10, 11, 12, 13, 14, 15]],
            "all": Ix[:, :, :], "none": Ix[:, 4:4]}


NINE_RUNS = [0, 2, 4, 6, 8, 10, 12, 14, 16]


def splice_mask(index, shape, wrong: str = "") -> torch.Tensor:
    """bool ``shape``: the elements ``t[index.as_index]`` selects (torch's own indexing).  ``wrong = "ignore_dim2"``:
    the position ranges (dimension 2 of the kernel's 4-d table) are ignored."""
    m = torch.zeros(shape, dtype=torch.bool)
    m[index.as_index] = True
    if wrong == "ignore_dim2":
        m = m.any(1, keepdim=True).expand(shape).clone()
    return m


def splice_src(kind: str, shape, seed: int, device="cpu") -> torch.Tensor:
    """bf16 source: ``contiguous`` [B, S, d], ``broadcast`` [1, S, d], or ``strided`` (every other row and column of
    a sentinel-filled [B, 2 S, 2 d] buffer)."""
    B, S, d = shape
    g = gen(seed)
    if kind == "broadcast":
        return (3.0 * torch.randn(1, S, d, generator=g)).bfloat16().to(device)
    v = (3.0 * torch.randn(B, S, d, generator=g)).bfloat16()
    if kind == "contiguous":
        return v.to(device)
    buf = filled((B, 2 * S, 2 * d), BF16, device)
    view = buf[:, ::2, ::2]
    view.copy_(v)
    return view


def embed_splice_fwd_ref(tok, W16, src, mask) -> torch.Tensor:
    return torch.where(mask, src.expand(mask.shape), W16[tok])


def embed_splice_bwd_ref(tok, dout, grad0, mask, wrong: str = "") -> dict:
    """Float64 ``grad0[v] + sum over the unspliced (t, c) with tok[t] == v of dout[t, c]`` with its bound and ``n``
    [vocab, d], the number of terms per element.  ``wrong``: ``not_zeroed`` (spliced elements add their gradient too),
    ``one_added`` (the first spliced element does)."""
    vocab, d = grad0.shape
    t = tok.reshape(-1)
    live = (~mask).reshape(-1, d)
    if wrong == "not_zeroed":
        live = torch.ones_like(live)
    elif wrong == "one_added":
        live = live.clone()
        live.view(-1)[int(mask.reshape(-1).nonzero()[0])] = True
    gd = dout.double().reshape(-1, d) * live
    ref = grad0.double().index_add(0, t, gd)
    ab = torch.zeros(vocab, d, dtype=torch.float64).index_add(0, t, gd.abs())
    n = torch.zeros(vocab, d, dtype=torch.float64).index_add(0, t, live.double())
    return {"grad": ref, "n": n, "tol": tol_sum(n, ab, grad0)}
