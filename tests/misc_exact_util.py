"""Helpers shared by the exact tests of the remaining kernels of csrc/kernels.hip: embedding forward / backward, the
three column-sum kernels, GELU forward and derivative, ``add_bf16``, ``shadow_refresh``, ``zero_chunks`` /
``zero_ranges``, ``sumsq_2d``, the ZeRO-1 entry points ``sumsq_spans`` / ``adam_spans`` and ``kl_rows``
(tests/test_embed_exact.py, tests/test_colsum_exact.py, tests/test_elementwise_exact.py and
tests/test_sumsq_kl_exact.py on the GPU, tests/test_misc_exact_ref.py on the CPU).  Conventions are those of
tests/kern_exact_util.py: float64 references of the same fp32 / bf16 inputs, comparators that return the mask of bad
elements (NaN and the buffer sentinel count as bad), ``E`` = 2^-24, ``U`` = 2^-8, every bound times ``SLACK``.

Bitwise kernels (``bad_bits`` against a torch expression in the kernel's operation order):

* ``embed_pos_fwd``: one IEEE add, ``W_E[tok] + W_pos[s]``.
* ``add_bf16``: ``(base + y.float()) + bias``, left to right (both kernel paths add in that order).
* ``shadow_refresh``: ``src.to(bf16)`` at ``dst[h dst_hs + i ld + j]``, or ``dst[c ld + r]`` when transposed.
* ``zero_chunks`` / ``zero_ranges``: +0.0 inside the ranges, every other bit kept.

Order-free sums (embedding / position backward, ``colsum_kernel``, ``colsum_vec_kernel``, ``colsum_multi_kernel``,
``sumsq_2d_kernel``): atomics, LDS combines and the grid leave the order of the additions open, so two families.

* ``exact``: integer-valued operands (|x| <= 64 for bf16 inputs, |g| <= 256 elsewhere, the prefill too) such that
  every partial sum is an integer below 2^24 -- :func:`int_operand` checks the limit against the case's term count --
  so the fp32 result is the float64 sum bit for bit in any order.  A dropped or doubled term shows as a wrong integer.
* ``random`` (normal data): ``|got - ref| <= (n + 3) E (sum |terms| + |prefill|)`` with n the number of terms added
  into that element (n - 1 additions in any order, the add into the prefill, and three spare roundings as in
  ``tol_dw``).  Embedding: n is the count of rows of that token, per (token, column); position and column sums: n = B
  or T.  An element that receives no term must keep its prefill bits (both families).
* ``sumsq_2d``: block b of G = min(items, 2048) adds its items b, b + G, ... (item = (row, 2048-column chunk)) into slot
  b & 63.  Every term is a square, so the bound is relative to the slot's sum: the square (1), 8 serial additions per
  thread per item, 6 shuffle levels + 2 over the waves to the block, one atomic per block of the slot and the
  prefill: ``n = 8 ceil(items / G) + 9 + ceil(G / 64)``, ``tol = (n + 3) E (sum + |prefill|)``.

GELU forward and derivative on bf16 inputs (every finite bf16 value with |x| <= 2^40), bf16 store ``U |ref|``:

* gelu_new in the sigmoid form of csrc/common.h, ``x rcp(1 + exp2(-m))``, ``m = x fma(c1, x^2, c0)``.  The reference is
  float64 ``x s``, ``s = 1 / (1 + exp(-2u))``, ``u = sqrt(2 / pi) (x + 0.044715 x^3)`` -- the same function as
  ``0.5 x (1 + tanh u)`` without its cancellation.  m carries x^2 (E), the two constants (E / 2), the fma (E) and the
  product (E): 4 E |m| on the exponent, i.e. ``4 ln2 E |m|`` relative on q = exp2(-m); ``v_exp_f32`` and ``v_rcp_f32``
  1 ulp = 2 E each, ``1 + q`` one rounding.  An error of q moves s by (1 - s) of it:
  ``rel_s = (1 - s) (2 + 4 ln2 |m|) E + 3 E``, ``tol = U |ref| + |ref| (rel_s + E) + |x| min(s, 2^-126) + 2^-126``
  (a denormal s, and a denormal input or result, may be flushed).  Only relative terms: the bound stays tight in the
  negative tail, where ``1 - 2 rcp(exp(2u) + 1)`` cancels (see the gelu_new note below).
* gelu_new derivative ``fma(x du, fma(-s, s, s), s)``, ``du = fma(c3, x^2, c2)``: with
  ``ds = s rel_s + min(s, 2^-126)``, ``tol' = ds (1 + |x du| |1 - 2 s|) + E (3 |x du s (1 - s)| + |ref'|)``; times
  |dpost|, plus the product and the store:
  ``tol = |dpost| tol' + (E + U) |ref| + 2^-126``.
* erf GELU ``0.5 x (1 + erff(x / sqrt 2))``: ``erff`` within ``ERF_K`` ulps (2 ERF_K E, |erf| <= 1), its argument's
  rounding (1.5 E |z| erf'(z) <= 0.73 E) and ``1 + erf`` (2 E) are ABSOLUTE errors of a factor that cancels to 0 in
  the negative tail: ``tol = U |ref| + E |ref| + (ERF_K + 1.4) E |x| + 2^-126``.
* erf derivative ``0.5 (1 + erff z) + x c exp(w)``, ``w = -x^2 / 2``: the first term as above without |x|; ``__expf`` is
  a product by log2(e) and ``v_exp_f32``: 2.5 E |w| on the exponent and 2 E, the products 2.5 E:
  ``tol' = (ERF_K + 1.4) E + |t2| (3 |w| + 5) E + E |ref'| + |x c| 2^-126``; ``tol`` as for gelu_new.
* ``ERF_K`` = 4: assumed (the accuracy the HIP math API states for ``erff``); nothing on the GPU had to exceed it:
  through the kernel on an MI355X the erf forward differs from the bf16 rounding of the exact value by at most
  0.45 E |x| (x = -4.44, over 2^-100 < |x| < 16) where this term allows 5.4 E |x|.  The worst errors of the four
  GELU kernels in units of their whole bound are 0.965 to 0.983: the bf16 store takes nearly all of it.
* The stand-alone gelu_new kernels used ``0.5 x (1 + t)``, ``t = 1 - 2 rcp(exp(2u) + 1)``, a second implementation
  beside ``gelu_new_f``.  Held to the bound above on an MI355X it failed at 159 of the 42754 inputs, x from -9.94 to
  -3.98, the worst 255 times the bound at x = -4.97 (``1 + t`` cancels where t -> -1; the fp32 emulation in
  tests/test_misc_exact_ref.py shows the same), so those kernels now call ``gelu_new_f``.
* Beyond about |x| = 2^42 ``gelu_new_grad_f`` forms ``inf * 0`` (``x du`` overflows while ``s (1 - s)`` is 0); the
  VALU-bound fused dgelu epilogue shares that helper, so the inputs stop at 2^40 and the limit is recorded, not
  changed, here.

``kl_rows`` (one 256-thread block per row; a thread adds ceil(V / 256) terms, then 6 shuffle levels, 3 additions over
the waves and the term's own product): ``lse`` within ``LSE_TOL max(1, |ref|)`` and exactly -inf for an all -inf row;
the three sums within ``(ceil(V / 256) + 10) E sum |terms|``; the terms of ``sum b log a`` carry 1 ulp of
``v_log_f32`` (2^-23 |log2 a| ln 2 = 2 E |log a|), the product by ln 2 with its constant (1.5 E) and ``b *`` (E):
``+ 4.5 E sum |b log a|``.  Entries with b == 0 contribute exactly 0, also where a = -inf (or a = 0 under the log).

``adam_spans``: :func:`span_index` maps a span table with ``local4 != start4`` onto the arena / shard index sets; the
gathered state goes through ``adam_ref`` and its bounds unchanged.

Kernel instantiations of csrc/kernels.hip that tests/kern_exact_util.py does not list, and a passing case of each:

=========================================  =====================================================================
embed_pos_fwd_kernel (float4)              test_embed_exact.py::test_embed_fwd, d = 4 ... 768
embed_pos_fwd_scalar_kernel                test_embed_fwd, d = 1 / 3 / 66 / 255 and test_embed_fwd_unaligned_rows
embed_bwd_pos_kernel                       test_embed_exact.py::test_embed_bwd (every pattern, both families)
embed_bwd_kernel (IIT_EMBED_BWD_POS=0)     test_launch_variants.py only (third variant, test_embed_bwd)
pos_bwd_kernel                             test_embed_exact.py::test_pos_bwd_vec
pos_bwd_scalar_kernel                      test_embed_exact.py::test_pos_bwd_scalar (d % 4 != 0, g offset one float)
colsum_kernel<f32 / bf16>                  test_colsum_exact.py::test_colsum_scalar, test_colsum_scalar_misaligned
colsum_vec_kernel<f32 / bf16>, R = 32      test_colsum_exact.py::test_colsum_vec
colsum_vec_kernel<bf16>, R = 64/128/256    test_colsum_exact.py::test_colsum_vec_rows_per_block
colsum_multi_kernel (both block forms)     test_colsum_exact.py::test_colsum_multi, 1 / 2 / 32 / 33 items
gelu_fwd_kernel<erf / new>                 test_elementwise_exact.py::test_gelu_fwd[vec-*], [vec_pad-*]
gelu_fwd_scalar_kernel<erf / new>          test_gelu_fwd[n7-*], [ld_odd-*], [misaligned-*]
dgelu_kernel<erf / new>, both bodies       test_elementwise_exact.py::test_dgelu[8 / tail]
add_bf16_kernel<true / false>              test_elementwise_exact.py::test_add_bf16
shadow_refresh_kernel (plain, transposed)  test_elementwise_exact.py::test_shadow_refresh
zero_chunks_kernel, zero_ranges_kernel     test_elementwise_exact.py::test_zero_chunks, test_zero_ranges
sumsq_2d_kernel                            test_sumsq_kl_exact.py::test_sumsq_2d
sumsq_span_kernel (gsq = null, spans)      test_sumsq_kl_exact.py::test_adam_spans
adam_span_kernel<true, 2>, nparts = 1      test_sumsq_kl_exact.py::test_adam_spans
kl_rows_kernel                             test_sumsq_kl_exact.py::test_kl_rows
attn_small_fwd / attn_small_bwd_kernel     tests/test_attn_exact.py (tests/attn_exact_util.py)
probe_tr16_kernel, probe_tr16b_kernel      diagnostics, not run by any test
=========================================  =====================================================================
"""
import math

import numpy as np
import torch

from kern_exact_util import (BF16_FILL, E, LSE_TOL, NAN, NINF, NSQ, SLACK, U, adam_ref, bad_bits,  # noqa: F401
                             bad_bound, filled, gen)

F32, BF16 = torch.float32, torch.bfloat16
FAMILIES = ["exact", "random"]
TINY = 2.0 ** -126
ERF_K = 4.0
LN2 = math.log(2.0)


# ================================================================================================ order-free sums
def int_operand(shape, dtype, seed: int, terms: int, lim: int = 0) -> torch.Tensor:
    """``exact`` family: integers in [-lim, lim] (default 64 for bf16, 256 for fp32); ``terms`` (the largest number of
    them, prefill included, that meet in one sum) times ``lim`` must stay below 2^24."""
    lim = lim or (64 if dtype == BF16 else 256)
    assert terms * lim < 2 ** 24, (terms, lim)
    return torch.randint(-lim, lim + 1, shape, generator=gen(seed)).to(dtype)


def operand(family: str, shape, dtype, seed: int, terms: int) -> torch.Tensor:
    if family == "exact":
        return int_operand(shape, dtype, seed, terms)
    return torch.randn(shape, generator=gen(seed)).to(dtype)


def tol_sum(n, abs_sum: torch.Tensor, prefill: torch.Tensor) -> torch.Tensor:
    """``(n + 3) E (sum |terms| + |prefill|)``; ``n`` a number or a tensor broadcast against the sums."""
    return (n + 3) * E * (abs_sum + prefill.double().abs()) * SLACK


def bad_sum(got: torch.Tensor, ref: torch.Tensor, tol: torch.Tensor, family: str, prefill=None, n=None):
    """Mask of bad elements of an order-free fp32 sum: bitwise the float64 sum (``exact``) or within ``tol``; where
    no term arrives (``n == 0``) the prefill's bits."""
    bad = bad_bits(got, ref.float()) if family == "exact" else bad_bound(got, ref, tol)
    if n is not None:
        n = torch.as_tensor(n).expand(got.shape)
        bad = torch.where(n == 0, bad_bits(got, prefill), bad)
    return bad


# ------------------------------------------------------------------------------------------------ embedding
EB = 32  # sequences per block of embed_bwd_pos_kernel
EMBED_PATTERNS = ["equal", "distinct", "runs", "zero_first"]


def embed_tokens(pattern: str, B: int, S: int, vocab: int) -> torch.Tensor:
    """int64 [B, S].  ``runs``: at position s the token changes after rows 7 + s % 3, 15 + s % 3, 31 + s % 3, ... --
    runs that end one before, at and one after the 8-row unroll and the 32-row chunk -- cycling through tokens that
    come back later (3, 0, vocab - 1, 3, ...).  ``zero_first``: the same with token 0 in the first row (next to the
    kernel's ``cur = -1`` start)."""
    if pattern == "equal":
        return torch.full((B, S), 5 % vocab, dtype=torch.int64)
    if pattern == "distinct":
        assert vocab >= B * S
        return vocab - 1 - torch.arange(B * S, dtype=torch.int64).view(B, S)
    cyc = [3 % vocab, 0, vocab - 1, 3 % vocab, 2 % vocab]
    tok = torch.empty(B, S, dtype=torch.int64)
    for s in range(S):
        cuts = sorted({c + s % 3 for c in (7, 15, 31, 39, 63)})
        for b in range(B):
            tok[b, s] = cyc[(sum(b >= c for c in cuts) + s) % len(cyc)]
    if pattern == "zero_first":
        tok[0, :] = 0
    return tok


def embed_fwd_ref(tok, WE, Wpos, S: int) -> torch.Tensor:
    """fp32 [T, d]: one IEEE add per element."""
    t = tok.reshape(-1)
    return WE[t] + Wpos[torch.arange(t.numel(), device=t.device) % S]


def embed_bwd_ref(tok, g, dWE0, dWpos0) -> dict:
    """Float64 ``dWE0[v] + sum_{tok == v} g`` and ``dWpos0[s] + sum_b g[b, s]`` of fp32 ``g`` [B, S, d] with their
    bounds; ``n_we`` [vocab, 1] the number of rows that meet in a row of dWE.  Only the first S rows of dWpos
    receive terms."""
    B, S, d = g.shape
    gd = g.double().view(B * S, d)
    t = tok.reshape(-1)
    out = {}
    if dWE0 is not None:
        vocab = dWE0.shape[0]
        we = dWE0.double().index_add(0, t, gd)
        ab = torch.zeros(vocab, d, dtype=torch.float64).index_add(0, t, gd.abs())
        n = torch.bincount(t, minlength=vocab).view(vocab, 1)
        out.update(dWE=we, n_we=n, tol_dWE=tol_sum(n.double(), ab, dWE0))
    if dWpos0 is not None:
        n = torch.zeros(dWpos0.shape[0], 1, dtype=torch.int64)
        n[:S] = B
        pos = dWpos0.double().clone()
        pos[:S] += g.double().sum(0)
        ab = torch.zeros_like(pos)
        ab[:S] = g.double().abs().sum(0)
        out.update(dWpos=pos, n_pos=n, tol_dWpos=tol_sum(n.double(), ab, dWpos0))
    return out


def embed_bwd_check(got: dict, ref: dict, pre: dict, family: str) -> dict:
    return {k: bad_sum(got[k], ref[k], ref["tol_" + k], family, pre[k], ref["n_we" if k == "dWE" else "n_pos"])
            for k in ("dWE", "dWpos") if got.get(k) is not None}


def embed_bwd_emul(tok, g, dWE0, bug: str = "") -> torch.Tensor:
    """fp32 emulation of embed_bwd_pos_kernel: per position, chunks of EB sequences, runs of equal tokens added in a
    register, one add into dWE per run.  ``bug``: ``reset_zero`` (a token change starts the run at 0 instead of the
    row's value), ``chunk_first_lost`` (a run that continues over a chunk boundary loses its first row there)."""
    B, S, d = g.shape
    out = dWE0.clone()
    for s in range(S):
        for b0 in range(0, B, EB):
            cur, acc = -1, torch.zeros(d)
            for b in range(b0, min(B, b0 + EB)):
                v = int(tok[b, s])
                if v != cur:
                    if cur >= 0:
                        out[cur] = out[cur] + acc
                    lost = bug == "reset_zero" or (bug == "chunk_first_lost" and b == b0 and b0 > 0
                                                   and v == int(tok[b - 1, s]))
                    cur, acc = v, (torch.zeros(d) if lost else g[b, s].clone())
                else:
                    acc = acc + g[b, s]
            if cur >= 0:
                out[cur] = out[cur] + acc
    return out


# ------------------------------------------------------------------------------------------------ column sums
def colsum_ref(x, out0) -> dict:
    """Float64 ``out0[n] + sum_t x[t][n]`` of an fp32 / bf16 [T, N] operand (any device) with its bound."""
    T = x.shape[0]
    xd = x.double()
    return {"out": out0.double() + xd.sum(0), "tol": tol_sum(T, xd.abs().sum(0), out0)}


def colsum_emul(x, out0, order: str) -> torch.Tensor:
    """fp32 column sums in a deliberately bad order: rows last to first, or pairwise."""
    v = x.float()
    if order == "reversed":
        s = torch.zeros(v.shape[1])
        for t in range(v.shape[0] - 1, -1, -1):
            s = s + v[t]
        return out0 + s
    while v.shape[0] > 1:
        if v.shape[0] % 2:
            v = torch.cat([v, torch.zeros(1, v.shape[1])])
        v = v[0::2] + v[1::2]
    return out0 + v[0]


def strided(x: torch.Tensor, ld: int, offset: int = 0, device="cpu") -> torch.Tensor:
    """``x`` [rows, cols] as a view with row stride ``ld`` at element ``offset`` of a sentinel-filled buffer, with
    ``ld`` spare elements behind the last row."""
    rows, cols = x.shape
    assert ld >= cols
    buf = filled((offset + rows * ld + ld,), x.dtype, device)
    view = buf[offset:offset + rows * ld].view(rows, ld)[:, :cols]
    view.copy_(x)
    return view


# ------------------------------------------------------------------------------------------------ sumsq_2d
def sumsq_plan(M: int, N: int):
    """(items, blocks, slot of every item [M, chunks]) of iit_sumsq_2d."""
    chunks = (N + 2047) // 2048
    items = M * chunks
    G = min(items, 2048)
    slot = ((torch.arange(items) % G) & 63).view(M, chunks)
    return items, G, slot


def sumsq_lim(M: int, N: int) -> int:
    """Largest |g| <= 256 of the ``exact`` family: the squares of one slot, and a prefill of lim^2, stay below 2^24."""
    items, G, slot = sumsq_plan(M, N)
    per_slot = int(torch.bincount(slot.reshape(-1), minlength=64).max()) * min(N, 2048) + 1
    lim = min(256, int(math.isqrt((2 ** 24 - 1) // per_slot)))
    assert lim >= 1 and per_slot * lim * lim < 2 ** 24
    return lim


def sumsq_ref(c, gsq0) -> dict:
    """Float64 per-slot sums of squares of fp32 ``c`` [M, N] added to ``gsq0`` [64], the bound, and ``n`` [64] the
    number of blocks that add into each slot (0: the slot keeps its bits)."""
    M, N = c.shape
    items, G, slot = sumsq_plan(M, N)
    chunks = slot.shape[1]
    sq = torch.zeros(M, chunks * 2048, dtype=torch.float64)
    sq[:, :N] = c.double() ** 2
    per_item = sq.view(M, chunks, 2048).sum(2)
    s = torch.zeros(64, dtype=torch.float64).index_add(0, slot.reshape(-1), per_item.reshape(-1))
    n = torch.bincount((torch.arange(G) & 63), minlength=64)
    terms = 8 * ((items + G - 1) // G) + 9 + (G + 63) // 64
    return {"gsq": gsq0.double() + s, "n": n, "tol": tol_sum(terms, s, gsq0)}


def sumsq_emul(c, gsq0) -> torch.Tensor:
    """fp32 emulation in another order: every item's squares added last to first, the items of a slot one by one."""
    M, N = c.shape
    _, _, slot = sumsq_plan(M, N)
    out = gsq0.clone()
    sq = c * c
    for r in range(M):
        for k in range(slot.shape[1]):
            seg = sq[r, k * 2048:min(N, (k + 1) * 2048)].flip(0)
            while seg.numel() > 1:  # pairwise
                if seg.numel() % 2:
                    seg = torch.cat([seg, torch.zeros(1)])
                seg = seg[0::2] + seg[1::2]
            out[slot[r, k]] = out[slot[r, k]] + seg[0]
    return out


# ================================================================================================ GELU
C_U = math.sqrt(2.0 / math.pi)
GELU_KINDS = ["new", "erf"]


def all_bf16(limit: float = 2.0 ** 40) -> torch.Tensor:
    """Every finite bf16 value with |x| <= ``limit`` (denormals, +0 and -0 included): 42754 at 2^40."""
    v = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(BF16)
    return v[torch.isfinite(v.float()) & (v.float().abs() <= limit)]


GELU_N = 43008  # = 21 * 2048 = 6144 * 7


def gelu_inputs() -> torch.Tensor:
    """:func:`all_bf16` filled up with normal values to GELU_N elements, so that it lays out as [21, 2048] (vector
    kernels) and as [6144, 7] (N = 7: scalar)."""
    v = all_bf16()
    return torch.cat([v, (2.0 * torch.randn(GELU_N - v.numel(), generator=gen(40))).bfloat16()])


def gelu_ref(x: torch.Tensor, kind: str) -> dict:
    """Float64 GELU and its derivative of bf16 ``x`` with the bounds of the bf16 results (``tol``; ``dtol`` is the
    bound of the fp32 derivative itself, to be scaled by |dpost|: see :func:`dgelu_ref`)."""
    x = x.double()
    ax = x.abs()
    if kind == "new":
        u2 = 2 * C_U * (x + 0.044715 * x ** 3)
        s = 1.0 / (1.0 + torch.exp(-u2))
        s1 = 1.0 / (1.0 + torch.exp(u2))  # 1 - s without the cancellation
        m = u2.abs() / LN2
        m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))  # saturated: (1 - s) or s is 0 there
        y = x * s
        rel_s = torch.where(s1 > 0, s1 * (2 + 4 * LN2 * m), torch.zeros_like(m)) * E + 3 * E
        flush = torch.minimum(s, torch.full_like(s, TINY))
        tol = U * y.abs() + y.abs() * (rel_s + E) + ax * flush + TINY
        du = 2 * C_U * (1 + 3 * 0.044715 * x * x)
        core = x * du * s * s1
        dy = s + core
        ds = s * rel_s + flush
        dtol = ds * (1 + (x * du).abs() * (1 - 2 * s).abs()) + E * (3 * core.abs() + dy.abs())
    else:
        z = x / math.sqrt(2.0)
        half = 0.5 * torch.erfc(-z)  # 0.5 (1 + erf z) without the cancellation
        y = x * half
        tol = U * y.abs() + E * y.abs() + (ERF_K + 1.4) * E * ax + TINY
        w = -0.5 * x * x
        c = 1.0 / math.sqrt(2.0 * math.pi)
        t2 = x * c * torch.exp(w)
        dy = half + t2
        wf = torch.where(t2 != 0, w.abs(), torch.zeros_like(w))
        dtol = (ERF_K + 1.4) * E + t2.abs() * (3 * wf + 5) * E + E * dy.abs() + (ax * c) * TINY
    return {"y": y, "tol": tol * SLACK, "dy": dy, "dtol": dtol}


def dgelu_ref(dpost: torch.Tensor, x: torch.Tensor, kind: str) -> dict:
    r = gelu_ref(x, kind)
    g = dpost.double()
    y = g * r["dy"]
    return {"y": y, "tol": (g.abs() * r["dtol"] + (E + U) * y.abs() + TINY) * SLACK}


def _f(v: float) -> torch.Tensor:
    return torch.tensor(v, dtype=F32)


def gelu_emul(x: torch.Tensor, form: str) -> torch.Tensor:
    """fp32 torch emulation of the kernels' own expressions on bf16 ``x`` (bf16 result).  ``sig``: ``gelu_new_f`` of
    csrc/common.h; ``tanh``: the ``1 - 2 rcp(exp(2u) + 1)`` form the stand-alone kernels used; ``erf``."""
    x = x.float()
    if form == "sig":
        m = x * (_f(0.10294324) * (x * x) + _f(2.3022082))
        return (x * (1.0 / (1.0 + torch.exp2(-m)))).bfloat16()
    if form == "tanh":
        u = _f(0.7978845608028654) * (x + _f(0.044715) * x * x * x)
        t = 1.0 - 2.0 * (1.0 / (torch.exp(2.0 * u) + 1.0))
        return (0.5 * x * (1.0 + t)).bfloat16()
    return (0.5 * x * (1.0 + torch.erf(x * _f(0.7071067811865476)))).bfloat16()


def dgelu_emul(dpost: torch.Tensor, x: torch.Tensor, kind: str) -> torch.Tensor:
    x, g = x.float(), dpost.float()
    if kind == "new":
        x2 = x * x
        s = 1.0 / (1.0 + torch.exp2(-(x * (_f(0.10294324) * x2 + _f(2.3022082)))))
        du = _f(0.21406445) * x2 + _f(1.5957691)
        d = (x * du) * (s - s * s) + s
    else:
        d = 0.5 * (1.0 + torch.erf(x * _f(0.7071067811865476))) + x * _f(0.3989422804014327) * torch.exp(-0.5 * x * x)
    return (g * d).bfloat16()


# ================================================================================================ bitwise kernels
def add_bf16_ref(base, y, bias) -> torch.Tensor:
    o = base + y.float()
    return o if bias is None else o + bias


def shadow_expected(dst0: torch.Tensor, src: torch.Tensor, ld: int, transpose: bool, dst_hs: int = 0,
                    wrong: str = "") -> torch.Tensor:
    """The flat bf16 destination after one descriptor: ``src`` [heads, rows, cols] (fp32) rounded to bf16 into a copy
    of the flat prefill ``dst0``.  ``wrong = "untransposed"`` writes a transposed tile in source order."""
    heads, rows, cols = src.shape
    out = dst0.clone()
    v = src.bfloat16()
    if transpose and wrong != "untransposed":
        assert heads == 1
        idx = torch.arange(cols).view(cols, 1) * ld + torch.arange(rows).view(1, rows)
        out[idx.reshape(-1)] = v[0].t().reshape(-1)
        return out
    if transpose:  # the bug: element (r, c) lands at r ld' + c of the [cols][ld] image, clipped to it
        idx = torch.arange(rows).view(rows, 1) * ld + torch.arange(cols).view(1, cols)
        keep = (idx < cols * ld).reshape(-1)
        out[idx.reshape(-1)[keep]] = v[0].reshape(-1)[keep]
        return out
    idx = (torch.arange(heads).view(heads, 1, 1) * dst_hs + torch.arange(rows).view(1, rows, 1) * ld
           + torch.arange(cols).view(1, 1, cols))
    out[idx.reshape(-1)] = v.reshape(-1)
    return out


def zero_expected(buf0: torch.Tensor, ranges) -> torch.Tensor:
    out = buf0.clone()
    for a, n in ranges:
        out[a:a + n] = 0.0
    return out


ZERO_LENS = [1, 2, 3, 4, 5, 255, 1024, 65536]


def zero_ranges_table():
    """(start, len) for every length of ZERO_LENS at all four start alignments, three untouched floats between
    neighbours; returns the list and the buffer size."""
    out, pos = [], 3
    for n in ZERO_LENS:
        for a in range(4):
            pos += (a - pos) % 4
            if out and pos < out[-1][0] + out[-1][1] + 3:
                pos += 4
            out.append((pos, n))
            pos += n + 3
    return out, pos + 8


# ================================================================================================ spans
SPAN_DTYPE = np.dtype([("start4", np.int64), ("local4", np.int64), ("len4", np.int32), ("pad", np.int32)])
SPAN_LENS = [1, 255, 256, 257, 1024]


def span_table():
    """Hand-built spans (start4, local4, len4) with ``local4 != start4`` and gaps between spans in the arena and in
    the shard (other gaps, other order of sizes); returns the list, the arena and the shard size in floats."""
    spans, a, s = [], 5, 2
    for i, n in enumerate(SPAN_LENS):
        spans.append((a, s, n))
        a += n + 3 + i
        s += n + 1 + 2 * (i % 2)
    assert all(x[0] != x[1] for x in spans)
    return spans, 4 * (a + 4), 4 * (s + 4)


def span_bytes(spans) -> torch.Tensor:
    arr = np.zeros(len(spans), dtype=SPAN_DTYPE)
    for i, (a, s, n) in enumerate(spans):
        arr[i] = (a, s, n, 0)
    return torch.from_numpy(arr.view(np.uint8).copy())


def span_index(spans, wrong: str = ""):
    """(arena indices, shard indices) of the elements of ``spans`` in table order.  ``wrong = "start4"`` reads the
    shard at the arena offset."""
    ia, il = [], []
    for a, s, n in spans:
        ia.append(4 * a + torch.arange(4 * n))
        il.append(4 * (a if wrong == "start4" else s) + torch.arange(4 * n))
    return torch.cat(ia), torch.cat(il)


def span_state(arena_n: int, shard_n: int, seed: int) -> dict:
    g = gen(seed)
    return {"p": torch.randn(arena_n, generator=g).float(), "g": torch.randn(shard_n, generator=g).float(),
            "m": (0.3 * torch.randn(shard_n, generator=g)).float(),
            "v": (0.1 * torch.rand(shard_n, generator=g)).float()}


def span_ref(st: dict, spans, t: int, clip, hyper: dict) -> dict:
    """``adam_ref`` over the gathered span elements, its bounds, and the float64 sum of squares."""
    ia, il = span_index(spans)
    ref = adam_ref(st["p"][ia], st["g"][il], st["m"][il], st["v"][il], t, clip=clip, **hyper)
    ref["ssq"] = (st["g"][il].double() ** 2).sum()
    return ref


def span_check(got: dict, st: dict, ref: dict, spans, mirror0: torch.Tensor) -> dict:
    """p, m, v of the span elements within the ``adam_ref`` bounds, the mirror bitwise the rounding of the new p, and
    every element outside the spans bit-unchanged in p, m, v and the mirror (g is an input: bitwise everywhere)."""
    ia, il = span_index(spans)
    out = {"p": bad_bound(got["p"][ia], ref["p"], ref["tol_p"]), "m": bad_bound(got["m"][il], ref["m"], ref["tol_m"]),
           "v": bad_bound(got["v"][il], ref["v"], ref["tol_v"]),
           "mirror": bad_bits(got["mirror"][ia], got["p"][ia].bfloat16()), "g": bad_bits(got["g"], st["g"])}
    off_a = torch.ones(st["p"].numel(), dtype=torch.bool)
    off_a[ia] = False
    off_l = torch.ones(st["g"].numel(), dtype=torch.bool)
    off_l[il] = False
    out["p_outside"] = bad_bits(got["p"], st["p"]) & off_a
    out["mirror_outside"] = bad_bits(got["mirror"], mirror0) & off_a
    out["m_outside"] = bad_bits(got["m"], st["m"]) & off_l
    out["v_outside"] = bad_bits(got["v"], st["v"]) & off_l
    return out


def span_emul(st: dict, spans, t: int, hyper: dict, wrong: str = "") -> dict:
    """fp32 step over the spans (no clip) written back into copies of the five buffers."""
    from kern_exact_util import adam_emul
    ia, il = span_index(spans, wrong)
    il = il % st["g"].numel()
    il_ok = span_index(spans)[1]
    e = adam_emul(st["p"][ia], st["g"][il], st["m"][il], st["v"][il], t, **hyper)
    out = {k: st[k].clone() for k in ("p", "g", "m", "v")}
    out["mirror"] = filled((st["p"].numel(),), BF16)
    out["p"][ia] = e["p"]
    out["mirror"][ia] = e["mirror"]
    out["m"][il if wrong else il_ok] = e["m"]
    out["v"][il if wrong else il_ok] = e["v"]
    return out


# ================================================================================================ kl_rows
KL_V = [1, 63, 255, 256, 257, 1000]
KL_ROWS = ["logits", "pmf", "masked", "all_masked", "b_zeros"]


def kl_inputs(V: int, seed: int):
    """fp32 ``a``, ``b`` [5, V], one row per entry of KL_ROWS, and the columns of the result to check per row.
    ``logits``: normal logits (log a is NaN: columns 0-2).  ``pmf``: a is a pmf (all four).  ``masked``: -inf logits
    where b = 0.  ``all_masked``: every logit -inf, b = 0.  ``b_zeros``: a pmf with exact zeros where b = 0, b with
    zeros elsewhere too."""
    g = gen(seed)
    b = torch.softmax(2.0 * torch.randn(5, V, generator=g), 1).float()
    a = (3.0 * torch.randn(5, V, generator=g)).float()
    a[1] = torch.softmax(a[1].double(), 0).float()
    dead = torch.arange(V) % 3 == 1
    if V > 1:
        a[2, dead] = NINF
        b[2, dead] = 0.0
    a[3] = NINF
    b[3] = 0.0
    a[4] = torch.softmax(a[4].double(), 0).float()
    if V > 1:
        a[4, dead] = 0.0
        b[4, dead] = 0.0
        b[4, torch.arange(V) % 5 == 2] = 0.0
    cols = torch.tensor([[1, 1, 1, 0], [1, 1, 1, 1], [1, 1, 1, 0], [1, 1, 1, 0], [1, 1, 1, 1]], dtype=torch.bool)
    return a, b, cols


def kl_ref(a, b, wrong: str = "") -> dict:
    """Float64 [R, 4] = (sum a, logsumexp a, sum b a, sum_{b != 0} b log a) with its bounds (NaN where a column has
    no meaning for the row: a negative ``a`` under the log)."""
    a, b = a.double(), b.double()
    V = a.shape[1]
    live = b != 0
    if wrong == "zero_b_counted":
        live = torch.ones_like(live)
    z = torch.zeros_like(a)
    ba = torch.where(live, b * a, z)
    bl = torch.where(live, b * torch.log(a), z)
    out = torch.stack([a.sum(1), torch.logsumexp(a, 1), ba.sum(1), bl.sum(1)], 1)
    n = ((V + 255) // 256 + 10) * E
    fin = torch.where(torch.isfinite(a), a.abs(), z)
    tol = torch.stack([n * fin.sum(1), LSE_TOL * out[:, 1].abs().clamp(min=1.0), n * ba.abs().sum(1),
                       (n + 4.5 * E) * bl.abs().sum(1)], 1) * SLACK
    return {"out": out, "tol": tol}


def kl_check(got: torch.Tensor, ref: dict, cols: torch.Tensor) -> torch.Tensor:
    """Mask [R, 4] of bad checked entries; an infinite reference (sum or lse of a row with -inf) must be met exactly."""
    r, tol = ref["out"], ref["tol"]
    inf = torch.isinf(r)
    bad = torch.where(inf, got.double() != r, bad_bound(got, torch.where(inf, torch.zeros_like(r), r),
                                                        torch.where(inf, torch.zeros_like(r), tol)))
    return bad & cols


def kl_emul(a, b) -> torch.Tensor:
    """fp32 emulation in the kernel's shape but another order: thread v % 256 adds its columns last to first, the 256
    threads meet neighbours first."""
    a, b = a.float(), b.float()
    R, V = a.shape
    per = (V + 255) // 256
    m = a.max(1, keepdim=True).values
    z = torch.zeros(R, V)
    live = b != 0
    terms = [a, torch.where(a == NINF, z, torch.exp(a - torch.where(m == NINF, torch.zeros(R, 1), m))),
             torch.where(live, b * a, z), torch.where(live, b * (torch.log2(a) * _f(0.6931471805599453)), z)]
    out = torch.zeros(R, 4)
    for c, t in enumerate(terms):
        pad = torch.zeros(R, per * 256)
        pad[:, :V] = t
        lanes = pad.view(R, per, 256)
        acc = torch.zeros(R, 256)
        for i in range(per - 1, -1, -1):
            acc = acc + lanes[:, i]
        while acc.shape[1] > 1:
            acc = acc[:, 0::2] + acc[:, 1::2]
        out[:, c] = acc[:, 0]
    out[:, 1] = m[:, 0] + torch.log(out[:, 1])
    return out
