"""Helpers for testing an fp32 attention kernel element by element (checked on the CPU by
tests/test_attn_f32_ref.py; the bf16 kernels have tests/attn_exact_util.py): a float64 reference of attention forward
+ backward with element-wise fp32 error bounds, two operand families, two fp32 re-implementations and the
perturbations the bounds must flag.

Operands are fp32 values, so the float64 reference sees exactly what a kernel sees.  Bounds, built from reference
quantities only, one term per rounding point of an fp32 implementation (``u`` = 2^-24, ``eta`` = 2^-126: an absolute
floor for a P that underflows in fp32 but not in float64; sums run over the allowed keys of a query; ``s`` is the
scaled score, ``dO`` the output gradient):

* ``A_ij    = scale sum_d |q_id| |k_jd|``
* ``e_i     = u ((dh + 2) max_j A_ij + 4 max_j |s_ij|)``   the score's fmaf chain (+ a split chain's add, the scale),
  the subtraction of the max / lse, the log2(e) product, the hardware exp's argument
* ``rho_i   = 2 e_i + (S + 8) u``                          P: numerator and denominator, the sum over S, exp, division
* ``rhob_i  = 2 rho_i``                                    P recomputed from the stored (rounded) lse
* ``tol_lse = e_i + (S + 8) u max(1, |lse_i|)``
* ``tol_z   = (rho_i + (S + 1) u) sum_j P |v| + eta sum_j |v|``
* ``ddP_ij  = (dh + 1) u sum_d |dO_id| |v_jd|``
* ``tol_D   = sum_d |dO| tol_z + (dh + 1) u sum_d |dO z| + sum_j (rhob P |dP| + P ddP) + (S + 1) u sum_j P |dP|
  + eta sum_j |dP|``                                       D formed as rowsum(dO o z) or as rowsum(P o dP)
* ``tol_dS  = (rhob_i + 4 u) |dS| + P (ddP + tol_D) + eta (|dP - D| + tol_D + ddP)``
* ``tol_dq  = scale sum_j (tol_dS + (S + 2) u |dS|) |k|``
* ``tol_dk  = scale sum_i (tol_dS + (S + 2) u |dS|) |q|``
* ``tol_dv  = sum_i ((rhob_i + (S + 1) u) P + eta) |dO|``

These are worst-case bounds: fp32 implementations that differ in summation order, exp2 against exp and the form of D
stay within a quarter of them and every perturbation, one bf16 rounding of an operand among them, exceeds one at
least 4-fold: the two figures tests/test_attn_f32_ref.py asserts (measured on the CPU: at most 0.08 of a bound, at
least 40-fold).
"""
import torch

from attn_exact_util import allowed_keys, selector_target

U = 2.0 ** -24
ETA = 2.0 ** -126
OUTPUTS = ("z", "lse", "dq", "dk", "dv")
SELECTOR_MARGIN = 110.0  # nats; e^-110 < 2^-158: below half the smallest fp32 denormal


# (B, S, H, dh, causal): S at the edges of 16-row tiles, dh a multiple of 16 or not, B H = 1, 9 and 8 (one wave, a
# ragged and a full group of four); a covering subset of the product
CASES = ((1, 1, 1, 16, True), (3, 3, 3, 4, False), (2, 15, 4, 20, True), (3, 16, 3, 16, True), (1, 16, 1, 64, False),
         (2, 17, 4, 64, True), (3, 17, 3, 4, False), (2, 33, 4, 16, False), (3, 33, 3, 20, True), (1, 64, 1, 64, True),
         (2, 64, 4, 16, False), (3, 64, 3, 64, False))


def case_id(c) -> str:
    return "B{}-S{}-H{}-dh{}-{}".format(*c[:4], "causal" if c[4] else "bidir")


def bf16_round(x: torch.Tensor) -> torch.Tensor:
    return x.float().bfloat16().to(x.dtype)


# ------------------------------------------------------------------------------ float64 reference
def reference(q, k, v, do, causal: bool, scale: float, wrong=None) -> dict:
    """Float64 attention forward + backward of q, k, v, dO ``[B,S,H,dh]``: z, lse ``[B,H,S]``, dq, dk, dv and their
    bounds ``tol_*`` (module docstring).  ``wrong`` (a set of names, see :data:`PERTURBATIONS`) computes a
    deliberately wrong result instead (no bounds)."""
    wrong = wrong or ()
    q, k, v, do = (t.double() for t in (q, k, v, do))
    B, S, H, dh = q.shape
    allow = allowed_keys(S, causal, q.device).expand(B, H, S, S).clone()
    if "one_key_too_many" in wrong:  # kj <= qi + 1
        allow = allow | torch.ones(S, S, dtype=torch.bool, device=q.device).tril(1)
    if "one_key_dropped" in wrong:  # every query with two or more keys loses its first
        drop = allow.sum(-1) > 1
        allow[..., 0] = allow[..., 0] & ~drop
    if "q_bf16" in wrong:
        q = bf16_round(q)
    if "k_bf16" in wrong:
        k = bf16_round(k)
    if "v_bf16" in wrong:
        v = bf16_round(v)
    if "do_bf16" in wrong:
        do = bf16_round(do)
    ks = k.roll(-1, 2) if "next_heads_k" in wrong else k  # head h reads head h + 1's k
    s = torch.einsum("bihd,bjhd->bhij", q, ks) * scale
    s = s.masked_fill(~allow, float("-inf"))
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse.unsqueeze(-1))
    if "lse_one_key_short" in wrong:  # the stored lse lacks each query's last key (P itself is right)
        last = allow.long().cumsum(-1).argmax(-1, keepdim=True)
        short = s.scatter(-1, last, float("-inf"))
        lse = torch.where(allow.sum(-1) > 1, torch.logsumexp(short, -1), lse)
    Pz = bf16_round(P) if "p_bf16" in wrong else P
    z = torch.einsum("bhij,bjhd->bihd", Pz, v)
    dP = torch.einsum("bihd,bjhd->bhij", do, v)
    D = (P * dP).sum(-1)  # [B,H,S]; = rowsum(dO o z)
    dS = P * (dP - D.unsqueeze(-1))
    dSr = bf16_round(dS) if "ds_bf16" in wrong else dS
    dq = (1.0 if "dq_lacks_scale" in wrong else scale) * torch.einsum("bhij,bjhd->bihd", dSr, ks)
    dk = scale * torch.einsum("bhij,bihd->bjhd", dSr, q)
    dv = torch.einsum("bhij,bihd->bjhd", P, do)
    out = {"z": z, "lse": lse, "dq": dq, "dk": dk, "dv": dv}
    if wrong:
        return out
    # bounds, from reference quantities only
    al = allow.double()
    A = scale * torch.einsum("bihd,bjhd->bhij", q.abs(), k.abs()) * al
    sabs = torch.where(allow, s.abs(), torch.zeros_like(s))
    e = U * ((dh + 2) * A.amax(-1) + 4 * sabs.amax(-1))  # [B,H,S]
    rho = 2 * e + (S + 8) * U
    rhob = 2 * rho
    tol_lse = e + (S + 8) * U * lse.abs().clamp(min=1.0)
    bihd = lambda t: t.permute(0, 2, 1).unsqueeze(-1)  # noqa: E731  [B,H,S] -> [B,S,H,1]
    tol_z = bihd(rho + (S + 1) * U) * torch.einsum("bhij,bjhd->bihd", P, v.abs()) \
        + ETA * torch.einsum("bhij,bjhd->bihd", al, v.abs())
    ddP = (dh + 1) * U * torch.einsum("bihd,bjhd->bhij", do.abs(), v.abs())
    PdP = (P * dP.abs()).sum(-1)
    tol_D = (do.abs() * tol_z).sum(-1).permute(0, 2, 1) + (dh + 1) * U * (do * z).abs().sum(-1).permute(0, 2, 1) \
        + rhob * PdP + (P * ddP).sum(-1) + (S + 1) * U * PdP + ETA * (al * dP.abs()).sum(-1)
    r3, tD = rhob.unsqueeze(-1), tol_D.unsqueeze(-1)
    tol_dS = ((r3 + 4 * U) * dS.abs() + P * (ddP + tD) + ETA * ((dP - D.unsqueeze(-1)).abs() + tD + ddP)) * al
    tds = tol_dS + (S + 2) * U * dS.abs()
    tol_dq = scale * torch.einsum("bhij,bjhd->bihd", tds, k.abs())
    tol_dk = scale * torch.einsum("bhij,bihd->bjhd", tds, q.abs())
    tol_dv = torch.einsum("bhij,bihd->bjhd", (r3 + (S + 1) * U) * P + ETA * al, do.abs())
    out.update(tol_z=tol_z, tol_lse=tol_lse, tol_dq=tol_dq, tol_dk=tol_dk, tol_dv=tol_dv)
    return out


def ratios(got: dict, ref: dict) -> dict:
    """name -> max over elements of |got - ref| / tol (inf for a NaN or for an error where the bound is 0)."""
    out = {}
    for n in OUTPUTS:
        err = (got[n].double().cpu() - ref[n]).abs()
        r = torch.where(err == 0, torch.zeros_like(err), err / ref["tol_" + n])
        out[n] = float(torch.nan_to_num(r, nan=float("inf")).max())
    return out


def bad(got: dict, ref: dict) -> dict:
    """name -> number of elements outside their bound (a NaN counts); no element is excluded."""
    return {n: int((~((got[n].double().cpu() - ref[n]).abs() <= ref["tol_" + n])).sum()) for n in OUTPUTS}


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and bool((bits(a.float().cpu()) == bits(b.float().cpu())).all())


# ------------------------------------------------------------------------------ operand families
def normal_case(B, S, H, dh, seed: int) -> dict:
    """Standard-normal fp32 q, k, v, dO."""
    g = torch.Generator().manual_seed(seed)
    return {n: torch.randn(B, S, H, dh, generator=g, dtype=torch.float32) for n in ("q", "k", "v", "do")}


def selector_case(B, S, H, dh, causal: bool, scale: float, seed: int) -> dict:
    """Integer-valued operands whose softmax is one-hot exactly in fp32: query i of head h selects key
    t = ``selector_target``.  k[j] = (j, -j^2, r...) and q[i] = c (2 t, 1, 0...) with c = 128 / scale, so the scaled
    score is 128 (t^2 - (t - j)^2): the selected key leads every other by >= 128 nats (asserted >=
    :data:`SELECTOR_MARGIN`), every other weight is exactly 0 with or without denormal flushing.  ``r`` (random
    integers in k's remaining columns) meets zeros in q.  V and dO are small integers.  ``scale`` must be a power of
    two (all products and sums are then exact, below 2^24).  Returns the operands and the closed forms ``want``:
    z = V[t], lse = the top score, dv[j] = the sum of dO over the queries that select j, dq = dk = 0."""
    assert dh >= 2 and 2.0 ** round(torch.log2(torch.tensor(scale)).item()) == scale
    g = torch.Generator().manual_seed(seed)
    t = selector_target(S, H, causal)  # [H,S]
    c = 128.0 / scale
    j = torch.arange(S, dtype=torch.float64)
    k = torch.randint(-3, 4, (B, S, H, dh), generator=g).double()
    k[..., 0] = j.view(1, S, 1)
    k[..., 1] = -(j * j).view(1, S, 1)
    q = torch.zeros(B, S, H, dh, dtype=torch.float64)
    q[..., 0] = 2 * c * t.t().double()
    q[..., 1] = c
    v = torch.randint(1, 9, (B, S, H, dh), generator=g).double() * (torch.randint(0, 2, (B, S, H, dh), generator=g) * 2 - 1)
    do = torch.randint(-4, 5, (B, S, H, dh), generator=g).double()
    s = torch.einsum("bihd,bjhd->bhij", q, k) * scale
    s = s.masked_fill(~allowed_keys(S, causal), float("-inf"))
    idx = t.expand(B, H, S).unsqueeze(-1)
    top = s.gather(-1, idx).squeeze(-1)
    margin = float((top - s.scatter(-1, idx, float("-inf")).amax(-1)).min()) if S > 1 else float("inf")
    assert margin >= SELECTOR_MARGIN and float(s[s.isfinite()].abs().max()) < 2.0 ** 24, (S, dh, margin)
    hh = torch.arange(H).unsqueeze(0).expand(S, H)
    z = v[:, t.t(), hh]
    dv = torch.zeros(B, S, H, dh, dtype=torch.float64)
    for h in range(H):
        dv[:, :, h].index_add_(1, t[h], do[:, :, h])
    want = {"z": z, "lse": top, "dq": torch.zeros_like(q), "dk": torch.zeros_like(k), "dv": dv}
    ops = {n: x.float() for n, x in (("q", q), ("k", k), ("v", v), ("do", do))}
    return {**ops, "want": {n: x.float() for n, x in want.items()}, "margin": margin}


# ------------------------------------------------------------------------------ two fp32 re-implementations
def impl_softmax(q, k, v, do, causal: bool, scale: float) -> dict:
    """fp32 torch: einsum scores, ``logsumexp`` / ``exp``, D = rowsum(dO o z)."""
    q, k, v, do = (t.float() for t in (q, k, v, do))
    S = q.shape[1]
    s = (torch.einsum("bihd,bjhd->bhij", q, k) * scale).masked_fill(~allowed_keys(S, causal, q.device), float("-inf"))
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse.unsqueeze(-1))
    z = torch.einsum("bhij,bjhd->bihd", P, v)
    D = (do * z).sum(-1).permute(0, 2, 1)
    dS = P * (torch.einsum("bihd,bjhd->bhij", do, v) - D.unsqueeze(-1))
    return {"z": z, "lse": lse, "dq": scale * torch.einsum("bhij,bjhd->bihd", dS, k),
            "dk": scale * torch.einsum("bhij,bihd->bjhd", dS, q), "dv": torch.einsum("bhij,bihd->bjhd", P, do)}


def impl_exp2(q, k, v, do, causal: bool, scale: float) -> dict:
    """fp32 torch in the order of operations of a tiled kernel: per-head matmuls summed the other way round (reversed
    d and key order), ``exp2`` of the log2-scaled difference from the row max, z normalised after the product, P
    recomputed from the stored lse, D = rowsum(P o dP), scale applied to dS."""
    q, k, v, do = (t.float().permute(0, 2, 1, 3).flip(-1) for t in (q, k, v, do))  # [B,H,S,dh], d reversed
    S = q.shape[2]
    allow = allowed_keys(S, causal, q.device)
    log2e, ln2 = 1.4426950408889634, 0.6931471805599453
    s = (q @ k.transpose(-1, -2)) * scale
    m = s.masked_fill(~allow, float("-inf")).amax(-1, keepdim=True)
    p = torch.where(allow, torch.exp2((s - m) * log2e), torch.zeros_like(s))
    tot = p.flip(-1).sum(-1, keepdim=True)
    lse = m + torch.log2(tot) * ln2
    z = (p @ v) * (1.0 / tot)
    P = torch.where(allow, torch.exp2((s - lse) * log2e), torch.zeros_like(s))
    dP = do @ v.transpose(-1, -2)
    D = (P * dP).sum(-1, keepdim=True)
    dS = P * (dP - D) * scale
    back = lambda t: t.flip(-1).permute(0, 2, 1, 3)  # noqa: E731
    return {"z": back(z), "lse": lse.squeeze(-1), "dq": back(dS @ k), "dk": back(dS.transpose(-1, -2) @ q),
            "dv": back(P.transpose(-1, -2) @ do)}


# ------------------------------------------------------------------------------ perturbations the bounds must flag
PERTURBATIONS = ("q_bf16", "k_bf16", "v_bf16", "do_bf16", "p_bf16", "ds_bf16", "one_key_too_many", "one_key_dropped",
                 "dq_lacks_scale", "next_heads_k", "lse_one_key_short")


def perturbed(case: dict, causal: bool, scale: float, name: str) -> dict:
    """The outputs of an implementation with the named defect (``one_key_too_many`` needs causal attention,
    ``next_heads_k`` H >= 2, the key-count ones S >= 2)."""
    assert name in PERTURBATIONS
    return reference(case["q"], case["k"], case["v"], case["do"], causal, scale, wrong={name})
