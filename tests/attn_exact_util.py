"""Helpers shared by the exact attention tests (tests/test_attn_exact.py on the GPU, tests/test_attn_exact_ref.py on
the CPU): a float64 reference of attention forward + backward with element-wise error bounds derived from the number
formats, three operand families, padded / strided buffers and the perturbations the comparators must flag.

Every operand value is exact in bf16, so the reference sees exactly what the kernels see.  A comparator returns the
boolean mask of elements outside their bound; a test passes only with no such element.

Bounds (``u`` = 2^-8, the unit roundoff of bf16 round-to-nearest, one term per bf16 rounding point of the kernels;
every bound is built from reference quantities alone and multiplied by 1 + 2^-8 for the fp32 accumulation and the
hardware exp / rcp):

* ``tol_z  = u (sum_j P |V| + |z|)``            P is rounded before the PV product, then the output is rounded
* ``tol_D  = sum_d |dO| tol_z``                 D = rowsum(dO o z) is built from the stored bf16 z
* ``tol_dS = u |dS| + P tol_D``                 dS = P (dP - D) is rounded before the dQ / dK products
* ``tol_dq = scale sum_j tol_dS |K| + u |dq|``
* ``tol_dk = scale sum_i tol_dS |Q| + u |dk|``  summed over the query heads of the KV group
* ``tol_dv = u (sum_i P |dO| + |dv|)``          summed over the query heads of the KV group
* ``lse``: ``|lse - ref| <= 2^-18 max(1, |ref|)`` -- 64 fp32 ulps of the score magnitude (the computation needs a
  handful: a product by scale * log2(e), one hardware log, a product by ln 2); one key too many or too few among at
  most 257 moves lse by at least 2^-9.
"""
import functools
import math

import torch

U = 2.0 ** -8
SLACK = 1.0 + 2.0 ** -8
LSE_TOL = 2.0 ** -18
EXACT_TOL = 2.0 ** -40  # selector family: P is one-hot to far below fp32 resolution
# Nats between the top score and the runner-up of the selector family.  40 would put the runner-up's weight far
# below fp32 resolution; 93 puts it below half the smallest bf16 denormal (e^-93 < 2^-134), so the P a kernel rounds to
# bf16 is one-hot exactly.  That is needed for dv: the MI355X MFMA accumulator does not round to nearest, so a weight
# of e^-80 (a normal bf16 number) times dO, added to an integer partial sum, moves it by one fp32 ulp towards zero
# (measured: dv = 4 - 2 - 2 came out as -2^-22 with leads of about 80 nats at dh 64, exact with 124 at dh 128).
SELECTOR_MARGIN = 93.0
BF16_FILL = -23168.0  # sentinel prefill of bf16 outputs (exact in bf16, outside every result's range)
NAN = float("nan")
OUTPUTS = ("z", "lse", "dq", "dk", "dv")


def bf16_exact(x: torch.Tensor) -> torch.Tensor:
    """``x`` rounded to bf16, kept in float64."""
    return x.float().bfloat16().double()


# ------------------------------------------------------------------------------ float64 reference
def allowed_keys(S: int, causal: bool, device="cpu") -> torch.Tensor:
    """[S, S] bool: query i may see key j."""
    m = torch.ones(S, S, dtype=torch.bool, device=device)
    return m.tril() if causal else m


def head_mask_sel(shape, head_mask: int, device="cpu") -> torch.Tensor:
    """The spliced-element mask [B,S,Hq,dh] of an interchange head mask."""
    sel = torch.zeros(shape, dtype=torch.bool, device=device)
    for h in range(shape[2]):
        if (head_mask >> h) & 1:
            sel[:, :, h] = True
    return sel


def reference(q, k, v, do, causal: bool, scale: float, sel=None, src=None, wrong=None) -> dict:
    """Float64 attention forward + backward of q [B,S,Hq,dh], k / v [B,S,Hkv,dh], dO [B,S,Hq,dh].

    ``sel`` (bool [B,S,Hq,dh]) with ``src`` (broadcastable to z): spliced elements of z take ``src`` and carry no
    gradient.  Returns z, lse [B,Hq,S], dq, dk, dv, their bounds ``tol_*`` (see the module docstring) and ``live``
    (bool [B,Hq,S]: rows whose lse a kernel has to produce -- rows with an unspliced element).

    ``wrong`` (dict) computes a deliberately wrong result instead, for :func:`perturbations`: ``admit`` (b, h, i, j)
    lets query i of head h see key j; ``kv_of`` {query head: KV head}; ``pad_keys`` n appends n zero keys (score 0,
    V = 0) that every query sees; ``dk_skip`` query head left out of dk."""
    wrong = wrong or {}
    q, k, v, do = (t.double() for t in (q, k, v, do))
    B, S, Hq, dh = q.shape
    Hkv = k.shape[2]
    rep = Hq // Hkv
    kv_of = torch.arange(Hq, device=q.device) // rep
    for h, hk in wrong.get("kv_of", {}).items():
        kv_of[h] = hk
    ke, ve = k[:, :, kv_of], v[:, :, kv_of]  # [B,S,Hq,dh]
    allow = allowed_keys(S, causal, q.device).expand(B, Hq, S, S).clone()
    if "admit" in wrong:
        b_, h_, i_, j_ = wrong["admit"]
        allow[b_, h_, i_, j_] = True
    npad = wrong.get("pad_keys", 0)
    if npad:
        zk = torch.zeros(B, npad, Hq, dh, dtype=torch.float64, device=q.device)
        ke, ve = torch.cat([ke, zk], 1), torch.cat([ve, zk], 1)
        allow = torch.cat([allow, torch.ones(B, Hq, S, npad, dtype=torch.bool, device=q.device)], -1)
    s = torch.einsum("bihd,bjhd->bhij", q, ke) * scale
    s = s.masked_fill(~allow, float("-inf"))
    lse = torch.logsumexp(s, -1)  # [B,Hq,S]
    P = torch.exp(s - lse.unsqueeze(-1))
    z = torch.einsum("bhij,bjhd->bihd", P, ve)
    if sel is None:
        sel = torch.zeros(B, S, Hq, dh, dtype=torch.bool, device=q.device)
    do_eff = torch.where(sel, torch.zeros_like(do), do)
    zout = z if src is None else torch.where(sel, src.double().expand_as(z), z)
    D = (do_eff * zout).sum(-1).permute(0, 2, 1)  # [B,Hq,S]
    dP = torch.einsum("bihd,bjhd->bhij", do_eff, ve)
    dS = P * (dP - D.unsqueeze(-1))
    dq = scale * torch.einsum("bhij,bjhd->bihd", dS, ke)
    dk_h = scale * torch.einsum("bhij,bihd->bjhd", dS, q)[:, :S]  # per query head
    dv_h = torch.einsum("bhij,bihd->bjhd", P, do_eff)[:, :S]
    if "dk_skip" in wrong:
        dk_h[:, :, wrong["dk_skip"]] = 0.0
    group = lambda t: t.reshape(B, S, Hkv, rep, dh).sum(3)  # noqa: E731
    if wrong.get("kv_of"):  # scatter by the (wrong) map
        dk = torch.zeros_like(k).index_add_(2, kv_of, dk_h)
        dv = torch.zeros_like(v).index_add_(2, kv_of, dv_h)
    else:
        dk, dv = group(dk_h), group(dv_h)
    out = {"z": zout, "lse": lse, "dq": dq, "dk": dk, "dv": dv, "live": ~sel.all(-1).permute(0, 2, 1)}
    if wrong:
        return out
    # bounds, from reference quantities only
    tol_z = U * (torch.einsum("bhij,bjhd->bihd", P, ve.abs()) + z.abs())
    tol_D = (do_eff.abs() * tol_z).sum(-1).permute(0, 2, 1)
    tol_dS = U * dS.abs() + P * tol_D.unsqueeze(-1)
    tol_dq = scale * torch.einsum("bhij,bjhd->bihd", tol_dS, ke.abs()) + U * dq.abs()
    tol_dk = group(scale * torch.einsum("bhij,bihd->bjhd", tol_dS, q.abs()) + U * dk_h.abs())
    tol_dv = group(U * (torch.einsum("bhij,bihd->bjhd", P, do_eff.abs()) + dv_h.abs()))
    tol_z = torch.where(sel, torch.zeros_like(tol_z), tol_z)  # spliced elements equal the source
    out.update(tol_z=tol_z * SLACK, tol_dq=tol_dq * SLACK, tol_dk=tol_dk * SLACK, tol_dv=tol_dv * SLACK)
    return out


# ------------------------------------------------------------------------------ comparators: bool masks of bad elements
def bad_bound(got: torch.Tensor, ref: torch.Tensor, tol: torch.Tensor) -> torch.Tensor:
    """Elements with ``|got - ref| > tol`` (NaN and the buffer sentinel count as bad)."""
    assert got.shape == ref.shape == tol.shape, (got.shape, ref.shape, tol.shape)
    return ~((got.double() - ref).abs() <= tol)


def bad_lse(got: torch.Tensor, ref: torch.Tensor, live=None) -> torch.Tensor:
    bad = ~((got.double() - ref).abs() <= LSE_TOL * ref.abs().clamp(min=1.0))
    return bad if live is None else bad & live


def bad_exact(got: torch.Tensor, want: torch.Tensor) -> torch.Tensor:
    return ~((got.double() - want.double()).abs() <= EXACT_TOL)


def check_bound(got: dict, ref: dict) -> dict:
    """The bound family's comparators: name -> mask of bad elements, for all five outputs."""
    out = {n: bad_bound(got[n], ref[n], ref["tol_" + n]) for n in ("z", "dq", "dk", "dv")}
    out["lse"] = bad_lse(got["lse"], ref["lse"], ref["live"])
    return out


def check_selector(got: dict, want: dict) -> dict:
    """The selector family's comparators against the closed forms of :func:`selector_case`."""
    out = {n: bad_exact(got[n], want[n]) for n in ("z", "dq", "dk", "dv")}
    out["lse"] = bad_lse(got["lse"], want["lse"], want["live"])
    return out


def check_count(got: dict, ref: dict, count: torch.Tensor) -> dict:
    """The count family: lse against log(number of unmasked keys) -- the scores are all 0 --, the rest under the
    bounds (the gradient that is identically zero has a zero bound)."""
    out = check_bound(got, ref)
    out["count"] = bad_lse(got["lse"], torch.log(count.double()).expand_as(ref["lse"]), ref["live"])
    return out


def n_bad(masks: dict) -> int:
    return int(sum(int(m.sum()) for m in masks.values()))


def norm_ratio(got: torch.Tensor, ref: torch.Tensor) -> float:
    """The criterion of the older tolerance tests: ||got - ref|| / ||ref|| (z passes below 1e-2, gradients 2e-2)."""
    return ((got.double() - ref.double()).norm() / ref.double().norm()).item()


def old_criterion_passes(got: dict, ref: dict) -> bool:
    """Whether the older tests would accept ``got``: the norm ratio of z and of each gradient (they never look at the
    flash lse)."""
    return norm_ratio(got["z"], ref["z"]) < 1e-2 and all(norm_ratio(got[n], ref[n]) < 2e-2 for n in ("dq", "dk", "dv"))


# ------------------------------------------------------------------------------ operand families
def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def bound_case(B, S, Hq, Hkv, dh, seed: int) -> dict:
    """randn rounded to bf16."""
    g = _gen(seed)
    r = lambda *sh: bf16_exact(torch.randn(*sh, generator=g))  # noqa: E731
    return {"q": r(B, S, Hq, dh), "k": r(B, S, Hkv, dh), "v": r(B, S, Hkv, dh), "do": r(B, S, Hq, dh)}


def selector_target(S: int, Hq: int, causal: bool) -> torch.Tensor:
    """t[h, i]: the key query i of head h selects; <= i when causal, different per head, hits both i and 0."""
    i = torch.arange(S).unsqueeze(0)
    h = torch.arange(Hq).unsqueeze(1)
    return (i * (h + 3) + h) % ((i + 1) if causal else S)


@functools.lru_cache(maxsize=None)
def codebook(dh: int, n: int, cmax: int) -> torch.Tensor:
    """[n, dh] +-1 codes whose pairwise dot products are all <= ``cmax``, picked greedily from a random pool (random
    codes alone exceed it among 257 keys of 64 bits)."""
    g = _gen(1234 + dh)
    pool = torch.randint(0, 2, (8192, dh), generator=g).float() * 2 - 1
    corr = pool @ pool.t()
    worst = torch.full((pool.shape[0],), -float(dh))
    chosen = []
    for i in range(pool.shape[0]):
        if worst[i] <= cmax:
            chosen.append(i)
            worst = torch.maximum(worst, corr[i])
            if len(chosen) == n:
                break
    assert len(chosen) == n, (dh, n, cmax, len(chosen))
    return pool[chosen].double()


def selector_case(B, S, Hq, Hkv, dh, causal: bool, scale: float, seed: int, sel=None, src=None) -> dict:
    """Keys are +-1 codes, q[b,i,h] = 16 k[b, t(h,i), h // rep]: the softmax is one-hot at t to far below fp32
    resolution (the builder asserts a lead of SELECTOR_MARGIN nats; the codes come from :func:`codebook`), so z, lse
    and dv have closed forms and dq = dk = 0.  V holds non-zero integers of +-[1, 8], dO integers of [-4, 4].
    Returns the operands, the closed forms (``want``) and the margin."""
    rep = Hq // Hkv
    t = selector_target(S, Hq, causal)  # [Hq,S]
    hk = torch.arange(Hq) // rep
    allow = allowed_keys(S, causal)
    for attempt in range(16):
        g = _gen(seed + 1000 * attempt)
        if dh < 32:  # too few random bits for distinct keys: distinct (dh - 1)-bit words plus a parity bit, so two
            # keys differ in >= 2 places and the lead is >= 64 scale nats (such cases run with scale 2)
            lowbits = min(dh - 1, 12)  # distinct in their low bits, random above
            assert S <= 2 ** lowbits
            words = torch.stack([torch.randperm(2 ** lowbits, generator=g)[:S] for _ in range(B * Hkv)])
            words = words + (torch.randint(0, 2 ** (dh - 1 - lowbits), words.shape, generator=g) << lowbits)
            words = words.view(B, Hkv, S).permute(0, 2, 1)
            kb = (words.unsqueeze(-1) >> torch.arange(dh - 1)) & 1
            k = torch.cat([kb, kb.sum(-1, keepdim=True) & 1], -1).double() * 2 - 1
        else:  # a random choice of S codes of the book per (batch, KV head), with random column signs
            cmax = math.floor(dh - SELECTOR_MARGIN / (16.0 * scale) - 1e-9)
            book = codebook(dh, max(S, 257), cmax)
            pick = torch.stack([torch.randperm(book.shape[0], generator=g)[:S] for _ in range(B * Hkv)])
            signs = torch.randint(0, 2, (B, 1, Hkv, dh), generator=g).double() * 2 - 1
            k = book[pick].view(B, Hkv, S, dh).permute(0, 2, 1, 3) * signs
        q = 16.0 * k[:, t.t(), hk.unsqueeze(0).expand(S, Hq)]  # [B,S,Hq,dh]
        s = torch.einsum("bihd,bjhd->bhij", q, k[:, :, hk]) * scale
        s = s.masked_fill(~allow, float("-inf"))
        top = s.gather(-1, t.expand(B, Hq, S).unsqueeze(-1)).squeeze(-1)
        rest = s.scatter(-1, t.expand(B, Hq, S).unsqueeze(-1), float("-inf")).amax(-1)
        margin = float((top - rest).min())
        if margin >= SELECTOR_MARGIN:
            break
    assert margin >= SELECTOR_MARGIN, (S, dh, margin)
    v = torch.randint(1, 9, (B, S, Hkv, dh), generator=g).double() * (torch.randint(0, 2, (B, S, Hkv, dh), generator=g) * 2 - 1)
    do = torch.randint(-4, 5, (B, S, Hq, dh), generator=g).double()
    z = v[:, t.t(), hk.unsqueeze(0).expand(S, Hq)]
    if sel is None:
        sel = torch.zeros(B, S, Hq, dh, dtype=torch.bool)
    do_eff = torch.where(sel, torch.zeros_like(do), do)
    if src is not None:
        z = torch.where(sel, src.double().expand_as(z), z)
    dv = torch.zeros(B, S, Hkv, dh, dtype=torch.float64)
    for h in range(Hq):
        dv[:, :, int(hk[h])].index_add_(1, t[h], do_eff[:, :, h])
    want = {"z": z, "lse": top, "dq": torch.zeros_like(q), "dk": torch.zeros_like(k), "dv": bf16_exact(dv),
            "dv_unrounded": dv, "live": ~sel.all(-1).permute(0, 2, 1)}
    return {"q": q, "k": k, "v": v, "do": do, "want": want, "margin": margin}


def count_cases(B, S, Hq, Hkv, dh, causal: bool, seed: int) -> list:
    """Two operand sets, q = 0 and k = 0, the rest random: every score is 0, so lse[i] = log(unmasked keys of i).
    Returns [(name, operands, count [S])]."""
    count = allowed_keys(S, causal).sum(-1)
    out = []
    for n, name in enumerate(("q0", "k0")):
        c = bound_case(B, S, Hq, Hkv, dh, seed + 7 * n)
        c["q" if name == "q0" else "k"].zero_()
        out.append((name, c, count))
    return out


# ------------------------------------------------------------------------------ padded, strided buffers
def embed(x: torch.Tensor, layout: str, dtype=torch.bfloat16, fill=NAN, device=None, align: int = 8):
    """A [B,S,H,dh] view holding ``x`` inside a larger ``fill``-ed buffer: extra rows after S in each batch, a padded
    head stride and a padded batch stride, every stride a multiple of ``align`` elements and no more (``align`` 8: the
    16-byte rows the attention inputs need; 4: the 8-byte stores of the flash gradients).  ``layout`` "contig" gives a
    plain contiguous tensor.  Returns (view, whole buffer)."""
    B, S, H, dh = x.shape
    device = device or x.device
    if layout == "contig":
        buf = x.to(device=device, dtype=dtype).contiguous().clone()
        return buf, buf
    assert layout == "padded"
    hs = dh + align
    ss = (H + 1) * hs + align
    bs = (S + 3) * ss + align
    buf = torch.full((B * bs + 2 * align,), fill, dtype=dtype, device=device)
    view = buf[align:].as_strided((B, S, H, dh), (bs, ss, hs, 1))  # first element at the minimum alignment too
    view.copy_(x.to(device=device, dtype=dtype))
    return view, buf


def embed_packed(q, k, v, dtype=torch.bfloat16, fill=NAN, device=None):
    """q, k, v (same head count) as the three views of one packed [B, S + 2, 3, H, dh] buffer with ``fill`` rows after
    S.  Returns ((qv, kv, vv), buffer)."""
    B, S, H, dh = q.shape
    assert k.shape == q.shape == v.shape
    device = device or q.device
    buf = torch.full((B, S + 2, 3, H, dh), fill, dtype=dtype, device=device)
    for n, t in enumerate((q, k, v)):
        buf[:, :S, n] = t.to(device=device, dtype=dtype)
    return tuple(buf[:, :S, n] for n in range(3)), buf


def out_like(shape, layout: str, dtype, device, align: int = 8):
    """A sentinel-prefilled output view (BF16_FILL for bf16, NaN for fp32) inside its padded buffer; returns (view,
    buffer, copy of the prefilled buffer)."""
    fill = NAN if dtype == torch.float32 else BF16_FILL
    if len(shape) == 4:
        view, buf = embed(torch.full(shape, fill), layout, dtype, fill, device, align)
    else:  # lse / D: [B,Hq,S] contiguous with a padded tail
        n = math.prod(shape)
        buf = torch.full((n + 16,), fill, dtype=dtype, device=device)
        view = buf[:n].view(shape)
    return view, buf, buf.clone()


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def padding_touched(views, buf: torch.Tensor, prefill: torch.Tensor) -> int:
    """Elements of ``buf`` outside ``views`` (one view or a list) that no longer hold their prefill bits."""
    views = [views] if isinstance(views, torch.Tensor) else list(views)
    keep = [v.clone() for v in views]
    for v in views:
        v.copy_(prefill.as_strided(v.shape, v.stride(), v.storage_offset() - buf.storage_offset()))
    n = int((bits(buf) != bits(prefill)).sum())
    for v, kp in zip(views, keep):
        v.copy_(kp)
    return n


# ------------------------------------------------------------------------------ perturbations a comparator must flag
PERTURBATIONS = ("causal_admits_next_key", "neighbour_kv_head", "pad_keys_take_part", "lse_block_from_next",
                 "dk_lacks_a_query_head", "z_chunks_swapped")


def perturbations(q, k, v, do, causal: bool, scale: float, ref: dict, at=(1, 1, 20)) -> dict:
    """Wrong results of the kinds a kernel produces at an edge: name -> dict of the five outputs.  Needs causal
    attention, Hkv >= 2 with Hq > Hkv, S >= 48 and S no multiple of 64.  ``at`` = (batch, query head, query row).

    * ``causal_admits_next_key``: one query row's causal mask admits key i + 1;
    * ``neighbour_kv_head``: one query head reads (and writes the gradients of) the neighbouring KV head;
    * ``pad_keys_take_part``: the keys past S of the last 64-key tile take part with score 0 (and V = 0);
    * ``lse_block_from_next``: one 16-row block's lse is the next block's;
    * ``dk_lacks_a_query_head``: dk of one KV head lacks one of its query heads;
    * ``z_chunks_swapped``: two 16-column chunks of one 16-row block of z are exchanged."""
    B, S, Hq, dh = q.shape
    Hkv = k.shape[2]
    assert causal and Hkv >= 2 and Hq > Hkv and S >= 48 and S % 64
    b, h, i = at
    hk = h // (Hq // Hkv)
    base = {n: ref[n] for n in OUTPUTS}
    out = {
        "causal_admits_next_key": reference(q, k, v, do, causal, scale, wrong={"admit": (b, h, i, i + 1)}),
        "neighbour_kv_head": reference(q, k, v, do, causal, scale, wrong={"kv_of": {h: (hk + 1) % Hkv}}),
        "pad_keys_take_part": reference(q, k, v, do, causal, scale, wrong={"pad_keys": -S % 64}),
        "dk_lacks_a_query_head": reference(q, k, v, do, causal, scale, wrong={"dk_skip": h}),
    }
    p = dict(base)
    p["lse"] = base["lse"].clone()
    p["lse"][b, h, 16:32] = base["lse"][b, h, 32:48]
    out["lse_block_from_next"] = p
    p = dict(base)
    p["z"] = base["z"].clone()
    p["z"][b, 16:32, h, 0:16] = base["z"][b, 16:32, h, 16:32]
    p["z"][b, 16:32, h, 16:32] = base["z"][b, 16:32, h, 0:16]
    out["z_chunks_swapped"] = p
    assert set(out) == set(PERTURBATIONS)
    return {n: {m: t[m] for m in OUTPUTS} for n, t in out.items()}
