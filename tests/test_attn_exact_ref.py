"""CPU checks of the exact attention test utilities (tests/attn_exact_util.py): the selector family's margin at every
shape the GPU module (tests/test_attn_exact.py) uses, a torch emulation of the flash kernels' rounding points that has
to stay inside every bound, and the perturbations the comparators have to flag -- with, as an asserted fact, how
many of them the older norm-ratio criterion lets through."""
import math

import pytest
import torch

import attn_exact_util as X

FLASH_S = [1, 16, 17, 63, 64, 65, 127, 128, 129, 193, 257]
FLASH_DH = [64, 128]
MFMA_S = [1, 3, 4, 5, 8, 13, 15, 16]
MFMA_DH = [32, 64, 96, 128]
VALU_S = [1, 17, 33, 63, 64]
VALU_DH = [16, 24, 96]
LAYOUTS = [(4, 4), (4, 2), (6, 1)]


def kernel_scale(dh: int) -> float:
    """The score scale the GPU cases pass: 1 / sqrt(dh) from dh 64 on; 1 at dh 32 and 2 below, where the selector
    codes are too short for the lead it needs at 1 / sqrt(dh) (16 sqrt(32) = 90.5 nats is the whole top score)."""
    return 1.0 / math.sqrt(dh) if dh >= 64 else (1.0 if dh >= 32 else 2.0)


# ------------------------------------------------------------------------------ emulation of the flash kernels
LOG2E, LN2 = 1.4426950408889634, 0.6931471805599453
f32, bf = (lambda t: t.float()), (lambda t: t.bfloat16().float())


def emulate_flash(q, k, v, do, causal, scale, sel=None, src=None, tile=64):
    """csrc/flash_attn.hip in fp32 torch with its bf16 rounding points: 64-key tiles with the online softmax in the
    log2 domain, P rounded before P V, z rounded; the backward recomputes P from the saved lse and the stored z,
    rounds P and dS before the dV / dK / dQ products and rounds the outputs."""
    q, k, v, do = (f32(t) for t in (q, k, v, do))
    B, S, Hq, dh = q.shape
    Hkv = k.shape[2]
    rep = Hq // Hkv
    ke, ve = k.repeat_interleave(rep, 2), v.repeat_interleave(rep, 2)
    allow = X.allowed_keys(S, causal)
    sl2 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    m = torch.full((B, Hq, S), float("-inf"))
    lsum = torch.zeros(B, Hq, S)
    o = torch.zeros(B, Hq, S, dh)
    for k0 in range(0, S, tile):
        k1 = min(S, k0 + tile)
        s = torch.einsum("bihd,bjhd->bhij", q, ke[:, k0:k1]) * sl2
        s = s.masked_fill(~allow[:, k0:k1], float("-inf"))
        mn = torch.maximum(m, s.amax(-1))
        alpha = torch.where(mn == float("-inf"), torch.ones_like(mn), torch.exp2(m - mn))
        p = torch.where(s == float("-inf"), torch.zeros_like(s), torch.exp2(s - mn.unsqueeze(-1)))
        p = torch.nan_to_num(p, nan=0.0)  # rows that have not met a key yet (mn = -inf)
        lsum = lsum * alpha + p.sum(-1)
        o = o * alpha.unsqueeze(-1) + torch.einsum("bhij,bjhd->bhid", bf(p), ve[:, k0:k1])
        m = mn
    z = bf(o / lsum.unsqueeze(-1)).permute(0, 2, 1, 3)
    lse = (m + torch.log2(lsum)) * torch.tensor(LN2, dtype=torch.float32)
    if sel is None:
        sel = torch.zeros(B, S, Hq, dh, dtype=torch.bool)
    if src is not None:
        z = torch.where(sel, f32(src).expand_as(z), z)
    do = torch.where(sel, torch.zeros_like(do), do)
    D = (do * z).sum(-1).permute(0, 2, 1)
    s = torch.einsum("bihd,bjhd->bhij", q, ke) * torch.tensor(scale, dtype=torch.float32)
    P = torch.where(allow, torch.exp(s - lse.unsqueeze(-1)), torch.zeros_like(s))
    dS = P * (torch.einsum("bihd,bjhd->bhij", do, ve) - D.unsqueeze(-1))
    group = lambda t: t.reshape(B, S, Hkv, rep, dh).sum(3)  # noqa: E731
    return {"z": z, "lse": lse,
            "dq": bf(torch.einsum("bhij,bjhd->bihd", bf(dS), ke) * scale),
            "dk": bf(group(torch.einsum("bhij,bihd->bjhd", bf(dS), q)) * scale),
            "dv": bf(group(torch.einsum("bhij,bihd->bjhd", bf(P), do)))}


def worst_ratio(got, ref):
    return max(float(((got[n].double() - ref[n]).abs() / ref["tol_" + n].clamp(min=1e-300)).nan_to_num(0.0).max())
               for n in ("z", "dq", "dk", "dv"))


# ------------------------------------------------------------------------------ selector margin
@pytest.mark.parametrize("kernel,Ss,dhs", [("flash", FLASH_S, FLASH_DH), ("mfma", MFMA_S, MFMA_DH),
                                           ("valu", VALU_S + [64], VALU_DH + [128])])
def test_selector_margin_at_every_gpu_shape(kernel, Ss, dhs):
    """selector_case asserts the lead of the top score itself; its closed forms agree with the float64 reference."""
    for n, S in enumerate(Ss):
        for dh in dhs:
            for causal in (True, False):
                Hq, Hkv = LAYOUTS[n % 3] if kernel == "flash" else (3, 3)
                scale = kernel_scale(dh)
                c = X.selector_case(2, S, Hq, Hkv, dh, causal, scale, seed=S + dh)
                assert c["margin"] >= X.SELECTOR_MARGIN
                if dh in (64, 24) and S in (17, 129, 16, 64):
                    ref = X.reference(c["q"], c["k"], c["v"], c["do"], causal, scale)
                    for name, want in (("z", "z"), ("lse", "lse"), ("dq", "dq"), ("dk", "dk"), ("dv", "dv_unrounded")):
                        assert float((ref[name] - c["want"][want]).abs().max()) <= X.EXACT_TOL, (S, dh, name)


# ------------------------------------------------------------------------------ the emulation stays inside every bound
@pytest.mark.parametrize("S,dh,heads", [(17, 64, (4, 2)), (65, 64, (6, 1)), (130, 64, (4, 4)), (129, 128, (4, 2)),
                                        (257, 64, (4, 2))])
@pytest.mark.parametrize("causal", [True, False])
def test_emulated_kernel_within_bounds(S, dh, heads, causal):
    Hq, Hkv = heads
    B, scale = 2, kernel_scale(dh)
    # bound family, plain and with a head mask (source = arbitrary bf16 values)
    c = X.bound_case(B, S, Hq, Hkv, dh, seed=S)
    for mask in (0, 0b10):
        sel = X.head_mask_sel((B, S, Hq, dh), mask) if mask else None
        src = X.bf16_exact(torch.randn(B, S, Hq, dh, generator=torch.Generator().manual_seed(1))) if mask else None
        ref = X.reference(c["q"], c["k"], c["v"], c["do"], causal, scale, sel, src)
        got = emulate_flash(c["q"], c["k"], c["v"], c["do"], causal, scale, sel, src)
        bad = X.check_bound(got, ref)
        assert X.n_bad(bad) == 0, {n: int(m.sum()) for n, m in bad.items()}
        assert worst_ratio(got, ref) <= 1.0
    # selector family
    sc = X.selector_case(B, S, Hq, Hkv, dh, causal, scale, seed=S)
    got = emulate_flash(sc["q"], sc["k"], sc["v"], sc["do"], causal, scale)
    bad = X.check_selector(got, sc["want"])
    assert X.n_bad(bad) == 0, {n: int(m.sum()) for n, m in bad.items()}
    # count family
    for name, cc, count in X.count_cases(B, S, Hq, Hkv, dh, causal, seed=S):
        ref = X.reference(cc["q"], cc["k"], cc["v"], cc["do"], causal, scale)
        got = emulate_flash(cc["q"], cc["k"], cc["v"], cc["do"], causal, scale)
        bad = X.check_count(got, ref, count)
        assert X.n_bad(bad) == 0, (name, {n: int(m.sum()) for n, m in bad.items()})


# ------------------------------------------------------------------------------ perturbations
PB, PS, PHQ, PHKV, PDH = 2, 100, 4, 2, 64
# what the selector family cannot see, by construction: its softmax is one-hot, so a key that is wrongly admitted
# with a low score changes nothing, dk is identically zero, and every row's lse is the same top score
SELECTOR_BLIND = {"causal_admits_next_key", "pad_keys_take_part", "lse_block_from_next", "dk_lacks_a_query_head"}


def _flags(check, perts):
    return {name: X.n_bad(check(got)) for name, got in perts.items()}


def test_every_perturbation_is_flagged():
    scale = kernel_scale(PDH)
    # bound family: every perturbation, each through the output it damages
    c = X.bound_case(PB, PS, PHQ, PHKV, PDH, seed=3)
    ref = X.reference(c["q"], c["k"], c["v"], c["do"], True, scale)
    perts = X.perturbations(c["q"], c["k"], c["v"], c["do"], True, scale, ref)
    flags = _flags(lambda got: X.check_bound(got, ref), perts)
    assert all(flags[n] > 0 for n in X.PERTURBATIONS), flags
    assert X.n_bad(X.check_bound({n: ref[n] for n in X.OUTPUTS}, ref)) == 0
    damaged = {"causal_admits_next_key": "z", "neighbour_kv_head": "z", "pad_keys_take_part": "lse",
               "lse_block_from_next": "lse", "dk_lacks_a_query_head": "dk", "z_chunks_swapped": "z"}
    for name, out in damaged.items():
        assert int(X.check_bound(perts[name], ref)[out].sum()) > 0, (name, out)
    # count family: every perturbation in at least one of its two runs
    seen = {n: 0 for n in X.PERTURBATIONS}
    for _, cc, count in X.count_cases(PB, PS, PHQ, PHKV, PDH, True, seed=3):
        cref = X.reference(cc["q"], cc["k"], cc["v"], cc["do"], True, scale)
        cp = X.perturbations(cc["q"], cc["k"], cc["v"], cc["do"], True, scale, cref)
        for n, f in _flags(lambda got: X.check_count(got, cref, count), cp).items():
            seen[n] += f
    assert all(seen[n] > 0 for n in X.PERTURBATIONS), seen
    # selector family: exact on indexing (wrong KV head, misplaced chunk), blind to the rest by construction
    sc = X.selector_case(PB, PS, PHQ, PHKV, PDH, True, scale, seed=3)
    sref = X.reference(sc["q"], sc["k"], sc["v"], sc["do"], True, scale)
    sp = X.perturbations(sc["q"], sc["k"], sc["v"], sc["do"], True, scale, sref)
    flags = _flags(lambda got: X.check_selector(got, sc["want"]), sp)
    assert {n for n in X.PERTURBATIONS if flags[n] == 0} == SELECTOR_BLIND, flags


def test_old_norm_ratio_criterion_passes_two_perturbations():
    """The criterion of tests/test_flash_attn.py (norm ratio of z below 1e-2, of each gradient below 2e-2, lse never
    looked at) accepts two of the six wrong results at this small shape (B 2, S 100, 4 heads): the causal mask that
    admits one key too many (ratios 0.006 for z, 0.012 for dq and dk, 0.005 for dv; the bounds flag 59 + 48 + 21 + 58
    elements and the row's lse) and the misplaced lse block, which it never reads.  The other four change a whole
    head or a 16 x 16 block of a small tensor and are caught; their norm ratio shrinks as the tensor grows."""
    scale = kernel_scale(PDH)
    c = X.bound_case(PB, PS, PHQ, PHKV, PDH, seed=3)
    ref = X.reference(c["q"], c["k"], c["v"], c["do"], True, scale)
    perts = X.perturbations(c["q"], c["k"], c["v"], c["do"], True, scale, ref)
    passed = sorted(n for n, got in perts.items() if X.old_criterion_passes(got, ref))
    assert passed == ["causal_admits_next_key", "lse_block_from_next"], passed


def test_small_attention_lds_arithmetic():
    """The dynamic LDS of the VALU short-sequence kernels: the backward at S = 64, dh = 128 exceeds a CU's 160 KiB
    (the forward fits), S = 64 with dh = 96 is the largest corner the dispatcher still sends there."""
    from iit_amd.ops import hip_kernels as K
    assert K.attn_small_lds(64, 128, False) == 115712 and K.attn_small_lds(64, 128, True) == 165376
    assert K.attn_small_lds(64, 96, True) == 132608
    assert K.ATTN_SMALL_LDS_MAX == 163840
    assert K.attn_small_lds(64, 128, True) > K.ATTN_SMALL_LDS_MAX >= K.attn_small_lds(64, 128, False)
    assert not K.attn_small_ok(64, 128) and K.attn_small_ok(64, 96) and K.attn_small_ok(16, 128)
    assert not K.attn_small_ok(65, 64) and not K.attn_small_ok(16, 136)
