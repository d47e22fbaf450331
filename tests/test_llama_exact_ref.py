"""CPU proof of the comparators of tests/llama_exact_util.py, no GPU needed.

* The bounds are not tighter than the arithmetic: an fp32 torch emulation of each kernel's own expression, and one in
  a deliberately different order (lanes added last to first and joined neighbours first; ``exp`` for the exp2 product
  and the products associated the other way round; the rotary sum through an fma), pass every comparator with no bad
  element.  The worst ``|got - ref| / bound`` are printed (``-s``) and recorded below.
* The ``exact`` families (the dw sum, rotary) are exact in fp32: bit for bit the float64 result in either order.
* Every listed perturbation puts at least one element outside its bound; the factor by which the worst element misses
  it, and whether the ``rel < 1e-2`` criterion of tests/test_llama_ops.py lets the perturbation through, are recorded
  below (the ``*_PERT`` tables hold the same facts as assertions).
* ``patch_spec`` returns None for an index that needs nine runs in one dimension (the table holds 8).
* ``K.rotary`` refuses operands the kernels cannot take before the library is touched.

Worst ``|emulation - ref| / bound`` over both orders: RMSNorm y 0.991, rstd 0.154, dx 0.992, dw 0.368; rotary 0.992;
SwiGLU post 0.986, dup 0.990, dgate 0.986 (the bf16 store takes nearly all of every bound of a bf16 result; where the
result is fp32 -- rstd, dw -- the emulations use a sixth to a third of it).

Perturbations: the worst miss in units of the bound (asserted from below at about half the figure) and the norm ratio
against the limit tests/test_llama_ops.py holds that output to (1e-2 for y, rotary and post, 2e-2 for dx, dw and the
SwiGLU gradients); "passes" marks the ones that criterion lets through.

==========================================  ==================  ===========  ======
perturbation                                worst / bound       norm ratio   passes
==========================================  ==================  ===========  ======
RMS mean over d - 8 columns, d = 520        y 2.3, rstd 6.4e3   4.5e-3       yes
RMS mean over d - 8 columns, d = 4104       y 1.1, rstd 227     1.7e-3       yes
RMS eps omitted (``tiny`` family)           y 115, rstd 5.1e5   0.42         no
RMS w shifted by 8 columns (forward)        y 5.6e4             0.59         no
RMS neighbouring row's rstd (backward)      dx 1.4e3 / 3.0e5    1.1e-2       yes
RMS w shifted by 8 columns (backward)       dx 2.3e4 / 1.1e7    0.21         no
RMS s not divided by d                      dx 5.8e5 / 2.4e7    4.2          no
RMS dres dropped                            dx 7.2e4 / 8.1e6    0.94         no
RMS one row dropped from dw                 dw 1.2e6            0.40         no
rotary table read at i1 for i0              5.7e4               1.0 (*)      yes
rotary offset ignored                       NaN (prefilled)     1.4          no
rotary pairing swapped                      2.0e5               1.05         no
rotary sign not applied (inverse)           2.4e4               1.4          no
rotary pass-through not copied              sentinel, bitwise   --           no
SwiGLU 1 % on the ``g (1 - s)`` term        dgate 900 (2.4 %)   1.7e-3       yes
SwiGLU s rounded to bf16                    post 1.9, dgate 162 1.8e-3       yes
SwiGLU dgate and dup swapped                1.3e10              > 1          no
splice position ranges ignored              bitwise             --           no
splice gradient not zeroed / one added      20 / 1 elements     --           --
==========================================  ==================  ===========  ======

(dx figures: bf16 / fp32 x.)  (*) on tables whose entries all differ; on the model's tables, the only ones
tests/test_llama_ops.py passes, the perturbed result is bit-identical
(``test_rotary_table_index_is_invisible_on_the_models_tables``).  The splice kernels have no norm-ratio test of
their own: tests/test_llama_ops.py compares them with the separate pass through a whole model.
"""
import pytest
import torch

import llama_exact_util as X

F32, BF16 = torch.float32, torch.bfloat16


def _norm_ratio(got, ref) -> float:
    got, ref = got.double(), ref.double()
    ok = torch.isfinite(got) & torch.isfinite(ref)
    return float((got[ok] - ref[ok]).norm() / ref[ok].norm().clamp(min=1e-300))


def _flagged(name, got, ref, tol, min_factor, passes_norm, limit=1e-2):
    """``got`` (a perturbed result) against ``ref`` / ``tol``: at least one element misses its bound, by at least
    ``min_factor``; the norm ratio is below ``limit`` (what tests/test_llama_ops.py asks of that output) exactly when
    ``passes_norm``."""
    bad = X.bad_bound(got, ref, tol)
    w = X.worst(got, ref, tol)
    nr = _norm_ratio(got, ref)
    print(f"{name}: {int(bad.sum())} bad, worst {w:.3g} x bound, norm ratio {nr:.3g}")
    assert int(bad.sum()) >= 1 and w >= min_factor, (name, int(bad.sum()), w)
    if passes_norm is not None:
        assert (nr < limit) == passes_norm, (name, nr)


# ================================================================================================ RMSNorm
@pytest.mark.parametrize("rev", [False, True], ids=["kernel_order", "other_order"])
@pytest.mark.parametrize("x_dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("family", X.RMS_FAMILIES)
@pytest.mark.parametrize("d", [8, 520, 1032, 4104, 8192])
def test_rms_emulations_stay_below_the_bounds(d, family, x_dtype, rev):
    T = 5
    for affine in (True, False):
        x, w = X.rms_inputs(family, T, d, d + T, x_dtype, affine)
        ref = X.rms_fwd_ref(x, w, X.RMS_EPS)
        got = X.rms_fwd_emul(x, w, X.RMS_EPS, rev)
        assert not X.count(X.rms_fwd_check(got, ref)), (affine, X.worst(got["y"], ref["y"], ref["tol_y"]))
        if family == "balanced":
            assert not int(X.bad_rms_balanced(got["y"], x).sum())
        b = X.rms_bwd_inputs("random", T, d, d, x_dtype)
        rstd = got["rstd"]
        for dres in (b["dres"], None):
            bref = X.rms_bwd_ref(b["dy"], x, rstd, w, dres, b["dw0"])
            bgot = X.rms_bwd_emul(b["dy"], x, rstd, w, rev, dres, b["dw0"])
            wdx = X.worst(bgot["dx"], bref["dx"], bref["tol_dx"])
            wdw = X.worst(bgot["dw"], bref["dw"], bref["tol_dw"])
            print(f"rms d={d} {family} y {X.worst(got['y'], ref['y'], ref['tol_y']):.3f} "
                  f"rstd {X.worst(got['rstd'], ref['rstd'], ref['tol_rstd']):.3f} dx {wdx:.3f} dw {wdw:.3f}")
            assert not int(X.bad_bound(bgot["dx"], bref["dx"], bref["tol_dx"]).sum()), wdx
            assert not int(X.bad_bound(bgot["dw"], bref["dw"], bref["tol_dw"]).sum()), wdw


@pytest.mark.parametrize("rev", [False, True])
@pytest.mark.parametrize("x_dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("T,d", [(1, 8), (65, 72), (129, 264)])
def test_rms_dw_exact_family_is_exact_in_fp32(T, d, x_dtype, rev):
    x, rstd = X.rms_exact_x(T, d, T + d, x_dtype)
    b = X.rms_bwd_inputs("exact", T, d, T, x_dtype)
    ref = X.rms_bwd_ref(b["dy"], x, rstd, None, None, b["dw0"])
    got = X.rms_bwd_emul(b["dy"], x, rstd, None, rev, None, b["dw0"])
    assert float(ref["dw"].abs().max()) < 2 ** 24
    assert not int(X.bad_bits(got["dw"], ref["dw"].float()).sum())
    drop = X.rms_bwd_ref(b["dy"], x, rstd, None, None, b["dw0"], wrong="dw_drop_row")
    assert int(X.bad_bits(drop["dw"].float(), ref["dw"].float()).sum())


# (perturbation, least factor by which the worst element misses its bound, passes rel < 1e-2)
RMS_FWD_PERT = [("mean_dm8", "random", 520, 3e3, True), ("mean_dm8", "random", 4104, 100.0, True),
                ("no_eps", "tiny", 520, 2e5, False), ("w_shift8", "random", 520, 2e4, False)]


@pytest.mark.parametrize("wrong,family,d,factor,passes", RMS_FWD_PERT)
def test_rms_fwd_perturbations_are_flagged(wrong, family, d, factor, passes):
    x, w = X.rms_inputs(family, 4, d, 3, BF16)
    ref = X.rms_fwd_ref(x, w, X.RMS_EPS)
    bad = X.rms_fwd_ref(x, w, X.RMS_EPS, wrong=wrong)
    # the perturbed result as the kernel would store it (bf16)
    _flagged(f"rms_fwd {wrong} {family} {d}", bad["y"].float().bfloat16(), ref["y"], ref["tol_y"],
             factor if wrong == "w_shift8" else 1.0, passes)
    if wrong != "w_shift8":
        _flagged(f"rms_fwd {wrong} {d} rstd", bad["rstd"].float(), ref["rstd"], ref["tol_rstd"], factor, None)


RMS_BWD_PERT = [("neighbour_rstd", "dx", 700.0, True), ("w_shift8", "dx", 1e4, False),
                ("s_not_div_d", "dx", 2e5, False), ("no_dres", "dx", 3e4, False), ("dw_drop_row", "dw", 5e5, False)]


@pytest.mark.parametrize("x_dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("wrong,key,factor,passes", RMS_BWD_PERT)
def test_rms_bwd_perturbations_are_flagged(wrong, key, factor, passes, x_dtype):
    T, d = 6, 520
    x, w = X.rms_inputs("random", T, d, 4, x_dtype)
    rstd = X.rms_fwd_emul(x, w, X.RMS_EPS, False)["rstd"]
    b = X.rms_bwd_inputs("random", T, d, 5, x_dtype)
    ref = X.rms_bwd_ref(b["dy"], x, rstd, w, b["dres"], b["dw0"])
    bad = X.rms_bwd_ref(b["dy"], x, rstd, w, b["dres"], b["dw0"], wrong=wrong)
    got = bad[key].float() if key == "dw" else bad[key].to(x_dtype)
    _flagged(f"rms_bwd {wrong}", got, ref[key], ref["tol_" + key], factor, passes, limit=2e-2)


# ================================================================================================ rotary
@pytest.mark.parametrize("other", [False, True], ids=["kernel_order", "fma_order"])
@pytest.mark.parametrize("family", X.FAMILIES)
@pytest.mark.parametrize("adjacent", [False, True], ids=["halves", "adjacent"])
@pytest.mark.parametrize("D,rd", X.ROT_SHAPES)
def test_rotary_emulations_stay_below_the_bound(D, rd, adjacent, family, other):
    for offset in X.ROT_OFFSETS:
        for inverse in (False, True):
            x, cos, sin = X.rotary_inputs(family, X.ROT_B, X.ROT_S, X.ROT_H, D, rd, offset, D + rd)
            ref = X.rotary_ref(x, cos, sin, rd, offset, adjacent, inverse)
            got = X.rotary_emul(x, cos, sin, rd, offset, adjacent, inverse, other)
            assert not bool(torch.isnan(ref["out"]).any())
            assert not X.count(X.rotary_check(got, x, ref, rd, family))
            if family == "exact":
                assert float(ref["out"].abs().max()) <= 64 and bool((ref["out"] * 4 == (ref["out"] * 4).round()).all())
            else:
                print(f"rotary {D} {rd} worst {X.worst(got[..., :rd], ref['out'][..., :rd], ref['tol'][..., :rd]):.3f}")


# (perturbation, inverse, D, rd, passes rel < 1e-2 on the model's tables)
ROT_PERT = [("table_i1", False, 128, 128, True), ("no_offset", False, 128, 64, False),
            ("swap_pairing", False, 16, 16, False), ("no_sign", True, 24, 16, False), ("no_pass", False, 24, 16, False)]


@pytest.mark.parametrize("family", X.FAMILIES)
@pytest.mark.parametrize("wrong,inverse,D,rd,passes_model", ROT_PERT)
def test_rotary_perturbations_are_flagged(wrong, inverse, D, rd, passes_model, family):
    x, cos, sin = X.rotary_inputs(family, X.ROT_B, X.ROT_S, X.ROT_H, D, rd, 3, 9)
    ref = X.rotary_ref(x, cos, sin, rd, 3, False, inverse)
    bad = X.rotary_ref(x, cos, sin, rd, 3, False, inverse, wrong=wrong)
    got = bad["out"].float().bfloat16()
    n = X.count(X.rotary_check(got, x, ref, rd, family))
    assert n, wrong
    assert ("pass" in n) == (wrong == "no_pass")
    print(f"rotary {wrong} {family}: {n}")
    if family == "random" and wrong != "no_pass":
        _flagged(f"rotary {wrong}", got[..., :rd], ref["out"][..., :rd], ref["tol"][..., :rd], 1e4, None)


def test_rotary_table_index_is_invisible_on_the_models_tables():
    """On tables that repeat each angle for both elements of a pair -- the only ones tests/test_llama_ops.py passes --
    a read at the partner's index changes nothing at all."""
    rd = 16
    ang = torch.arange(8, dtype=torch.float64).view(8, 1) * (10000.0 ** (-torch.arange(0, rd, 2).double() / rd))
    ang = torch.cat([ang, ang], 1)
    cos, sin = ang.cos().float(), ang.sin().float()
    x = torch.randn(2, 5, 3, rd, generator=X.gen(1)).bfloat16()
    ref = X.rotary_ref(x, cos, sin, rd, 3, False, False)
    bad = X.rotary_ref(x, cos, sin, rd, 3, False, False, wrong="table_i1")
    assert torch.equal(ref["out"], bad["out"])


# ================================================================================================ SwiGLU
def _sweep(seed: int):
    g = X.all_bf16()
    gn = X.gen(seed)
    return g, torch.randn(g.numel(), generator=gn).bfloat16(), torch.randn(g.numel(), generator=gn).bfloat16()


@pytest.mark.parametrize("other", [False, True], ids=["kernel_order", "other_order"])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_swiglu_emulations_stay_below_the_bounds(seed, other):
    """Every finite bf16 gate with |g| <= 2^40, normal u and dv, four seeds."""
    g, u, dv = _sweep(seed)
    assert g.numel() == 42754
    ref = X.swiglu_ref(g, u, dv)
    got = X.swiglu_emul(g, u, dv, other)
    w = {k: X.worst(got[k], ref[k], ref["tol_" + k]) for k in ("post", "dup", "dgate")}
    print(f"swiglu seed {seed} other {other}: {w}")
    assert not X.count(X.swiglu_check(got, ref)), w
    assert max(w.values()) < 1.0


SW_PERT = [("term_1pct", "dgate", 450.0, True), ("s_bf16", "post", 1.5, True), ("s_bf16", "dgate", 80.0, True),
           ("swap", "dgate", 1e9, False)]


@pytest.mark.parametrize("wrong,key,factor,passes", SW_PERT)
def test_swiglu_perturbations_are_flagged(wrong, key, factor, passes):
    g, u, dv = _sweep(0)
    ref = X.swiglu_ref(g, u, dv)
    bad = X.swiglu_ref(g, u, dv, wrong=wrong)
    got = bad[key].float().bfloat16()
    _flagged(f"swiglu {wrong} {key}", got, ref[key], ref["tol_" + key], factor, None)
    frac = float(X.bad_bound(got, ref[key], ref["tol_" + key]).double().mean())
    print(f"swiglu {wrong} {key}: {100 * frac:.2f} % of the inputs flagged")
    # the criterion of tests/test_llama_ops.py on its own kind of data (normal gate)
    gn = torch.randn(12040, generator=X.gen(5)).bfloat16()
    un, dn = torch.randn(12040, generator=X.gen(6)).bfloat16(), torch.randn(12040, generator=X.gen(7)).bfloat16()
    rn, bn = X.swiglu_ref(gn, un, dn), X.swiglu_ref(gn, un, dn, wrong=wrong)
    assert (_norm_ratio(bn[key].float().bfloat16(), rn[key]) < (2e-2 if key != "post" else 1e-2)) == passes


# ================================================================================================ splice
def test_patch_spec_refuses_nine_runs():
    from iit_amd.core.index import Ix
    from iit_amd.ops.splice import patch_spec
    shape = (X.SPL_B, X.SPL_S, X.SPL_D)
    assert patch_spec(Ix[:, X.NINE_RUNS], shape) is None
    assert patch_spec(Ix[:, X.NINE_RUNS[:8]], shape) is not None


def test_splice_masks_and_specs_agree():
    """The reference mask (torch indexing) and the range table of ``patch_spec`` select the same elements."""
    from iit_amd.ops.splice import patch_spec
    shape = (X.SPL_B, X.SPL_S, X.SPL_D)
    runs_seen = set()
    for name, ix in X.splice_indices().items():
        spec = patch_spec(ix, shape)
        assert spec is not None, name
        m = torch.ones(shape, dtype=torch.bool)
        for dim, (n, runs, _) in enumerate(spec.dims[1:]):
            sel = torch.zeros(n, dtype=torch.bool)
            for lo, hi in runs:
                sel[lo:hi] = True
            runs_seen.add(len(runs))
            m &= sel.view([-1 if i == dim else 1 for i in range(3)])
        assert torch.equal(m, X.splice_mask(ix, shape)), name
    assert {0, 1, 2, 3, 8} <= runs_seen
    assert not int(X.splice_mask(X.splice_indices()["none"], shape).sum())


@pytest.mark.parametrize("family", X.FAMILIES)
def test_splice_perturbations_are_flagged(family):
    shape = (X.SPL_B, X.SPL_S, X.SPL_D)
    B, S, d = shape
    ix = X.splice_indices()["inner_3_13"]
    mask = X.splice_mask(ix, shape)
    # forward: the position ranges ignored -> unselected elements take src
    src = X.splice_src("contiguous", shape, 1)
    W16 = (3.0 * torch.randn(9, d, generator=X.gen(2))).bfloat16()
    tok = torch.randint(0, 9, (B, S), generator=X.gen(3))
    ref = X.embed_splice_fwd_ref(tok, W16, src, mask)
    bad = X.embed_splice_fwd_ref(tok, W16, src, X.splice_mask(ix, shape, wrong="ignore_dim2"))
    assert int(X.bad_bits(bad, ref).sum()) and not int(X.bad_bits(ref.clone(), ref).sum())
    # backward
    vocab = 9
    terms = B * S + 1
    dout = X.int_operand(shape, F32, 4, terms) if family == "exact" else torch.randn(shape, generator=X.gen(4))
    dout[mask] = dout[mask].abs().clamp(min=1.0)  # no spliced gradient is zero
    g0 = X.int_operand((vocab, d), F32, 5, terms) if family == "exact" else torch.randn(vocab, d, generator=X.gen(5))
    r = X.embed_splice_bwd_ref(tok, dout, g0, mask)
    acc = g0.clone()  # fp32, rows last to first
    for t in range(B * S - 1, -1, -1):
        acc[tok.reshape(-1)[t]] += torch.where(mask.reshape(-1, d)[t], torch.zeros(d), dout.reshape(-1, d)[t])
    assert not int(X.bad_sum(acc, r["grad"], r["tol"], family, g0, r["n"]).sum())
    for wrong in ("not_zeroed", "one_added"):
        b = X.embed_splice_bwd_ref(tok, dout, g0, mask, wrong=wrong)
        n = int(X.bad_sum(b["grad"].float(), r["grad"], r["tol"], family, g0, r["n"]).sum())
        assert n >= 1, wrong
        print(f"embed_splice_bwd {wrong} {family}: {n} bad")
    # swiglu backward: a spliced gradient that is not zeroed is any non-zero value where == 0 is asked
    assert int(((dout != 0) & mask).sum()) == int(mask.sum())


# ================================================================================================ K.rotary refusals
def test_rotary_refuses_bad_operands_before_the_library_is_touched(monkeypatch):
    from iit_amd.ops import hip_kernels as K

    def no_lib():
        raise AssertionError("lib() reached")
    monkeypatch.setattr(K, "lib", no_lib)
    B, S, H, D, rd, off = 2, 5, 3, 16, 16, 3
    x = torch.zeros(B, S, H, D, dtype=BF16)
    out = torch.zeros(B, S, H, D, dtype=BF16)
    cos, sin = torch.zeros(off + S, rd), torch.zeros(off + S, rd)
    bad = {"x fp32": (x.float(), cos, sin),
           "x inner stride": (torch.zeros(B, S, H, 2 * D, dtype=BF16)[..., ::2], cos, sin),
           "cos fp64": (x, cos.double(), sin), "sin bf16": (x, cos, sin.bfloat16()),
           "cos strided": (x, torch.zeros(off + S, 2 * rd)[:, :rd], sin),
           "sin transposed": (x, cos, torch.zeros(rd, off + S).t()),
           "cos too narrow": (x, torch.zeros(off + S, rd - 2), sin),
           "sin too wide": (x, cos, torch.zeros(off + S, rd + 2)),
           "cos short": (x, cos[:off + S - 1].contiguous(), sin), "sin short": (x, cos, sin[:off + S - 1].contiguous())}
    for name, (xx, cc, ss) in bad.items():
        with pytest.raises(ValueError):
            K.rotary(xx, out, cc, ss, rd, off, False, False)
    with pytest.raises(AssertionError, match="lib\\(\\) reached"):  # a good call gets as far as the library
        K.rotary(x, out, cos, sin, rd, off, False, False)
