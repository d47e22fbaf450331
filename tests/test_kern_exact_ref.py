"""CPU proof of the comparators of tests/kern_exact_util.py (layer norm, cross-entropy, fused Adam), no GPU needed.

* The bounds are not tighter than the arithmetic: an fp32 emulation of each operation with another summation order
  (forward, and reversed) passes every comparator on every operand family with no bad element.
* Every listed perturbation is flagged by a comparator; whether the criterion of tests/test_hip_kernels.py (norm
  ratios below 1e-2 / 1e-3 / 1e-4, ``allclose`` for lse and Adam) also sees it is recorded below and asserted.
"""
import pytest
import torch

import kern_exact_util as X

F32, BF16 = torch.float32, torch.bfloat16


def _count(bad: dict) -> dict:
    return {n: int(m.sum()) for n, m in bad.items() if int(m.sum())}


# ================================================================================================ layer norm
LN_EMUL_D = [1, 3, 4, 66, 255, 256, 260, 1023, 1024, 1028, 2049, 4095, 4096]


@pytest.mark.parametrize("rev", [False, True])
@pytest.mark.parametrize("family", X.LN_FAMILIES)
@pytest.mark.parametrize("d", LN_EMUL_D)
def test_ln_bounds_hold_for_fp32_emulation(d, family, rev):
    T = 5
    for affine in (True, False):
        x, w, b = X.ln_inputs(family, T, d, seed=d, affine=affine)
        ref = X.ln_fwd_ref(x, w, b, X.LN_EPS)
        got = X.ln_fwd_emul(x, w, b, X.LN_EPS, rev)
        assert not _count(X.ln_fwd_check(got, ref)), (affine, _count(X.ln_fwd_check(got, ref)))
        if family == "balanced" and d % 2 == 0:
            assert not int(X.bad_balanced(got["y"], x).sum())
        mean32, rstd32 = ref["mean"].float(), ref["rstd"].float()
        for bf16_dy in (False, True):
            i = X.ln_bwd_inputs(T, d, seed=d, bf16_dy=bf16_dy)
            kw = dict(dres=i["dres"], dx0=i["dx0"], dy2=i["dy2"], dw0=i["dw0"], db0=i["db0"])
            r = X.ln_bwd_ref(i["dy"], x, mean32, rstd32, w, **kw)
            g = X.ln_bwd_emul(i["dy"], x, mean32, rstd32, w, rev, **kw)
            assert not _count(X.ln_bwd_check(g, r)), (affine, bf16_dy, _count(X.ln_bwd_check(g, r)))
        if not affine:  # the bf16-xhat backward
            xh = got["y"]
            i = X.ln_bwd_inputs(T, d, seed=d + 1, bf16_dy=True)
            r = X.ln_bwd_ref(i["dy"], xh, None, rstd32, None, dres=i["dres"], xh16=True)
            g = X.ln_bwd_emul(i["dy"], xh, None, rstd32, None, rev, dres=i["dres"], xh16=True)
            assert not _count({"dx": X.bad_bound(g["dx"], r["dx"], r["tol_dx"])})


@pytest.mark.parametrize("rev", [False, True])
@pytest.mark.parametrize("T,d", [(149, 8), (1021, 16), (257, 130)])
def test_ln_affine_gradient_bounds_hold_over_many_rows(T, d, rev):
    x, w, b = X.ln_inputs("random", T, d, seed=T)
    ref = X.ln_fwd_ref(x, w, b, X.LN_EPS)
    mean32, rstd32 = ref["mean"].float(), ref["rstd"].float()
    i = X.ln_bwd_inputs(T, d, seed=T, bf16_dy=False)
    dead = X.sel_dead(T, 3, 0b101)
    r = X.ln_bwd_ref(i["dy"], x, mean32, rstd32, w, dw0=i["dw0"], db0=i["db0"])
    g = X.ln_bwd_emul(i["dy"], x, mean32, rstd32, w, rev, dw0=i["dw0"], db0=i["db0"])
    assert not _count(X.ln_bwd_check(g, r))
    assert int(dead.sum()) and not bool(dead.all())


# name -> (d, family, whether tests/test_hip_kernels.py's criterion also flags it)
LN_FWD_PERTURBATIONS = {
    "var_dm1": (4096, "random", False),
    "stats_pad4": (1023, "random", False),
    "stats_drop_last": (1024, "random", False),
    "eps_after": (256, "lowvar", True),
    "no_bias": (260, "random", True),
    "swap_groups": (260, "random", True),
    "last_row_missing": (260, "random", True),
}


@pytest.mark.parametrize("name", sorted(LN_FWD_PERTURBATIONS))
def test_ln_forward_perturbation_is_flagged(name):
    d, family, old_flags = LN_FWD_PERTURBATIONS[name]
    x, w, b = X.ln_inputs(family, 5, d, seed=7)
    ref = X.ln_fwd_ref(x, w, b, X.LN_EPS)
    bad = X.ln_fwd_ref(x, w, b, X.LN_EPS, wrong=name)
    got = {"y": bad["y"].float().bfloat16(), "mean": bad["mean"].float(), "rstd": bad["rstd"].float()}
    assert _count(X.ln_fwd_check(got, ref)), name
    ratio = X.norm_ratio(got["y"].float(), ref["y"])
    assert (not ratio < 1e-2) == old_flags, (name, ratio)


def test_ln_balanced_family_flags_divisor_and_tail():
    """w = 1, b = 0 and rows of m -+ 2^k: all |y| of a row are one bf16 value; the divisor d - 1 at d = 8 and a
    dropped tail column change it."""
    x, w, b = X.ln_inputs("balanced", 5, 8, seed=3)
    ok = X.ln_fwd_ref(x, w, b, X.LN_EPS)
    assert not int(X.bad_balanced(ok["y"].float().bfloat16(), x).sum())
    for wrong in ("stats_drop_last", "swap_groups"):
        y = X.ln_fwd_ref(x, w, b, X.LN_EPS, wrong=wrong)["y"].float().bfloat16()
        assert int(X.bad_balanced(y, x).sum()), wrong
    y = X.ln_fwd_ref(x, w, b, X.LN_EPS, wrong="var_dm1")["y"].float().bfloat16()
    assert int(X.bad_bound(y, ok["y"], ok["tol_y"]).sum())


# name -> whether the old criterion (dx ratio < 1e-3, dw / db ratio < 1e-4) also flags it
LN_BWD_PERTURBATIONS = {"no_mean_g": True, "dead_in_dw": True, "last_row_missing": True}


@pytest.mark.parametrize("name", sorted(LN_BWD_PERTURBATIONS))
def test_ln_backward_perturbation_is_flagged(name):
    T, d = 9, 260
    x, w, b = X.ln_inputs("random", T, d, seed=11)
    f = X.ln_fwd_ref(x, w, b, X.LN_EPS)
    mean32, rstd32 = f["mean"].float(), f["rstd"].float()
    i = X.ln_bwd_inputs(T, d, seed=11, bf16_dy=False)
    dead = X.sel_dead(T, 3, 0b101)
    ref = X.ln_bwd_ref(i["dy"], x, mean32, rstd32, w, dres=i["dres"], dead=dead)
    bad = X.ln_bwd_ref(i["dy"], x, mean32, rstd32, w, dres=i["dres"], dead=dead, wrong=name)
    got = {k: bad[k].float() for k in ("dx", "dw", "db")}
    assert _count(X.ln_bwd_check(got, ref)), name
    old = not (X.norm_ratio(got["dx"], ref["dx"]) < 1e-3 and X.norm_ratio(got["dw"], ref["dw"]) < 1e-4
               and X.norm_ratio(got["db"], ref["db"]) < 1e-4)
    assert old == LN_BWD_PERTURBATIONS[name], name


# ================================================================================================ cross-entropy
CE_EMUL_V = [1, 3, 7, 8, 9, 255, 257, 1025, 4097]


@pytest.mark.parametrize("rev", [False, True])
@pytest.mark.parametrize("family", X.CE_FAMILIES)
@pytest.mark.parametrize("V", CE_EMUL_V)
def test_ce_bounds_hold_for_fp32_emulation(V, family, rev):
    R = 3
    x, labels = X.ce_inputs(family, R, V, seed=V)
    gs, inv = 0.75, 1.0 / R
    ref = X.ce_ref(x, labels, gs, inv)
    assert bool(torch.isfinite(ref["lse"]).all())  # no row is entirely -inf
    assert not _count(X.ce_fwd_check(X.ce_fwd_emul(x, labels, rev), ref))
    g = X.ce_bwd_emul(x, labels, ref["lse32"], gs, inv)
    assert not int(X.bad_bound(g, ref["grad"], ref["tol_grad"]).sum())
    assert not int(X.bad_bound(g.bfloat16(), ref["grad"], ref["tol_grad16"]).sum())
    if family == "equal":
        assert torch.equal(ref["amax"], torch.zeros(R, dtype=torch.int64))
        want = x[:, 0].double() + torch.log(torch.tensor(float(V), dtype=torch.float64))
        assert float((ref["lse"] - want).abs().max()) < 1e-12
    if family == "ties":
        tc = X.ce_tie_columns(V)
        assert ref["amax"].tolist() == [tc[r % len(tc)] for r in range(R)]
    if family.startswith("masked"):
        dead = torch.isinf(x)
        assert V < 4 or bool(dead.any())
        assert bool((ref["tol_grad"][dead] == 0).all()) and bool((ref["grad"][dead] == 0).all())


def test_ce_families_reach_the_seams():
    assert X.ce_label_columns(1025) == [0, 1023, 1024] and X.ce_label_columns(8200) == [0, 8199]
    assert X.ce_label_columns(4097) == [0, 4095, 4096]
    assert X.ce_tie_columns(8200) == [3, 4, 255, 256, 4095, 4096, 8199]
    x, _ = X.ce_inputs("masked_scatter", 1, 8200, 0)
    assert bool(torch.isinf(x[0, 4:8]).all()) and bool(torch.isinf(x[0, 4100:4104]).all())  # thread 1's whole share


# name -> whether the old criterion (lse atol 1e-4, amax equal, gradient ratio < 1e-5, pad == 0) also flags it
CE_PERTURBATIONS = {
    "lse_drop_last": True,
    "lse_reads_pad": True,
    "tie_highest": False,  # random logits have no ties: the old test cannot see the rule
    "onehot_shift": True,
    "no_inv_rows": True,
    "pad_prefill": False,  # the old pad check covers one shape with ld_out == pad8(V) only
}


@pytest.mark.parametrize("name", sorted(CE_PERTURBATIONS))
def test_ce_perturbation_is_flagged(name):
    R, V = 3, 1025
    gs, inv = 0.75, 1.0 / R
    x, labels = X.ce_inputs("ties" if name == "tie_highest" else "random", R, V, seed=5)
    ref = X.ce_ref(x, labels, gs, inv)
    ld_out = X.pad8(V) + 8
    buf, prefill = X.ce_out(R, ld_out, F32)
    rows = buf[:R * ld_out].view(R, ld_out)
    rows.zero_()
    if name == "pad_prefill":
        rows[:, :V] = ref["grad"].float()
        rows[1, ld_out - 1] = X.NAN
        got_f = {k: ref[k].float() for k in ("lse", "loss")}
        got_f["amax"] = ref["amax"]
    else:
        bad = X.ce_ref(x, labels, gs, inv, wrong=name)
        rows[:, :V] = bad["grad"].float()
        got_f = {"lse": bad["lse"].float(), "loss": bad["loss"].float(), "amax": bad["amax"]}
    flagged = _count(X.ce_fwd_check(got_f, ref)) or _count(X.ce_grad_check(buf, prefill, ref, R, V, ld_out))
    assert flagged, name
    # the old criterion on its own inputs: random logits and labels, dense, ld_out = pad8(V)
    xo, lo = X.ce_inputs("random", R, V, seed=5)
    ro = X.ce_ref(xo, lo, gs, inv)
    if name == "pad_prefill":
        old = False
    else:
        bo = X.ce_ref(xo, lo, gs, inv, wrong=name)
        old = not (torch.allclose(bo["lse"], ro["lse"], atol=1e-4) and torch.equal(bo["amax"], ro["amax"])
                   and X.norm_ratio(bo["grad"], ro["grad"]) < 1e-5)
    assert old == CE_PERTURBATIONS[name], name


# ================================================================================================ fused Adam
def _adam_case(family, seed=0, n=4 * 700):
    active = torch.ones(n, dtype=torch.bool)
    active[40:52] = False
    return X.adam_state(family, n, active, seed), active


@pytest.mark.parametrize("rev", [False, True])
@pytest.mark.parametrize("t", X.ADAM_T)
@pytest.mark.parametrize("wd", [0.0, 0.1])
@pytest.mark.parametrize("clip", [None, 1e6, 0.5])
@pytest.mark.parametrize("family", ["random", "tiny"])
def test_adam_bounds_hold_for_fp32_emulation(family, clip, wd, t, rev):
    st, active = _adam_case(family)
    if family == "tiny" and clip == 0.5:
        clip = 1e-11  # below the norm of the tiny gradients
    kw = dict(X.ADAM_HYPER, wd=wd, clip=clip, active=active)
    ref = X.adam_ref(st["p"], st["g"], st["m"], st["v"], t, **kw)
    got = X.adam_emul(st["p"], st["g"], st["m"], st["v"], t, rev=rev, **kw)
    assert not _count(X.adam_check(got, ref, active)), _count(X.adam_check(got, ref, active))
    assert torch.equal(got["p"][~active], st["p"][~active])


# name -> (family, whether allclose(atol=1e-5, rtol=1e-4) on the updated weights also flags it)
ADAM_PERTURBATIONS = {
    "bc2_no_sqrt": ("random", True),
    "eps_in_sqrt": ("tiny", True),
    "decay_unclipped": ("random", True),
    "coef_sq": ("random", True),
    "t_off": ("random", True),
    "mirror_early": ("random", False),  # the old tests never read the mirror the kernel wrote
}


@pytest.mark.parametrize("name", sorted(ADAM_PERTURBATIONS))
def test_adam_perturbation_is_flagged(name):
    family, old_flags = ADAM_PERTURBATIONS[name]
    st, active = _adam_case(family, seed=2)
    kw = dict(X.ADAM_HYPER, wd=0.1, clip=1e-11 if family == "tiny" else 0.5, active=active)
    ref = X.adam_ref(st["p"], st["g"], st["m"], st["v"], 2, **kw)
    bad = X.adam_ref(st["p"], st["g"], st["m"], st["v"], 2, wrong=name, **kw)
    got = {k: bad[k].float() for k in ("p", "m", "v")}
    got["mirror"] = bad["mirror"]
    assert _count(X.adam_check(got, ref, active)), name
    old = not torch.allclose(got["p"], ref["p"].float(), atol=1e-5, rtol=1e-4)
    assert old == old_flags, name


def test_adam_arena_spans():
    """The restricted embedding cuts the arena into spans of every length around the 256-thread stride and its
    unrolled multiples."""
    from iit_amd.engine.flat import FlatParams
    m = X.adam_model()
    flat = FlatParams(m)
    assert flat.restrict_rows(m["emb"].weight, X.adam_live_rows())
    tab, n = flat.span_table()
    lens = tab[:n, 2].tolist()
    assert flat.offset_of(m["emb"].weight) == 0
    for want in (1, 255, 256, 257, 1023, 1024):
        assert want in lens, (want, lens)
    assert lens.count(1024) >= 2 and lens.count(1) >= 2  # 1024 itself, and 1025 = 1024 + 1
    assert m["lin"].weight.numel() % 4 and m["lin"].bias.numel() % 4
