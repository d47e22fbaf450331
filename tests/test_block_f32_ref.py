"""The references and bounds of tests/block_f32_util.py, proved on the CPU: an fp32 torch emulation of each kernel's
own expression order (csrc/block_f32.hip, the GELU epilogues of csrc/gemm_f32.hip) must pass every bound, the integer
selector case must come out bit for bit, and results with a known defect must be flagged.  Nothing here needs a GPU;
it passes before tests/test_block_f32_kernel.py runs anywhere."""
import pytest
import torch

import block_f32_util as B


def _none(bad: dict):
    return {k: int(v.sum()) for k, v in bad.items() if v.any()}


def test_gelu_bounds_hold_for_the_fp32_emulation():
    x = B.gelu_inputs(20000, 1)
    r = B.gelu_ref(x)
    assert not B.bad_bound(B.gelu_emul(x), r["y"], r["tol"]).any()
    g = (4.0 * torch.randn(x.numel(), generator=B.gen(2))).float()
    d = B.dgelu_ref(g, x)
    assert not B.bad_bound(B.dgelu_emul(g, x), d["y"], d["tol"]).any()


def test_gelu_bound_is_an_fp32_bound():
    """A bf16-rounded result, and the cancelling tanh form, fail where they differ from the exact value."""
    x = B.gelu_inputs(20000, 3)
    r = B.gelu_ref(x)
    rounded = B.gelu_emul(x).bfloat16().float()
    bad = B.bad_bound(rounded, r["y"], r["tol"])
    assert bad.sum() > 0.9 * (rounded != B.gelu_emul(x)).sum() > 0
    u = B._f(0.7978845608028654) * (x + B._f(0.044715) * x * x * x)
    tanh_form = 0.5 * x * (1.0 + (1.0 - 2.0 * (1.0 / (torch.exp(2.0 * u) + 1.0))))
    assert B.bad_bound(tanh_form, r["y"], r["tol"])[(x > -10) & (x < -4)].any()


@pytest.mark.parametrize("family", B.LN_FAMILIES)
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("d", B.LN_D)
def test_ln_bounds_hold_for_the_fp32_emulation(d, affine, family):
    for T in B.LN_T:
        x, w, b = B.ln_inputs(family, T, d, 10 * d + T, affine)
        ref = B.ln_fwd_ref(x, w, b, B.LN_EPS)
        dy = torch.randn(T, d, generator=B.gen(d + T)).float()
        for vec in ([False, True] if d % 4 == 0 else [False]):
            got = B.ln_fwd_emul(x, w, b, B.LN_EPS, vec)
            assert not _none(B.ln_fwd_check(got, ref)), (T, vec)
            bref = B.ln_bwd_ref(dy, x, got["mean"], got["rstd"], w)
            bgot = B.ln_bwd_emul(dy, x, got["mean"], got["rstd"], w, vec)
            assert not _none(B.ln_bwd_check(bgot, bref, affine)), (T, vec)


def test_ln_partial_sums_bound_over_several_blocks():
    T, d = 3 * B.PART_ROWS + 5, 68
    x, w, b = B.ln_inputs("random", T, d, 7, True)
    fwd = B.ln_fwd_emul(x, w, b, B.LN_EPS, True)
    dy = torch.randn(T, d, generator=B.gen(8)).float()
    ref = B.ln_bwd_ref(dy, x, fwd["mean"], fwd["rstd"], w)
    assert not _none(B.ln_bwd_check(B.ln_bwd_emul(dy, x, fwd["mean"], fwd["rstd"], w, True), ref, True))


def test_ln_bounds_flag_known_defects():
    T, d = 5, 768
    x, w, b = B.ln_inputs("random", T, d, 9, True)
    ref = B.ln_fwd_ref(x, w, b, B.LN_EPS)
    good = B.ln_fwd_emul(x, w, b, B.LN_EPS, True)
    assert B.bad_bound(good["y"].bfloat16().float(), ref["y"], ref["tol_y"]).float().mean() > 0.5  # a bf16 y
    biased = torch.rsqrt(x.var(1, unbiased=True) + B.LN_EPS)  # variance over d - 1
    assert B.bad_bound(biased, ref["rstd"], ref["tol_rstd"]).all()
    dy = torch.randn(T, d, generator=B.gen(10)).float()
    bref = B.ln_bwd_ref(dy, x, good["mean"], good["rstd"], w)
    bgot = B.ln_bwd_emul(dy, x, good["mean"], good["rstd"], w, True)
    assert B.bad_bound(bgot["dw"] - dy[T - 1] * ((x[T - 1] - good["mean"][T - 1]) * good["rstd"][T - 1]),
                       bref["dw"], bref["tol_dw"]).float().mean() > 0.9  # the last row dropped
    no_w = B.ln_bwd_emul(dy, x, good["mean"], good["rstd"], None, True)  # g = dy instead of dy * w
    assert B.bad_bound(no_w["dx"], bref["dx"], bref["tol_dx"]).float().mean() > 0.5


@pytest.mark.parametrize("d", [64, 256])
def test_selector_case_is_exact(d):
    T = 37
    x, w, b, dy, ref = B.selector_case(T, d, d)
    for vec in (False, True):
        got = B.ln_fwd_emul(x, w, b, 0.0, vec)
        got.update(B.ln_bwd_emul(dy, x, got["mean"], got["rstd"], w, vec))
        for k, v in ref.items():
            assert not B.bad_bits(got[k], v).any(), (k, vec)
