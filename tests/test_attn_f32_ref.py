"""The fp32 attention bounds of tests/attn_f32_util.py checked on the CPU, ahead of the fp32 attention kernel they
are written for: two fp32 re-implementations stay far inside them, the selector family is exact in fp32, every
perturbation is flagged well outside."""
import functools

import pytest
import torch

import attn_exact_util as E
import attn_f32_util as A


@functools.lru_cache(maxsize=None)
def _case(c):
    B, S, H, dh, causal = c
    case = A.normal_case(B, S, H, dh, seed=100 + S + dh)
    scale = dh ** -0.5
    return case, scale, A.reference(case["q"], case["k"], case["v"], case["do"], causal, scale)


@pytest.mark.parametrize("c", A.CASES, ids=A.case_id)
def test_fp32_implementations_use_a_quarter_of_every_bound(c):
    case, scale, ref = _case(c)
    for impl in (A.impl_softmax, A.impl_exp2):
        r = A.ratios(impl(case["q"], case["k"], case["v"], case["do"], c[4], scale), ref)
        print(impl.__name__, {n: round(x, 4) for n, x in r.items()})
        assert max(r.values()) <= 0.25, (impl.__name__, r)


def test_reference_values_agree_with_the_bf16_tests_reference():
    B, S, H, dh, causal = 2, 17, 3, 16, True
    case = A.normal_case(B, S, H, dh, seed=5)
    ref = A.reference(case["q"], case["k"], case["v"], case["do"], causal, 0.25)
    old = E.reference(case["q"], case["k"], case["v"], case["do"], causal, 0.25)
    for n in A.OUTPUTS:
        assert torch.allclose(ref[n], old[n], rtol=1e-12, atol=1e-12), n


@pytest.mark.parametrize("S,dh,causal", [(16, 16, True), (33, 64, False), (33, 4, True)])
def test_selector_family_is_exact_in_fp32(S, dh, causal):
    scale = dh ** -0.5
    sc = A.selector_case(2, S, 3, dh, causal, scale, seed=7)
    for impl in (A.impl_softmax, A.impl_exp2):
        got = impl(sc["q"], sc["k"], sc["v"], sc["do"], causal, scale)
        for n in A.OUTPUTS:
            assert torch.equal(got[n], sc["want"][n]), (impl.__name__, n)


@pytest.mark.parametrize("name", A.PERTURBATIONS)
def test_every_perturbation_is_flagged(name):
    c = (3, 17, 3, 16, True)
    case, scale, ref = _case(c)
    r = A.ratios(A.perturbed(case, True, scale, name), ref)
    print(name, {n: round(x, 1) for n, x in r.items()})
    assert max(r.values()) >= 4.0, r
