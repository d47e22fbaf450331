"""CPU checks of the arithmetic tests/test_gemm_f32.py rests on (helpers: tests/gemm_f32_util.py).

* Every exact family keeps every sum below 2^24 at every K the GPU module uses, so bitwise comparison is sound.
* fp32 ``torch.mm`` is exact on them, and the bitwise comparator flags the four perturbations of
  ``gemm_exact_util.perturbations``, a product with bf16-rounded operands (F2, F3, F3M) and the three-term bf16 split
  product (F3, F3M).
* The real-valued bound passes CPU fp32 and flags bf16-rounded operands on most elements at K = 64 and K = 256
  (not claimed at K = 1024, where the bound has grown past most of the bf16 error).
"""
import pytest
import torch

import gemm_exact_util as U
import gemm_f32_util as F

M, N = 128, 130  # two tiles of 64 each way (the perturbations swap tiles (0, 0) and (1, 1))
KS = (64, 256, 1024)


@pytest.mark.parametrize("family", F.EXACT)
def test_sums_stay_exact(family):
    assert max(F.K_USED) <= U.K_LIMIT
    for K in F.K_USED:
        assert F.worst_sum(family, K) < F.LIMIT, (family, K)
    if family == F.F2:
        assert F.F2_A * F.F2_B * 1024 == 12_579_840
    for K in F.K_USED:  # the generated operands respect the family's ranges
        a, b = F.operands(family, 9, 7, K, seed=K)
        assert torch.equal(a, a.round()) and torch.equal(b, b.round())
        worst = (a.double().abs() @ b.double().abs()).max().item() + U.BIAS_MAX + 2 * U.ADD_MAX
        assert worst <= F.worst_sum(family, K), (family, K, worst)
        if family == F.F3:
            assert int((a != 0).sum(1).max()) <= F.F3_NNZ and a.abs().max() < 2 ** 22 and b.abs().max() <= 1
        if family == F.F3M:
            assert int((b != 0).sum(0).max()) <= F.F3_NNZ and b.abs().max() < 2 ** 22 and a.abs().max() <= 1


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("family", F.EXACT)
def test_fp32_mm_is_exact_and_comparator_flags(family, K):
    a, b = F.operands(family, M, N, K, seed=100 + K)
    bias = U.ints((N,), -U.BIAS_MAX, U.BIAS_MAX, seed=7)
    ref = U.exact_mm(a, b) + bias
    assert not U.bad_f32(a @ b + bias, ref).any()  # fp32 in any summation order
    assert not U.bad_f32((a[:, :K // 2] @ b[:K // 2] + a[:, K // 2:] @ b[K // 2:]) + bias, ref).any()  # two splits
    for name, wrong in U.perturbations(a, b, bias).items():
        assert U.bad_f32(wrong, ref).any(), (family, K, name)
    frac16 = U.bad_f32(F.bf16_rounded_mm(a, b) + bias, ref).float().mean().item()
    frac3 = U.bad_f32(F.bf16_split3_mm(a, b) + bias, ref).float().mean().item()
    print(f"{family} K={K}: bf16-rounded operands flagged on {frac16:.3f}, three-term split on {frac3:.3f}")
    if family == F.F1:
        assert frac16 == 0.0 and frac3 == 0.0  # F1 is exact in bf16: it tests indexing, not precision
    else:
        assert frac16 > 0.5, (family, K, frac16)
    if family in (F.F3, F.F3M):
        assert frac3 > 0.5, (family, K, frac3)


@pytest.mark.parametrize("K", KS)
def test_real_bound(K):
    a, b = F.operands(F.REAL, M, N, K, seed=200 + K)
    g = torch.Generator().manual_seed(5)
    bias, resid = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    ref, mag = F.real_reference(a, b, bias, resid)
    got = (a @ b + bias) + resid
    worst = F.real_ratio(got, ref, mag, K).max().item()
    print(f"real K={K}: CPU fp32 worst ratio {worst:.4f}")
    assert worst <= 1.0
    for splits in (4,):  # a split sum passes with its own n
        h = K // splits
        parts = [a[:, i * h:(i + 1) * h] @ b[i * h:(i + 1) * h] for i in range(splits)]
        s = parts[0]
        for p in parts[1:]:
            s = s + p
        assert not F.bad_real((s + bias) + resid, ref, mag, K, splits).any()
    wrong = (a.bfloat16().float() @ b.bfloat16().float() + bias) + resid
    frac = F.bad_real(wrong, ref, mag, K).float().mean().item()
    print(f"real K={K}: bf16-rounded operands flagged on {frac:.3f}")
    if K in F.K_REAL:
        assert frac > 0.5, (K, frac)
    # one wrong element is flagged whatever K is
    got2 = got.clone()
    got2[3, 5] += 1.0
    assert F.bad_real(got2, ref, mag, K)[3, 5]


def test_lds_helper():
    out = F.lds([64, 64, 130, 130, 1])
    assert len(set(out)) == 5 and all(v % 4 == 0 for v in out)
    assert all(v > w for v, w in zip(out, [64, 64, 130, 130, 1]))
