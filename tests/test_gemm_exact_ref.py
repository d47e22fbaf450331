"""CPU checks of the reference side of tests/test_gemm_exact.py: the integer operands really make fp32 GEMM results
order-independent, fp32 arithmetic keeps the two GELU bounds with margin, and every comparator flags a wrong result
that the older norm-ratio criterion lets through."""
import pytest
import torch

import gemm_exact_util as U


@pytest.mark.parametrize("amax,bmax", U.RANGES_USED)
def test_sums_are_exact_in_fp32(amax, bmax):
    """Worst case below 2^24 for every K in use, and the fp32 matmul equals the float64 one -- on random operands and
    on the extreme ones (every product at its maximum)."""
    assert max(U.K_USED) == U.K_LIMIT
    for Kd in U.K_USED:
        assert U.worst_sum(Kd, amax, bmax) < 2 ** 24
        a = U.ints((24, Kd), -amax, amax, Kd)
        b = U.ints((Kd, 40), -bmax, bmax, Kd + 1)
        a[0], b[:, 0] = amax, bmax  # the largest possible sum
        a[1] = -amax
        ref = a.double() @ b.double()
        assert ref[0, 0] == amax * bmax * Kd and ref[1, 0] == -amax * bmax * Kd
        assert torch.equal((a @ b).double(), ref)
        assert torch.equal((a.bfloat16().float() @ b.bfloat16().float()).double(), ref)  # operands exact in bf16
        assert torch.equal(a.flip(1) @ b.flip(0), a @ b)  # another summation order, the same bits
        full = ref + U.BIAS_MAX + 2 * U.ADD_MAX
        assert torch.equal(full.float().double(), full)


def test_bf16_sentinel_is_exact_and_out_of_range():
    s = torch.tensor(U.BF16_FILL)
    assert s.bfloat16().float() == s and abs(U.BF16_FILL) > U.worst_sum(U.K_LIMIT)


def _gelu32(x, erf):
    from iit_amd.ops.torch_ops import gelu_new
    return torch.nn.functional.gelu(x) if erf else gelu_new(x)


def _dgelu32(x, erf):
    p = x.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(_gelu32(p, erf).sum(), p)
    return g


@pytest.mark.parametrize("erf", [False, True])
def test_gelu_bound_holds_for_fp32_with_margin(erf):
    """fp32 torch GELU of every integer pre-activation in [-256, 256], rounded to bf16, uses at most about half of
    the bound (0.29 tanh / 0.35 erf measured here, 0.55 over non-integer inputs): room for the reference's own error,
    none for a wrong kernel."""
    pre = torch.arange(-256, 257, dtype=torch.float32)
    got = _gelu32(pre, erf).bfloat16()
    ref = U.gelu64(pre, erf)
    ratio = ((got.double() - ref).abs() / (2.0 ** -7 * ref.abs() + 2.0 ** -14)).max().item()
    print(f"gelu erf={erf}: worst |err| / bound = {ratio:.3f}")
    assert ratio <= 0.6
    assert not U.bad_gelu(got, pre, erf).any()


@pytest.mark.parametrize("erf", [False, True])
def test_dgelu_bound_holds_for_fp32_with_margin(erf):
    """fp32 torch ``s * gelu'(pre)`` rounded to bf16, for integer sums s and random bf16 pre: about half of the bound
    (0.49-0.50 measured: rounding the output to bf16 alone costs up to 2^-8 |ref|, half of the relative term)."""
    g = torch.Generator().manual_seed(5)
    pre = torch.randn(512, 384, generator=g).bfloat16().float()
    s = U.exact_mm(U.ints((512, 256), -U.A_MAX, U.A_MAX, 1), U.ints((256, 384), -U.B_MAX, U.B_MAX, 2))
    got = (s * _dgelu32(pre, erf)).bfloat16()
    ref = s.double() * U.dgelu64(pre, erf)
    bound = 2.0 ** -7 * ref.abs() + 2.0 ** -14 * s.double().abs().clamp(min=1.0)
    ratio = ((got.double() - ref).abs() / bound).max().item()
    print(f"dgelu erf={erf}: worst |err| / bound = {ratio:.3f}")
    assert ratio <= 0.6
    assert not U.bad_dgelu(got, s, pre, erf).any()


def _problem(amax, bmax):
    M, N, Kd = 256, 384, 640  # the output of the older tolerance tests
    a = U.ints((M, Kd), -amax, amax, 21)
    b = U.ints((Kd, N), -bmax, bmax, 22)
    bias = U.ints((N,), -U.BIAS_MAX, U.BIAS_MAX, 23)
    return a, b, bias


def test_linear_comparators_flag_what_the_norm_ratio_passes():
    a, b, bias = _problem(U.A_MAX, U.B_MAX)
    ref = U.exact_mm(a, b) + bias
    assert not U.bad_f32(ref.clone(), ref).any() and not U.bad_bf16(ref.bfloat16(), ref).any()
    # (the element of smallest magnitude: +-1 is visible in bf16 only below 256, where bf16 holds every integer)
    wrong = U.perturbations(a, b, bias)
    assert set(wrong) == {"one_off", "tiles_swapped", "bias_shifted", "k_slice_missing"}
    for name, p in wrong.items():
        assert U.bad_f32(p, ref).any(), name
        assert U.bad_bf16(p.bfloat16(), ref).any(), name
        for got in (p, p.bfloat16()):
            r = U.norm_ratio(got.float(), ref)
            print(f"{name} ({got.dtype}): norm ratio {r:.2e}")
            if name in ("one_off", "bias_shifted"):  # the recorded reason for the exact tests
                assert r < 1e-2, (name, r)
    assert int(U.bad_f32(wrong["one_off"], ref).sum()) == 1
    nan = ref.clone()
    nan[3, 5] = float("nan")
    assert int(U.bad_f32(nan, ref).sum()) == 1 and int(U.bad_bf16(nan.bfloat16(), ref).sum()) == 1


@pytest.mark.parametrize("erf", [False, True])
def test_gelu_comparator_flags_wrong_pre_activations(erf):
    a, b, bias = _problem(U.UNIT_MAX, U.UNIT_MAX)
    pre = U.exact_mm(a, b) + bias
    assert pre.abs().max() <= 256
    assert not U.bad_gelu(_gelu32(pre, erf).bfloat16(), pre, erf).any()
    # GELU is flat far below zero: the single wrong element is taken where the function moves (the smallest |pre|)
    for name, p in U.perturbations(a, b, bias).items():
        assert U.bad_gelu(_gelu32(p, erf).bfloat16(), pre, erf).any(), name
        assert U.bad_bf16(p.bfloat16(), pre).any(), name  # the stored pre-activation
    nan = _gelu32(pre, erf).bfloat16()
    nan[0, 0] = float("nan")
    assert int(U.bad_gelu(nan, pre, erf).sum()) == 1


@pytest.mark.parametrize("erf", [False, True])
def test_dgelu_comparator_flags_wrong_sums(erf):
    a, b, bias = _problem(U.A_MAX, U.B_MAX)
    g = torch.Generator().manual_seed(6)
    pre = torch.randn(256, 384, generator=g).bfloat16().float()
    gp = _dgelu32(pre, erf)
    s = U.exact_mm(a, b) + bias
    assert not U.bad_dgelu((s * gp).bfloat16(), s, pre, erf).any()
    # +-1 in s shows where gelu' is not small and |s| is: 1 * gelu' against 2^-7 |s gelu'|
    at = divmod(int((s.abs() + 1000.0 * (gp.abs() < 0.5)).argmin()), s.shape[1])
    for name, p in U.perturbations(a, b, bias, at=at).items():
        assert U.bad_dgelu((p * gp).bfloat16(), s, pre, erf).any(), name


def test_padding_check_sees_one_touched_element():
    for dtype in (torch.float32, torch.bfloat16):
        buf, pre = U.out_buffer(8, 5, 16, dtype, "cpu", init=torch.ones(8, 5))
        assert torch.equal(buf[:, :5].float(), torch.ones(8, 5)) and U.padding_touched(buf, pre, 5) == 0
        buf[:, :5] = 2.0
        assert U.padding_touched(buf, pre, 5) == 0
        buf[7, 15] = 0.0
        assert U.padding_touched(buf, pre, 5) == 1
    x = U.padded(torch.ones(4, 3), 8, torch.bfloat16)
    assert x.dtype == torch.bfloat16 and torch.isnan(x[:, 3:]).all() and torch.equal(x[:, :3].float(), torch.ones(4, 3))


def test_cpu_fallback_keeps_the_gpu_library_gemms_in_fp32():
    """The dispatcher's fp32 library GEMM falls back to a bf16-output GEMM where ``torch.mm(out_dtype=...)`` is
    missing; that fallback rounds the product, so a CPU call that needs it must not switch it on for the GPU (it did:
    the ``blas`` candidate then returned 260 for an exact 259)."""
    from iit_amd.ops import gemm_dispatch as gd
    a = U.ints((32, 512), -U.A_MAX, U.A_MAX, 1).bfloat16()
    b = U.ints((512, 48), -U.B_MAX, U.B_MAX, 2).bfloat16()
    got = gd._mm_f32(a, b)
    c = torch.empty(32, 48)
    gd._mm_f32_into(c, a, b)
    gd._addmm_f32(c, torch.zeros(32, 48), a, b)
    exact = U.exact_mm(a, b)
    assert got.dtype == torch.float32 and (torch.equal(got, exact) or torch.equal(got, exact.bfloat16().float()))
    assert all(dev_type == "cpu" for (_, dev_type), ok in gd._BLAS_OK.items() if not ok), gd._BLAS_OK
