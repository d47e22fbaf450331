"""Element-wise cross-entropy tests on the GPU: ``ce_fwd``, ``ce_bwd`` (fp32, bf16, fp32 + ``out16``) and ``ce_bwd16``
of csrc/kernels.hip against the float64 reference and the derived bounds of tests/kern_exact_util.py (proved on the
CPU by tests/test_kern_exact_ref.py).

Every V around the float4 / wave / 1024-thread edges, R = 1, 3, 8, four logits layouts (dense, ``ld = V + 3`` whose
rows alternate between the aligned and the unaligned path, ``ld = pad8(V) + 8``, a base pointer one float past a
16-byte boundary) with NaN in every pad column, six operand families (random, a common offset of 1e4, all-equal, ties
across the float4 / thread / wave / seam boundaries, a block and a scattered third of the vocabulary at -inf), labels
at 0, V - 1 and both sides of the vector/scalar seam, ``gscale`` = 0.75 and ``inv_rows`` = 1 / R.  The gradient kernels
get the fp32 rounding of the reference lse.  Pad columns [V, ld_out) must be exactly zero, ``out16`` bitwise the bf16
rounding of the fp32 gradient, ``ce_bwd16`` bitwise ``out16``, and nothing past the last row may change.

Measured on an MI355X: 264 cases, 264 passed, none skipped, 3.8 s for the module; the slowest case is the first
launch (0.24 s), every other case 0.01 s or less.  Before the fix of ``online_add`` in csrc/kernels.hip the
``test_ce_fwd`` cases failed in the masked families from V = 8 on (all six that ran before the run was cut short: V = 8,
R = 1 / 3, three layouts): a thread whose first logit is -inf computed ``exp(-inf - (-inf))`` = NaN and poisoned the
row's lse and loss.  As a check of the module itself, a library whose cross-thread merge resolves ties to the highest
index failed all 120 ``test_ce_fwd`` cases with V > 1 and nothing else.
"""
import pytest
import torch

import kern_exact_util as X

pytestmark = pytest.mark.gpu

dev = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
GS = 0.75


@pytest.fixture(scope="module")
def K():
    from iit_amd.ops import hip_kernels
    hip_kernels.lib()
    old = hip_kernels.CHECK_BOUNDS
    hip_kernels.CHECK_BOUNDS = True
    yield hip_kernels
    hip_kernels.CHECK_BOUNDS = old


def _count(bad: dict) -> dict:
    return {n: int(m.sum()) for n, m in bad.items() if int(m.sum())}


def _fwd_out(R):
    return X.filled((R + 2,), F32, dev), X.filled((R + 2,), F32, dev), X.filled((R + 2,), torch.int64, dev)


@pytest.mark.parametrize("layout", X.CE_LAYOUTS)
@pytest.mark.parametrize("R", X.CE_R)
@pytest.mark.parametrize("V", X.CE_V)
def test_ce_fwd(K, V, R, layout):
    for family in X.CE_FAMILIES:
        x, labels = X.ce_inputs(family, R, V, seed=13 * V + R)
        ref = X.ce_ref(x, labels, GS, 1.0 / R)
        logits, ld = X.ce_layout(x.to(dev), layout)
        lab = labels.to(dev)
        loss, lse, amax = _fwd_out(R)
        K.ce_fwd(logits, ld, lab, loss, lse, amax, R, V)
        torch.cuda.synchronize()
        got = {"loss": loss[:R].cpu(), "lse": lse[:R].cpu(), "amax": amax[:R].cpu()}
        bad = _count(X.ce_fwd_check(got, ref))
        assert not bad, (family, bad, got["lse"], ref["lse"])
        assert bool(torch.isnan(loss[R:]).all()) and bool(torch.isnan(lse[R:]).all()) and bool((amax[R:] == -7).all())
        # without labels no loss, without amax no argmax: those outputs keep their prefill
        loss2, lse2, amax2 = _fwd_out(R)
        K.ce_fwd(logits, ld, None, loss2, lse2, None, R, V)
        torch.cuda.synchronize()
        assert not int(X.bad_bits(lse2[:R], lse[:R]).sum())
        assert bool(torch.isnan(loss2).all()) and bool((amax2 == -7).all())


@pytest.mark.parametrize("layout", X.CE_LAYOUTS)
@pytest.mark.parametrize("R", X.CE_R)
@pytest.mark.parametrize("V", X.CE_V)
def test_ce_bwd(K, V, R, layout):
    inv = 1.0 / R
    gscale = torch.tensor([GS], dtype=F32, device=dev)
    for k, family in enumerate(X.CE_FAMILIES):
        ld_out = X.pad8(V) + 8 * (k % 2)
        x, labels = X.ce_inputs(family, R, V, seed=13 * V + R)
        ref = X.ce_ref(x, labels, GS, inv)
        logits, ld = X.ce_layout(x.to(dev), layout)
        lab, lse = labels.to(dev), ref["lse32"].to(dev)
        (o32, p32), (o16, p16), (b16, pb16), (only16, po16) = (X.ce_out(R, ld_out, F32, dev), X.ce_out(R, ld_out, BF16, dev),
                                                              X.ce_out(R, ld_out, BF16, dev), X.ce_out(R, ld_out, BF16, dev))
        K.ce_bwd(logits, ld, lab, lse, gscale, inv, o32, ld_out, R, V, out16=o16)
        K.ce_bwd(logits, ld, lab, lse, gscale, inv, b16, ld_out, R, V)
        K.ce_bwd16(logits, ld, lab, lse, gscale, inv, only16, ld_out, R, V)
        torch.cuda.synchronize()
        for name, buf, pre in (("fp32", o32, p32), ("out16", o16, p16), ("bf16", b16, pb16), ("bwd16", only16, po16)):
            bad = _count(X.ce_grad_check(buf.cpu(), pre.cpu(), ref, R, V, ld_out))
            assert not bad, (family, name, bad)
        n = R * ld_out
        assert not int(X.bad_bits(o16[:n], o32[:n].bfloat16()).sum()), family
        assert not int(X.bad_bits(only16[:n], o16[:n]).sum()), family
        assert not int(X.bad_bits(b16[:n], o16[:n]).sum()), family
