"""Element-wise tests of the RMSNorm kernels of csrc/llama_ops.hip on the GPU (``rms_fwd_kernel<1 .. 16>``,
``rms_bwd_kernel<1 .. 16>``, ``rms_dw_vec_kernel`` and, under ``IIT_LLAMA_VEC=0`` from tests/test_launch_variants.py,
``rms_dw_kernel``) against the float64 references and bounds of tests/llama_exact_util.py (proved on the CPU by
tests/test_llama_exact_ref.py).  The kernels are called through ``iit_amd.ops.hip_kernels``, so ``rstd``, the prefills
and the buffers are the test's own: every output lies in a sentinel-filled buffer with spare elements behind it, and
the spare elements must keep their bits.

* forward / backward: ``d`` at both ends of every ``VB`` instantiation, T = 1, 3, 5, 9 (four rows per block), ``x`` bf16
  and fp32, ``w`` given and null, ``dres`` given and null, four operand families.
* ``dw``: T around the 64-row block, ``d`` around the 256-column (vector) and 64-column (scalar) block, integer operands
  bit for bit and normal data under the order-free bound, a non-zero prefill, columns past ``d`` untouched.
* the entry points refuse ``d % 8 != 0``, ``d = 8200`` and a view offset by one element, and write nothing.
* ``RMSNormFn`` / ``RMSNormForkFn`` on a non-contiguous and on an offset-by-one ``x`` (the ``_c16`` clone).

Measured on an MI355X: 256 cases, 256 passed, none skipped, 4.4 s for the module (the slowest case 0.8 s: the first
use of an autograd Function).  Worst ``|got - ref| / bound``: y 0.992 and dx 0.992 at every ``VB`` (the bf16 store takes
nearly all of the bound), rstd 0.178 / 0.144 / 0.095 /
0.070 / 0.044 at VB = 1 / 2 / 4 / 8 / 16, dw 0.36 (both dw kernels).  As a check of the module itself, a library with
in-bounds defects -- the mean summed over d - 8 columns, the previous row's rstd, row 64 left out of either dw kernel
-- failed all 80 ``test_rms_fwd`` cases, all 80 ``test_rms_bwd`` cases and the dw assertion of all 32 ``test_rms_dw``
cases with T > 64 (under ``IIT_LLAMA_VEC=0`` too).
"""
import pytest
import torch

import llama_exact_util as X

pytestmark = pytest.mark.gpu

dev = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
DT = {"bf16": BF16, "f32": F32}


@pytest.fixture(scope="module")
def K():
    from iit_amd.ops import hip_kernels
    hip_kernels.lib()
    return hip_kernels


def _out(T: int, d: int, dtype, spare: int = 8):
    """A [T, d] output view at the front of a sentinel-filled flat buffer with ``spare`` elements behind it."""
    buf = X.filled((T * d + spare,), dtype, dev)
    return buf, buf[:T * d].view(T, d)


def _tail_kept(buf: torch.Tensor, n: int) -> bool:
    tail = buf[n:].cpu()
    return not int(X.bad_bits(tail, X.filled(tuple(tail.shape), tail.dtype)).sum())


def _opt(t):
    return None if t is None else t.to(dev)


@pytest.mark.parametrize("family", X.RMS_FAMILIES)
@pytest.mark.parametrize("xt", sorted(DT))
@pytest.mark.parametrize("d", X.RMS_D)
def test_rms_fwd(K, d, xt, family):
    worst = {"y": 0.0, "rstd": 0.0}
    for T in X.RMS_T:
        for affine in (True, False):
            x, w = X.rms_inputs(family, T, d, 7 * d + T, DT[xt], affine)
            ref = X.rms_fwd_ref(x, w, X.RMS_EPS)
            ybuf, y = _out(T, d, BF16)
            rbuf = X.filled((T + 4,), F32, dev)
            K.rms_fwd(x.to(dev), _opt(w), y, rbuf[:T], T, d, X.RMS_EPS)
            torch.cuda.synchronize()
            got = {"y": y.cpu(), "rstd": rbuf[:T].cpu()}
            for k in worst:
                worst[k] = max(worst[k], X.worst(got[k], ref[k], ref["tol_" + k]))
            assert not X.count(X.rms_fwd_check(got, ref)), (T, affine, worst)
            assert _tail_kept(ybuf, T * d) and _tail_kept(rbuf, T), (T, affine)
            if family == "balanced":
                assert not int(X.bad_rms_balanced(got["y"], x).sum()), (T, affine)
    print(f"WORST rms_fwd<{X.rms_vb(d)}> y {worst['y']:.3f} rstd {worst['rstd']:.3f}")


@pytest.mark.parametrize("family", X.RMS_FAMILIES)
@pytest.mark.parametrize("xt", sorted(DT))
@pytest.mark.parametrize("d", X.RMS_D)
def test_rms_bwd(K, d, xt, family):
    """dx alone (``dw`` null); ``rstd`` is the fp32 rounding of the float64 value."""
    worst = 0.0
    for T in X.RMS_T:
        for affine in (True, False):
            x, w = X.rms_inputs(family, T, d, 5 * d + T, DT[xt], affine)
            rstd = X.rms_fwd_ref(x, w, X.RMS_EPS)["rstd"].float()
            b = X.rms_bwd_inputs("random", T, d, d + T, DT[xt])
            for dres in (b["dres"], None):
                ref = X.rms_bwd_ref(b["dy"], x, rstd, w, dres)
                dbuf, dx = _out(T, d, DT[xt])
                K.rms_bwd(b["dy"].to(dev), x.to(dev), rstd.to(dev), _opt(w), dx, None, T, d, dres=_opt(dres))
                torch.cuda.synchronize()
                got = dx.cpu()
                worst = max(worst, X.worst(got, ref["dx"], ref["tol_dx"]))
                bad = X.bad_bound(got, ref["dx"], ref["tol_dx"])
                assert not int(bad.sum()), (T, affine, dres is not None, int(bad.sum()), worst)
                assert _tail_kept(dbuf, T * d)
    print(f"WORST rms_bwd<{X.rms_vb(d)}> dx {worst:.3f}")


@pytest.mark.parametrize("family", X.FAMILIES)
@pytest.mark.parametrize("d", X.RMS_DW_D)
@pytest.mark.parametrize("T", X.RMS_DW_T)
def test_rms_dw(K, T, d, family):
    """The weight gradient (``rms_dw_vec_kernel``; ``rms_dw_kernel`` when the process runs under ``IIT_LLAMA_VEC=0``)
    accumulated into a non-zero prefill inside a buffer 8 columns wider than ``d``."""
    worst = 0.0
    for xt in sorted(DT):
        b = X.rms_bwd_inputs(family, T, d, 3 * T + d, DT[xt])
        if family == "exact":
            x, rstd = X.rms_exact_x(T, d, T + 11 * d, DT[xt])
        else:
            x, _ = X.rms_inputs("random", T, d, T + 11 * d, DT[xt], False)
            rstd = (0.5 + torch.rand(T, generator=X.gen(T))).float()
        w = (1.0 + 0.5 * torch.randn(d, generator=X.gen(d))).float()
        wide0 = torch.cat([b["dw0"], torch.arange(1.0, 9.0)])
        wide = wide0.to(dev)
        ref = X.rms_bwd_ref(b["dy"], x, rstd, w, b["dres"], b["dw0"])
        dbuf, dx = _out(T, d, DT[xt])
        K.rms_bwd(b["dy"].to(dev), x.to(dev), rstd.to(dev), w.to(dev), dx, wide, T, d, dres=b["dres"].to(dev))
        torch.cuda.synchronize()
        got = wide.cpu()
        bad = X.bad_sum(got[:d], ref["dw"], ref["tol_dw"], family)
        worst = max(worst, X.worst(got[:d], ref["dw"], ref["tol_dw"]))
        assert not int(bad.sum()), (xt, int(bad.sum()), worst)
        assert not int(X.bad_bits(got[d:], wide0[d:]).sum()), "columns past d written"
        assert not int(X.bad_bound(dx.cpu(), ref["dx"], ref["tol_dx"]).sum()) and _tail_kept(dbuf, T * d)
    if family == "random":
        print(f"WORST rms_dw {worst:.3f}")


def _refused(K, T, d, xt, misalign: bool):
    """Forward and backward entry points raise and leave the sentinel-filled outputs untouched."""
    pad = 8
    xbuf = torch.ones(T * d + pad, dtype=DT[xt], device=dev)
    x = xbuf[1:1 + T * d].view(T, d) if misalign else xbuf[:T * d].view(T, d)
    assert (x.data_ptr() % 16 != 0) == misalign
    w = torch.ones(d + pad, dtype=F32, device=dev)[:d]
    dy = torch.ones(T, d, dtype=BF16, device=dev)
    rstd = torch.ones(T, dtype=F32, device=dev)
    ybuf, y = _out(T, d, BF16)
    rbuf = X.filled((T,), F32, dev)
    dbuf, dx = _out(T, d, DT[xt])
    dw = torch.full((d + pad,), 3.0, device=dev)
    with pytest.raises(RuntimeError, match="rms_fwd"):
        K.rms_fwd(x, w, y, rbuf, T, d, X.RMS_EPS)
    with pytest.raises(RuntimeError, match="rms_bwd"):
        K.rms_bwd(dy, x, rstd, w, dx, dw, T, d)
    torch.cuda.synchronize()
    assert _tail_kept(ybuf, 0) and _tail_kept(rbuf, 0) and _tail_kept(dbuf, 0)
    assert bool((dw == 3.0).all())


@pytest.mark.parametrize("xt", sorted(DT))
@pytest.mark.parametrize("d,misalign", [(12, False), (516, False), (8200, False), (520, True)],
                         ids=["d12", "d516", "d8200", "offset1"])
def test_rms_refusals(K, d, misalign, xt):
    """The offset view is rejected by the entry point's alignment check before any launch."""
    _refused(K, 3, d, xt, misalign)


@pytest.mark.parametrize("fork", [False, True], ids=["RMSNormFn", "RMSNormForkFn"])
@pytest.mark.parametrize("view", ["noncontiguous", "offset1"])
@pytest.mark.parametrize("xt", sorted(DT))
def test_rms_functions_clone_path(K, xt, view, fork):
    """The autograd Functions on an ``x`` the kernels cannot take as it is (``_c16``): forward, dx (with the fork's
    skip gradient) and dw against the float64 reference, the saved ``rstd`` being the kernel's own."""
    from iit_amd.ops import hip_ops
    B, S, d = 2, 3, 520
    T = B * S
    x0, w0 = X.rms_inputs("random", T, d, 21, DT[xt])
    if view == "noncontiguous":
        xv = torch.zeros(B, S, 2 * d, dtype=DT[xt], device=dev)[..., ::2]
        assert not xv.is_contiguous()
    else:
        xv = torch.zeros(T * d + 8, dtype=DT[xt], device=dev)[1:1 + T * d].view(B, S, d)
        assert xv.is_contiguous() and xv.data_ptr() % 16 != 0
    xv.copy_(x0.view(B, S, d))
    x = xv.detach().requires_grad_()
    w = w0.to(dev).requires_grad_()
    b = X.rms_bwd_inputs("random", T, d, 22, DT[xt])
    if fork:
        y, xp = hip_ops.RMSNormForkFn.apply(x, w, X.RMS_EPS)
        torch.autograd.backward([y, xp], [b["dy"].to(dev).view(B, S, d), b["dres"].to(dev).view(B, S, d)])
    else:
        y = hip_ops.RMSNormFn.apply(x, w, X.RMS_EPS)
        y.backward(b["dy"].to(dev).view(B, S, d))
    torch.cuda.synchronize()
    ref = X.rms_fwd_ref(x0, w0, X.RMS_EPS)
    assert not int(X.bad_bound(y.detach().cpu().view(T, d), ref["y"], ref["tol_y"]).sum())
    # the backward saw the kernel's own fp32 rstd, within rel_r of the reference: its reference takes the rounded
    # reference value and the bound grows by what that difference moves dx and dw (first order in rel_r)
    rstd = ref["rstd"].float()
    bref = X.rms_bwd_ref(b["dy"], x0, rstd, w0, b["dres"] if fork else None, torch.zeros(d))
    rel_r = float((ref["tol_rstd"] / ref["rstd"]).max()) + X.E
    g = b["dy"].double() * w0.double()
    xh = x0.double() * rstd.double().view(T, 1)
    s = (g * xh).mean(1, keepdim=True)
    extra_dx = rel_r * rstd.double().view(T, 1) * (g.abs() + 3 * (xh * s).abs())
    extra_dw = rel_r * (b["dy"].double() * xh).abs().sum(0)
    assert x.grad.dtype == DT[xt] and x.grad.shape == x.shape
    assert not int(X.bad_bound(x.grad.cpu().view(T, d), bref["dx"], bref["tol_dx"] + extra_dx).sum())
    assert not int(X.bad_bound(w.grad.cpu(), bref["dw"], bref["tol_dw"] + extra_dw).sum())
