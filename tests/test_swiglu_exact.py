"""Element-wise tests of ``swiglu_fwd_kernel`` / ``swiglu_bwd_kernel`` of csrc/llama_ops.hip on the GPU against the
float64 reference and bounds of tests/llama_exact_util.py (proved on the CPU by tests/test_llama_exact_ref.py).

* ``test_swiglu_sweep``: ``gate`` is EVERY finite bf16 value with |g| <= 2^40, padded to 21 x 2048 elements and
  repeated four times so that each of the kernel's ``SW_U`` = 4 chunk slots sees every value; ``up`` and ``dpost``
  normal; forward and backward.  This covers the ``__expf`` / ``v_rcp_f32`` range, the saturated tails and the zero of
  ``silu'`` at g = -1.278, where ``1 + g (1 - s)`` cancels.
* ``test_swiglu_sizes``: element counts around the per-chunk guards (2048 elements per chunk slot, 8192 per block), in
  a sentinel-filled buffer whose spare elements must keep their bits.
* ``n % 8 != 0`` is refused and nothing is written; ``SwiGLUFn`` takes a non-contiguous ``up``.

Measured on an MI355X: 12 cases, 12 passed, none skipped, 4.0 s for the module (1.0 s of it the first use of
``SwiGLUFn``, the sweep 0.16 s).  Worst ``|got - ref| / bound`` over the sweep: post 0.984, dup 0.990, dgate 0.991.  As
a check of the module itself, a library with ``1 + 1.01 g (1 - s)`` in the backward and s rounded to bf16 in chunk slot
3 of the forward failed the sweep, all eight sizes and the Function case.
"""
import pytest
import torch

import llama_exact_util as X

pytestmark = pytest.mark.gpu

dev = "cuda"
BF16 = torch.bfloat16
_CACHE = {}


@pytest.fixture(scope="module")
def K():
    from iit_amd.ops import hip_kernels
    hip_kernels.lib()
    return hip_kernels


def _sweep():
    """gate, up, dpost of the sweep and their float64 reference, computed once and left unchanged."""
    if "sweep" not in _CACHE:
        g = X.swiglu_sweep()
        gn = X.gen(41)
        u, dv = torch.randn(g.numel(), generator=gn).bfloat16(), torch.randn(g.numel(), generator=gn).bfloat16()
        _CACHE["sweep"] = (g, u, dv, X.swiglu_ref(g, u, dv))
    return _CACHE["sweep"]


def _report(bad: dict, got: dict, ref: dict, g: torch.Tensor) -> str:
    out = []
    g = g.reshape(-1)
    for k, m in bad.items():
        m = m.reshape(-1)
        if int(m.sum()):
            ratio = ((got[k].double() - ref[k]).abs() / ref["tol_" + k]).reshape(-1)
            i = int(torch.nan_to_num(ratio, nan=float("inf")).argmax())
            gs = g[m].float()
            out.append(f"{k}: {int(m.sum())} bad, worst {float(ratio[i]):.3g} x bound at g = {float(g[i])}; "
                       f"bad g from {float(gs.min())} to {float(gs.max())}")
    return "; ".join(out)


def _launch(K, g, u, dv):
    """Forward and backward of flat bf16 operands into sentinel-filled buffers 8 elements longer; returns the results
    on the CPU and whether every spare element kept its bits."""
    n = g.numel()
    bufs = {k: X.filled((n + 8,), BF16, dev) for k in ("post", "dgate", "dup")}
    gd, ud, dd = g.to(dev), u.to(dev), dv.to(dev)
    K.swiglu_fwd(gd, ud, bufs["post"][:n])
    K.swiglu_bwd(dd, gd, ud, bufs["dgate"][:n], bufs["dup"][:n])
    torch.cuda.synchronize()
    kept = all(bool((b[n:].float() == X.BF16_FILL).all()) for b in bufs.values())
    return {k: b[:n].cpu() for k, b in bufs.items()}, kept


def test_swiglu_sweep(K):
    g, u, dv, ref = _sweep()
    assert g.numel() == X.SW_SWEEP_N and g.numel() % 8192 == 0
    got, kept = _launch(K, g, u, dv)
    bad = X.swiglu_check(got, ref)
    print("WORST swiglu " + " ".join(f"{k} {X.worst(got[k], ref[k], ref['tol_' + k]):.3f}" for k in got))
    assert not X.count(bad), _report(bad, got, ref, g)
    assert kept
    # each of the four chunk slots saw every value: slot = (element / 2048) % 4
    slot = (torch.arange(g.numel()) // 2048) % 4
    every = X.all_bf16().view(torch.int16).long()
    for k in range(4):
        seen = torch.zeros(65536, dtype=torch.bool)
        seen[g[slot == k].view(torch.int16).long() + 32768] = True
        assert bool(seen[every + 32768].all()), k


@pytest.mark.parametrize("n", X.SW_SIZES)
def test_swiglu_sizes(K, n):
    gn = X.gen(n)
    g = (3.0 * torch.randn(n, generator=gn)).bfloat16()
    u, dv = torch.randn(n, generator=gn).bfloat16(), torch.randn(n, generator=gn).bfloat16()
    ref = X.swiglu_ref(g, u, dv)
    got, kept = _launch(K, g, u, dv)
    bad = X.swiglu_check(got, ref)
    assert not X.count(bad), _report(bad, got, ref, g)
    assert kept, "written past n"


@pytest.mark.parametrize("n", [7, 2052])
def test_swiglu_refuses_n_not_multiple_of_8(K, n):
    ops = [torch.ones(n + 4, dtype=BF16, device=dev)[:n] for _ in range(3)]
    outs = [X.filled((n + 4,), BF16, dev) for _ in range(3)]
    with pytest.raises(RuntimeError, match="swiglu_fwd"):
        K.swiglu_fwd(ops[0], ops[1], outs[0][:n])
    with pytest.raises(RuntimeError, match="swiglu_bwd"):
        K.swiglu_bwd(ops[2], ops[0], ops[1], outs[1][:n], outs[2][:n])
    torch.cuda.synchronize()
    assert all(bool((o.float() == X.BF16_FILL).all()) for o in outs)


def test_swiglu_function_noncontiguous_up(K):
    from iit_amd.ops import hip_ops
    shape = (3, 5, 264)
    gn = X.gen(9)
    g = (3.0 * torch.randn(shape, generator=gn)).bfloat16()
    u, dv = torch.randn(shape, generator=gn).bfloat16(), torch.randn(shape, generator=gn).bfloat16()
    wide = torch.zeros(3, 5, 2 * 264, dtype=BF16, device=dev)
    uv = wide[..., ::2]
    uv.copy_(u)
    assert not uv.is_contiguous()
    gd, ud = g.to(dev).requires_grad_(), uv.detach().requires_grad_()
    post = hip_ops.SwiGLUFn.apply(gd, ud)
    post.backward(dv.to(dev))
    torch.cuda.synchronize()
    ref = X.swiglu_ref(g, u, dv)
    got = {"post": post.detach().cpu(), "dgate": gd.grad.cpu(), "dup": ud.grad.cpu()}
    bad = X.swiglu_check(got, ref)
    assert not X.count(bad), _report(bad, got, ref, g)
