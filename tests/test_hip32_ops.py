"""The ``hip32`` op backend (iit_amd/ops/hip32_ops.py): ``LinearF32Fn`` bitwise against float64 autograd on exact
operands, eager and replayed from a captured graph, and a two-layer ``HookedTransformer`` -- with and without its
parameters in a ``FlatParams`` arena -- against the same weights computed in float64 on the CPU.

Model criterion, per tensor (logits, every cached hook activation, every parameter gradient of
``logits.logsumexp(-1).sum()``): ``e = max|t - oracle| / max|oracle|`` and ``e_hip32 <= 4 e_torch + 2^-20``, where
``torch`` is the library-GEMM fp32 backend on the same GPU.  Both are fp32 chains with the same worst-case bound and
differ only in summation order; bf16 contamination would sit near 2^-9.  The floor is 16 fp32 ulps, for tensors the
library happens to get exact.  The measured pairs are recorded in profiles/hip32_parity.txt.
"""
import pytest
import torch

import gemm_exact_util as U
import gemm_f32_util as F
from iit_amd.engine.flat import FlatParams
from iit_amd.models.transformer import HookedTransformer
from iit_amd.ops import select_ops
from iit_amd.ops.torch_ops import TorchOps

gpu = pytest.mark.gpu
dev = "cuda"
CFG = dict(n_layers=2, d_model=64, n_heads=4, d_head=16, d_mlp=256, d_vocab=97, n_ctx=16, act_fn="gelu_new",
           normalization_type="LN")
FLOOR, FACTOR = 2.0 ** -20, 4.0


def _model(device, dtype=torch.float32):
    torch.manual_seed(0)
    m = HookedTransformer(dict(CFG, device=device, dtype=dtype))
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():  # every parameter nonzero, biases included, LayerNorm weights around 1
        for name, p in m.named_parameters():
            v = torch.randn(p.shape, generator=g) * 0.1
            if name.endswith(".w"):
                v = v + 1.0
            p.copy_(v.to(p.dtype))
    return m


# ------------------------------------------------------------------------------ LinearF32Fn
def _linear_case(resid: bool):
    T, Kd, N = 24, 64, 72
    x, W = F.operands(F.F2, T, N, Kd, seed=11, device=dev)
    b = U.ints((N,), -U.BIAS_MAX, U.BIAS_MAX, 12, dev)
    r = U.ints((T, N), -U.ADD_MAX, U.ADD_MAX, 13, dev) if resid else None
    dy = U.ints((T, N), -3, 3, 14, dev)  # |dX| <= 3 * 3 * 72, |dW| <= 4095 * 3 * 24, |db| <= 3 * 24: all exact
    return x, W, b, r, dy


def _linear_ref(x, W, b, r, dy):
    xs = [t.double().requires_grad_() for t in (x, W, b)]
    y = xs[0] @ xs[1] + xs[2]
    if r is not None:
        y = y + r.double()
    y.backward(dy.double())
    return [y.detach().float()] + [t.grad.float() for t in xs]


def _linear_run(x, W, b, r, dy):
    from iit_amd.ops.hip32_ops import LinearF32Fn
    leaves = [t.clone().requires_grad_() for t in (x, W, b)]
    rr = None if r is None else r.clone().requires_grad_()
    y = LinearF32Fn.apply(*leaves, rr)
    y.backward(dy)
    out = [y.detach()] + [t.grad for t in leaves]
    if rr is not None:
        assert torch.equal(rr.grad, dy)
    return out


@gpu
@pytest.mark.parametrize("resid", [False, True])
def test_linear_f32_bitwise_against_float64_autograd(resid):
    case = _linear_case(resid)
    for name, got, ref in zip(("y", "dX", "dW", "db"), _linear_run(*case), _linear_ref(*case)):
        bad = U.bad_f32(got.contiguous(), ref)
        assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.numel()} elements differ"


@gpu
def test_linear_f32_graph_replay_equals_eager():
    from iit_amd.ops.hip32_ops import LinearF32Fn
    x, W, b, r, dy = _linear_case(True)
    eager = _linear_run(x, W, b, r, dy)
    leaves = [t.clone().requires_grad_() for t in (x, W, b)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside capture
        torch.autograd.grad(LinearF32Fn.apply(*leaves, r), leaves, dy)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = LinearF32Fn.apply(*leaves, r)
        grads = torch.autograd.grad(y, leaves, dy)
    for _ in range(2):
        for t in (y,) + tuple(grads):
            t.detach().fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for name, got, ref in zip(("y", "dX", "dW", "db"), (y,) + tuple(grads), eager):
            assert not U.bad_bits(got.contiguous(), ref.contiguous()).any(), name


# ------------------------------------------------------------------------------ model level
def _run(model, tokens, backend, splice=None):
    """logits, cached activations and parameter gradients of ``logits.logsumexp(-1).sum()`` as float64 CPU tensors;
    ``splice``: tokens of a second prompt whose ``blocks.0.attn.hook_z`` replaces the first one's (forward only)."""
    model.set_op_backend(backend)
    if splice is not None:
        with torch.no_grad():
            _, c2 = model.run_with_cache(splice, names_filter="blocks.0.attn.hook_z")
            src = c2["blocks.0.attn.hook_z"]
            logits = model.run_with_hooks(tokens, fwd_hooks=[("blocks.0.attn.hook_z", lambda t, hook: src)])
        return {"spliced logits": logits.double().cpu()}
    for p in model.parameters():
        if p.grad is not None:
            p.grad.zero_()
    logits, cache = model.run_with_cache(tokens)
    logits.logsumexp(-1).sum().backward()
    out = {"logits": logits.detach().double().cpu()}
    out.update({"act " + k: v.detach().double().cpu() for k, v in cache.items()})
    out.update({"grad " + n: p.grad.detach().double().cpu().clone() for n, p in model.named_parameters()})
    return out


def _err(t, oracle):
    """``max|t - oracle| / max|oracle|`` over the oracle's finite entries; the others (the -inf of causally masked
    attention scores) must be the same values in the same places."""
    fin = oracle.isfinite()
    assert torch.equal(t[~fin], oracle[~fin])
    return ((t[fin] - oracle[fin]).abs().max() / oracle[fin].abs().max()).item()


@pytest.fixture(scope="module", params=["arena", "plain"])
def parity(request):
    """One model per layout, run on ``hip32``, on ``torch`` and in float64 on the CPU (computed once, shared)."""
    from iit_amd.ops.hip32_ops import HipF32Ops
    arena = request.param == "arena"
    model = _model(dev)
    if arena:
        FlatParams(model)
        assert model.unembed.W_U.stride() == (104, 1)
        assert model.blocks[0].attn.W_Q.stride() == (16, 192, 1)
    oracle = _model("cpu", torch.float64)
    oracle.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    oracle.set_op_backend("torch")
    g = torch.Generator().manual_seed(3)
    tokens = torch.randint(0, 97, (3, 8), generator=g)
    other = torch.randint(0, 97, (3, 8), generator=g)
    res = {"arena": arena, "model": model, "tokens": tokens.to(dev)}
    res["oracle"] = {**_run(oracle, tokens, "torch"), **_run(oracle, tokens, "torch", other)}
    res["torch"] = {**_run(model, tokens.to(dev), "torch"), **_run(model, tokens.to(dev), "torch", other.to(dev))}
    HipF32Ops.calls.clear()
    res["hip32"] = _run(model, tokens.to(dev), "hip32")
    res["calls"] = dict(HipF32Ops.calls)
    res["hip32"].update(_run(model, tokens.to(dev), "hip32", other.to(dev)))
    model.set_op_backend(None)
    return res


@gpu
def test_model_matches_float64_as_well_as_the_library_path(parity):
    o, t, h = parity["oracle"], parity["torch"], parity["hip32"]
    assert set(o) == set(t) == set(h) and len(o) > 40
    lines, failed = [], []
    for k in sorted(o):
        eh, et = _err(h[k], o[k]), _err(t[k], o[k])
        lines.append(f"{'arena' if parity['arena'] else 'plain'} {k}: e_hip32 {eh:.3e} e_torch {et:.3e}")
        if not eh <= FACTOR * et + FLOOR:
            failed.append(lines[-1])
    print("\n".join(lines))
    assert not failed, "\n".join(failed)


@gpu
def test_kernel_ran_instead_of_a_fallback(parity):
    want = {"o_proj": 2, "mlp_in": 2, "mlp_out": 2, "unembed": 1}
    want["qkv" if parity["arena"] else "qkv_fallback"] = 2
    assert parity["calls"] == want


@gpu
def test_two_runs_give_identical_gradients(parity):
    model, tokens = parity["model"], parity["tokens"]
    a = _run(model, tokens, "hip32")
    b = _run(model, tokens, "hip32")
    model.set_op_backend(None)
    for k in a:
        assert torch.equal(a[k], b[k]), k
        assert torch.equal(a[k], parity["hip32"][k]), k


@gpu
def test_backend_none_is_still_torch(parity):
    model = parity["model"]
    model.set_op_backend(None)
    ops = select_ops(model, None)
    assert type(ops) is TorchOps and ops.name == "torch"
    assert select_ops(model, "hip32").name == "hip32"


def test_hip32_on_a_cpu_model_raises():
    with pytest.raises(RuntimeError):
        select_ops(_model("cpu"), "hip32")
