"""The ``hip32n`` op backend (``HipF32NOps``: ``hip32x`` plus LayerNorm on csrc/block_f32.hip, the GELU epilogues of
csrc/gemm_f32.hip and the residual epilogues) at model level, by the recipe of tests/test_hip32x_ops.py: the same
two-layer model, arena and plain layouts, float64 CPU oracle and criterion (per tensor
``e = max|t - oracle| / max|oracle|``, ``e_hip32n <= 4 e_torch + 2^-20``).

A kernel runs when no hook inside its op is live, so the model is run four ways: caching only ``hook_resid_post``
(every kernel), with ``mlp.hook_post`` cached (``MlpInF32Fn`` and the residual projection instead of the fused MLP),
with the LayerNorm hooks cached (the torch LayerNorm), and the spliced-logits run.  Every tensor of every run meets the
criterion.  The measured pairs are recorded in profiles/hip32_parity.txt.
"""
import pytest
import torch

import gemm_exact_util as U
import gemm_f32_util as F
from iit_amd.engine.flat import FlatParams
from iit_amd.ops import select_ops
from iit_amd.ops.torch_ops import TorchOps
from test_hip32_ops import FACTOR, FLOOR, _err, _model
from test_hip32_ops import _run as _run_full

gpu = pytest.mark.gpu
dev = "cuda"
FILTERS = {
    "resid": lambda n: n.endswith("hook_resid_post"),
    "mlp": lambda n: n.endswith(("hook_resid_post", "mlp.hook_post")),
    "ln": lambda n: n.endswith(("hook_resid_post", "hook_scale", "hook_normalized")),
}


def _run(model, tokens, backend, which):
    """``test_hip32_ops._run`` with the cache restricted by ``FILTERS[which]``: logits, the cached activations and the
    parameter gradients of ``logits.logsumexp(-1).sum()`` as float64 CPU tensors."""
    model.set_op_backend(backend)
    for p in model.parameters():
        if p.grad is not None:
            p.grad.zero_()
    logits, cache = model.run_with_cache(tokens, names_filter=FILTERS[which])
    logits.logsumexp(-1).sum().backward()
    out = {f"{which} logits": logits.detach().double().cpu()}
    out.update({f"{which} act {k}": v.detach().double().cpu() for k, v in cache.items()})
    out.update({f"{which} grad {n}": p.grad.detach().double().cpu().clone() for n, p in model.named_parameters()})
    return out


def _all(model, tokens, other, backend, calls=None):
    res = {}
    for which in FILTERS:
        if calls is not None:
            calls[0].clear()
        res.update(_run(model, tokens, backend, which))
        if calls is not None:
            calls[1][which] = dict(calls[0])
    res.update(_run_full(model, tokens, backend, other))
    return res


@pytest.fixture(scope="module", params=["arena", "plain"])
def parity(request):
    """One model per layout, run on ``hip32n``, on ``torch`` and in float64 on the CPU (computed once, shared)."""
    from iit_amd.ops.hip32_ops import HipF32NOps, HipF32Ops, HipF32XOps
    arena = request.param == "arena"
    model = _model(dev)
    if arena:
        FlatParams(model)
    oracle = _model("cpu", torch.float64)
    oracle.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    g = torch.Generator().manual_seed(3)
    tokens = torch.randint(0, 97, (3, 8), generator=g)
    other = torch.randint(0, 97, (3, 8), generator=g)
    td, od = tokens.to(dev), other.to(dev)
    res = {"arena": arena, "model": model, "tokens": td}
    res["oracle"] = _all(oracle, tokens, other, "torch")
    res["torch"] = _all(model, td, od, "torch")
    before = dict(HipF32Ops.calls), dict(HipF32XOps.calls)
    res["calls"] = {}
    res["hip32n"] = _all(model, td, od, "hip32n", (HipF32NOps.calls, res["calls"]))
    res["others untouched"] = (dict(HipF32Ops.calls), dict(HipF32XOps.calls)) == before
    model.set_op_backend(None)
    return res


@gpu
def test_model_matches_float64_as_well_as_the_library_path(parity):
    o, t, h = parity["oracle"], parity["torch"], parity["hip32n"]
    assert set(o) == set(t) == set(h) and len(o) > 100 and "spliced logits" in o
    assert any(k.startswith("ln act") and k.endswith("hook_scale") for k in o)
    lines, failed = [], []
    for k in sorted(o):
        eh, et = _err(h[k], o[k]), _err(t[k], o[k])
        lines.append(f"{'arena' if parity['arena'] else 'plain'} {k}: e_hip32n {eh:.3e} e_torch {et:.3e}")
        if not eh <= FACTOR * et + FLOOR:
            failed.append(lines[-1])
    print("\n".join(lines))
    assert not failed, "\n".join(failed)


@gpu
def test_every_kernel_ran_with_only_resid_post_cached(parity):
    want = {"layer_norm": 5, "mlp_fused": 2, "attention": 2, "o_proj": 2, "unembed": 1}
    want["qkv" if parity["arena"] else "qkv_fallback"] = 2
    assert parity["calls"]["resid"] == want
    assert parity["others untouched"]


@gpu
def test_a_cached_mlp_post_takes_the_unfused_mlp_kernels(parity):
    calls = parity["calls"]["mlp"]
    assert calls.get("mlp_in") == 2 and calls.get("mlp_out") == 2 and "mlp_fused" not in calls, calls
    assert calls.get("layer_norm") == 5 and not [k for k in calls if k.endswith("_fallback") and k != "qkv_fallback"]


@gpu
def test_live_layer_norm_hooks_fall_back_to_the_torch_layer_norm(parity):
    calls = parity["calls"]["ln"]
    assert calls.get("layer_norm_fallback") == 5 and "layer_norm" not in calls, calls
    assert calls.get("mlp_fused") is None and calls.get("mlp_in") == 2  # ln2's hooks are inside the fused op


@gpu
def test_two_runs_give_identical_tensors(parity):
    model, tokens = parity["model"], parity["tokens"]
    for which in FILTERS:
        a = _run(model, tokens, "hip32n", which)
        b = _run(model, tokens, "hip32n", which)
        for k in a:
            assert torch.equal(a[k], b[k]), k
            assert torch.equal(a[k], parity["hip32n"][k]), k
    model.set_op_backend(None)


@gpu
def test_other_backends_are_still_selected_as_before(parity):
    from iit_amd.ops.hip32_ops import HipF32NOps, HipF32Ops, HipF32XOps
    model = parity["model"]
    model.set_op_backend(None)
    ops = select_ops(model, None)
    assert type(ops) is TorchOps and ops.name == "torch"
    assert type(select_ops(model, "hip32")) is HipF32Ops and type(select_ops(model, "hip32x")) is HipF32XOps
    n = select_ops(model, "hip32n")
    assert type(n) is HipF32NOps and n.name == "hip32n" and not n.fused
    assert n.native_layer_norm and n.fuses_residual and n.native_attention
    assert HipF32NOps.calls is not HipF32XOps.calls and HipF32NOps.calls is not HipF32Ops.calls


# ------------------------------------------------------------------------------ the autograd functions under a graph
def _ln_case():
    from iit_amd.ops.hip32_ops import LayerNormF32Fn
    import block_f32_util as B
    x, w, b, dy, _ = B.selector_case(37, 64, 5)
    return (lambda x, w, b: LayerNormF32Fn.apply(x, w, b, 0.0)), [t.to(dev) for t in (x, w, b)], dy.to(dev)


def _mlp_operands():
    T, d, dm = 24, 64, 72
    x, W_in = F.operands(F.F1, T, dm, d, seed=21, device=dev)
    _, W_out = F.operands(F.F1, T, d, dm, seed=22, device=dev)
    b_in = U.ints((dm,), -U.BIAS_MAX, U.BIAS_MAX, 23, dev)
    b_out = U.ints((d,), -U.BIAS_MAX, U.BIAS_MAX, 24, dev)
    resid = U.ints((T, d), -U.ADD_MAX, U.ADD_MAX, 25, dev)
    return [x * 0.125, W_in, b_in * 0.25, W_out, b_out, resid]


def _mlp_in_case():
    from iit_amd.ops.hip32_ops import MlpInF32Fn
    return MlpInF32Fn.apply, _mlp_operands()[:3], U.ints((24, 72), -3, 3, 26, dev)


def _mlp_fused_case():
    from iit_amd.ops.hip32_ops import MlpGeluResidualF32Fn
    return MlpGeluResidualF32Fn.apply, _mlp_operands(), U.ints((24, 64), -3, 3, 27, dev)


@gpu
@pytest.mark.parametrize("case", [_ln_case, _mlp_in_case, _mlp_fused_case])
def test_autograd_functions_graph_replay_equals_eager(case):
    fn, operands, dy = case()
    first = [t.clone().requires_grad_() for t in operands]  # the eager run has leaves of its own
    y = fn(*first)
    eager = [y.detach().clone()] + [g.clone() for g in torch.autograd.grad(y, first, dy)]
    assert all(t.isfinite().all() and t.abs().sum() > 0 for t in eager)
    # fresh leaves, first used on the side stream: a leaf first used on the default stream would make autograd order
    # that stream after the capturing one
    leaves = [t.clone().requires_grad_() for t in operands]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside capture
        torch.autograd.grad(fn(*leaves), leaves, dy)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = fn(*leaves)
        grads = torch.autograd.grad(y, leaves, dy)
    for _ in range(2):
        for t in (y,) + tuple(grads):
            if t.data_ptr() != dy.data_ptr():  # dresid is dY itself, the graph's input
                t.detach().fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for i, (got, ref) in enumerate(zip((y,) + tuple(grads), eager)):
            assert not U.bad_bits(got.detach().contiguous(), ref.contiguous()).any(), i
