"""The ``hip32x`` op backend (``HipF32XOps``: ``hip32`` plus attention on csrc/attn_fp32.hip) at model level, by the
recipe of tests/test_hip32_ops.py: the same two-layer model, arena and plain layouts, float64 CPU oracle and criterion
(per tensor ``e = max|t - oracle| / max|oracle|``, ``e_hip32x <= 4 e_torch + 2^-20``).

The kernel runs when neither ``hook_attn_scores`` nor ``hook_pattern`` is live, so the parity run caches every other
activation; with the full cache the backend falls back to the torch op and must reproduce its pattern.  The measured
pairs are recorded in profiles/hip32_parity.txt.
"""
import pytest
import torch

from iit_amd.engine.flat import FlatParams
from iit_amd.ops import select_ops
from iit_amd.ops.torch_ops import TorchOps
from test_hip32_ops import FACTOR, FLOOR, _err, _model
from test_hip32_ops import _run as _run_full

gpu = pytest.mark.gpu
dev = "cuda"


def _no_scores(name: str) -> bool:
    return not name.endswith(("hook_attn_scores", "hook_pattern"))


def _run(model, tokens, backend):
    """``test_hip32_ops._run`` without the score and pattern hooks: logits, the other cached activations and the
    parameter gradients of ``logits.logsumexp(-1).sum()`` as float64 CPU tensors."""
    model.set_op_backend(backend)
    for p in model.parameters():
        if p.grad is not None:
            p.grad.zero_()
    logits, cache = model.run_with_cache(tokens, names_filter=_no_scores)
    logits.logsumexp(-1).sum().backward()
    out = {"logits": logits.detach().double().cpu()}
    out.update({"act " + k: v.detach().double().cpu() for k, v in cache.items()})
    out.update({"grad " + n: p.grad.detach().double().cpu().clone() for n, p in model.named_parameters()})
    return out


@pytest.fixture(scope="module", params=["arena", "plain"])
def parity(request):
    """One model per layout, run on ``hip32x``, on ``torch`` and in float64 on the CPU (computed once, shared)."""
    from iit_amd.ops.hip32_ops import HipF32Ops, HipF32XOps
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
    res["oracle"] = {**_run(oracle, tokens, "torch"), **_run_full(oracle, tokens, "torch", other)}
    res["torch"] = {**_run(model, td, "torch"), **_run_full(model, td, "torch", od)}
    res["oracle full"] = _run_full(oracle, tokens, "torch")
    res["torch full"] = _run_full(model, td, "torch")
    hip32_before = dict(HipF32Ops.calls)
    HipF32XOps.calls.clear()
    res["hip32x"] = _run(model, td, "hip32x")
    res["calls"] = dict(HipF32XOps.calls)
    res["hip32x"].update(_run_full(model, td, "hip32x", od))
    HipF32XOps.calls.clear()
    res["hip32x full"] = _run_full(model, td, "hip32x")
    res["calls full"] = dict(HipF32XOps.calls)
    res["hip32 untouched"] = dict(HipF32Ops.calls) == hip32_before
    model.set_op_backend(None)
    return res


@gpu
def test_model_matches_float64_as_well_as_the_library_path(parity):
    o, t, h = parity["oracle"], parity["torch"], parity["hip32x"]
    assert set(o) == set(t) == set(h) and len(o) > 40 and "spliced logits" in o
    assert not any(k.endswith(("hook_attn_scores", "hook_pattern")) for k in o)
    lines, failed = [], []
    for k in sorted(o):
        eh, et = _err(h[k], o[k]), _err(t[k], o[k])
        lines.append(f"{'arena' if parity['arena'] else 'plain'} {k}: e_hip32x {eh:.3e} e_torch {et:.3e}")
        if not eh <= FACTOR * et + FLOOR:
            failed.append(lines[-1])
    print("\n".join(lines))
    assert not failed, "\n".join(failed)


@gpu
def test_attention_kernel_ran_and_hip32_counters_are_untouched(parity):
    calls = parity["calls"]
    assert calls.get("attention") == 2 and "attention_fallback" not in calls, calls
    want = {"attention": 2, "o_proj": 2, "mlp_in": 2, "mlp_out": 2, "unembed": 1}
    want["qkv" if parity["arena"] else "qkv_fallback"] = 2
    assert calls == want
    assert parity["hip32 untouched"]


@gpu
def test_live_score_hooks_fall_back_to_the_torch_pattern(parity):
    calls = parity["calls full"]
    assert calls.get("attention_fallback") == 2 and "attention" not in calls, calls
    full, ref, o = parity["hip32x full"], parity["torch full"], parity["oracle full"]
    # the projections differ (gemm_f32 against the library), so "equal" is the file's criterion, on every tensor of
    # the full cache, scores and patterns among them
    assert set(full) == set(ref) == set(o)
    for k in sorted(o):
        eh, et = _err(full[k], o[k]), _err(ref[k], o[k])
        assert eh <= FACTOR * et + FLOOR, f"{k}: e_hip32x {eh:.3e} e_torch {et:.3e}"
    k = "act blocks.0.attn.hook_pattern"
    # the fallback is the torch op itself: fed the hip32x run's own q and k it reproduces the cached pattern bitwise
    q, kk = full["act blocks.0.attn.hook_q"].float().to(dev), full["act blocks.0.attn.hook_k"].float().to(dev)
    seen = {}
    TorchOps.attention(None, q, kk, kk, True, parity["model"].blocks[0].attn.attn_scale,
                       hook_pattern=lambda t: seen.setdefault("p", t))
    assert torch.equal(seen["p"].double().cpu(), full[k])


@gpu
def test_two_runs_give_identical_gradients(parity):
    model, tokens = parity["model"], parity["tokens"]
    a = _run(model, tokens, "hip32x")
    b = _run(model, tokens, "hip32x")
    model.set_op_backend(None)
    for k in a:
        assert torch.equal(a[k], b[k]), k
        assert torch.equal(a[k], parity["hip32x"][k]), k


@gpu
def test_other_backends_are_still_selected_as_before(parity):
    from iit_amd.ops.hip32_ops import HipF32Ops, HipF32XOps
    model = parity["model"]
    model.set_op_backend(None)
    ops = select_ops(model, None)
    assert type(ops) is TorchOps and ops.name == "torch"
    assert type(select_ops(model, "hip32")) is HipF32Ops
    x = select_ops(model, "hip32x")
    assert type(x) is HipF32XOps and x.name == "hip32x" and not x.fused
    assert HipF32XOps.calls is not HipF32Ops.calls
