"""The fp32 attention kernels of csrc/attn_fp32.hip and ``AttentionF32Fn`` on the GPU, element by element against the
float64 reference and bounds of tests/attn_f32_util.py.

* normal family: every output element of the twelve ``CASES`` inside its bound, and the largest error at most a
  quarter of its bound (the factor tests/test_attn_f32_ref.py holds fp32 implementations to);
* selector family: integer operands whose softmax is one-hot exactly in fp32; all five outputs equal the closed
  forms (``lse`` is the top score bit for bit, so the row max is not carried in the log2 domain);
* layouts: packed q | k | v views, a base offset by one float, a q with permuted strides, all bitwise equal to the
  contiguous run, with NaN around every operand and output;
* determinism: two runs and two replays of a captured graph give identical bits;
* refusals (before any launch) and partial gradients.

Sensitivity.  The library was built three times with one deliberate defect in csrc/attn_fp32.hip each (the builds are
not kept) and this module run against it:

* P rounded once to bf16 before the z product: ``test_normal_family_within_a_quarter_of_the_bounds`` fails on z in
  the eleven cases with S > 1 (the first assertion, ``A.bad``; z at 21 to 1438 times its bound, every other output
  unchanged; at S = 1 the only weight is 1.0, which bf16 holds);
* the causal mask admitting key i + 1: the same test fails in the five causal cases with S > 1 on all five outputs
  (3e4 to 6e7 times a bound), and ``test_partial_gradients`` fails on its bound for dq and for dv.  The selector test
  does not see it: the extra key trails the selected one by 128 nats or more and still gets weight 0;
* dq without the scale: the same test fails on dq alone in the eleven cases with S > 1 (1e4 to 8e4 times its bound;
  at S = 1 dq is 0), and ``test_partial_gradients[q]`` fails.

The kernels themselves measured at most 0.11 of a bound (lse at S = 3; at most 0.06 on the other outputs).
"""
import functools
import types

import pytest
import torch

import attn_f32_util as A

gpu = pytest.mark.gpu
dev = "cuda"
NAMES = ("q", "k", "v", "do")


def _kernels():
    from iit_amd.ops import hip_kernels as K
    return K


def _guarded(shape, offset=0, pad=32):
    """An uninitialised-looking (NaN) fp32 view of ``shape`` inside a larger NaN buffer, ``offset`` floats off a
    16-byte aligned address; returns (view, buffer, slice of the view in the buffer)."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * pad + offset,), float("nan"), dtype=torch.float32, device=dev)
    sl = slice(pad + offset, pad + offset + n)
    return buf[sl].view(shape), buf, sl


def _untouched(buf, sl) -> bool:
    return bool(buf[:sl.start].isnan().all()) and bool(buf[sl.stop:].isnan().all())


def _run(ops: dict, causal: bool, scale: float, outs=None) -> dict:
    """Forward + backward through the wrappers; ``ops``: q, k, v, do on the GPU in any layout; ``outs``: optional
    (view, buffer, slice) per output name, else guarded contiguous ones.  Asserts nothing was written around an
    output and returns the five outputs on the CPU."""
    K = _kernels()
    B, S, H, dh = ops["q"].shape
    outs = outs or {}
    got = {n: outs.get(n) or _guarded((B, S, H, dh)) for n in ("z", "dq", "dk", "dv")}
    got["lse"] = _guarded((B, H, S))
    K.attn_f32_fwd(ops["q"], ops["k"], ops["v"], got["z"][0], got["lse"][0], scale, causal)
    K.attn_f32_bwd(ops["q"], ops["k"], ops["v"], ops["do"], got["lse"][0], got["dq"][0], got["dk"][0], got["dv"][0],
                   scale, causal)
    torch.cuda.synchronize()
    for n, (_, buf, sl) in got.items():
        assert _untouched(buf, sl), f"{n}: a store outside the tensor"
    return {n: t[0].detach().cpu().contiguous() for n, t in got.items()}


def _gpu(case: dict) -> dict:
    return {n: case[n].to(dev) for n in NAMES}


@functools.lru_cache(maxsize=None)
def _normal(c):
    """(operands, scale, float64 reference, the kernels' outputs run contiguous) of one of ``A.CASES``, once."""
    B, S, H, dh, causal = c
    case = A.normal_case(B, S, H, dh, seed=100 + S + dh)
    scale = dh ** -0.5
    ref = A.reference(case["q"], case["k"], case["v"], case["do"], causal, scale)
    return case, scale, ref, _run(_gpu(case), causal, scale)


# ------------------------------------------------------------------------------ normal family
@gpu
@pytest.mark.parametrize("c", A.CASES, ids=A.case_id)
def test_normal_family_within_a_quarter_of_the_bounds(c):
    _, _, ref, got = _normal(c)
    r = A.ratios(got, ref)
    print(A.case_id(c), {n: round(x, 4) for n, x in r.items()})
    bad = A.bad(got, ref)
    assert not any(bad.values()), bad
    assert max(r.values()) <= 0.25, r


# ------------------------------------------------------------------------------ selector family
@gpu
@pytest.mark.parametrize("S,dh,causal", [(16, 16, True), (33, 64, False), (33, 4, True), (64, 64, True)])
def test_selector_family_is_exact(S, dh, causal):
    scale = dh ** -0.5
    sc = A.selector_case(2, S, 3, dh, causal, scale, seed=7)
    got = _run(_gpu(sc), causal, scale)
    for n in A.OUTPUTS:
        assert torch.equal(got[n], sc["want"][n]), n  # zero signs are not compared


# ------------------------------------------------------------------------------ layouts
def _packed(case: dict):
    """q, k, v as views of one NaN-guarded packed ``[B][S][3 H dh]`` buffer, and dq, dk, dv as views of another."""
    B, S, H, dh = case["q"].shape
    ops, outs = {}, {}
    src, _, _ = _guarded((B, S, 3, H, dh))
    dst = _guarded((B, S, 3, H, dh))
    for i, n in enumerate(("q", "k", "v")):
        src[:, :, i].copy_(case[n])
        ops[n] = src[:, :, i]
        # the three gradients share one buffer: each one's surroundings are the other two and the NaN guard
        outs["d" + n] = (dst[0][:, :, i], dst[1], dst[2])
    ops["do"] = case["do"].to(dev)
    return ops, outs


def _offset(case: dict):
    """Every operand and output one float off a 16-byte aligned base."""
    shape = case["q"].shape
    ops = {}
    for n in NAMES:
        ops[n] = _guarded(shape, offset=1)[0]
        ops[n].copy_(case[n])
        assert ops[n].data_ptr() % 16 == 4
    return ops, {n: _guarded(shape, offset=1) for n in ("z", "dq", "dk", "dv")}


def _permuted(case: dict):
    """q stored ``[S][B][H][dh]`` (batch and position strides swapped)."""
    B, S, H, dh = case["q"].shape
    ops = _gpu(case)
    store = _guarded((S, B, H, dh))[0]
    store.copy_(case["q"].permute(1, 0, 2, 3))
    ops["q"] = store.permute(1, 0, 2, 3)
    assert ops["q"].stride() == (H * dh, B * H * dh, dh, 1)
    return ops, {}


@gpu
@pytest.mark.parametrize("layout,c", [(_packed, (2, 15, 4, 20, True)), (_packed, (3, 16, 3, 16, True)),
                                      (_offset, (2, 15, 4, 20, True)), (_offset, (3, 17, 3, 4, False)),
                                      (_permuted, (2, 15, 4, 20, True)), (_permuted, (3, 17, 3, 4, False))],
                         ids=lambda p: p.__name__.strip("_") if callable(p) else A.case_id(p))
def test_layouts_equal_the_contiguous_run_bitwise(layout, c):
    case, scale, _, want = _normal(c)
    ops, outs = layout(case)
    got = _run(ops, c[4], scale, outs)
    for n in A.OUTPUTS:
        assert A.same_bits(got[n], want[n]), n


# ------------------------------------------------------------------------------ determinism
def _fn_step(leaves, do, causal, scale):
    from iit_amd.ops.hip32_ops import AttentionF32Fn
    z = AttentionF32Fn.apply(*leaves, causal, scale)
    return (z,) + tuple(torch.autograd.grad(z, leaves, do))


@gpu
def test_two_runs_and_the_function_give_identical_bits():
    c = (2, 33, 4, 16, False)
    case, scale, _, want = _normal(c)
    again = _run(_gpu(case), c[4], scale)
    for n in A.OUTPUTS:
        assert A.same_bits(again[n], want[n]), n
    ops = _gpu(case)
    leaves = [ops[n].clone().requires_grad_() for n in ("q", "k", "v")]
    for n, t in zip(("z", "dq", "dk", "dv"), _fn_step(leaves, ops["do"], c[4], scale)):
        assert A.same_bits(t.detach(), want[n]), n


@gpu
def test_graph_replay_equals_eager():
    c = (2, 17, 4, 64, True)
    case, scale, _, want = _normal(c)
    ops = _gpu(case)
    leaves = [ops[n].clone().requires_grad_() for n in ("q", "k", "v")]  # fresh leaves, first used on the side stream
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside capture
        _fn_step(leaves, ops["do"], c[4], scale)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = _fn_step(leaves, ops["do"], c[4], scale)
    for _ in range(2):
        for t in outs:
            t.detach().fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for n, t in zip(("z", "dq", "dk", "dv"), outs):
            assert A.same_bits(t.detach(), want[n]), n


# ------------------------------------------------------------------------------ refusals, partial gradients
@gpu
def test_refusals_raise_before_any_launch():
    K = _kernels()
    good = torch.zeros(2, 8, 2, 16, device=dev)
    assert K.attn_f32_ok(good, good, good)
    wide = torch.zeros(2, 8, 2, 32, device=dev)[..., ::2]  # inner stride 2
    refused = {"S65": torch.zeros(1, 65, 2, 16, device=dev), "dh65": torch.zeros(1, 8, 2, 65, device=dev),
               "bf16": good.bfloat16(), "inner stride": wide}
    for name, q in refused.items():
        other = q if name in ("S65", "dh65") else good  # k, v of q's shape; only q is at fault in the last two
        assert not K.attn_f32_ok(q, other, other), name
        shape = tuple(q.shape)
        z = torch.full(shape, float("nan"), device=dev)
        lse = torch.full((shape[0], shape[2], shape[1]), float("nan"), device=dev)
        grads = [torch.full(shape, float("nan"), device=dev) for _ in range(3)]
        with pytest.raises(ValueError):
            K.attn_f32_fwd(q, other, other, z, lse, 0.25, True)
        with pytest.raises(ValueError):
            K.attn_f32_bwd(q, other, other, other, lse, *grads, 0.25, True)
        torch.cuda.synchronize()
        assert all(bool(t.isnan().all()) for t in [z, lse] + grads), name  # nothing ran


@gpu
@pytest.mark.parametrize("only", ["q", "v"])
def test_partial_gradients(only):
    from iit_amd.ops.hip32_ops import AttentionF32Fn
    c = (3, 16, 3, 16, True)
    case, scale, ref, want = _normal(c)
    ops = _gpu(case)
    leaves = {n: ops[n].clone().requires_grad_(n == only) for n in ("q", "k", "v")}
    z = AttentionF32Fn.apply(leaves["q"], leaves["k"], leaves["v"], c[4], scale)
    z.backward(ops["do"])
    for n, t in leaves.items():
        assert (t.grad is None) == (n != only), n

    # the Function's backward itself hands autograd None for the inputs that need no gradient
    need = tuple(n == only for n in ("q", "k", "v")) + (False, False)
    ctx = types.SimpleNamespace(saved_tensors=(ops["q"], ops["k"], ops["v"], want["lse"].to(dev)), causal=c[4],
                                scale=scale, needs_input_grad=need)
    back = AttentionF32Fn.backward(ctx, ops["do"])
    assert [g is not None for g in back] == list(need)
    name = "d" + only
    assert A.same_bits(back[("q", "k", "v").index(only)], leaves[only].grad)
    err = (leaves[only].grad.double().cpu() - ref[name]).abs()
    assert bool((err <= ref["tol_" + name]).all()), name
