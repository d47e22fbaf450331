"""The ``hip32p`` op backend (``HipF32POps``: ``hip32n`` plus the paired source + base forward) on the two-layer model of
tests/test_hip32_ops.py with its parameters in a ``FlatParams`` arena.

Reference: the same model on ``hip32n`` through ``run_capture`` + ``RunPlan.with_splices``, which is what
``ll_source_cache`` / ``ll_intervened_forward`` run.  Criterion: the output, every captured source activation and
every parameter gradient of ``logits.logsumexp(-1).sum()`` are bitwise equal.  That is derived, not measured: the base
rows see the same values through the same kernels -- every forward GEMM of this model takes the 64 x 64 tile and the
same number of K splits at T and at 2T rows (asserted; the split sum has a fixed order), the attention and LayerNorm
kernels compute a row from that row alone -- and the backwards are the unpaired ones on identical saved tensors.  A
tensor that differs means the paired path composed other kernels than the two forwards for that site.

Precondition, asserted first: the two-forward reference repeats itself bit for bit on the same input.  A tensor that
does not (only torch's own embedding backward could) is compared by the parity criterion of tests/test_hip32_ops.py
against the float64 oracle instead: ``e_hip32p <= FACTOR e_torch + FLOOR``, ``torch`` the library-GEMM fp32 backend.
"""
import pytest
import torch

from iit_amd.core.index import Ix
from iit_amd.engine.flat import FlatParams
from iit_amd.engine.plan import RunPlan
from test_hip32_ops import CFG, FACTOR, FLOOR, _err, _model

gpu = pytest.mark.gpu
dev = "cuda"
B, S = 3, 8

SITES = {
    "whole z": {"blocks.0.attn.hook_z": [Ix[[None]]]},
    "one head": {"blocks.0.attn.hook_z": [Ix[:, :, 2]]},
    "positions": {"blocks.0.attn.hook_z": [Ix[:, [3, 7]]]},
    "features": {"blocks.0.attn.hook_z": [Ix[:, :, :, 1:7]]},
    "neurons": {"blocks.0.mlp.hook_post": [Ix[:, :, 5:70]]},
    "batch subset": {"blocks.0.mlp.hook_post": [Ix[1:3]]},
    "two layers": {"blocks.0.attn.hook_z": [Ix[[None]]], "blocks.1.attn.hook_z": [Ix[:, :, 1]]},
    "mlp then head": {"blocks.0.mlp.hook_post": [Ix[:, 2:5]], "blocks.1.attn.hook_z": [Ix[:, :, [0, 3]]]},
    "final block head": {"blocks.1.attn.hook_z": [Ix[:, :, 1]]},
    "final block neurons": {"blocks.1.mlp.hook_post": [Ix[:, -1, :128]]},
    "two indexes": {"blocks.0.attn.hook_z": [Ix[:, :, 0], Ix[:, 2:4]]},
    "whole mlp": {"blocks.0.mlp.hook_post": [Ix[[None]]]},
    "whole mlp twice": {"blocks.0.mlp.hook_post": [Ix[[None]]], "blocks.1.mlp.hook_post": [Ix[[None]]]},
}
# paired ops every run of the pattern must have counted (a subset of the counters)
COUNTS = {
    "whole z": {"pair_embed": 1},
    "one head": {"pair_embed": 1, "pair_layer_norm": 1, "pair_qkv": 1, "pair_attention": 1},
    "positions": {"pair_attention": 1},
    "features": {"pair_attention": 1},
    "neurons": {"pair_attention": 1, "pair_o_proj": 1, "pair_layer_norm": 2, "pair_mlp_in": 1},
    "batch subset": {"pair_mlp_in": 1},
    "two layers": {"pair_o_proj": 1, "pair_mlp_fused": 1, "pair_attention": 1},
    "mlp then head": {"pair_mlp_in": 1, "pair_mlp_out": 1, "pair_attention": 2},
    "final block head": {"pair_mlp_fused": 1, "pair_attention": 2, "pair_qkv": 2},
    "final block neurons": {"pair_mlp_fused": 1, "pair_mlp_in": 1},
    "two indexes": {"pair_attention": 1, "pair_splice": 2},
    "whole mlp": {"pair_attention": 1, "pair_o_proj": 1},
    "whole mlp twice": {"pair_attention": 2, "pair_o_proj": 2, "pair_mlp_out": 1},
}


@pytest.fixture(scope="module")
def setup():
    model = _model(dev)
    FlatParams(model)
    g = torch.Generator().manual_seed(5)
    base = torch.randint(0, 97, (B, S), generator=g).to(dev)
    src = torch.randint(0, 97, (B, S), generator=g).to(dev)
    yield model, base, src
    model.set_op_backend(None)


def _zero(model):
    for p in model.parameters():
        if p.grad is not None:
            p.grad.zero_()


def _collect(model, out, cache, sites):
    out.logsumexp(-1).sum().backward()
    torch.cuda.synchronize()
    res = {"out": out.detach().clone()}
    res.update({"act " + n: cache[n].detach().clone() for n in sites})
    res.update({"grad " + n: p.grad.detach().clone() for n, p in model.named_parameters()})
    return res


def _two_forwards(model, base, src, sites, logits, backend="hip32n"):
    model.set_op_backend(backend)
    _zero(model)
    cache = model.run_capture(src, list(sites))
    plan = RunPlan.with_splices([(n, ix, cache[n]) for n, ixs in sites.items() for ix in ixs], logits=logits)
    return _collect(model, model(base, plan=plan), cache, sites)


def _paired(model, base, src, sites, logits):
    model.set_op_backend("hip32p")
    _zero(model)
    res = model.run_paired(base, src, sites, logits=logits)
    assert res is not None, "the paired path was not taken"
    out, cache = res
    assert all(not cache[n].requires_grad for n in sites)
    return _collect(model, out, cache, sites)


def _oracle(model, base, src, sites, logits):
    o = _model("cpu", torch.float64)
    o.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    return _two_forwards(o, base.cpu(), src.cpu(), sites, logits, backend="torch")


def _same(a, b) -> bool:
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


@gpu
def test_forward_gemms_take_one_tile_and_the_same_splits_at_t_and_2t_rows():
    """What the bitwise criterion rests on.  Every forward GEMM with K = d_model takes one split; W_out's (K = d_mlp
    = 256) takes two, at T rows and at 2T rows alike, summed in split order."""
    from iit_amd.ops import hip_kernels as K
    from iit_amd.ops.hip32_ops import _tile
    d, dm, n_qkv = CFG["d_model"], CFG["d_mlp"], 3 * CFG["n_heads"] * CFG["d_head"]
    gemms = {"qkv": (n_qkv, d), "o_proj": (d, CFG["n_heads"] * CFG["d_head"]), "mlp_in": (dm, d), "mlp_out": (d, dm),
             "unembed": (CFG["d_vocab"], d)}
    for name, (N, Kd) in gemms.items():
        per_rows = []
        for M in (B, B * S, 2 * B * S):  # last-position rows, T, 2T
            assert _tile(M, N) == 0, (name, M)
            per_rows.append(K.gemm_f32_splits(M, N, Kd, 0))
        assert len(set(per_rows)) == 1, (name, per_rows)
        assert per_rows[0] == (1 if Kd == d else 2), (name, per_rows)


@gpu
@pytest.mark.parametrize("logits", ["last", "full"])
@pytest.mark.parametrize("pattern", list(SITES))
def test_paired_equals_two_forwards_bitwise(setup, pattern, logits):
    from iit_amd.ops.hip32_ops import HipF32NOps, HipF32Ops, HipF32POps, HipF32XOps
    model, base, src = setup
    sites = SITES[pattern]
    ref = _two_forwards(model, base, src, sites, logits)
    again = _two_forwards(model, base, src, sites, logits)
    loose = [k for k in ref if not _same(ref[k], again[k])]
    assert all(k.startswith("grad ") and ("embed" in k) for k in loose), loose  # the precondition

    others = [dict(c.calls) for c in (HipF32NOps, HipF32XOps, HipF32Ops)]
    HipF32POps.calls.clear()
    got = _paired(model, base, src, sites, logits)
    calls = dict(HipF32POps.calls)
    assert [dict(c.calls) for c in (HipF32NOps, HipF32XOps, HipF32Ops)] == others
    assert not [k for k in calls if k.endswith("_fallback")], calls
    for k, n in COUNTS[pattern].items():
        assert calls.get(k) == n, (k, calls)

    assert set(got) == set(ref)
    bad = [k for k in ref if k not in loose and not _same(got[k], ref[k])]
    assert not bad, bad
    if loose:
        oracle = _oracle(model, base, src, sites, logits)
        lib = _two_forwards(model, base, src, sites, logits, backend="torch")
        for k in loose:
            o = oracle[k].double()
            e_lib, e_got = _err(lib[k].double().cpu(), o), _err(got[k].double().cpu(), o)
            print(f"{pattern} {logits} {k}: e_hip32p {e_got:.3e} e_torch {e_lib:.3e}")
            assert e_got <= FACTOR * e_lib + FLOOR, (k, e_got, e_lib)


@gpu
def test_plain_model_falls_back_before_any_paired_op():
    from iit_amd.ops.hip32_ops import HipF32POps
    model = _model(dev)  # parameters outside an arena: QKV is not packed
    model.set_op_backend("hip32p")
    g = torch.Generator().manual_seed(6)
    base = torch.randint(0, 97, (B, S), generator=g).to(dev)
    src = torch.randint(0, 97, (B, S), generator=g).to(dev)
    HipF32POps.calls.clear()
    assert model.run_paired(base, src, SITES["one head"], logits="last") is None
    assert dict(HipF32POps.calls) == {"paired_fallback": 1}


@gpu
def test_registration():
    from iit_amd.ops import select_ops
    from iit_amd.ops.hip32_ops import HipF32NOps, HipF32POps, get_hip32p_ops
    model = _model(dev)
    ops = select_ops(model, "hip32p")
    assert type(ops) is HipF32POps and ops is get_hip32p_ops(model) and ops.name == "hip32p"
    assert ops.supports_pairs and not ops.fused and HipF32POps.calls is not HipF32NOps.calls
    assert not getattr(select_ops(model, "hip32n"), "supports_pairs", False)
    assert model.set_op_backend("hip32p").ops() is ops
    assert select_ops(model, None).name == "torch"  # never chosen automatically


@gpu
def test_model_pair_intervention_takes_the_paired_forward():
    """``BaseModelPair.ll_intervention`` on ``hip32p``: the bits and the ``ll_cache`` entries of ``hip32n``'s two
    forwards, through ``ll_paired_intervention``."""
    from iit_amd.model_pairs import IOI_ModelPair
    from iit_amd.models.transformer import HookedTransformer
    from iit_amd.ops.hip32_ops import HipF32POps
    from iit_amd.tasks.ioi import NAMES, make_ioi_corr, make_ioi_dataset_and_hl
    torch.manual_seed(0)
    ll = HookedTransformer(dict(CFG, d_vocab=50257, device=dev, dtype=torch.float32))
    FlatParams(ll)
    ds, hl = make_ioi_dataset_and_hl(64, ll, NAMES, device=dev)
    pair = IOI_ModelPair(hl, ll, make_ioi_corr(2), training_args={"lr_scheduler": None})
    x = ds.prompts[:, :-1].to(dev)
    base, src = x[:16], x[16:32]
    for node in pair.corr.keys():
        nodes = list(pair.corr[node])
        got = {}
        for backend in ("hip32n", "hip32p"):
            ll.set_op_backend(backend)
            HipF32POps.calls.clear()
            out = pair.ll_intervention(base, src, nodes)
            got[backend] = (out.detach().clone(), {n.name: pair.ll_cache[n.name].detach().clone() for n in nodes})
            if backend == "hip32p":
                assert HipF32POps.calls.get("pair_embed") == 1 and "paired_fallback" not in HipF32POps.calls
        assert _same(got["hip32p"][0], got["hip32n"][0]), node
        assert set(got["hip32p"][1]) == set(got["hip32n"][1])
        for name, t in got["hip32n"][1].items():
            assert _same(got["hip32p"][1][name], t), (node, name)
