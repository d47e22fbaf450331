"""What the ``hip32n`` backend must leave alone, and what it adds, checked without a GPU: the selection rules, the
entry point's option and the torch path through ``LayerNormSite.run``."""
import pytest
import torch

from iit_amd.models.transformer import HookedTransformer
from iit_amd.ops import select_ops
from iit_amd.ops.torch_ops import TorchOps

CFG = dict(n_layers=2, d_model=64, n_heads=4, d_head=16, d_mlp=256, d_vocab=97, n_ctx=16, act_fn="gelu_new",
           normalization_type="LN", device="cpu", dtype=torch.float32)


def _model():
    torch.manual_seed(0)
    m = HookedTransformer(dict(CFG))
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    return m


def test_hip32n_on_a_cpu_model_raises_runtime_error():
    with pytest.raises(RuntimeError):
        select_ops(_model(), "hip32n")
    with pytest.raises(ValueError):
        select_ops(_model(), "hip32m")


def test_train_ioi_accepts_the_backend():
    from iit_amd.entry import train_ioi
    assert train_ioi.parse(["--fp32-backend", "hip32n"]).fp32_backend == "hip32n"
    assert train_ioi.parse([]).fp32_backend == "torch"


def test_backend_class_attributes():
    from iit_amd.ops.hip32_ops import HipF32NOps, HipF32Ops, HipF32XOps
    assert issubclass(HipF32NOps, HipF32XOps) and HipF32NOps.name == "hip32n" and HipF32NOps.fused is False
    assert HipF32NOps.native_layer_norm is True and HipF32NOps.fuses_residual is True
    assert HipF32NOps.calls is not HipF32XOps.calls and HipF32NOps.calls is not HipF32Ops.calls
    assert not hasattr(HipF32XOps, "native_layer_norm")


def test_torch_backend_layer_norm_site_is_unchanged():
    """A torch-backend ``run_with_cache`` is bit-identical to a plain forward, and every cached ``hook_normalized`` is
    ``TorchOps.layer_norm`` of the cached residual: ``LayerNormSite.run`` takes the torch branch as before."""
    m = _model()
    m.set_op_backend("torch")
    ops = select_ops(m, "torch")
    assert type(ops) is TorchOps and not getattr(ops, "native_layer_norm", False)
    tokens = torch.randint(0, 97, (3, 8), generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        logits, cache = m.run_with_cache(tokens)
        plain = m(tokens)
    assert torch.equal(logits, plain)
    for layer, block in enumerate(m.blocks):
        want = TorchOps.layer_norm(ops, cache[f"blocks.{layer}.hook_resid_pre"], block.ln1.w, block.ln1.b, block.ln1.eps)
        assert torch.equal(want, cache[f"blocks.{layer}.ln1.hook_normalized"])
