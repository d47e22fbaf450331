"""What the ``hip32x`` backend must leave alone, checked without a GPU: selection rules, the entry point's option, the
torch path through ``Attention.compute_z`` and the CPU table of scripts/bench_attn_f32.py."""
import importlib.util
import os

import pytest
import torch

from iit_amd.models.transformer import HookedTransformer
from iit_amd.ops import select_ops
from iit_amd.ops.torch_ops import TorchOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


def test_hip32x_on_a_cpu_model_raises_runtime_error():
    with pytest.raises(RuntimeError):
        select_ops(_model(), "hip32x")
    with pytest.raises(ValueError):
        select_ops(_model(), "hip33")


def test_train_ioi_accepts_the_backend():
    from iit_amd.entry import train_ioi
    assert train_ioi.parse(["--fp32-backend", "hip32x"]).fp32_backend == "hip32x"
    assert train_ioi.parse([]).fp32_backend == "torch"


def test_torch_backend_with_a_cached_pattern_is_unchanged():
    """The layer's z with ``hook_pattern`` live is ``TorchOps.attention`` of the cached q, k, v bit for bit, and the
    logits equal a run without any hook."""
    m = _model()
    m.set_op_backend("torch")
    ops = select_ops(m, "torch")
    assert type(ops) is TorchOps and not hasattr(ops, "native_attention")
    tokens = torch.randint(0, 97, (3, 8), generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        logits, cache = m.run_with_cache(tokens)
        plain = m(tokens)
    assert torch.equal(logits, plain)
    for layer, block in enumerate(m.blocks):
        pre = f"blocks.{layer}.attn.hook_"
        seen = {}
        z = TorchOps.attention(ops, cache[pre + "q"], cache[pre + "k"], cache[pre + "v"], True, block.attn.attn_scale,
                               hook_pattern=lambda t: seen.setdefault("p", t))
        assert torch.equal(z, cache[pre + "z"])
        assert torch.equal(seen["p"], cache[pre + "pattern"])


def test_bench_candidates_on_the_cpu_are_torch_alone():
    spec = importlib.util.spec_from_file_location("bench_attn_f32", os.path.join(ROOT, "scripts", "bench_attn_f32.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert set(mod.CANDIDATES) == {"torch"}
    assert set(mod.candidates("cpu")) == {"torch"}
    assert set(mod.candidates("cuda")) == {"torch", "hip32x"}
