"""What the ``hip32p`` backend adds and leaves alone, checked without a GPU: the selection rules, the entry point's
option, the class attributes, the head-list spec, and that the torch backend's ``run_paired`` is as before."""
import pytest
import torch

import attn_f32_pair_util as P
from iit_amd.core.index import Ix
from iit_amd.ops import select_ops
from test_hip32n_cpu import _model


def test_hip32p_on_a_cpu_model_raises_runtime_error():
    with pytest.raises(RuntimeError):
        select_ops(_model(), "hip32p")


def test_train_ioi_accepts_the_backend():
    from iit_amd.entry import train_ioi
    assert train_ioi.parse(["--fp32-backend", "hip32p"]).fp32_backend == "hip32p"


def test_backend_class_attributes_and_protocol():
    from iit_amd.ops.hip32_ops import HipF32NOps, HipF32POps, HipF32XOps
    assert issubclass(HipF32POps, HipF32NOps) and HipF32POps.name == "hip32p" and HipF32POps.fused is False
    assert HipF32POps.supports_pairs is True and not hasattr(HipF32NOps, "supports_pairs")
    assert HipF32POps.calls is not HipF32NOps.calls and HipF32POps.calls is not HipF32XOps.calls
    for op in ("begin_forward", "fwd_prefetch", "pair_heads_ok", "pair_model_ok", "pair_embed_pos",
               "pair_layer_norm_fork", "pair_qkv", "pair_attention", "pair_attention_spliced", "attention_dual",
               "pair_splice", "pair_o_proj_residual", "pair_mlp_in", "pair_mlp_gelu_residual", "pair_mlp_out_residual"):
        assert callable(getattr(HipF32POps, op)), op
        assert not hasattr(HipF32NOps, op), op


def test_head_list_spec_selects_whole_heads():
    from iit_amd.ops.hip32_ops import _heads_spec
    shape = (2, 5, 6, 4)
    spec = _heads_spec([4, 0, 1, 4], shape)
    assert [d[1] for d in spec.dims][2] == [(0, 2), (4, 5)]
    assert torch.equal(P.selection_mask(spec, shape), P.index_mask(Ix[:, :, [0, 1, 4]], shape))
    assert not P.selection_mask(_heads_spec([], shape), shape).any()
    assert _heads_spec(range(0, 18, 2), (1, 1, 18, 4)) is None  # nine runs: more than the table holds


def test_torch_backend_run_paired_is_unchanged():
    """A backend without ``supports_pairs`` still gets None from ``run_paired`` (the two forwards run)."""
    m = _model()
    m.set_op_backend("torch")
    tokens = torch.randint(0, 97, (3, 8), generator=torch.Generator().manual_seed(3))
    assert m.run_paired(tokens, tokens, {"blocks.0.attn.hook_z": [Ix[:, :, 1]]}) is None
