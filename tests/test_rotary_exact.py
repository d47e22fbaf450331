"""Element-wise tests of the rotary kernels of csrc/llama_ops.hip on the GPU (``rotary_vec_kernel`` and the per-pair
``rotary_kernel``) against the float64 reference and bound of tests/llama_exact_util.py.  The tables are the test's
own, [offset + S, rd] with a different value in every entry and NaN in every row before ``offset``, so a read at the
partner's index, at another position or past the table shows (the model's tables repeat each angle for both elements
of a pair).  B, S, H = 2, 5, 3 (the last block is partial), offset 0 and 3, both pairings, forward and inverse, an
``exact`` family (bitwise) and a ``random`` one; the output lies in a sentinel-filled buffer whose spare elements must
keep their bits, and the pass-through features are compared bit for bit.

Which kernel a case takes follows ``iit_rotary``: the vector kernel needs D % 8 == 0, rd % 16 == 0 (halves) or
rd % 8 == 0 (adjacent), strides that are multiples of 8 and 16-byte aligned bases; ``test_rotary_views`` forces the
per-pair kernel at D = rd = 128 by a view offset by one element and by head / position strides that are no multiple of
8, and runs the vector kernel on a strided packed-QKV view.  Under ``IIT_LLAMA_VEC=0`` (tests/test_launch_variants.py)
every case takes the per-pair kernel.

Measured on an MI355X: 46 cases, 46 passed, none skipped, 3.6 s for the module (0.9 s of it the first use of
``RotaryFn``).  Worst ``|got - ref| / bound``: 0.990 through the vector kernel, 0.984 through the per-pair kernel.  As
a check of the module itself, a library whose vector kernel reads ``sin`` for the first half at the partner's index and
whose per-pair kernel reads ``cos`` there failed every halves case of the vector kernel, every per-pair case and (under
``IIT_LLAMA_VEC=0``) 44 of 46 cases, while ``test_rotary_function_with_model_tables`` -- the model's tables -- passed.
"""
import pytest
import torch

import llama_exact_util as X

pytestmark = pytest.mark.gpu

dev = "cuda"
BF16 = torch.bfloat16
B, S, H = X.ROT_B, X.ROT_S, X.ROT_H


@pytest.fixture(scope="module")
def K():
    from iit_amd.ops import hip_kernels
    hip_kernels.lib()
    return hip_kernels


def _run(K, xv, x, cos, sin, rd, offset, adjacent, inverse, family, tag):
    """``xv``: the device view handed to the kernel, ``x`` its CPU values."""
    D = x.shape[-1]
    n = x.numel()
    obuf = X.filled((n + 8,), BF16, dev)
    out = obuf[:n].view(x.shape)
    K.rotary(xv, out, cos.to(dev), sin.to(dev), rd, offset, adjacent, inverse)
    torch.cuda.synchronize()
    ref = X.rotary_ref(x, cos, sin, rd, offset, adjacent, inverse)
    got = out.cpu()
    bad = X.count(X.rotary_check(got, x, ref, rd, family))
    w = X.worst(got[..., :rd], ref["out"][..., :rd], ref["tol"][..., :rd])
    assert not bad, (tag, offset, inverse, bad, w)
    assert bool((obuf[n:].float() == X.BF16_FILL).all()), "written past the output"
    assert D == out.shape[-1]
    return w


def _id(D, rd, adjacent):
    return f"{'vec' if X.rotary_vec_ok(D, rd, adjacent) else 'scalar'}-{D}-{rd}-{'adjacent' if adjacent else 'halves'}"


SHAPES = [(D, rd, adj) for D, rd in X.ROT_SHAPES for adj in (False, True)]


@pytest.mark.parametrize("family", X.FAMILIES)
@pytest.mark.parametrize("D,rd,adjacent", SHAPES, ids=[_id(*c) for c in SHAPES])
def test_rotary(K, D, rd, adjacent, family):
    worst = 0.0
    for offset in X.ROT_OFFSETS:
        for inverse in (False, True):
            x, cos, sin = X.rotary_inputs(family, B, S, H, D, rd, offset, 3 * D + rd + offset)
            worst = max(worst, _run(K, x.to(dev), x, cos, sin, rd, offset, adjacent, inverse, family, "contiguous"))
    if family == "random":
        print(f"WORST rotary {_id(D, rd, adjacent)} {worst:.3f}")


@pytest.mark.parametrize("family", X.FAMILIES)
@pytest.mark.parametrize("adjacent", [False, True], ids=["halves", "adjacent"])
@pytest.mark.parametrize("view", ["offset1", "stride_odd", "packed_qkv"])
def test_rotary_views(K, view, adjacent, family):
    """D = rd = 128.  ``offset1``: a contiguous view one element into its buffer (misaligned base); ``stride_odd``:
    head stride 132 and position stride 3 * 132 (multiples of 4, not of 8); both must fall back to the per-pair
    kernel -- the vector kernel's 16-byte loads would be misaligned.  ``packed_qkv``: the q slice of a [B, S, 3, H, D]
    projection, strides all multiples of 8 (vector kernel)."""
    D = rd = 128
    offset = 3
    x, cos, sin = X.rotary_inputs(family, B, S, H, D, rd, offset, 77)
    if view == "offset1":
        buf = X.filled((x.numel() + 8,), BF16, dev)
        xv = buf[1:1 + x.numel()].view(B, S, H, D)
        assert xv.data_ptr() % 16 != 0
    elif view == "stride_odd":
        sh, ss = D + 4, H * (D + 4)
        buf = X.filled((B * S * ss + 8,), BF16, dev)
        xv = buf.as_strided((B, S, H, D), (S * ss, ss, sh, 1))
        assert sh % 8 and ss % 8 and xv.data_ptr() % 16 == 0
    else:
        packed = X.filled((B, S, 3, H, D), BF16, dev)
        xv = packed[:, :, 1]
        assert not xv.is_contiguous() and all(s % 8 == 0 for s in xv.stride()[:3])
    xv.copy_(x)
    for inverse in (False, True):
        _run(K, xv, x, cos, sin, rd, offset, adjacent, inverse, family, view)


@pytest.mark.parametrize("adjacent", [False, True], ids=["halves", "adjacent"])
def test_rotary_function_with_model_tables(K, adjacent):
    """``RotaryFn`` with ``rotary_tables`` of a config: the forward against the float64 rotation and the gradient
    against float64 autograd of that rotation, both under the element-wise bound (the backward is the kernel's
    inverse: the reference of the gradient is the inverse rotation of the bf16 ``g``)."""
    from iit_amd.models.config import HookedTransformerConfig
    from iit_amd.models.transformer import rotary_tables
    from iit_amd.ops import hip_ops
    D, rd, offset = 128, 64, 3
    cfg = HookedTransformerConfig.from_dict(dict(n_layers=1, d_model=256, n_heads=2, d_head=D, n_ctx=16, d_vocab=16,
                                                 act_fn="silu", rotary_dim=rd, rotary_adjacent_pairs=adjacent,
                                                 positional_embedding_type="rotary"))
    sin, cos = rotary_tables(cfg)
    x = (2.0 * torch.randn(B, S, H, D, generator=X.gen(5))).bfloat16()
    g = torch.randn(B, S, H, D, generator=X.gen(6)).bfloat16()
    xd = x.to(dev).requires_grad_()
    y = hip_ops.RotaryFn.apply(xd, cos.to(dev), sin.to(dev), rd, offset, adjacent)
    y.backward(g.to(dev))
    torch.cuda.synchronize()
    ref = X.rotary_ref(x, cos, sin, rd, offset, adjacent, False)
    assert not X.count(X.rotary_check(y.detach().cpu(), x, ref, rd, "random"))
    # float64 autograd of the float64 forward
    x64 = x.double().requires_grad_()
    c = cos[offset:offset + S].double().view(1, S, 1, rd)
    s = sin[offset:offset + S].double().view(1, S, 1, rd)
    i0, i1 = X.rotary_pairs(rd, adjacent)
    rot = torch.zeros(B, S, H, rd, dtype=torch.float64)
    rot = rot.index_add(3, i0, -x64[..., i1]).index_add(3, i1, x64[..., i0])
    y64 = torch.cat([x64[..., :rd] * c + rot * s, x64[..., rd:]], -1)
    assert float((y64.detach() - ref["out"]).abs().max()) < 1e-12
    y64.backward(g.double())
    gref = X.rotary_ref(g, cos, sin, rd, offset, adjacent, True)
    assert float((x64.grad - gref["out"]).abs().max()) < 1e-12
    assert not X.count(X.rotary_check(xd.grad.cpu(), g, {"out": x64.grad, "tol": gref["tol"]}, rd, "random"))
