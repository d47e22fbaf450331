"""The paired fp32 attention forward (``iit_attn_f32_fwd_pair``) and the masked backward (``iit_attn_f32_bwd_masked``)
of csrc/attn_fp32.hip on the GPU, bit for bit against compositions of the plain kernels' results
(tests/attn_f32_pair_util.py; the plain kernels are held to float64 by tests/test_attn_f32_kernel.py):

* ``z[B:]`` and all of ``lse`` are the plain forward's over the same 2B rows; ``z[:B]`` is
  ``where(mask, z_plain[B:], z_plain[:B])``;
* dq, dk, dv of the masked backward are the plain backward's fed ``where(mask, 0, dz)``, also when ``dz`` holds NaN at
  the selected elements;
* in every layout -- contiguous, packed q | k | v views, every tensor one float off a 16-byte boundary (the scalar
  path), a z whose row pitch is wider than ``H dh`` -- with NaN around every output and a sentinel in the pitch gaps;
* a captured graph replays forward + backward to the eager bits; every refusal raises before any launch.

The four shapes are the smallest that reach each path (``attn_f32_pair_util.CASES``), each causal and bidirectional,
with the seven indexes of ``attn_f32_pair_util.attn_indexes``.
"""
import functools

import pytest
import torch

import attn_f32_pair_util as P
import attn_f32_util as A

gpu = pytest.mark.gpu
dev = "cuda"
SENTINEL = -12345.0


def _kernels():
    from iit_amd.ops import hip_kernels as K
    return K


def _spec(index, shape):
    from iit_amd.ops.splice import patch_spec
    return patch_spec(index, tuple(shape))


def _guarded(shape, offset=0, pad=32):
    """A NaN fp32 view of ``shape`` inside a larger NaN buffer, ``offset`` floats off a 16-byte aligned address;
    returns (view, buffer, slice of the view in the buffer)."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * pad + offset,), float("nan"), dtype=torch.float32, device=dev)
    sl = slice(pad + offset, pad + offset + n)
    return buf[sl].view(shape), buf, sl


def _untouched(buf, sl) -> bool:
    return bool(buf[:sl.start].isnan().all()) and bool(buf[sl.stop:].isnan().all())


@functools.lru_cache(maxsize=None)
def _plain(c, causal):
    """(operands of the 2B rows on the GPU, dz of the B base rows, scale, the plain forward's z and lse over the 2B
    rows), computed once per case."""
    K = _kernels()
    B, S, H, dh = c
    case = A.normal_case(2 * B, S, H, dh, seed=300 + S + dh)
    ops = {n: case[n].to(dev) for n in ("q", "k", "v")}
    dz = case["do"][:B].to(dev)
    scale = dh ** -0.5
    z = torch.empty(2 * B, S, H, dh, device=dev)
    lse = torch.empty(2 * B, H, S, device=dev)
    K.attn_f32_fwd(ops["q"], ops["k"], ops["v"], z, lse, scale, causal)
    torch.cuda.synchronize()
    return ops, dz, scale, z, lse


def _plain_bwd(c, causal, dz):
    K = _kernels()
    ops, _, scale, _, lse = _plain(c, causal)
    B = c[0]
    out = [torch.empty(c, device=dev) for _ in range(3)]
    K.attn_f32_bwd(ops["q"][:B], ops["k"][:B], ops["v"][:B], dz, lse[:B].contiguous(), *out, scale, causal)
    return out


# ------------------------------------------------------------------------------ layouts
def _contiguous(ops, dz, c):
    B, S, H, dh = c
    outs = {"z": _guarded((2 * B, S, H, dh))}
    outs.update({n: _guarded(c) for n in ("dq", "dk", "dv")})
    return dict(ops), dz.clone(), outs, None


def _packed(ops, dz, c):
    """q, k, v views of one packed ``[2B][S][3][H][dh]`` buffer, dq, dk, dv views of another over the B base rows."""
    B, S, H, dh = c
    src = _guarded((2 * B, S, 3, H, dh))[0]
    dst = _guarded((B, S, 3, H, dh))
    o, outs = {}, {"z": _guarded((2 * B, S, H, dh))}
    for i, n in enumerate(("q", "k", "v")):
        src[:, :, i].copy_(ops[n])
        o[n] = src[:, :, i]
        outs["d" + n] = (dst[0][:, :, i], dst[1], dst[2])
    return o, dz.clone(), outs, None


def _offset(ops, dz, c):
    """Every operand and output one float off a 16-byte aligned base: the scalar path."""
    B, S, H, dh = c
    o = {}
    for n in ("q", "k", "v"):
        o[n] = _guarded((2 * B, S, H, dh), offset=1)[0]
        o[n].copy_(ops[n])
        assert o[n].data_ptr() % 16 == 4
    d = _guarded(c, offset=1)[0]
    d.copy_(dz)
    outs = {"z": _guarded((2 * B, S, H, dh), offset=1)}
    outs.update({n: _guarded(c, offset=1) for n in ("dq", "dk", "dv")})
    return o, d, outs, None


def _pitched(ops, dz, c):
    """z (and dz) with a row pitch of ``H dh + 4`` floats, the gaps holding a sentinel."""
    B, S, H, dh = c
    pitch = H * dh + 4
    o, d, outs, _ = _contiguous(ops, dz, c)
    view, buf, sl = _guarded((2 * B, S, pitch))
    view.fill_(SENTINEL)
    outs["z"] = (view.as_strided((2 * B, S, H, dh), (S * pitch, pitch, dh, 1), view.storage_offset()), buf, sl)
    dwide = torch.full((B, S, pitch), float("nan"), device=dev)
    d = dwide.as_strided((B, S, H, dh), (S * pitch, pitch, dh, 1))
    d.copy_(dz)
    return o, d, outs, view


LAYOUTS = (_contiguous, _packed, _offset, _pitched)


def _check_case(c, causal, layout, names=None):
    K = _kernels()
    B, S, H, dh = c
    ops0, dz0, scale, z_plain, lse_plain = _plain(c, causal)
    for name, index in P.attn_indexes(c).items():
        if names is not None and name not in names:
            continue
        what = f"{layout.__name__} {name}"
        spec = _spec(index, c)
        mask = P.selection_mask(spec, c).to(dev)
        ops, dz, outs, gaps = layout(ops0, dz0, c)
        lse = _guarded((2 * B, H, S))
        K.attn_f32_fwd_pair(ops["q"], ops["k"], ops["v"], outs["z"][0], lse[0], scale, causal, spec)
        z = outs["z"][0]
        assert A.same_bits(lse[0], lse_plain), what
        assert A.same_bits(z[B:], z_plain[B:]), what
        assert A.same_bits(z, P.paired_z(z_plain, mask)), what
        if gaps is not None:
            assert bool((gaps[..., H * dh:] == SENTINEL).all()), what
        want = _plain_bwd(c, causal, P.masked_dz(dz0, mask))
        for fill in (None, float("nan")):
            if fill is not None:
                dz.copy_(P.masked_dz(dz0, mask, fill))
                for n in ("dq", "dk", "dv"):
                    outs[n][0].fill_(float("nan"))
            K.attn_f32_bwd_masked(ops["q"][:B], ops["k"][:B], ops["v"][:B], dz, lse[0][:B], outs["dq"][0],
                                  outs["dk"][0], outs["dv"][0], scale, causal, spec)
            for n, w in zip(("dq", "dk", "dv"), want):
                assert bool(outs[n][0].isfinite().all()), (what, n, fill)
                assert A.same_bits(outs[n][0], w), (what, n, fill)
        torch.cuda.synchronize()
        for n, (_, buf, sl) in list(outs.items()) + [("lse", lse)]:
            assert _untouched(buf, sl), f"{what} {n}: a store outside the tensor"


@gpu
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "bidir"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda f: f.__name__.strip("_"))
@pytest.mark.parametrize("c", P.CASES, ids=P.case_id)
def test_paired_forward_and_masked_backward_are_compositions_of_the_plain_kernels(c, layout, causal):
    _check_case(c, causal, layout)


@gpu
def test_lse_of_a_wholly_selected_base_head_is_still_written():
    """No early exit for a base wave all of whose z is replaced: the backward reads its lse."""
    K = _kernels()
    c = P.CASES[3]
    B, S, H, dh = c
    ops, _, scale, _, lse_plain = _plain(c, True)
    z = torch.full((2 * B, S, H, dh), float("nan"), device=dev)
    lse = torch.full((2 * B, H, S), float("nan"), device=dev)
    K.attn_f32_fwd_pair(ops["q"], ops["k"], ops["v"], z, lse, scale, True, _spec(P.Ix[:, :, 1], c))
    assert A.same_bits(lse[:B, 1], lse_plain[:B, 1])


@gpu
def test_graph_replay_equals_eager():
    K = _kernels()
    c, causal = P.CASES[1], True
    B, S, H, dh = c
    ops, dz, scale, z_plain, lse_plain = _plain(c, causal)
    index = P.attn_indexes(c)["heads x positions"]
    spec = _spec(index, c)
    mask = P.selection_mask(spec, c).to(dev)
    want_z = P.paired_z(z_plain, mask)
    want = _plain_bwd(c, causal, P.masked_dz(dz, mask))
    z = torch.empty(2 * B, S, H, dh, device=dev)
    lse = torch.empty(2 * B, H, S, device=dev)
    grads = [torch.empty(c, device=dev) for _ in range(3)]

    def step():
        K.attn_f32_fwd_pair(ops["q"], ops["k"], ops["v"], z, lse, scale, causal, spec)
        K.attn_f32_bwd_masked(ops["q"][:B], ops["k"][:B], ops["v"][:B], dz, lse[:B], *grads, scale, causal, spec)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside capture
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for _ in range(2):
        for t in [z, lse] + grads:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert A.same_bits(z, want_z) and A.same_bits(lse, lse_plain)
        for n, g, w in zip(("dq", "dk", "dv"), grads, want):
            assert A.same_bits(g, w), n


@gpu
def test_refusals_raise_before_any_launch():
    K = _kernels()
    shape = (4, 8, 2, 16)
    good = torch.zeros(shape, device=dev)
    spec = _spec(P.Ix[:, :, 1], (2, 8, 2, 16))

    def outputs(sh):
        z = torch.full(sh, float("nan"), device=dev)
        lse = torch.full((sh[0], sh[2], sh[1]), float("nan"), device=dev)
        return z, lse, [torch.full(sh, float("nan"), device=dev) for _ in range(3)]

    def refused_fwd(q, sp, sh):
        z, lse, _ = outputs(sh)
        with pytest.raises(ValueError):
            K.attn_f32_fwd_pair(q, q, q, z, lse, 0.25, True, sp)
        torch.cuda.synchronize()
        assert bool(z.isnan().all()) and bool(lse.isnan().all())

    def refused_bwd(q, sp, sh):
        _, lse, grads = outputs(sh)
        with pytest.raises(ValueError):
            K.attn_f32_bwd_masked(q, q, q, q, lse, *grads, 0.25, True, sp)
        torch.cuda.synchronize()
        assert all(bool(g.isnan().all()) for g in grads)

    odd = torch.zeros(3, 8, 2, 16, device=dev)
    refused_fwd(odd, _spec(P.Ix[:, :, 1], (1, 8, 2, 16)), tuple(odd.shape))  # odd B2
    refused_fwd(good, None, shape)  # no spec
    refused_fwd(good, _spec(P.Ix[:, :, 1], shape), shape)  # a spec over the 2B rows, not over the base shape
    refused_fwd(good, _spec(P.Ix[:, :, 1], (2, 8, 2, 8)), shape)  # another dh
    refused_bwd(good, None, shape)
    refused_bwd(good, spec, shape)  # a spec over half the rows
    for q in (torch.zeros(2, 65, 2, 16, device=dev), torch.zeros(2, 8, 2, 65, device=dev), good.bfloat16(),
              torch.zeros(4, 8, 2, 32, device=dev)[..., ::2]):
        sh = tuple(q.shape)
        sp = _spec(P.Ix[:, :, 1], (sh[0] // 2,) + sh[1:])
        refused_fwd(q, sp, sh)
        refused_bwd(q, _spec(P.Ix[:, :, 1], sh), sh)
    # the library entry itself refuses too (nothing is launched: the outputs keep their NaN)
    z, lse, _ = outputs(shape)
    lib = K.lib()
    strides = K._strides3(good, good, good, z)
    stream = torch.cuda.current_stream().cuda_stream
    args = (good.data_ptr(), good.data_ptr(), good.data_ptr(), z.data_ptr(), lse.data_ptr(), strides)
    assert lib.iit_attn_f32_fwd_pair(*args, 4, 8, 2, 16, 0.25, 1, None, stream) != 0
    assert lib.iit_attn_f32_fwd_pair(*args, 3, 8, 2, 16, 0.25, 1, spec.ptr, stream) != 0
    assert lib.iit_attn_f32_fwd_pair(*args, 4, 8, 2, 16, 0.25, 1, _spec(P.Ix[:, :, 1], shape).ptr, stream) != 0
    torch.cuda.synchronize()
    assert bool(z.isnan().all()) and bool(lse.isnan().all())
