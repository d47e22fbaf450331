"""Element-wise tests of the producer-side splice kernels of csrc/llama_ops.hip on the GPU
(``swiglu_splice_fwd_kernel``, ``swiglu_splice_bwd_kernel``, ``embed_splice_fwd_kernel``,
``embed_splice_bwd_kernel<__bf16>`` / ``<float>``), called through ``iit_amd.ops.hip_kernels`` with specs from ``patch_spec`` on ``Ix`` indices over [B, S, d].  The reference
mask comes from torch's own indexing (tests/llama_exact_util.py), so the range table is under test too.

Indices: one position, a position list of three runs, eight runs (the table's limit), innermost ranges that are no
multiples of 8 (``3:13``) and two runs (``0:5`` and ``9:16``), everything, nothing.  Sources: contiguous, a broadcast
[1, S, d], a strided view (every other row and column of a sentinel-filled buffer).

* ``swiglu_splice_fwd``: selected elements equal ``src`` bit for bit, the others lie within the SwiGLU bound;
  ``swiglu_splice_bwd``: selected ``dgate`` / ``dup`` are == 0, the others within the bound.  ``gate`` is the sweep of
  every finite bf16 value up to 2^40 (shape [2, 17, 1264] holds it once).
* ``embed_splice_fwd``: ``W16[tok]`` or ``src`` bit for bit, ``W16`` with a row stride ``ld > d``, repeated tokens.
* ``embed_splice_bwd``, bf16 and fp32 ``dout``: integer operands with a non-zero integer prefill bit for bit, normal
  data within ``tol_sum`` (n = the unspliced rows of that token); ``ldg > d``; all tokens equal, and a mixed pattern
  with a token that occurs at fully spliced rows only; rows of tokens that never receive a term, the ``ldg - d`` gap and
  the spare elements keep the prefill's bits.

Measured on an MI355X: 98 cases, 98 passed, none skipped, 2.6 s for the module.  Worst ``|got - ref| / bound`` of the
``random`` embedding gradient: 0.217 (bf16 ``dout``), 0.264 (fp32); the SwiGLU parts share the figures of
tests/test_swiglu_exact.py.  As a check of the module itself, a library whose ``swiglu_splice_bwd`` ignores the
position ranges, whose ``embed_splice_bwd`` still adds element 3 of a spliced chunk and whose ``embed_splice_fwd``
ignores the source's innermost stride failed 18 of 21, 48 of 56 and 6 of 21 cases (the rest select everything or
nothing, hold no spliced element 3, or have a unit-stride source).
"""
import pytest
import torch

import llama_exact_util as X

pytestmark = pytest.mark.gpu

dev = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
SW_SHAPE = (X.SPL_B, X.SPL_S, 1264)  # 42976 elements >= the 42754 of the sweep
EM_SHAPE = (X.SPL_B, X.SPL_S, X.SPL_D)
INDICES = sorted(X.splice_indices())
SRC_KINDS = ["contiguous", "broadcast", "strided"]
VOCAB = 9
_CACHE = {}


@pytest.fixture(scope="module")
def K():
    from iit_amd.ops import hip_kernels
    hip_kernels.lib()
    return hip_kernels


def _spec(name, shape, src):
    from iit_amd.ops.splice import patch_spec
    ix = X.splice_indices()[name]
    spec = patch_spec(ix, shape, src)
    assert spec is not None and spec.dims[3][0] % 8 == 0, name
    return spec, X.splice_mask(ix, shape)


def _swiglu_operands():
    """gate (the sweep, filled up with normal values), up, dpost [2, 17, 1264] and their float64 reference, once."""
    if "sw" not in _CACHE:
        n = SW_SHAPE[0] * SW_SHAPE[1] * SW_SHAPE[2]
        v = X.all_bf16()
        gn = X.gen(50)
        g = torch.cat([v, (2.0 * torch.randn(n - v.numel(), generator=gn)).bfloat16()]).view(SW_SHAPE)
        u, dv = torch.randn(SW_SHAPE, generator=gn).bfloat16(), torch.randn(SW_SHAPE, generator=gn).bfloat16()
        dv[dv == 0] = 1.0  # a spliced gradient that is not zeroed cannot hide behind dpost == 0
        _CACHE["sw"] = (g, u, dv, X.swiglu_ref(g, u, dv))
    return _CACHE["sw"]


def _buf(shape, dtype):
    n = 1
    for s in shape:
        n *= s
    buf = X.filled((n + 8,), dtype, dev)
    return buf, buf[:n].view(shape)


def _spare_kept(buf, n):
    tail = buf[n:].cpu()
    return not int(X.bad_bits(tail, X.filled(tuple(tail.shape), tail.dtype)).sum())


@pytest.mark.parametrize("kind", SRC_KINDS)
@pytest.mark.parametrize("name", INDICES)
def test_swiglu_splice(K, name, kind):
    g, u, dv, ref = _swiglu_operands()
    src = X.splice_src(kind, SW_SHAPE, 3, dev)
    spec, mask = _spec(name, SW_SHAPE, src)
    n = g.numel()
    bufs = {k: _buf(SW_SHAPE, BF16) for k in ("post", "dgate", "dup")}
    gd, ud = g.to(dev), u.to(dev)
    K.swiglu_splice_fwd(gd, ud, bufs["post"][1], src, spec.ptr)
    K.swiglu_splice_bwd(dv.to(dev), gd, ud, bufs["dgate"][1], bufs["dup"][1], spec.ptr)
    torch.cuda.synchronize()
    got = {k: v.cpu() for k, (_, v) in bufs.items()}
    within = X.swiglu_check(got, ref)
    want = src.cpu().expand(SW_SHAPE)
    bad = {"post_src": X.bad_bits(got["post"], want.contiguous()) & mask,
           "dgate_zero": (got["dgate"].float() != 0) & mask, "dup_zero": (got["dup"].float() != 0) & mask}
    bad.update({k: m & ~mask for k, m in within.items()})
    assert not X.count(bad), (X.count(bad), int(mask.sum()))
    assert all(_spare_kept(b, n) for b, _ in bufs.values())
    assert int(mask.sum()) == {"all": n, "none": 0}.get(name, int(mask.sum()))


def _tokens(pattern: str, mask: torch.Tensor) -> torch.Tensor:
    """int64 [B, S] in [0, VOCAB - 1): ``equal`` -- all 5; ``mixed`` -- repeated tokens from 0 .. 6, token 7 at every
    fully spliced row and nowhere else (it receives no gradient); token 8 never occurs."""
    Bn, Sn, _ = mask.shape
    if pattern == "equal":
        return torch.full((Bn, Sn), 5, dtype=torch.int64)
    tok = torch.randint(0, 7, (Bn, Sn), generator=X.gen(60))
    tok[mask.all(2)] = 7
    return tok


@pytest.mark.parametrize("kind", SRC_KINDS)
@pytest.mark.parametrize("name", INDICES)
def test_embed_splice_fwd(K, name, kind):
    Bn, Sn, d = EM_SHAPE
    ld = d + 8
    src = X.splice_src(kind, EM_SHAPE, 4, dev)
    spec, mask = _spec(name, EM_SHAPE, src)
    tok = _tokens("mixed", mask)
    assert int(torch.bincount(tok.reshape(-1)).max()) > 1
    W = (3.0 * torch.randn(VOCAB, d, generator=X.gen(61))).bfloat16()
    W16 = X.strided(W.to(dev), ld, 0, dev)
    assert W16.stride(0) == ld
    obuf, out = _buf(EM_SHAPE, BF16)
    K.embed_splice_fwd(tok.reshape(-1).to(dev), W16, out, src, spec.ptr)
    torch.cuda.synchronize()
    ref = X.embed_splice_fwd_ref(tok, W, src.cpu(), mask)
    assert not int(X.bad_bits(out.cpu(), ref.contiguous()).sum())
    assert _spare_kept(obuf, out.numel())


@pytest.mark.parametrize("family", X.FAMILIES)
@pytest.mark.parametrize("pattern", ["equal", "mixed"])
@pytest.mark.parametrize("gt", ["bf16", "f32"])
@pytest.mark.parametrize("name", INDICES)
def test_embed_splice_bwd(K, name, gt, pattern, family):
    Bn, Sn, d = EM_SHAPE
    T, ldg = Bn * Sn, d + 8
    dtype = BF16 if gt == "bf16" else F32
    spec, mask = _spec(name, EM_SHAPE, None)
    tok = _tokens(pattern, mask)
    if family == "exact":
        dout = X.int_operand(EM_SHAPE, dtype, 62, T + 1)
        pre = X.int_operand((VOCAB * ldg + 8,), F32, 63, T + 1)
        pre[pre == 0] = 3.0
    else:
        dout = torch.randn(EM_SHAPE, generator=X.gen(62)).to(dtype)
        pre = torch.randn(VOCAB * ldg + 8, generator=X.gen(63)).float()
    dout[dout == 0] = 1.0
    gbuf = pre.to(dev)
    grad = gbuf[:VOCAB * ldg].view(VOCAB, ldg)[:, :d]
    assert grad.stride(0) == ldg
    K.embed_splice_bwd(tok.reshape(-1).to(dev), dout.reshape(T, d).to(dev), grad, spec.ptr)
    torch.cuda.synchronize()
    whole = gbuf.cpu()
    got = whole[:VOCAB * ldg].view(VOCAB, ldg)
    grad0 = pre[:VOCAB * ldg].view(VOCAB, ldg)[:, :d]
    ref = X.embed_splice_bwd_ref(tok, dout, grad0, mask)
    bad = X.bad_sum(got[:, :d], ref["grad"], ref["tol"], family, grad0, ref["n"])
    assert not int(bad.sum()), (int(bad.sum()), X.worst(got[:, :d], ref["grad"], ref["tol"]))
    keep = torch.ones(VOCAB * ldg + 8, dtype=torch.bool)
    keep[:VOCAB * ldg].view(VOCAB, ldg)[:, :d] = False
    assert not int((X.bad_bits(whole, pre) & keep).sum()), "the ldg - d gap or the spare elements were written"
    assert bool((ref["n"][8] == 0).all())
    if pattern == "mixed" and bool(mask.all(2).any()):
        assert bool((tok == 7).any()) and bool((ref["n"][7] == 0).all())
    if family == "random" and int(ref["n"].max()):
        print(f"WORST embed_splice_bwd<{gt}> {X.worst(got[:, :d], ref['grad'], ref['tol']):.3f}")
