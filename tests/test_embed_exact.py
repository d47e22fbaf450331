"""Element-wise tests of the embedding kernels of csrc/kernels.hip on the GPU (``embed_pos_fwd_kernel`` and its scalar
twin, ``embed_bwd_pos_kernel``, ``pos_bwd_kernel``, ``pos_bwd_scalar_kernel``; ``embed_bwd_kernel`` when
tests/test_launch_variants.py runs ``test_embed_bwd`` with ``IIT_EMBED_BWD_POS=0``) against the references and bounds
of tests/misc_exact_util.py (proved on the CPU by tests/test_misc_exact_ref.py).

The forward is one IEEE add and is compared bit for bit, in a prefilled buffer whose spare tail must keep its bits.
The backward sums have no fixed order: every case runs on the ``exact`` family (integers, bitwise the float64 sum)
and on the ``random`` one (``(n + 3) E`` bound), into prefilled gradients; rows that receive no term keep their bits.

Measured on an MI355X: 153 cases, 153 passed, none skipped, 2.8 s for the module; the slowest case is the first (0.3 s,
one-time initialisation), every other case 0.01 s or less.  As a check of the module itself, a library whose
``embed_bwd_pos_kernel`` starts a run at ``acc = 0`` instead of the row's value at a token change failed all 64 cases
of ``test_embed_bwd`` and both ``test_embed_bwd_one_gradient_only[dWpos-*]`` (the two that compute dW_E); the other 87
cases, which do not run that kernel, passed.  The forward cases d = 1, 3, 66, 255 and the unaligned rows were not
run against the float4-only forward they replace: it would issue misaligned 16-byte accesses.
"""
import pytest
import torch

import misc_exact_util as X

pytestmark = pytest.mark.gpu

dev = "cuda"
F32 = torch.float32
VOCAB = 200
SD = [(1, 1), (3, 66), (1, 255), (3, 256), (1, 257), (3, 768)]  # every S of {1, 3} and every d of the backward


@pytest.fixture(scope="module")
def K():
    from iit_amd.ops import hip_kernels
    hip_kernels.lib()
    old = hip_kernels.CHECK_BOUNDS
    hip_kernels.CHECK_BOUNDS = True
    yield hip_kernels
    hip_kernels.CHECK_BOUNDS = old


def _count(bad: dict) -> dict:
    return {n: int(m.sum()) for n, m in bad.items() if int(m.sum())}


def _offset_view(x: torch.Tensor, off: int = 1) -> torch.Tensor:
    """A device copy of ``x`` that starts ``off`` floats into a larger NaN buffer (rows not 16-byte aligned)."""
    buf = X.filled((x.numel() + off + 3,), x.dtype, dev)
    view = buf[off:off + x.numel()].view(x.shape)
    view.copy_(x)
    return view


# ================================================================================================ forward
def _fwd_case(K, B, S, d, seed, we_off=0, pos_off=0, out_off=0):
    g = X.gen(seed)
    vocab = 11
    tok = torch.randint(0, vocab, (B, S), generator=g)
    tok.view(-1)[0] = 0
    tok.view(-1)[-1] = vocab - 1
    if B * S > 4:
        tok.view(-1)[1] = vocab - 1  # a repeat
        tok.view(-1)[3] = 0
    WE, Wpos = torch.randn(vocab, d, generator=g), torch.randn(S + 2, d, generator=g)
    T = B * S
    buf = X.filled((out_off + T * d + 8,), F32, dev)
    pre = buf.clone()
    out = buf[out_off:out_off + T * d].view(T, d)
    we = _offset_view(WE, we_off) if we_off else WE.to(dev)
    wp = _offset_view(Wpos, pos_off) if pos_off else Wpos.to(dev)
    K.embed_pos_fwd(tok.to(dev), we, wp, out, B, S, d)
    torch.cuda.synchronize()
    ref = X.embed_fwd_ref(tok, WE, Wpos, S)
    assert not int(X.bad_bits(out.cpu(), ref).sum()), int(X.bad_bits(out.cpu(), ref).sum())
    keep = torch.ones(buf.numel(), dtype=torch.bool)
    keep[out_off:out_off + T * d] = False
    assert not int((X.bad_bits(buf.cpu(), pre.cpu()) & keep).sum())


@pytest.mark.parametrize("B,S", [(1, 1), (3, 5)])
@pytest.mark.parametrize("d", [4, 64, 252, 256, 260, 768, 1, 3, 66, 255])
def test_embed_fwd(K, d, B, S):
    _fwd_case(K, B, S, d, seed=d)


@pytest.mark.parametrize("which", ["W_E", "W_pos", "out"])
def test_embed_fwd_unaligned_rows(K, which):
    """d = 64 with one operand an odd-offset view of a larger buffer: no row of it is 16-byte aligned."""
    _fwd_case(K, 3, 5, 64, seed=64, we_off=which == "W_E", pos_off=which == "W_pos", out_off=which == "out")


# ================================================================================================ backward
def _bwd_case(K, tok, g, pre, family, g_dev=None):
    """One iit_embed_pos_bwd launch into prefilled gradients (``pre`` entries may be None)."""
    B, S, d = g.shape
    got = {k: (None if v is None else v.to(dev)) for k, v in pre.items()}
    K.embed_pos_bwd(tok.to(dev), g.to(dev) if g_dev is None else g_dev, got["dWE"], got["dWpos"], B, S, d)
    torch.cuda.synchronize()
    got = {k: (None if v is None else v.cpu()) for k, v in got.items()}
    ref = X.embed_bwd_ref(tok, g, pre["dWE"], pre["dWpos"])
    bad = _count(X.embed_bwd_check(got, ref, pre, family))
    assert not bad, (B, S, d, bad)


def _operands(family, B, S, d, seed, pos_rows=None):
    g = X.operand(family, (B, S, d), F32, seed, B * S + 1)
    pre = {"dWE": X.operand(family, (VOCAB, d), F32, seed + 1, 1),
           "dWpos": X.operand(family, (pos_rows or S + 2, d), F32, seed + 2, 1)}
    return g, pre


@pytest.mark.parametrize("family", X.FAMILIES)
@pytest.mark.parametrize("pattern", X.EMBED_PATTERNS)
@pytest.mark.parametrize("B", [1, 7, 8, 9, 31, 32, 33, 65])
def test_embed_bwd(K, B, pattern, family):
    for S, d in SD:
        g, pre = _operands(family, B, S, d, seed=B + d)
        _bwd_case(K, X.embed_tokens(pattern, B, S, VOCAB), g, pre, family)


@pytest.mark.parametrize("family", X.FAMILIES)
@pytest.mark.parametrize("missing", ["dWE", "dWpos"])
def test_embed_bwd_one_gradient_only(K, missing, family):
    for B, S, d in ((33, 3, 66), (9, 1, 256)):
        g, pre = _operands(family, B, S, d, seed=B)
        pre[missing] = None
        _bwd_case(K, X.embed_tokens("runs", B, S, VOCAB), g, pre, family)


@pytest.mark.parametrize("family", X.FAMILIES)
@pytest.mark.parametrize("B", [1, 3, 4, 5, 9])
@pytest.mark.parametrize("d", [4, 252, 256, 260, 768])
def test_pos_bwd_vec(K, d, B, family):
    g, pre = _operands(family, B, 3, d, seed=d + B)
    pre["dWE"] = None
    _bwd_case(K, X.embed_tokens("equal", B, 3, VOCAB), g, pre, family)


@pytest.mark.parametrize("family", X.FAMILIES)
@pytest.mark.parametrize("d", [1, 3, 66, 255, 257, 64])
def test_pos_bwd_scalar(K, d, family):
    """d % 4 != 0, and d = 64 with the gradient a view offset by one float."""
    for B in (1, 5):
        g, pre = _operands(family, B, 3, d, seed=d + B)
        pre["dWE"] = None
        _bwd_case(K, X.embed_tokens("equal", B, 3, VOCAB), g, pre, family, g_dev=_offset_view(g) if d == 64 else None)
