"""CPU checks of the arithmetic tests/test_conv_f32_kernel.py rests on (helpers: tests/conv_f32_util.py).

* The index-arithmetic references equal ``F.conv2d``, ``torch.nn.grad.conv2d_input`` and ``conv2d_weight`` in float64 on
  every test shape.
* The exact families keep every sum below 2^24 on every shape and pass, so bitwise comparison is sound.
* The comparators reject wrong kernels: operands rounded to bf16 and the three-term bf16 split, an off-by-one pad, an
  input gradient without the divisibility test, a weight gradient that skips the last partial K-tile, and kh / kw
  swapped (on the non-square shape).
* An fp32 emulation of the stated chain stays inside the ``REAL`` bound on every shape, unsplit and split.
"""
import pytest
import torch
import torch.nn.functional as TF

import conv_f32_util as C
import gemm_f32_util as F

SHAPES = list(C.SHAPES)
NONSQUARE = (2, 5, 7, 8, 12, 3, 1, 1)
STRIDED = (2, 6, 6, 4, 8, 3, 2, 1)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


@pytest.mark.parametrize("shape", SHAPES)
def test_references_equal_torch_in_float64(shape):
    N, H, W, Cin, Cout, k, s, pad = shape
    x, w, dy = (t.double() for t in C.tensors(C.REAL, C.FWD, shape))
    xn, wn, dyn = _nchw(x), _nchw(w), _nchw(dy)
    y, _ = C.reference(C.FWD, shape, x, w, dy)
    dx, _ = C.reference(C.DGRAD, shape, x, w, dy)
    dw, _ = C.reference(C.WGRAD, shape, x, w, dy)
    OH, OW = C.out_hw(shape)
    assert [tuple(t.shape) for t in (y, dx, dw)] == [C.mnk(p, shape)[:2] for p in C.PASSES]
    want_y = TF.conv2d(xn, wn, stride=s, padding=pad).permute(0, 2, 3, 1).reshape(-1, Cout)
    want_dx = torch.nn.grad.conv2d_input(xn.shape, wn, dyn, stride=s, padding=pad).permute(0, 2, 3, 1).reshape(-1, Cin)
    want_dw = torch.nn.grad.conv2d_weight(xn, wn.shape, dyn, stride=s, padding=pad).permute(0, 2, 3, 1).reshape(Cout, -1)
    for got, want in ((y, want_y), (dx, want_dx), (dw, want_dw)):
        assert (got - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())


@pytest.mark.parametrize("pass_", C.PASSES)
@pytest.mark.parametrize("shape", SHAPES)
def test_sums_stay_exact(shape, pass_):
    M, N, K = C.mnk(pass_, shape)
    for family in C.EXACT:
        assert C.worst_sum(family, pass_, shape) < F.LIMIT
        x, w, dy = C.tensors(family, pass_, shape)
        for t in (x, w, dy):
            assert torch.equal(t, t.round())
        ref, mag = C.expected(family, pass_, shape)
        assert mag.max().item() <= C.worst_sum(family, pass_, shape), (family, mag.max().item())
        a, b = C.gemm_operands(pass_, shape, x, w, dy)
        assert a.shape == (M, K) and b.shape == (K, N)
        # fp32 in any order is exact, so the chain emulation is bitwise the reference, split or not
        assert not C.bad(family, C.chain_f32(a, b), ref, mag, K).any()
        assert not C.bad(family, C.chain_f32(a, b, splits=3), ref, mag, K, 3).any()


@pytest.mark.parametrize("pass_", C.PASSES)
def test_bitwise_comparator_flags_reduced_precision(pass_):
    shape = C.SPLIT_SHAPE
    K = C.mnk(pass_, shape)[2]
    for family in (C.F2, C.F3):
        a, b = C.gemm_operands(pass_, shape, *C.tensors(family, pass_, shape))
        ref, mag = C.expected(family, pass_, shape)
        frac16 = C.bad(family, F.bf16_rounded_mm(a, b), ref, mag, K).float().mean().item()
        frac3 = C.bad(family, F.bf16_split3_mm(a, b), ref, mag, K).float().mean().item()
        print(f"pass {pass_} {family}: bf16-rounded operands flagged on {frac16:.3f}, three-term split on {frac3:.3f}")
        assert frac16 > 0.5, (family, frac16)
        if family == C.F3:
            assert frac3 > 0.5, frac3


def _wrong(pass_, shape, family, **kw):
    x, w, dy = C.tensors(family, pass_, shape)
    a, b = C.gemm_operands(pass_, shape, x.double(), w.double(), dy.double(), **kw)
    return (a @ b).float()


@pytest.mark.parametrize("family", (C.F1, C.REAL))
def test_comparators_flag_wrong_indexing(family):
    def flagged(pass_, shape, got):
        ref, mag = C.expected(family, pass_, shape)
        return C.bad(family, got, ref, mag, C.mnk(pass_, shape)[2]).any().item()

    for shape in (NONSQUARE, STRIDED):
        N, H, W, Cin, Cout, k, s, pad = shape
        for pass_ in (C.FWD, C.WGRAD):
            assert not flagged(pass_, shape, _wrong(pass_, shape, family))  # the right gather passes
            assert flagged(pass_, shape, _wrong(pass_, shape, family, gather_pad=pad - 1)), (shape, pass_)
            assert flagged(pass_, shape, _wrong(pass_, shape, family, gather_pad=pad + 1)), (shape, pass_)
    for pass_ in (C.FWD, C.WGRAD):  # kh / kw swapped: the non-square input shows it
        assert flagged(pass_, NONSQUARE, _wrong(pass_, NONSQUARE, family, swap=True)), pass_
    # an input gradient without the divisibility test, on both stride-2 geometries
    for shape in (STRIDED, (2, 6, 6, 8, 16, 1, 2, 0)):
        assert not flagged(C.DGRAD, shape, _wrong(C.DGRAD, shape, family))
        assert flagged(C.DGRAD, shape, _wrong(C.DGRAD, shape, family, no_div=True)), shape
    # a weight gradient that skips the last partial K-tile (P = 70 is 2 K-tiles of 32 and 6 pixels)
    for tile, (_, _, bk) in C.TILES.items():
        x, w, dy = C.tensors(family, C.WGRAD, NONSQUARE)
        a, b = C.gemm_operands(C.WGRAD, NONSQUARE, x.double(), w.double(), dy.double())
        P = a.shape[1]
        assert P % bk != 0
        full = P // bk * bk
        assert flagged(C.WGRAD, NONSQUARE, (a[:, :full] @ b[:full]).float()), tile


@pytest.mark.parametrize("pass_", C.PASSES)
@pytest.mark.parametrize("shape", SHAPES)
def test_fp32_chain_meets_the_real_bound(shape, pass_):
    K = C.mnk(pass_, shape)[2]
    a, b = C.gemm_operands(pass_, shape, *C.tensors(C.REAL, pass_, shape))
    ref, mag = C.expected(C.REAL, pass_, shape)
    for splits, bk in ((1, 32), (3, 16)):
        got = C.chain_f32(a, b, splits, bk)
        worst = F.real_ratio(got, ref, mag, K, splits)
        worst = worst[mag > 0].max().item() if (mag > 0).any() else 0.0
        print(f"{shape} pass {pass_} splits {splits}: worst ratio {worst:.4f}")
        assert not C.bad(C.REAL, got, ref, mag, K, splits).any()
    # rounding the operands to bf16 leaves the bound on most elements
    wrong = F.bf16_rounded_mm(a, b)
    frac = C.bad(C.REAL, wrong, ref, mag, K).float().mean().item()
    if K <= 256 and (mag > 0).float().mean().item() > 0.9:
        assert frac > 0.5, (shape, pass_, frac)
