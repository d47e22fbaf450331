"""CPU proof of the comparators of tests/misc_exact_util.py, no GPU needed.

* The bounds are not tighter than the arithmetic: an fp32 torch emulation of each bounded kernel's own expression, with
  its sums in a deliberately bad order, passes its comparator on every family with no bad element.
* Every listed perturbation is flagged: an element moved by twice its bound, a dropped last row or column group, a row
  added twice, a run of equal tokens that loses its first row after a chunk boundary, an untouched tail of d % 4
  columns, a transposed tile written untransposed, a zero one past a range, a span updated at ``start4`` where
  ``local4`` was meant.  The ``1 - 2 rcp(exp(2u) + 1)`` form of gelu_new is flagged by the bound of the sigmoid form
  from x = -4 down (159 inputs, the worst 255 times the bound at x = -4.97: the very figures the kernel gave on an
  MI355X), which is why the stand-alone kernels now share ``gelu_new_f``.
* The ``exact`` families' sums stay below 2^24 at the shapes the GPU modules use.
"""
import pytest
import torch

import misc_exact_util as X

F32, BF16 = torch.float32, torch.bfloat16


def _count(bad: dict) -> dict:
    return {n: int(m.sum()) for n, m in bad.items() if int(m.sum())}


def _twice(ref: torch.Tensor, tol: torch.Tensor, i) -> torch.Tensor:
    """fp32 image of ``ref`` with element ``i`` moved by twice its bound (plus the fp32 spacing, so the move survives
    the rounding)."""
    got = ref.float().clone()
    got[i] = (ref[i] + 2 * tol[i] + 4 * X.E * ref[i].abs() + 2 * X.TINY).float()
    return got


# ================================================================================================ embedding
@pytest.mark.parametrize("family", X.FAMILIES)
@pytest.mark.parametrize("pattern", X.EMBED_PATTERNS)
def test_embed_bwd_emulation_passes_and_lost_rows_are_flagged(pattern, family):
    B, S, d, vocab = 65, 3, 5, 200
    tok = X.embed_tokens(pattern, B, S, vocab)
    g = X.operand(family, (B, S, d), F32, 1, B * S + 1)
    pre = {"dWE": X.operand(family, (vocab, d), F32, 2, 1), "dWpos": X.operand(family, (S + 2, d), F32, 3, 1)}
    ref = X.embed_bwd_ref(tok, g, pre["dWE"], pre["dWpos"])
    pos = pre["dWpos"].clone()
    for b in range(B - 1, -1, -1):
        pos[:S] = pos[:S] + g[b]
    got = {"dWE": X.embed_bwd_emul(tok, g, pre["dWE"]), "dWpos": pos}
    assert not _count(X.embed_bwd_check(got, ref, pre, family))
    assert int((ref["n_we"] == 0).sum()) and int((ref["n_pos"] == 0).sum()) == 2
    if pattern != "distinct":  # (all distinct: no run continues over a chunk boundary)
        lost = {"dWE": X.embed_bwd_emul(tok, g, pre["dWE"], bug="chunk_first_lost"), "dWpos": pos}
        assert _count(X.embed_bwd_check(lost, ref, pre, family)), "chunk_first_lost"
    zero = {"dWE": X.embed_bwd_emul(tok, g, pre["dWE"], bug="reset_zero"), "dWpos": pos}
    assert _count(X.embed_bwd_check(zero, ref, pre, family)), "reset_zero"
    touched = {"dWE": got["dWE"].clone(), "dWpos": pos}  # one element of a row that receives no term
    dead = int((ref["n_we"][:, 0] == 0).nonzero()[0])
    touched["dWE"][dead, 1] += 1.0
    assert _count(X.embed_bwd_check(touched, ref, pre, family)) == {"dWE": 1}


def test_embed_bwd_moved_element_is_flagged():
    tok = X.embed_tokens("runs", 33, 2, 50)
    g = X.operand("random", (33, 2, 4), F32, 4, 0)
    pre = {"dWE": torch.randn(50, 4, generator=X.gen(5)), "dWpos": torch.randn(2, 4, generator=X.gen(6))}
    ref = X.embed_bwd_ref(tok, g, pre["dWE"], pre["dWpos"])
    got = {"dWE": _twice(ref["dWE"], ref["tol_dWE"], (3, 1)), "dWpos": _twice(ref["dWpos"], ref["tol_dWpos"], (1, 2))}
    assert _count(X.embed_bwd_check(got, ref, pre, "random")) == {"dWE": 1, "dWpos": 1}


@pytest.mark.parametrize("d", [1, 3, 66, 255])
def test_embed_fwd_untouched_tail_is_flagged(d):
    """What the float4 kernel leaves of d % 4 != 0: the last d % 4 columns of every row keep the prefill."""
    g = X.gen(d)
    tok = torch.randint(0, 9, (3, 5), generator=g)
    WE, Wpos = torch.randn(9, d, generator=g), torch.randn(7, d, generator=g)
    ref = X.embed_fwd_ref(tok, WE, Wpos, 5)
    assert ref.shape == (15, d)
    got = X.filled((15, d), F32)
    got[:, :d - d % 4] = ref[:, :d - d % 4]
    assert int(X.bad_bits(got, ref).sum()) == 15 * (d % 4)
    assert not int(X.bad_bits(ref.clone(), ref).sum())


# ================================================================================================ column sums
@pytest.mark.parametrize("order", ["reversed", "pairwise"])
@pytest.mark.parametrize("family", X.FAMILIES)
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("T,N", [(1, 8), (129, 65), (300, 16), (1990, 8)])
def test_colsum_bound_holds_for_bad_orders(T, N, dtype, family, order):
    x = X.operand(family, (T, N), dtype, T, T + 1)
    out0 = X.operand(family, (N,), F32, N, 1)
    ref = X.colsum_ref(x, out0)
    got = X.colsum_emul(x, out0, order)
    assert not int(X.bad_sum(got, ref["out"], ref["tol"], family).sum())


@pytest.mark.parametrize("family", X.FAMILIES)
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_colsum_perturbations_are_flagged(dtype, family):
    T, N = 129, 24
    x = X.operand(family, (T, N), dtype, 11, T + 1)
    x[T - 1] = x[T - 1].float().abs().clamp(min=1.0).to(dtype)  # the last row is no row of zeros
    x[5] = x[T - 1]
    out0 = X.operand(family, (N,), F32, 12, 1)
    ref = X.colsum_ref(x, out0)
    check = lambda got: int(X.bad_sum(got, ref["out"], ref["tol"], family).sum())  # noqa: E731
    assert not check(X.colsum_emul(x, out0, "reversed"))
    assert check(X.colsum_emul(x[:T - 1], out0, "reversed")) == N, "dropped last row"
    assert check(X.colsum_emul(torch.cat([x, x[5:6]]), out0, "reversed")) == N, "row added twice"
    group = X.colsum_emul(x, out0, "reversed")
    group[N - 8:] = out0[N - 8:]
    assert check(group) == 8, "dropped last column group"
    if family == "random":
        assert check(_twice(ref["out"], ref["tol"], 7)) == 1


@pytest.mark.parametrize("family", X.FAMILIES)
@pytest.mark.parametrize("M,N", [(1, 1), (3, 2047), (2, 2049), (5, 4100), (2100, 8)])
def test_sumsq_2d_bound_holds_and_perturbations_are_flagged(M, N, family):
    if family == "exact":
        c = X.int_operand((M, N), F32, M, 1, lim=X.sumsq_lim(M, N))
        g0 = torch.full((64,), float(X.sumsq_lim(M, N)) ** 2)
    else:
        c = torch.randn(M, N, generator=X.gen(M))
        g0 = torch.rand(64, generator=X.gen(N))
    c[M - 1, N - 1] = c[M - 1, N - 1].abs().clamp(min=1.0)
    ref = X.sumsq_ref(c, g0)
    check = lambda got: int(X.bad_sum(got, ref["gsq"], ref["tol"], family, g0, ref["n"]).sum())  # noqa: E731
    got = X.sumsq_emul(c, g0)
    assert not check(got)
    assert int((ref["n"] == 0).sum()) == max(0, 64 - X.sumsq_plan(M, N)[1])
    if family == "exact":
        assert float(ref["gsq"].max()) < 2 ** 24
        drop = c.clone()
        drop[M - 1, N - 1] = 0.0
        assert check(X.sumsq_emul(drop, g0)) == 1, "dropped last element"
    else:
        assert check(_twice(ref["gsq"], ref["tol"], 0)) == 1
    if X.sumsq_plan(M, N)[1] < 64:
        got[63] = 0.0
        assert check(got) == 1, "slot past the block count touched"


# ================================================================================================ GELU
def test_gelu_bounds_hold_for_fp32_emulation_over_every_bf16_value():
    x = X.gelu_inputs()
    assert X.all_bf16().numel() == 42754 and x.numel() == X.GELU_N == 21 * 2048 == 6144 * 7
    for kind, form in (("new", "sig"), ("erf", "erf")):
        ref = X.gelu_ref(x, kind)
        bad = X.bad_bound(X.gelu_emul(x, form), ref["y"], ref["tol"])
        assert not int(bad.sum()), (kind, x[bad][:8])
        for dpost in (torch.ones_like(x), -torch.ones_like(x), torch.randn(x.shape, generator=X.gen(1)).bfloat16()):
            r = X.dgelu_ref(dpost, x, kind)
            bad = X.bad_bound(X.dgelu_emul(dpost, x, kind), r["y"], r["tol"])
            assert not int(bad.sum()), (kind, x[bad][:8])


def test_gelu_new_tanh_form_misses_the_bound_in_the_negative_tail():
    """``0.5 x (1 + (1 - 2 rcp(exp(2u) + 1)))`` cancels where tanh(u) -> -1: from x = -4 down its error exceeds the
    bound of the sigmoid form; at every x > -3.5 it is inside."""
    x = X.all_bf16()
    ref = X.gelu_ref(x, "new")
    bad = X.bad_bound(X.gelu_emul(x, "tanh"), ref["y"], ref["tol"])
    assert int(bad.sum()) > 100
    assert float(x[bad].float().max()) <= -3.5
    assert int((bad & (x.float() <= -4.0) & (x.float() >= -8.0)).sum()) > 50


@pytest.mark.parametrize("kind", X.GELU_KINDS)
def test_gelu_moved_element_is_flagged(kind):
    """The bf16 neighbour two steps away (each step is 2 U |ref| or more, the bound about U |ref|) and a derivative
    moved by 2.5 bounds."""
    x = torch.tensor([-3.0, -0.5, 0.25, 2.0, 9.0]).bfloat16()
    ref = X.gelu_ref(x, kind)
    r = X.dgelu_ref(torch.ones_like(x), x, kind)
    assert not int(X.bad_bound(ref["y"].float().bfloat16(), ref["y"], ref["tol"]).sum())
    for i in range(x.numel()):
        got = ref["y"].float().bfloat16()
        got.view(torch.int16)[i] += 2
        flagged = X.bad_bound(got, ref["y"], ref["tol"])
        assert bool(flagged[i]) and int(flagged.sum()) == 1, (kind, i)
        dgot = r["y"].float()
        dgot[i] = float(r["y"][i] + 2.5 * r["tol"][i])
        assert bool(X.bad_bound(dgot, r["y"], r["tol"])[i]), (kind, i)
    tail = X.gelu_ref(torch.tensor([-6.0]).bfloat16(), "new")  # gelu_new: the bound stays relative in the tail
    assert float(tail["tol"][0]) < 1.01 * X.U * abs(float(tail["y"][0]))


# ================================================================================================ bitwise kernels
def test_add_bf16_reference_order():
    g = X.gen(3)
    base, y, bias = torch.randn(4, 9, generator=g) * 100, torch.randn(4, 9, generator=g).bfloat16(), torch.randn(
        9, generator=g) * 1e-3
    ref = X.add_bf16_ref(base, y, bias)
    other = base + (y.float() + bias)
    assert int(X.bad_bits(other, ref).sum()), "the other association differs somewhere: the order is checked"
    assert not int(X.bad_bits(X.add_bf16_ref(base, y, None), base + y.float()).sum())


@pytest.mark.parametrize("rows,cols,ld", [(31, 33, 31), (32, 32, 32), (33, 65, 40)])
def test_shadow_untransposed_tile_is_flagged(rows, cols, ld):
    src = torch.randn(1, rows, cols, generator=X.gen(rows))
    dst0 = X.filled((cols * ld + 8,), BF16)
    ref = X.shadow_expected(dst0, src, ld, True)
    assert not int(X.bad_bits(ref[:cols * ld].view(cols, ld)[:, :rows], src[0].t().bfloat16()).sum())
    assert not int(X.bad_bits(ref[cols * ld:], dst0[cols * ld:]).sum())
    if ld > rows:
        assert bool((ref[:cols * ld].view(cols, ld)[:, rows:].float() == X.BF16_FILL).all())
    assert int(X.bad_bits(X.shadow_expected(dst0, src, ld, True, wrong="untransposed"), ref).sum())


def test_shadow_plain_layout_with_heads():
    src = torch.randn(3, 4, 6, generator=X.gen(1))
    dst0 = X.filled((3 * 50,), BF16)
    ref = X.shadow_expected(dst0, src, 10, False, dst_hs=50)
    for h in range(3):
        img = ref[h * 50:h * 50 + 40].view(4, 10)
        assert not int(X.bad_bits(img[:, :6], src[h].bfloat16()).sum())
        assert bool((img[:, 6:].float() == X.BF16_FILL).all())


def test_zero_table_and_one_past_a_range():
    ranges, n = X.zero_ranges_table()
    assert len(ranges) == 4 * len(X.ZERO_LENS)
    for L in X.ZERO_LENS:
        assert sorted(a % 4 for a, k in ranges if k == L) == [0, 1, 2, 3]
    ends = [0] + [a + k for a, k in ranges]
    assert all(a >= e + 3 for (a, _), e in zip(ranges, ends)) and ends[-1] <= n
    buf0 = torch.randn(n, generator=X.gen(2))
    ref = X.zero_expected(buf0, ranges)
    assert int((ref == 0).sum()) == sum(k for _, k in ranges)
    for a, k in ranges[:8]:
        for i in (a - 1, a + k):
            got = ref.clone()
            got[i] = 0.0
            assert int(X.bad_bits(got, ref).sum()) == 1
    neg = ref.clone()
    neg[ranges[0][0]] = -0.0
    assert int(X.bad_bits(neg, ref).sum()) == 1


# ================================================================================================ spans
def test_span_emulation_passes_and_start4_offset_is_flagged():
    from kern_exact_util import ADAM_HYPER
    spans, an, sn = X.span_table()
    st = X.span_state(an, sn, 7)
    mirror0 = X.filled((an,), BF16)
    ref = X.span_ref(st, spans, 3, None, ADAM_HYPER)
    got = X.span_emul(st, spans, 3, ADAM_HYPER)
    assert not _count(X.span_check(got, st, ref, spans, mirror0))
    wrong = X.span_emul(st, spans, 3, ADAM_HYPER, wrong="start4")
    bad = _count(X.span_check(wrong, st, ref, spans, mirror0))
    assert bad.get("p") and bad.get("m") and bad.get("m_outside"), bad
    ia, il = X.span_index(spans)
    assert ia.numel() == il.numel() == 4 * sum(X.SPAN_LENS) and ia.unique().numel() == ia.numel()
    assert int(ia.max()) < an and int(il.max()) < sn
    gaps = torch.ones(sn, dtype=torch.bool)
    gaps[il] = False
    assert int(gaps.sum()) >= 4 * len(spans)


# ================================================================================================ kl_rows
@pytest.mark.parametrize("V", X.KL_V)
def test_kl_rows_bounds_hold_and_perturbations_are_flagged(V):
    a, b, cols = X.kl_inputs(V, V)
    ref = X.kl_ref(a, b)
    got = X.kl_emul(a, b)
    assert not int(X.kl_check(got, ref, cols).sum()), X.kl_check(got, ref, cols)
    assert float(ref["out"][3, 1]) == float("-inf") and float(got[3, 1]) == float("-inf")
    assert bool(torch.isfinite(ref["out"][[2, 4]][:, 2]).all()) and bool(torch.isfinite(ref["out"][4, 3]))
    for r, c in ((0, 0), (1, 3), (0, 1), (4, 2)):
        moved = got.clone()
        moved[r, c] = float(ref["out"][r, c] + 2 * ref["tol"][r, c] + 4 * X.E * ref["out"][r, c].abs() + X.TINY)
        assert bool(X.kl_check(moved, ref, cols)[r, c]), (r, c)
    if V > 1:  # b = 0 entries counted: 0 * -inf
        counted = X.kl_ref(a, b, wrong="zero_b_counted")["out"].float()
        assert bool(X.kl_check(counted, ref, cols)[2, 2])
    if V > 256:  # the last column dropped
        short = X.kl_emul(a[:, :V - 1], b[:, :V - 1])
        assert bool(X.kl_check(short, ref, cols)[1, 0])


# ================================================================================================ exact families
def test_exact_families_stay_below_2_24():
    for dtype, lim, T in ((BF16, 64, 7940), (F32, 256, 300), (F32, 256, 65 * 3)):
        x = X.int_operand((T, 8), dtype, 1, T + 1)
        assert float(x.float().abs().max()) <= lim
        assert float(x.double().abs().sum(0).max()) + lim < 2 ** 24
        assert bool((x.float() == x.float().round()).all())
    with pytest.raises(AssertionError):
        X.int_operand((4, 4), F32, 1, 2 ** 16)
    for M, N in ((1, 1), (3, 2047), (3, 2048), (2, 2049), (5, 4100), (2100, 8)):
        lim = X.sumsq_lim(M, N)
        c = torch.full((M, N), float(lim))
        assert float(X.sumsq_ref(c, torch.full((64,), float(lim * lim)))["gsq"].max()) < 2 ** 24
