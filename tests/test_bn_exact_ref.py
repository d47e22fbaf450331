"""CPU proof of the comparators of tests/bn_exact_util.py, no GPU needed.

* The bounds are not tighter than the arithmetic: an fp32 torch emulation of each kernel's own expressions, with its
  sums in a deliberately bad order (rows last to first; pairwise), passes every comparator on every family with no bad
  element -- forward (training and eval, spliced and not), backward, the tile combine and the max pool.
* :func:`bn_exact_util.bn_plan` equals values worked out by hand: one per C in 8, 16, 64, 512, 2048, the capped grid,
  and ``rows = 0`` with ``target = 64``; the environment variables are clamped as the kernel clamps them.
* Each listed defect is flagged by the comparator that should see it, each in a fixed, named case.  Forward:
  ``moved_element``, ``drop_last`` (M % rpi != 0), ``row_twice``, ``naive_var`` (E[x^2] - mean^2 in fp32 on the
  ``offset`` family), ``pivot_unspliced`` (row 0 spliced, the finalize's pivot read from x), ``biased_running`` (no
  M / (M - 1) at M = 9), ``momentum_swapped``, ``relu_first`` (the ReLU before the residual add).  Backward:
  ``mask_sign_dy``, ``splice_kept``, ``hull8`` (a splice channel range widened to its 8-aligned hull), ``dw_stored``.
  Tile combine: ``no_cross`` (without 2 d_t S1_t), ``r_is_t`` (R taken as the tile count).  Max pool: ``last_tie``,
  ``clipped_numbering``, ``skip_nan``.
* The ``exact`` families' sums stay below 2^24 at the shapes the GPU modules use.
"""
import pytest
import torch

import bn_exact_util as X

F32, BF16 = torch.float32, torch.bfloat16
ORDERS = ["rev", "pair"]
SHAPES = [(1, 8), (9, 8), (37, 16), (300, 64), (5, 512)]


def _count(bad: dict) -> dict:
    return {n: int(m.sum()) for n, m in bad.items() if int(m.sum())}


def _twice(ref: torch.Tensor, tol: torch.Tensor, i, dtype=F32) -> torch.Tensor:
    """Image of ``ref`` in ``dtype`` with element ``i`` moved by twice its bound (plus the spacing of the type, so the
    move survives the rounding)."""
    got = ref.to(dtype).clone()
    sp = 4 * (X.E if dtype == F32 else X.U)
    got[i] = (ref[i] + 2 * tol[i] + sp * ref[i].abs() + 2.0 ** -100).to(dtype)
    return got


def _depth(M: int, C: int) -> int:
    return X.bn_plan(M, C, 8, 1024)["atomic"]


def _fwd_case(family, M, C, dtype, seed, *, training=True, res=True, relu=True, mom=0.1, nbt0=41):
    x = X.bn_x(family, M, C, dtype, seed)
    pr = X.bn_params(C, seed)
    r = torch.randn(M, C, generator=X.gen(seed + 1)).to(dtype) if res else None
    kw = dict(eps=X.BN_EPS, mom=mom, relu=relu, training=training)
    ref = X.bn_fwd_ref(x, r, pr["w"], pr["b"], pr["rm"], pr["rv"], nbt0, depth=_depth(M, C), exact=family == "exact",
                       **kw)
    return x, r, pr, kw, ref


# ================================================================================================ the plan
@pytest.mark.parametrize("M,C,rows,target,want", [
    (2049, 8, 8, 1024, dict(G=1, rpi=256, grid=2, rpt=5, atomic=270, two=268)),
    (8195, 16, 8, 1024, dict(G=2, rpi=128, grid=9, rpt=8, atomic=146, two=143)),
    (4347, 64, 8, 1024, dict(G=8, rpi=32, grid=17, rpt=8, atomic=51, two=47)),
    (1, 512, 8, 1024, dict(G=64, rpi=4, grid=1, rpt=1, atomic=14, two=12)),
    (131, 2048, 8, 1024, dict(G=256, rpi=1, grid=17, rpt=8, atomic=20, two=16)),
    (65541, 512, 8, 1024, dict(G=64, rpi=4, grid=2048, rpt=9, atomic=277, two=51)),  # the capped grid
    (4347, 64, 0, 64, dict(G=8, rpi=32, grid=46, rpt=3, atomic=49, two=42)),
])
def test_bn_plan_matches_hand_values(M, C, rows, target, want):
    assert X.bn_plan(M, C, rows, target) == want


def test_bn_plan_reads_the_environment_as_the_kernel_does(monkeypatch):
    monkeypatch.delenv("IIT_BN_ROWS", raising=False)
    monkeypatch.delenv("IIT_BN_GRID", raising=False)
    assert X.bn_plan(4347, 64) == X.bn_plan(4347, 64, 8, 1024)
    monkeypatch.setenv("IIT_BN_ROWS", "0")
    monkeypatch.setenv("IIT_BN_GRID", "64")
    assert X.bn_plan(4347, 64) == X.bn_plan(4347, 64, 0, 64)
    monkeypatch.setenv("IIT_BN_ROWS", "257")  # out of [0, 256]: the default
    monkeypatch.setenv("IIT_BN_GRID", "63")   # out of [64, 2048]: the default
    assert X.bn_plan(4347, 64) == X.bn_plan(4347, 64, 8, 1024)
    monkeypatch.setenv("IIT_BN_ROWS", "abc")  # atoi gives 0, which is in range
    monkeypatch.setenv("IIT_BN_GRID", "2048x")
    assert X.bn_plan(4347, 64) == X.bn_plan(4347, 64, 0, 2048)


def test_bn_rows_are_the_path_changes():
    assert X.bn_rows(8) == [1, 255, 256, 257, 2049, 16387, 34811]
    assert X.bn_rows(2048) == [1, 2, 9, 67, 131]
    for C in X.BN_C:
        grids = [X.bn_plan(M, C, 8, 1024)["grid"] for M in X.bn_rows(C)]
        assert {1, 2, 9, 17} <= set(grids), (C, grids)


# ================================================================================================ forward
FAM_DTYPES = [(f, d) for f in X.X_FAMILIES for d in (BF16, F32) if not (f == "offset" and d == BF16)]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("family,dtype", FAM_DTYPES,
                         ids=[f"{f}-{'bf16' if d == BF16 else 'f32'}" for f, d in FAM_DTYPES])
@pytest.mark.parametrize("M,C", SHAPES)
def test_forward_emulation_passes(M, C, family, dtype, order):
    for k, (training, res, relu, mom, nbt0) in enumerate([(True, True, True, 0.1, 41), (True, False, False, 1.0, None),
                                                          (False, True, True, 0.1, 41)]):
        x, r, pr, kw, ref = _fwd_case(family, M, C, dtype, M + C + k, training=training, res=res, relu=relu, mom=mom,
                                      nbt0=nbt0)
        got = X.bn_fwd_emul(x, x, r, pr["w"], pr["b"], pr["rm"], pr["rv"], nbt0, order=order, **kw)
        assert not _count(X.bn_fwd_check(got, ref)), (training, _count(X.bn_fwd_check(got, ref)))
        if not training:
            assert torch.equal(got["rm"], pr["rm"]) and float(ref["tol_rm"].max()) == 0.0


def test_lowvar_constant_channel_clamps_to_rsqrt_eps():
    x, r, pr, kw, ref = _fwd_case("lowvar", 37, 16, F32, 3)
    assert float(ref["rstd"][15]) == pytest.approx(X.f32(X.BN_EPS) ** -0.5, rel=1e-12)
    assert float(ref["tol_rstd"][15]) <= 3 * X.E * float(ref["rstd"][15])


def test_forward_moved_element_is_flagged():
    for dtype in (F32, BF16):
        x, r, pr, kw, ref = _fwd_case("random", 37, 16, dtype, 5)
        got = X.bn_fwd_emul(x, x, r, pr["w"], pr["b"], pr["rm"], pr["rv"], 41, order="rev", **kw)
        pos = int((ref["y"][7] > 0.1).nonzero()[0])
        got["y"] = _twice(ref["y"], ref["tol_y"], (7, pos), dtype)
        for k in ("rm", "rv"):
            got[k] = _twice(ref[k], ref["tol_" + k], 3)
        got["save"] = torch.cat([_twice(ref["mean"], ref["tol_mean"], 2), _twice(ref["rstd"], ref["tol_rstd"], 4)])
        got["nbt"] = 43
        assert _count(X.bn_fwd_check(got, ref)) == {"mean": 1, "rstd": 1, "rm": 1, "rv": 1, "y": 1, "nbt": 1}


@pytest.mark.parametrize("family", ["random", "exact"])
@pytest.mark.parametrize("bug", ["drop_last", "row_twice"])
def test_forward_lost_and_doubled_rows_are_flagged(bug, family):
    M, C = 37, 16  # rpi = 128: M % rpi != 0
    assert M % X.rpi_of(C)
    x, r, pr, kw, ref = _fwd_case(family, M, C, F32, 7)
    got = X.bn_fwd_emul(x, x, r, pr["w"], pr["b"], pr["rm"], pr["rv"], 41, order="pair", bug=bug, **kw)
    bad = _count(X.bn_fwd_check(got, ref))
    assert bad.get("mean", 0) >= C - 2 and bad.get("rstd", 0) >= C - 2 and bad.get("rv", 0) >= C - 2, bad
    if bug == "drop_last":
        assert int(X.bn_fwd_check(got, ref)["y"][M - 1].sum()) == C


def test_forward_naive_variance_is_flagged_on_offset():
    x, r, pr, kw, ref = _fwd_case("offset", 300, 64, F32, 9)
    got = X.bn_fwd_emul(x, x, r, pr["w"], pr["b"], pr["rm"], pr["rv"], 41, order="rev", bug="naive_var", **kw)
    bad = _count(X.bn_fwd_check(got, ref))
    assert bad.get("rstd", 0) >= 48 and bad.get("rv", 0) >= 48, bad


def test_forward_biased_running_variance_is_flagged_at_m9():
    x, r, pr, kw, ref = _fwd_case("random", 9, 8, F32, 11)
    got = X.bn_fwd_emul(x, x, r, pr["w"], pr["b"], pr["rm"], pr["rv"], 41, order="rev", bug="biased_running", **kw)
    assert _count(X.bn_fwd_check(got, ref)) == {"rv": 8}


def test_forward_swapped_momentum_is_flagged():
    x, r, pr, kw, ref = _fwd_case("random", 37, 16, BF16, 13)
    got = X.bn_fwd_emul(x, x, r, pr["w"], pr["b"], pr["rm"], pr["rv"], 41, order="rev", bug="momentum_swapped", **kw)
    assert _count(X.bn_fwd_check(got, ref)) == {"rm": 16, "rv": 16}


def test_forward_relu_before_residual_is_flagged():
    x, r, pr, kw, ref = _fwd_case("random", 37, 16, BF16, 15)
    got = X.bn_fwd_emul(x, x, r, pr["w"], pr["b"], pr["rm"], pr["rv"], 41, order="rev", bug="relu_first", **kw)
    bad = _count(X.bn_fwd_check(got, ref))
    assert set(bad) == {"y"} and bad["y"] > 37 * 16 // 4, bad


def _splice_case(name, dtype, seed):
    _, shape, ranges, layout = next(c for c in X.SPLICE_CASES if c[0] == name)
    N, C, H, W = shape
    M = N * H * W
    x = X.bn_x("random", M, C, dtype, seed)
    st, src4, strides = X.splice_source(shape, layout, dtype, seed)
    hit = X.rows_of(X.splice_mask(shape, ranges))
    xp = torch.where(hit, X.rows_of(src4), x)
    return shape, ranges, strides, x, xp, hit


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("name", [c[0] for c in X.SPLICE_CASES])
def test_spliced_emulation_passes_and_specs_are_as_described(name, dtype):
    shape, ranges, strides, x, xp, hit = _splice_case(name, dtype, 17)
    N, C, H, W = shape
    M = N * H * W
    dims = X.spec_dims(shape, ranges, strides)
    assert [d[0] for d in dims] == list(shape)
    assert bool(hit[0].any()) == name.startswith("pivot_in")  # row 0 inside / outside the splice
    assert all((hi - lo) % 8 for lo, hi in ranges[1]) and 0 < int(hit.sum()) < M * C
    assert int(hit.any(1).sum()) < M and not bool(hit.all(1).any())  # partial rows only: no hit byte is 0xff
    pr = X.bn_params(C, 3)
    kw = dict(eps=X.BN_EPS, mom=0.1, relu=True, training=True)
    ref = X.bn_fwd_ref(xp, None, pr["w"], pr["b"], pr["rm"], pr["rv"], 41, depth=_depth(M, C), **kw)
    got = X.bn_fwd_emul(x, xp, None, pr["w"], pr["b"], pr["rm"], pr["rv"], 41, order="rev", **kw)
    assert not _count(X.bn_fwd_check(got, ref))
    wrong = X.bn_fwd_emul(x, xp, None, pr["w"], pr["b"], pr["rm"], pr["rv"], 41, order="rev", bug="pivot_unspliced",
                          **kw)
    n_piv = int(hit[0].sum())
    bad = X.bn_fwd_check(wrong, ref)
    assert int(bad["mean"].sum()) == n_piv and bool((bad["mean"] == hit[0]).all()), "pivot_unspliced"
    # backward on the emulation's own save / y
    dy = X.bn_dy("random", M, C, dtype, 19)
    for training in (True, False):
        bref = X.bn_bwd_ref(dy, got["y"], xp, hit, got["save"], pr["w"], pr["dw0"], pr["db0"], training=training,
                            depth=_depth(M, C))
        for order in ORDERS:
            bgot = X.bn_bwd_emul(dy, got["y"], xp, hit, got["save"], pr["w"], pr["dw0"], pr["db0"], training=training,
                                 order=order)
            assert not _count(X.bn_bwd_check(bgot, bref)), (training, order)
        kept = X.bn_bwd_emul(dy, got["y"], xp, hit, got["save"], pr["w"], pr["dw0"], pr["db0"], training=training,
                             order="rev", bug="splice_kept")
        bad = _count(X.bn_bwd_check(kept, bref))
        assert set(bad) == {"dx", "dx_spliced"} and bad["dx_spliced"] > 0, ("splice_kept", bad)
        wide = X.rows_of(X.splice_mask(shape, [ranges[0], X.hull8(ranges[1]), ranges[2], ranges[3]]))
        assert int(wide.sum()) > int(hit.sum())
        hull = X.bn_bwd_emul(dy, got["y"], xp, wide, got["save"], pr["w"], pr["dw0"], pr["db0"], training=training,
                             order="rev")
        bad = _count(X.bn_bwd_check(hull, bref))
        assert set(bad) == {"dx"} and bad["dx"] > 0, ("hull8", bad)


# ================================================================================================ backward
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("family", X.DY_FAMILIES)
@pytest.mark.parametrize("M,C", SHAPES)
def test_backward_emulation_passes(M, C, family, dtype, order):
    x, r, pr, kw, ref = _fwd_case("exact" if family == "exact" else "random", M, C, dtype, M + C)
    pr = X.bn_params(C, M, exact=family == "exact")
    fwd = X.bn_fwd_emul(x, x, r, pr["w"], pr["b"], pr["rm"], pr["rv"], 41, order="rev", **kw)
    dy = X.bn_dy(family, M, C, dtype, M)
    for training, y, dw0, db0 in [(True, fwd["y"], pr["dw0"], pr["db0"]), (False, fwd["y"], None, None),
                                  (True, None, pr["dw0"], pr["db0"])]:
        bref = X.bn_bwd_ref(dy, y, x, None, fwd["save"], pr["w"], dw0, db0, training=training, depth=_depth(M, C),
                            exact=family == "exact")
        got = X.bn_bwd_emul(dy, y, x, None, fwd["save"], pr["w"], dw0, db0, training=training, order=order)
        assert not _count(X.bn_bwd_check(got, bref)), (training, _count(X.bn_bwd_check(got, bref)))
        if family == "exact":
            assert float(bref["tol_coef"][:C].max()) == 0.0
            if dw0 is not None:
                assert float(bref["tol_db"].max()) == 0.0


def _bwd_case(dtype=BF16, family="random"):
    M, C = 37, 16
    x, r, pr, kw, ref = _fwd_case("random", M, C, dtype, 21)
    fwd = X.bn_fwd_emul(x, x, r, pr["w"], pr["b"], pr["rm"], pr["rv"], 41, order="rev", **kw)
    dy = X.bn_dy(family, M, C, dtype, 23)
    bref = X.bn_bwd_ref(dy, fwd["y"], x, None, fwd["save"], pr["w"], pr["dw0"], pr["db0"], training=True,
                        depth=_depth(M, C), exact=family == "exact")
    return x, pr, fwd, dy, bref


def test_backward_mask_from_sign_of_dy_is_flagged():
    x, pr, fwd, dy, bref = _bwd_case()
    got = X.bn_bwd_emul(dy, fwd["y"], x, None, fwd["save"], pr["w"], pr["dw0"], pr["db0"], training=True, order="rev",
                        bug="mask_sign_dy")
    bad = _count(X.bn_bwd_check(got, bref))
    assert {"coef", "dx", "dres", "dw", "db"} <= set(bad), bad


def test_backward_stored_dw_is_flagged():
    x, pr, fwd, dy, bref = _bwd_case()
    got = X.bn_bwd_emul(dy, fwd["y"], x, None, fwd["save"], pr["w"], pr["dw0"], pr["db0"], training=True, order="rev",
                        bug="dw_stored")
    assert _count(X.bn_bwd_check(got, bref)) == {"dw": 16}


def test_backward_moved_element_and_lost_row_are_flagged():
    x, pr, fwd, dy, bref = _bwd_case(F32)
    got = X.bn_bwd_emul(dy, fwd["y"], x, None, fwd["save"], pr["w"], pr["dw0"], pr["db0"], training=True, order="rev")
    assert not _count(X.bn_bwd_check(got, bref))
    got["dx"] = _twice(bref["dx"], bref["tol_dx"], (5, 3))
    got["coef"] = _twice(bref["coef"], bref["tol_coef"], 17)
    got["dw"] = _twice(bref["dw"], bref["tol_dw"], 1)
    got["db"] = _twice(bref["db"], bref["tol_db"], 2)
    got["dres"][4, 4] += 1.0
    assert _count(X.bn_bwd_check(got, bref)) == {"coef": 1, "dx": 1, "dw": 1, "db": 1, "dres": 1}
    x, pr, fwd, dy, bref = _bwd_case(BF16, "exact")  # the integer sum: one lost row is a wrong integer
    lost = X.bn_bwd_emul(dy[:36], fwd["y"][:36], x[:36], None, fwd["save"], pr["w"], pr["dw0"], pr["db0"],
                         training=False, order="rev")
    nz = int((bref["dz"][36] != 0).sum())
    assert int(X.bad_bound(lost["coef"][:16], bref["coef"][:16], bref["tol_coef"][:16]).sum()) == nz > 0


# ================================================================================================ tile records
TILE_SHAPES = [(1, 64, 64), (2, 64, 64), (255, 64, 64), (256, 64, 64), (257, 128, 64), (1000, 64, 64), (8, 128, 8),
               (8, 128, 2048)]


@pytest.mark.parametrize("family", ["random", "offset"])
@pytest.mark.parametrize("T,R,C", [(1, 64, 16), (2, 64, 16), (257, 16, 16), (40, 8, 64)])
def test_tile_combine_emulation_passes_and_defects_are_flagged(T, R, C, family):
    M = T * R
    xb = X.bn_x(family, M, C, BF16, T + R)  # the kernel's activation is bf16; the records are cut from it
    cstat = X.tile_records(xb, T, R)
    pr = X.bn_params(C, 5)
    kw = dict(eps=X.BN_EPS, mom=0.1)
    ref = X.tile_ref(cstat, T, R, pr["rm"], pr["rv"], 41, **kw)
    # the combine of exact records is the statistics of the rows
    xd = xb.double()
    assert torch.allclose(ref["mean"], xd.mean(0), rtol=1e-6, atol=1e-6)
    assert torch.allclose(ref["rstd"], (xd.var(0, unbiased=False) + X.f32(X.BN_EPS)).rsqrt(), rtol=1e-4)
    for order in ORDERS:
        got = X.tile_emul(cstat, T, R, pr["rm"], pr["rv"], order=order, **kw)
        X.tile_apply(ref, xb, None, pr["w"], pr["b"], True)
        got.update(nbt=42, y=X.bn_fwd_emul(xb, xb, None, pr["w"], pr["b"], pr["rm"], pr["rv"], 41, relu=True,
                                           training=True, order="pair", **kw)["y"])
        bad = _count(X.bn_fwd_check(got, ref))
        assert not bad, (order, bad)
    if T > 1:
        for wrong in ("no_cross", "r_is_t"):
            w = X.tile_ref(cstat, T, R, pr["rm"], pr["rv"], 41, wrong=wrong, **kw)
            got = {"save": torch.cat([w["mean"], w["rstd"]]).float(), "rm": w["rm"].float(), "rv": w["rv"].float(),
                   "nbt": 42, "y": X.filled((M, C), BF16)}
            bad = _count(X.bn_fwd_check(got, ref))
            assert bad.get("rstd", 0) >= C // 2 and bad.get("rv", 0) >= C // 2, (wrong, bad)


# ================================================================================================ max pool
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("family", X.POOL_FAMILIES)
@pytest.mark.parametrize("shape", X.POOL_SHAPES)
def test_pool_references_agree_and_defects_are_flagged(shape, family, dtype):
    N, C, H, W = shape
    x = X.pool_x(family, shape, dtype, H * W + C)
    y1, t1 = X.pool_ref_torch(x)
    y2, t2 = X.pool_ref_scan(x)
    assert not int(X.bad_pool_y(y2, y1).sum()) and torch.equal(t1, t2)
    OH, OW = X.pool_out(H, W)
    assert y1.shape == (N, C, OH, OW) and int(t1.max()) <= 8
    if family == "specials":
        assert bool(torch.isnan(y1.float()).any()) or H * W == 1
        assert bool((y1.float() == -X.INF).any())
        if H * W >= 2:  # the NaN of channel 1 wins over the 100 that follows it
            assert bool(torch.isnan(y1[:, 1, 0, 0].float()).all())
            bad = X.pool_ref_scan(x, "skip_nan")
            assert int(X.bad_pool_y(bad[0], y1).sum()) > 0, "skip_nan"
    if family == "ties" and H * W > 1:
        bad = X.pool_ref_scan(x, "last_tie")
        assert int((bad[1] != t1).sum()) > 0, "last_tie"  # (the value differs only where -0 ties with +0)
    if H > 1:  # windows clipped at the top / left number their taps from 0
        bad = X.pool_ref_scan(x, "clipped_numbering")
        assert int((bad[1] != t1).sum()) > 0, "clipped_numbering"
    # backward: the emulation against a float64 scatter (one to four terms per element: exact up to the rounding)
    dy = torch.randn(N, C, OH, OW, generator=X.gen(5)).to(dtype)
    dx = X.pool_bwd_emul(dy, t1, H, W)
    assert dx.shape == (N, C, H, W) and dx.dtype == dtype
    flat = torch.zeros(N, C, H * W, dtype=torch.float64)
    ih = 2 * torch.arange(OH).view(1, 1, OH, 1) - 1 + (t1 // 3).long()
    iw = 2 * torch.arange(OW).view(1, 1, 1, OW) - 1 + (t1 % 3).long()
    flat.scatter_add_(2, (ih * W + iw).view(N, C, -1), dy.double().view(N, C, -1))
    tol = (3 * X.E + (X.U if dtype == BF16 else 0.0)) * flat.abs() + 4 * X.E * 4.0
    assert not int(X.bad_bound(dx.view(N, C, -1), flat, tol * 4).sum())
    chosen = torch.zeros(N, C, H * W, dtype=torch.bool).scatter_(2, (ih * W + iw).view(N, C, -1),
                                                                 torch.ones(N, C, OH * OW, dtype=torch.bool))
    assert not int((X.bad_bits(dx, torch.zeros_like(dx)).view(N, C, -1) & ~chosen).sum())


# ================================================================================================ exact families
def test_exact_families_stay_below_2_24_at_the_gpu_shapes():
    for C in X.BN_C:
        for M in X.bn_rows(C):
            lim = X.exact_lim(M)
            assert M * (2 * lim) ** 2 < 2 ** 24 and 1 <= lim <= 64
            x = X.bn_x("exact", min(M, 300), C, BF16, M, lim=lim)
            assert float(x.float().abs().max()) <= lim and bool((x.float() == x.float().round()).all())
    assert 65541 * (2 * 7) ** 2 < 2 ** 24  # the grid-cap case
    for T, R, C in TILE_SHAPES:
        assert T * R < 2 ** 24
    # the references assert the limit themselves: one row too many raises
    x = torch.full((4, 8), 2048.0)
    x[0] = -2048.0
    pr = X.bn_params(8, 1)
    with pytest.raises(AssertionError):
        X.bn_fwd_ref(x, None, pr["w"], pr["b"], pr["rm"], pr["rv"], 0, eps=1e-5, mom=0.1, relu=False, training=True,
                     depth=10, exact=True)
