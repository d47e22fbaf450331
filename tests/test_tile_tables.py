"""The tile tables of the LDS-DMA GEMM family (csrc/gemm_tiles.h), on the host: the library's exported rows against
the tables of iit_amd/ops/hip_kernels.py, the ``_ok`` predicates against the rows (so the numbers that size the
split-K tickets and the BatchNorm tile records are the numbers the kernels use), and the load-time check that refuses
a drifted Python table.  No launch, no device memory: the operand addresses are 16-byte-aligned dummies."""
import pytest

from iit_amd.ops import hip_kernels as HK

PTR, LD = 0x1000, 768
MODE_3 = HK.MODE_AKM | HK.MODE_BKM


@pytest.fixture(scope="module")
def K():
    HK.lib()
    return HK


@pytest.fixture(scope="module")
def T(K):
    return {f: K.tile_table(f) for f in K.TILE_FAMILIES}


def glds_ok(K, tile, M, N, Kd, mode=MODE_3, epi=HK.EPI_F32_STORE):
    return bool(K.lib().iit_gemm_glds_ok(PTR, PTR, PTR, None, None, LD, LD, LD, 0, 0, M, N, Kd, mode, epi, 0, tile, 1, 0))


def dual_ok(K, wt, xt, w, x):
    """``w`` / ``x``: (M, N, K) of the dW (mode 3, fp32 store) / dX (mode 0, bf16) problem"""
    return bool(K.lib().iit_gemm_dual_ok(PTR, PTR, PTR, LD, LD, LD, *w, K.EPI_F32_STORE, wt, 1, 0,
                                         PTR, PTR, PTR, None, LD, LD, LD, 0, *x, K.EPI_BF16, xt))


def test_exported_tables_equal_the_python_tables(K, T):
    pairs = lambda tiles: {t: tuple(tiles[t]) for t in tiles}
    lib_pairs = lambda f: {t: (r["bm"], r["bn"]) for t, r in T[f].items()}
    assert lib_pairs("glds") == pairs(K.GLDS_TILES)
    assert lib_pairs("edge") == {t: K.GLDS_TILES[t] for t in K.GLDS_EDGE_TILES}
    assert lib_pairs("dual_w") == pairs(K.DUAL_W_TILES) and lib_pairs("dual_x") == pairs(K.DUAL_X_TILES)
    assert lib_pairs("conv") == pairs(K.CONV_TILES) and lib_pairs("conv_wgrad") == pairs(K.CONV_WG_TILES)
    assert {t: (r["nw"], r["occ"]) for t, r in T["dual_w"].items()} == K.DUAL_W_WAVES
    assert {t: (r["nw"], r["occ"]) for t, r in T["dual_x"].items()} == K.DUAL_X_WAVES
    assert set(K.GLDS_DISPATCH_TILES) <= set(T["glds"]) and K.conv3x3_tiles() == len(T["conv"])
    for f in ("dual_w", "dual_x"):  # aux: the single-launch tile whose shape checks the pair borrows
        for t, r in T[f].items():
            g = T["glds"][r["aux"]]
            assert (g["bm"], g["bn"], g["bk"]) == (r["bm"], r["bn"], r["bk"]), (f, t)
    for t, r in T["edge"].items():  # an edge tile is the glds tile of the same id
        assert r == T["glds"][t], t
    K.check_tile_tables()


def test_glds_ok_uses_the_rows(K, T):
    assert {40, 41, 42} < set(T["glds"])  # the 256 x 256 kernels of gemm_8ph.hip / gemm_4w.hip share the ids
    for t, r in T["glds"].items():
        bm, bn, bk = r["bm"], r["bn"], r["bk"]
        assert glds_ok(K, t, bm, bn, bk), t
        assert not glds_ok(K, t, bm + 16, bn, bk), t
        assert not glds_ok(K, t, bm, bn + 16, bk), t
        assert not glds_ok(K, t, bm, bn, bk + 32), t


def test_edge_ok_uses_the_rows(K, T):
    ok = lambda t, M, Kd: bool(K.lib().iit_gemm_glds_edge_ok(PTR, PTR, PTR, None, LD, LD, LD, M, 129, Kd, MODE_3,
                                                             K.EPI_F32_STORE, t))
    for t, r in T["edge"].items():
        assert ok(t, r["bm"], r["bk"]), t
        assert not ok(t, r["bm"] + 16, r["bk"]) and not ok(t, r["bm"], r["bk"] + 32), t
    assert not ok(9, 128, 64)  # not an edge tile


def test_conv_ok_uses_the_rows(K, T):
    # 3 x 3 / stride 1 / pad 1 on 4 x 4 images: M = 16 images, K = 9 Cs
    ok = lambda t, M, Cs, Co: K.conv2d_ok(M // 16, 4, 4, Cs, 4, 4, Co, 3, 1, 1, False, t)
    for t, r in T["conv"].items():
        assert ok(t, r["bm"], r["bk"], r["bn"]), t
        assert not ok(t, r["bm"] + 16, r["bk"], r["bn"]), t
        assert not ok(t, r["bm"], r["bk"], r["bn"] + 16), t
        assert not ok(t, r["bm"], r["bk"] + 32, r["bn"]), t
    assert not ok(-1, 128, 64, 128) and not ok(len(T["conv"]), 128, 64, 128)


def test_conv_wgrad_ok_uses_the_rows(K, T):
    # M = Cout, N = 9 Cin in tiles of BN channels of one tap, K = the output pixels of ``imgs`` 4 x 4 images
    ok = lambda t, Cout, Cin, imgs=4: K.conv2d_wgrad_ok(imgs, 4, 4, Cin, 4, 4, Cout, 3, 1, 1, t, 1)
    for t, r in T["conv_wgrad"].items():
        assert ok(t, r["bm"], r["bn"]), t
        assert not ok(t, r["bm"] + 16, r["bn"]) and not ok(t, r["bm"], r["bn"] + 16), t
        assert not ok(t, r["bm"], r["bn"], imgs=6), t  # K = 96
        for cin in (64, 128, 192, 256):  # whole 64-channel K-tiles: BN alone decides
            assert ok(t, r["bm"], cin) == (cin % r["bn"] == 0), (t, cin)
    assert not ok(-1, 128, 128) and not ok(len(T["conv_wgrad"]), 128, 128)


def test_retired_and_unknown_tiles_are_refused(K, T):
    for t in (19, 35, 36, 37, -1, 43):
        assert t not in T["glds"] and t not in K.GLDS_TILES
        for mode, epi in ((MODE_3, K.EPI_F32_STORE), (K.MODE_BKM, K.EPI_BF16), (K.MODE_NN, K.EPI_BF16)):
            assert not glds_ok(K, t, 2304, 2304, 2304, mode, epi), t  # a multiple of every BM, BN and BK ever offered


def test_dual_ok_uses_the_rows_and_the_families_agree(K, T):
    W, X = T["dual_w"], T["dual_x"]
    shape = lambda r, dm=0, dn=0: (r["bm"] + dm, r["bn"] + dn, r["bk"])
    for wt, xt in ((0, 3), (5, 4), (7, 8)):  # one pair per family
        assert dual_ok(K, wt, xt, shape(W[wt]), shape(X[xt]))
        for d in ((16, 0), (0, 16)):
            assert not dual_ok(K, wt, xt, shape(W[wt], *d), shape(X[xt])), (wt, xt, d)
            assert not dual_ok(K, wt, xt, shape(W[wt]), shape(X[xt], *d)), (wt, xt, d)
    assert len(W) * len(X) == 81
    for wt in W:
        for xt in X:
            assert dual_ok(K, wt, xt, shape(W[wt]), shape(X[xt])) == K.dual_family_ok(wt, xt), (wt, xt)
    assert not dual_ok(K, 9, 0, (128, 128, 64), shape(X[0])) and not dual_ok(K, 0, -1, shape(W[0]), (128, 128, 64))


DRIFTS = [("GLDS_TILES", "glds", 9), ("DUAL_W_TILES", "dual_w", 8), ("DUAL_X_TILES", "dual_x", 4),
          ("CONV_TILES", "conv", 2), ("CONV_WG_TILES", "conv_wgrad", 3)]


@pytest.mark.parametrize("name,family,tile", DRIFTS)
def test_load_check_names_a_drifted_table(K, monkeypatch, name, family, tile):
    table = getattr(K, name)
    bm, bn = table[tile]
    monkeypatch.setattr(K, name, {**table, tile: (bm * 2, bn)})  # one BM changed
    with pytest.raises(RuntimeError, match=rf"'{family}', tile {tile}: .* has \({bm * 2}, {bn}.* has \({bm}, {bn}"):
        K.check_tile_tables()
    monkeypatch.setattr(K, name, {t: v for t, v in table.items() if t != tile})  # the row removed
    with pytest.raises(RuntimeError, match=rf"'{family}', tile {tile}: hip_kernels.py has None"):
        K.check_tile_tables()
    monkeypatch.setattr(K, name, {**table, 99: (128, 128)})  # a row the library does not have
    with pytest.raises(RuntimeError, match=rf"'{family}', tile 99: .*the library has None"):
        K.check_tile_tables()
    monkeypatch.setattr(K, name, table)
    K.check_tile_tables()


def test_load_check_covers_the_edge_ids_and_the_dual_waves(K, monkeypatch):
    monkeypatch.setattr(K, "GLDS_EDGE_TILES", (0, 7))
    with pytest.raises(RuntimeError, match="'edge', tile 25"):
        K.check_tile_tables()
    monkeypatch.setattr(K, "GLDS_EDGE_TILES", (0, 7, 25))
    monkeypatch.setattr(K, "DUAL_X_WAVES", {**K.DUAL_X_WAVES, 4: (4, 2)})
    with pytest.raises(RuntimeError, match="'dual_x', tile 4"):
        K.check_tile_tables()
