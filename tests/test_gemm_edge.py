"""The ragged-N variant of the LDS-DMA GEMM (csrc/gemm_edge.hip) on the GPU, element by element.

For every edge-capable tile: N = BN + r for r in {1, 7, 8, 9, 81} and 2 BN - 1, M = BM and 2 BM, K = 2 BK and 3 BK;
the forward layout (mode 2) with the fp32-store + bias and the bf16 + bias epilogues, the weight-gradient layout
(mode 3) with fp32 store and fp32 accumulate, both with the fused column sums ``bsum`` and the store also with the sum
of squares ``gsq``.  Operands are small integers (tests/gemm_exact_util.py): results are compared bitwise.  Row pads of
every operand are NaN, every operand's last row is followed by a NaN-filled neighbour, outputs are pre-filled and
everything outside the [M][N] result must keep its bits (tests/gemm_edge_util.py).  The dispatcher must offer the
whole ragged problem on these tiles beside the bulk + tail split, and every such candidate must be exact.
"""
import pytest
import torch

import gemm_edge_util as E
from iit_amd.ops import hip_kernels as HK

pytestmark = pytest.mark.gpu
dev = "cuda"

EPILOGUES = [(E.MODE_BKM, E.EPI_F32_STORE), (E.MODE_BKM, E.EPI_BF16), (E.MODE_3, E.EPI_F32_STORE),
             (E.MODE_3, E.EPI_F32_ACC)]


@pytest.fixture(scope="module")
def K():
    HK.lib()
    old = HK.CHECK_BOUNDS
    HK.CHECK_BOUNDS = True  # host-side extent check of every raw-pointer operand before each launch
    yield HK
    HK.CHECK_BOUNDS = old


def test_tiles_match_the_library(K):
    edge = K.tile_table("edge")  # the library's own rows
    assert tuple(sorted(E.EDGE_TILES)) == tuple(sorted(K.GLDS_EDGE_TILES)) == tuple(sorted(edge))
    for t, (bm, bn) in E.EDGE_TILES.items():
        assert K.GLDS_TILES[t] == (bm, bn) == (edge[t]["bm"], edge[t]["bn"]) and edge[t]["bk"] == E.BK
    assert (E.MODE_BKM, E.MODE_3, E.EPI_BF16, E.EPI_F32_ACC, E.EPI_F32_STORE) == (
        K.MODE_BKM, K.MODE_AKM | K.MODE_BKM, K.EPI_BF16, K.EPI_F32_ACC, K.EPI_F32_STORE)


@pytest.mark.parametrize("mode,epi", EPILOGUES)
@pytest.mark.parametrize("tile", sorted(E.EDGE_TILES))
def test_n_edge_exact(K, tile, mode, epi):
    errs = []
    for i, (M, N, Kd) in enumerate(E.edge_shapes(tile)):
        c = E.make_case(mode, epi, M, N, Kd, 1000 * tile + 10 * i, dev)
        kw = dict(M=M, N=N, K=Kd, lda=c["lda"], ldb=c["ldb"], ldc=c["ldc"], mode=mode, epi=epi, bias0=c["bias0"],
                  tile=tile)
        assert K.gemm_glds_edge_ok(c["A"], c["B"], c["C"], **kw), (tile, M, N, Kd)
        K.gemm_glds_edge(c["A"], c["B"], c["C"], bsum=c["bsum"], gsq=c["gsq"], **kw)
        torch.cuda.synchronize()
        errs += E.check_case(c, f"tile {tile} mode {mode} epi {epi} M {M} N {N} K {Kd}")
    assert not errs, errs[:5]


def test_refusals(K):
    """What the variant does not cover is refused on the host, never launched."""
    c = E.make_case(E.MODE_BKM, E.EPI_F32_STORE, 128, 129, 128, 5, dev)
    kw = dict(M=128, N=129, K=128, lda=c["lda"], ldb=c["ldb"], ldc=c["ldc"], mode=E.MODE_BKM, epi=E.EPI_F32_STORE)
    assert K.gemm_glds_edge_ok(c["A"], c["B"], c["C"], tile=25, **kw)
    assert not K.gemm_glds_edge_ok(c["A"], c["B"], c["C"], tile=9, **kw)  # not an edge tile
    assert not K.gemm_glds_edge_ok(c["A"], c["B"], c["C"], tile=7, **kw)  # M % 256
    assert not K.gemm_glds_edge_ok(c["A"], c["B"], c["C"], tile=25, **{**kw, "K": 96})
    assert not K.gemm_glds_edge_ok(c["A"], c["B"], c["C"], tile=25, **{**kw, "ldb": 128})  # rows shorter than pad8(N)
    assert not K.gemm_glds_edge_ok(c["A"], c["B"], c["C"], tile=25, **{**kw, "mode": 0})
    assert not K.gemm_glds_edge_ok(c["A"], c["B"], c["C"], tile=25, **{**kw, "epi": K.EPI_GELU})
    with pytest.raises(RuntimeError):
        K.gemm_glds_edge(c["A"], c["B"], c["C"], tile=9, **kw)


@pytest.mark.parametrize("mode,epi", [(E.MODE_BKM, E.EPI_F32_STORE), (E.MODE_3, E.EPI_F32_STORE)])
def test_dispatcher_offers_the_whole_ragged_problem(K, mode, epi):
    """``_candidates`` of a ragged problem holds one ``glds{tile}e`` per edge tile, each exact with its fused sums."""
    from iit_amd.ops import gemm_dispatch as gd
    M, N, Kd = 256, 128 + 81, 128
    names = None
    for tile in sorted(E.EDGE_TILES):
        c = E.make_case(mode, epi, M, N, Kd, 77, dev)
        calls = gd._candidates(c["A"], c["B"], c["C"], None, M, N, Kd, c["lda"], c["ldb"], c["ldc"], mode, epi,
                               c["bias0"], None, None, None, 0, None, 0, 0, (0, 0, 0), None, None, "auto")
        names = sorted(n for n in calls if n.endswith("e"))
        assert names == sorted(f"glds{t}e" for t in E.EDGE_TILES), sorted(calls)
        calls[f"glds{tile}e"](c["C"], None, None, bs=c["bsum"], sq=c["gsq"])
        torch.cuda.synchronize()
        errs = E.check_case(c, f"glds{tile}e")
        assert not errs, errs


def test_shipped_table_runs_the_headline_unembed_whole(K, monkeypatch):
    """The table's "edge" section sends the headline forward unembed (256 x 50257, K = 768), which its "ragged"
    section splits, to ONE launch of the ragged-N kernel; the result is the split path's bit for bit, and
    ``IIT_GEMM_TAIL_LIBRARY`` (or a missing entry) keeps bulk + tail."""
    from iit_amd.ops import gemm_dispatch as gd
    V, Vp, d, T = 50257, 50264, 768, 256
    rkey = (T, V, d, K.MODE_BKM, K.EPI_F32_STORE, True, False, gd.deterministic())
    assert gd._ragged_table().get(repr(rkey)) is True
    assert gd._edge_table().get(repr(rkey)) in {f"glds{t}e" for t in K.GLDS_EDGE_TILES}
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(T, d, device=dev, generator=g).bfloat16()
    W = torch.full((d, Vp), float("nan"), device=dev, dtype=torch.bfloat16)
    W[:, :V] = (torch.randn(d, V, device=dev, generator=g) / 16).bfloat16()
    b = torch.randn(V, device=dev, generator=g)
    kw = dict(M=T, N=V, K=d, lda=d, ldb=Vp, ldc=Vp, mode=K.MODE_BKM, epi=K.EPI_F32_STORE, bias0=b)
    launches = []
    real = K.gemm_glds_edge
    monkeypatch.setattr(K, "gemm_glds_edge", lambda *a, **k: (launches.append(k["tile"]), real(*a, **k)))
    C = torch.full((T, Vp), 7.0, device=dev)
    assert gd.gemm(x, W, C, **kw) == gd._edge_table()[repr(rkey)] and len(launches) == 1
    monkeypatch.setattr(gd, "_TAIL_LIBRARY", True)
    C2 = torch.full((T, Vp), 7.0, device=dev)
    gd.gemm(x, W, C2, **kw)
    assert len(launches) == 1  # bulk + tail this time
    torch.cuda.synchronize()
    assert torch.equal(C, C2) and bool((C[:, V:] == 7.0).all())
    exp = x.float() @ W[:, :V].float() + b
    assert ((C[:, :V] - exp).norm() / exp.norm()).item() < 1e-2
