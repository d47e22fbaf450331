"""Exact element-wise tests of the GEMM kernels (csrc/gemm_glds*.{hip,h}, gemm_dual.hip, gemm_8ph.hip, gemm_4w.hip,
gemm.hip): every tile x layout x epilogue, every K-loop length around the LDS ring depth, every tile order, the dual
launch with unequal problems and with prefetch workgroups, the older kernel on ragged shapes, and every candidate the
dispatcher offers for reduced step shapes.

Operands are small integers (tests/gemm_exact_util.py; the exactness conditions are checked on the CPU in
tests/test_gemm_exact_ref.py), so fp32 outputs are compared bitwise with the exact result, bf16 outputs bitwise with
the exact result rounded once, and only the GELU epilogues use a bound.  Every operand and output has its own padded
leading dimension; outputs are pre-filled with NaN (fp32) or a sentinel (bf16) and the padding must keep those bits.
"""
import os
from types import SimpleNamespace

import pytest
import torch

import gemm_exact_util as U
from iit_amd.ops import hip_kernels as HK

pytestmark = pytest.mark.gpu
dev = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
GELUS, DGELUS = (HK.EPI_GELU, HK.EPI_GELU_ERF), (HK.EPI_DGELU, HK.EPI_DGELU_ERF)
ERF = (HK.EPI_GELU_ERF, HK.EPI_DGELU_ERF)


@pytest.fixture(scope="module")
def K():
    HK.lib()
    old = HK.CHECK_BOUNDS
    HK.CHECK_BOUNDS = True  # host-side extent check of every raw-pointer operand before each launch
    yield HK
    HK.CHECK_BOUNDS = old


def _lds(widths):
    """One leading dimension per width: a multiple of 8 elements, padded, all distinct."""
    out = []
    for i, w in enumerate(widths):
        ld = (w + 7) // 8 * 8 + 8 * (i + 1)
        while ld in out:
            ld += 8 * (len(widths) + 1)
        out.append(ld)
    assert len(set(out)) == len(out)
    return out


def _bk(tile: int) -> int:
    return 128 if 15 <= tile <= 18 else 64  # tiles 15-18 take 128-deep K-tiles


def _first(bad: torch.Tensor):
    return tuple(int(v) for v in bad.nonzero()[0])


def _case(K, mode, epi, M, N, Kd, seed, bias=True):
    """One GEMM problem ``C = A @ B (+ epilogue)``: operands in the layout of ``mode`` (bf16, or fp32 where the mode
    says so), the epilogue's operands, pre-filled outputs and the exact check of what a launch left in them."""
    assert Kd in U.K_USED, Kd
    gelu, dg = epi in GELUS, epi in DGELUS
    amax, bmax = (U.UNIT_MAX, U.UNIT_MAX) if gelu else (U.A_MAX, U.B_MAX)
    akm, bkm = bool(mode & K.MODE_AKM), bool(mode & K.MODE_BKM)
    lda, ldb, ldc, ldc2, ldr = _lds([M if akm else Kd, N if bkm else Kd, N, N, N])
    a = U.ints((M, Kd), -amax, amax, seed, dev)
    b = U.ints((Kd, N), -bmax, bmax, seed + 1, dev)
    c = SimpleNamespace(M=M, N=N, K=Kd, epi=epi, mode=mode)
    c.A = U.padded(a.t() if akm else a, lda, F32 if mode & K.MODE_AF32 else BF16)
    c.B = U.padded(b if bkm else b.t(), ldb, F32 if mode & K.MODE_BF32 else BF16)
    prod = U.exact_mm(a, b)
    init = U.ints((M, N), -U.ADD_MAX, U.ADD_MAX, seed + 2, dev) if epi == K.EPI_F32_ACC else None
    c.C, c.C0 = U.out_buffer(M, N, ldc, F32 if epi in (K.EPI_F32_RESID, K.EPI_F32_ACC, K.EPI_F32_STORE) else BF16, dev,
                             init)
    c.kw = dict(M=M, N=N, K=Kd, lda=lda, ldb=ldb, ldc=ldc, mode=mode, epi=epi)
    c.bias = [None, None, None]
    c.bias_cols = c.ldr = c.ldc2 = 0
    c.resid = c.C2 = c.C20 = c.pre = None
    bvec = resid = None
    if epi == K.EPI_BF16_BIAS3:
        c.bias_cols = (N + 2) // 3
        c.bias = [U.ints((c.bias_cols,), -U.BIAS_MAX, U.BIAS_MAX, seed + 10 + i, dev) for i in range(3)]
        bvec = torch.cat(c.bias)[:N]
    elif bias and not dg and epi != K.EPI_F32_ACC:
        bvec = c.bias[0] = U.ints((N,), -U.BIAS_MAX, U.BIAS_MAX, seed + 10, dev)
    if epi == K.EPI_F32_RESID:
        resid = U.ints((M, N), -U.ADD_MAX, U.ADD_MAX, seed + 3, dev)
        c.resid, c.ldr = U.padded(resid, ldr), ldr
    if gelu:
        c.C2, c.C20 = U.out_buffer(M, N, ldc2, BF16, dev)
        c.ldc2 = ldc2
    if dg:  # the saved pre-activation: random bf16
        g = torch.Generator(device=dev).manual_seed(seed + 4)
        pre = torch.randn(M, N, device=dev, generator=g).bfloat16()
        c.pre, c.ldc2 = U.padded(pre, ldc2), ldc2

    def reset():
        c.C.copy_(c.C0)
        if c.C2 is not None:
            c.C2.copy_(c.C20)

    def check(tag="", bf16_product=False, zeroed=False):
        """``bf16_product``: the implementation rounds the product to bf16 before the fp32 additions (the documented
        definition of the dispatcher's ``blas16``); ``zeroed``: C was zeroed before an accumulate."""
        torch.cuda.synchronize()
        got = c.C[:, :N]
        lin = prod.bfloat16().float() if bf16_product else prod
        for t in (bvec, resid, None if zeroed else init):
            if t is not None:
                lin = lin + t
        if c.C.dtype == F32:
            bad = U.bad_f32(got, lin)
        elif gelu:
            bad = U.bad_gelu(got, lin, epi in ERF)
            bad2 = U.bad_bf16(c.C2[:, :N], lin)
            assert not bad2.any(), f"{tag}: {int(bad2.sum())} of {bad2.numel()} stored pre-activations wrong"
            assert U.padding_touched(c.C2, c.C20, N) == 0, f"{tag}: padding of the pre-activation buffer written"
        elif dg:
            bad = U.bad_dgelu(got, prod, pre, epi in ERF)
        else:
            bad = U.bad_bf16(got, lin)
        assert not bad.any(), (f"{tag}: {int(bad.sum())} of {bad.numel()} elements wrong, first at {_first(bad)}: "
                               f"got {got[bad][:4].tolist()}, exact {lin[bad][:4].tolist()}")
        assert U.padding_touched(c.C, c.C0, N) == 0, f"{tag}: padding of C written"

    c.reset, c.check = reset, check
    return c


def _glds_args(c):
    """The epilogue operands of ``c`` as ``gemm_glds`` / ``gemm_glds_ok`` take them."""
    ok = dict(C2=c.pre if c.pre is not None else c.C2, resid=c.resid, ldc2=c.ldc2, ldr=c.ldr, bias_cols=c.bias_cols)
    run = dict(ok, bias0=c.bias[0], bias1=c.bias[1], bias2=c.bias[2])
    return ok, run


# what ``gemm_glds_ok`` refuses of the cases below, by (tile, mode): tile 20 with a k-contiguous A -- these tests found
# its mode 0 / 2 kernels wrong (one 16-row fragment per wave row: csrc/gemm_glds.hip says why), and it now serves the
# weight gradients only.  Such a case is skipped, never forced; any other refusal fails.
REFUSED = {(20, 0), (20, 2)}


def _glds_launch(K, c, tile, tag, extra=None):
    ok, run = _glds_args(c)
    if not K.gemm_glds_ok(c.A, c.B, c.C, tile=tile, **c.kw, **ok):
        assert (tile, c.mode) in REFUSED, f"gemm_glds_ok refuses tile {tile} for {c.kw}"
        pytest.skip(f"gemm_glds_ok refuses tile {tile} in mode {c.mode} (offered for weight gradients only)")
    assert (tile, c.mode) not in REFUSED, f"tile {tile} is offered in mode {c.mode} again: csrc/gemm_glds.hip"
    K.gemm_glds(c.A, c.B, c.C, tile=tile, **c.kw, **run, **(extra or {}))
    c.check(tag)


# ------------------------------------------------------------------------------ A: layout x epilogue, every tile
GLDS_CASES = [(0, 0), (0, 5), (0, 7), (2, 0), (2, 1), (2, 2), (2, 3), (2, 8), (2, 5), (2, 7), (3, 5), (3, 7),
              (0, 4), (0, 9)]  # CASES of tests/test_gemm_glds.py + the DGELU epilogues


@pytest.mark.parametrize("tile", sorted(HK.GLDS_TILES))
@pytest.mark.parametrize("mode,epi", GLDS_CASES)
def test_glds_layout_epilogue_matrix_exact(K, mode, epi, tile):
    """5 x 3 = 15 output tiles (no multiple of the 8 XCDs, a 4 + 1 partial group at the shipped height), 3 K-tiles;
    with the fused sums where the epilogue has them: ``bsum`` (mode 3, bitwise), ``gsq`` and ``csum`` (the
    tolerances of tests/test_gemm_dual.py)."""
    bm, bn = K.GLDS_TILES[tile]
    M, N, Kd = 5 * bm, 3 * bn, 3 * _bk(tile)
    assert (M // bm) * (N // bn) % 8 != 0 and (M // bm) % K.GEMM_GROUP_M != 0
    c = _case(K, mode, epi, M, N, Kd, 1000 * tile + 10 * mode + epi, bias=mode != 3)
    extra, bs0 = {}, None
    if mode == 3:
        bs0 = U.ints((N,), -U.ADD_MAX, U.ADD_MAX, tile + 77, dev)
        extra["bsum"] = bs0.clone()
        if epi == K.EPI_F32_STORE:
            extra["gsq"] = torch.zeros(64, device=dev)
    if epi in DGELUS:
        cs0 = U.ints((N,), -U.ADD_MAX, U.ADD_MAX, tile + 78, dev)
        extra["csum"] = cs0.clone()
    _glds_launch(K, c, tile, f"tile {tile}", extra)
    if mode == 3:
        colsum = c.B[:, :N].double().sum(0).float()  # B is dY [K][N]
        assert not U.bad_f32(extra["bsum"], bs0 + colsum).any(), "bsum"
        if "gsq" in extra:
            torch.testing.assert_close(extra["gsq"].sum(), c.C[:, :N].double().pow(2).sum().float(), rtol=1e-4,
                                       atol=1e-2)
    if epi in DGELUS:
        torch.testing.assert_close(extra["csum"], cs0 + c.C[:, :N].float().sum(0), rtol=1e-4, atol=1e-2)


# ------------------------------------------------------------------------------ B: K-loop length vs ring depth
@pytest.mark.parametrize("tile", sorted(HK.GLDS_TILES))
@pytest.mark.parametrize("mode", [0, 2, 3])
def test_glds_k_loop_length_exact(K, mode, tile):
    """1 to 9 K-tiles: shorter than, equal to and longer than every LDS ring depth (2 to 8) -- the ``nt < NS`` paths
    of the prologue and of the counted waits."""
    bm, bn = K.GLDS_TILES[tile]
    for nt in range(1, 10):
        c = _case(K, mode, K.EPI_F32_STORE, 2 * bm, bn, nt * _bk(tile), 100 * tile + 10 * nt + mode, bias=mode != 3)
        _glds_launch(K, c, tile, f"tile {tile}, {nt} K-tiles")


# ------------------------------------------------------------------------------ C: tile order
GRIDS = [(1, 1), (1, 9), (9, 1), (5, 3), (11, 3), (8, 8), (13, 5)]  # (tiles_m, tiles_n)
HEIGHTS = [1, 2, 3, 4, 8, 16]


def _loaded(var: str, default: int) -> int:
    """The group height ``hip_kernels.lib()`` set when it loaded the library."""
    v = os.environ.get(var, str(default))
    return int(v) if v else 0


def test_shipped_group_heights(K):
    assert (K.GEMM_GROUP_M, K.GEMM_DUAL_GROUP_M) == (4, 2)


@pytest.mark.parametrize("tile", [3, 30])
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_glds_tile_order_exact(K, grid, tile):
    """``xcd_remap`` with tile counts that are no multiple of 8 and ``grouped_tile`` with full, partial and
    single-row groups: every output tile is computed exactly once, by the workgroup that holds its operands."""
    bm, bn = K.GLDS_TILES[tile]
    assert (bm, bn) == (64, 64)
    c = _case(K, K.MODE_BKM, K.EPI_F32_STORE, grid[0] * bm, grid[1] * bn, 64, 7 * grid[0] + grid[1] + tile)
    try:
        for gm in HEIGHTS:
            K.gemm_glds_set_group_m(gm)
            c.reset()
            _glds_launch(K, c, tile, f"grid {grid}, group height {gm}")
    finally:
        K.gemm_glds_set_group_m(_loaded("IIT_GEMM_GROUP_M", K.GEMM_GROUP_M))


# ------------------------------------------------------------------------------ dual launches (C, D, E)
def _dual(K, wt, xt, wepi, xepi, splits, reduce, wgrid=(2, 3), xgrid=(5, 2), Kw=None, Kx=448, seed=0):
    """Two independent problems for one dual launch: dW = X^T dY ([Kw][Mw] and [Kw][Nw] operands, fp32 store /
    accumulate, ``bsum`` and ``gsq``) and dX = dY' W^T ([Mx][Kx] and [Nx][Kx] operands, bf16 or DGELU + ``csum``),
    with unequal dims and seven distinct padded leading dimensions."""
    (wbm, wbn), (xbm, xbn) = K.DUAL_W_TILES[wt], K.DUAL_X_TILES[xt]
    Mw, Nw, Mx, Nx = wgrid[0] * wbm, wgrid[1] * wbn, xgrid[0] * xbm, xgrid[1] * xbn
    Kw = Kw or {1: 576, 2: 896, 4: 768}[splits]
    assert Kw in U.K_USED and Kx in U.K_USED and Kw % (64 * splits) == 0
    wlda, wldb, wldc, xlda, xldb, xldc, xldc2 = _lds([Mw, Nw, Nw, Kx, Kx, Nx, Nx])
    d = SimpleNamespace(splits=splits, reduce=reduce, Mw=Mw, Nw=Nw, wt=wt, xt=xt)
    xa = U.ints((Kw, Mw), -U.A_MAX, U.A_MAX, seed + 1, dev)
    dy = U.ints((Kw, Nw), -U.B_MAX, U.B_MAX, seed + 2, dev)
    ax = U.ints((Mx, Kx), -U.A_MAX, U.A_MAX, seed + 3, dev)
    bx = U.ints((Kx, Nx), -U.B_MAX, U.B_MAX, seed + 4, dev)
    prodw, prodx = U.exact_mm(xa.t(), dy), U.exact_mm(ax, bx)
    initw = U.ints((Mw, Nw), -U.ADD_MAX, U.ADD_MAX, seed + 5, dev) if wepi == K.EPI_F32_ACC else None
    wC, wC0 = U.out_buffer(Mw, Nw, wldc, F32, dev, initw)
    xC, xC0 = U.out_buffer(Mx, Nx, xldc, BF16, dev)
    bs0 = U.ints((Nw,), -U.ADD_MAX, U.ADD_MAX, seed + 6, dev)
    bsum, gsq = bs0.clone(), torch.zeros(64, device=dev)
    pre = prebuf = csum = cs0 = None
    if xepi == K.EPI_DGELU:
        g = torch.Generator(device=dev).manual_seed(seed + 7)
        pre = torch.randn(Mx, Nx, device=dev, generator=g).bfloat16()
        prebuf = U.padded(pre, xldc2)
        cs0 = U.ints((Nx,), -U.ADD_MAX, U.ADD_MAX, seed + 8, dev)
        csum = cs0.clone()
    d.w = dict(A=U.padded(xa, wlda, BF16), B=U.padded(dy, wldb, BF16), C=wC, M=Mw, N=Nw, K=Kw, lda=wlda, ldb=wldb,
               ldc=wldc, epi=wepi, bsum=bsum, gsq=gsq)
    d.x = dict(A=U.padded(ax, xlda, BF16), B=U.padded(bx.t(), xldb, BF16), C=xC, C2=prebuf, M=Mx, N=Nx, K=Kx,
               lda=xlda, ldb=xldb, ldc=xldc, ldc2=xldc2 if prebuf is not None else 0, epi=xepi, csum=csum)
    assert K.gemm_dual_ok(d.w, d.x, wt, xt, splits, reduce), f"gemm_dual_ok refuses pair ({wt}, {xt})"

    def reset():
        wC.copy_(wC0)
        xC.copy_(xC0)
        bsum.copy_(bs0)
        gsq.zero_()
        if csum is not None:
            csum.copy_(cs0)

    def run(prefetch=None):
        K.gemm_dual(d.w, d.x, wt, xt, splits, reduce, prefetch=prefetch)

    def tickets():
        return K.split_workspace(Mw, Nw, K.DUAL_W_TILES[wt], splits, wC.device)[1]

    def check(tag=""):
        torch.cuda.synchronize()
        bad = U.bad_f32(wC[:, :Nw], prodw + (initw if initw is not None else 0))
        assert not bad.any(), f"{tag}: dW {int(bad.sum())} of {bad.numel()} wrong, first at {_first(bad)}"
        assert not U.bad_f32(bsum, bs0 + dy.double().sum(0).float()).any(), f"{tag}: bsum"
        if wepi == K.EPI_F32_STORE:
            torch.testing.assert_close(gsq.sum(), wC[:, :Nw].double().pow(2).sum().float(), rtol=1e-4, atol=1e-3)
        else:
            assert float(gsq.abs().sum()) == 0.0, f"{tag}: gsq written by an accumulate"
        if xepi == K.EPI_DGELU:
            bad = U.bad_dgelu(xC[:, :Nx], prodx, pre, False)
            torch.testing.assert_close(csum, cs0 + xC[:, :Nx].float().sum(0), rtol=1e-4, atol=1e-2)
        else:
            bad = U.bad_bf16(xC[:, :Nx], prodx)
        assert not bad.any(), f"{tag}: dX {int(bad.sum())} of {bad.numel()} wrong, first at {_first(bad)}"
        assert U.padding_touched(wC, wC0, Nw) == 0 and U.padding_touched(xC, xC0, Nx) == 0, f"{tag}: padding written"
        if reduce:
            assert int(tickets().abs().sum()) == 0, f"{tag}: reduction tickets not re-armed"

    def outputs():
        """Everything that must not depend on the launch geometry, bit for bit (``csum`` / ``gsq`` are fp32 atomics
        of non-integers: their order may differ)."""
        torch.cuda.synchronize()
        return [wC.clone(), xC.clone(), bsum.clone()]

    d.reset, d.run, d.check, d.outputs, d.tickets = reset, run, check, outputs, tickets
    return d


def _same(xs, ys) -> bool:
    return all(not U.bad_bits(x, y).any() for x, y in zip(xs, ys))


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_dual_tile_order_exact(K, grid):
    """The dual launch's group height (``iit_gemm_dual_set_group_m``) on the same grids, both problems: the 64 x 64
    dW tile and the 64 x 96 dX tile, one K-tile each."""
    d = _dual(K, 4, 1, K.EPI_F32_STORE, K.EPI_BF16, 1, False, wgrid=grid, xgrid=grid, Kw=64, Kx=64,
              seed=grid[0] * 16 + grid[1])
    try:
        for gm in HEIGHTS:
            K.gemm_dual_set_group_m(gm)
            d.reset()
            d.run()
            d.check(f"grid {grid}, group height {gm}")
    finally:
        K.gemm_dual_set_group_m(_loaded("IIT_GEMM_DUAL_GROUP_M", K.GEMM_DUAL_GROUP_M))


# D: every pair and variant of tests/test_gemm_dual.py
PAIRS = ([(wt, xt) for wt in range(5) for xt in range(4)] + [(wt, xt) for wt in (5, 6) for xt in (4, 5, 6)]
         + [(wt, xt) for wt in (7, 8) for xt in (7, 8)])
VARIANTS = [("store", "bf16", 1, False), ("store", "dgelu", 2, True), ("acc", "bf16", 4, True),
            ("acc", "dgelu", 2, False)]


def _epis(K, wepi_s, xepi_s):
    return (K.EPI_F32_STORE if wepi_s == "store" else K.EPI_F32_ACC, K.EPI_BF16 if xepi_s == "bf16" else K.EPI_DGELU)


@pytest.mark.parametrize("wt,xt", PAIRS)
@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: f"{v[0]}-{v[1]}-{'r' if v[3] else 'k'}{v[2]}")
def test_dual_exact(K, wt, xt, variant):
    """dW 2 x 3 tiles over 576 / 896 / 768 tokens, dX 5 x 2 tiles over K = 448: M, N and K differ within each
    problem and K between them, and all seven leading dimensions differ, so an ``lda`` / ``ldb`` / ``ldc`` or an M / N
    taken from the wrong place shows.  Two launches: the second runs on the
    tickets the first re-armed."""
    wepi_s, xepi_s, splits, reduce = variant
    wepi, xepi = _epis(K, wepi_s, xepi_s)
    d = _dual(K, wt, xt, wepi, xepi, splits, reduce, seed=100 * wt + 10 * xt)
    dims = [d.w["M"], d.w["N"], d.w["K"], d.x["M"], d.x["N"], d.x["K"]]
    assert d.w["M"] != d.w["N"] != d.w["K"] and d.x["M"] != d.x["N"] != d.x["K"] and d.w["K"] != d.x["K"], dims
    for rep in range(2):
        d.reset()
        d.run()
        d.check(f"pair ({wt}, {xt}), launch {rep}")


# E: prefetch workgroups
@pytest.fixture(scope="module")
def prefetch_sets():
    """name -> (tensors to prefetch, their clones)."""
    def t(nbytes, seed):
        n = nbytes // 2
        return (torch.arange(n, device=dev, dtype=torch.int32) % (251 + seed)).to(BF16)

    sets = {"256B": (t(256, 0), None), "1MiB+3MiB": (t(2 ** 20, 1), t(3 * 2 ** 20, 2)), "cap": (t(65 * 2 ** 20, 3),),
            "32mod64": (t(2 ** 17 + 32, 4),)}
    return {k: (v, tuple(None if x is None else x.clone() for x in v)) for k, v in sets.items()}


def test_prefetch_byte_counts_are_whole_granules(K, prefetch_sets):
    """The prefetch workgroups load 4 bytes at the start of every 64-byte granule, so ``_prefetch_args`` passes whole
    granules only and drops a range that holds none."""
    t33 = torch.zeros(33, device=dev, dtype=BF16)  # 66 bytes
    assert K._prefetch_args((t33,))[:4] == (t33.data_ptr(), 64, None, 0)
    t16 = torch.zeros(16, device=dev, dtype=BF16)  # 32 bytes: no whole granule
    assert K._prefetch_args((t16,)) == (None, 0, None, 0, 0)
    assert K._prefetch_args((t16, t33))[:4] == (t33.data_ptr(), 64, None, 0)
    (odd,), _ = prefetch_sets["32mod64"]
    nb = odd.numel() * odd.element_size()
    assert nb % 64 == 32 and K._prefetch_args((odd,))[:2] == (odd.data_ptr(), nb - 32)
    (big,), _ = prefetch_sets["cap"]
    a, b = prefetch_sets["1MiB+3MiB"][0]
    assert K._prefetch_args((a, b))[:4] == (a.data_ptr(), 2 ** 20, b.data_ptr(), 3 * 2 ** 20)
    small = prefetch_sets["256B"][0]
    assert K._prefetch_args(small)[:4] == (small[0].data_ptr(), 256, None, 0)
    if K._PF_PER_MB == 16:  # the shipped workgroups per MiB: the floor of 8, 16 per MiB, the cap
        assert [K._prefetch_args(p)[4] for p in ((t33,), small, (a, b), (big,))] == [8, 8, 64, 1024]


@pytest.mark.parametrize("wt,xt", [(1, 3), (5, 5), (7, 7), (3, 1), (0, 1)])
@pytest.mark.parametrize("split", [False, True], ids=["plain", "r2"])
def test_dual_prefetch_exact(K, prefetch_sets, wt, xt, split):
    """The launch with prefetch workgroups (every tile's block index shifted by their count) gives the bits of the
    launch without them and of the exact reference, leaves the prefetched tensors alone, and replays from a graph."""
    wepi, xepi = _epis(K, *(("acc", "dgelu") if split else ("store", "bf16")))
    d = _dual(K, wt, xt, wepi, xepi, 2 if split else 1, split, seed=1000 + 100 * wt + 10 * xt)
    d.run()
    d.check("no prefetch")
    base = d.outputs()
    for name, (pf, clones) in prefetch_sets.items():
        d.reset()
        d.run(pf)
        d.check(name)
        assert _same(d.outputs(), base), f"{name}: differs from the launch without prefetch"
        d.reset()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            d.run(pf)
        for rep in range(2):
            d.reset()
            g.replay()
            assert _same(d.outputs(), base), f"{name}: graph replay {rep} differs"
            if split:
                assert int(d.tickets().abs().sum()) == 0, f"{name}: tickets after replay {rep}"
        assert all(x is None or torch.equal(x, y) for x, y in zip(pf, clones)), f"{name}: prefetched tensor changed"


# ------------------------------------------------------------------------------ F: the older kernel (csrc/gemm.hip)
HIP_COMBOS = ([(0, e) for e in (0, 1, 2, 3, 8, 4, 9, 7, 5)] + [(2, e) for e in (0, 1, 2, 3, 8, 7, 5)]
              + [(4, e) for e in (0, 4, 5, 7)] + [(1, 5), (3, 5), (3, 6), (3, 7), (11, 5)])  # (mode, epilogue)
# ragged shapes; 2000 x 1890 is 16 x 15 = 240 tiles of 128 x 128, the size at which ``_tiling`` leaves the 64-wide path
HIP_SHAPES = [(32, 128, 512), (200, 130, 72), (256, 81, 768), (2000, 1890, 64)]
HIP_SPLIT_SHAPE = (64, 96, 1024)  # accumulate epilogues: the automatic split-K factor is 2 here, 1 on the shapes above
HIP_PARAMS = [(s, m, e) for s in HIP_SHAPES for m, e in HIP_COMBOS if e != HK.EPI_F32_ACC_QKV or s[1] % 3 == 0] + \
             [(HIP_SPLIT_SHAPE, m, e) for m, e in HIP_COMBOS if e in (HK.EPI_F32_ACC, HK.EPI_F32_ACC_QKV)]


def _hip_qkv(K, mode, M, N, Kd, seed, splits):
    """The head-blocked QKV scatter: column w * H * dh + h * dh + j of row r is added to element [h][r][j] of the
    w-th of three [H][M][dh] buffers (N = 3 H dh)."""
    dh = next(x for x in (63, 9, 8) if N % (3 * x) == 0)
    H = N // (3 * dh)
    c = _case(K, mode, K.EPI_F32_ACC, M, N, Kd, seed)  # operands only
    prod = U.exact_mm(c.A[:, :M].float().t(), c.B[:, :N].float())
    n, guard = H * M * dh, 64
    bufs, inits = [], []
    for w in range(3):
        buf = torch.full((n + guard,), U.F32_FILL, device=dev)
        inits.append(U.ints((n,), -U.ADD_MAX, U.ADD_MAX, seed + 20 + w, dev))
        buf[:n] = inits[w]
        bufs.append(buf)
    kw = dict(c.kw, epi=K.EPI_F32_ACC_QKV)
    K.gemm(c.A, c.B, bufs[0], C2=bufs[1], C3=bufs[2], qkv=(dh, H, M), splits=splits, **kw)
    torch.cuda.synchronize()
    for w in range(3):
        exp = inits[w] + prod[:, w * H * dh:(w + 1) * H * dh].reshape(M, H, dh).permute(1, 0, 2).reshape(-1)
        bad = U.bad_f32(bufs[w][:n], exp)
        assert not bad.any(), f"buffer {w}, splits {splits}: {int(bad.sum())} of {n} wrong"
        assert torch.isnan(bufs[w][n:]).all(), f"buffer {w}: written past its end"


@pytest.mark.parametrize("shape,mode,epi", HIP_PARAMS,
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_hip_kernel_exact(K, shape, mode, epi):
    """Every (layout, epilogue) the older kernel dispatches, fp32-operand modes included (integers convert to bf16
    exactly), on ragged M / N / K, with one split and with the automatic split-K factor."""
    M, N, Kd = shape
    assert K._tiling(M, N, Kd, False)[0] == (1 if shape == HIP_SHAPES[3] else 0)
    can_split = epi in (K.EPI_F32_ACC, K.EPI_F32_ACC_QKV)
    auto = K._tiling(M, N, Kd, can_split)[1]
    assert auto == (2 if shape == HIP_SPLIT_SHAPE else 1)
    seed = 31 * mode + epi + M
    for splits in ((1, None) if can_split and auto != 1 else (None,)):
        if epi == K.EPI_F32_ACC_QKV:
            _hip_qkv(K, mode, M, N, Kd, seed, splits)
            continue
        c = _case(K, mode, epi, M, N, Kd, seed)
        K.gemm(c.A, c.B, c.C, C2=c.C2, bias0=c.bias[0], bias1=c.bias[1], bias2=c.bias[2], resid=c.resid, ldr=c.ldr,
               aux=c.pre, ldc2=c.ldc2, bias_cols=c.bias_cols, splits=splits, **c.kw)
        c.check(f"splits {splits}")


# ------------------------------------------------------------------------------ G: every dispatcher candidate
STEP_SHAPES = {  # reduced step shapes (M, N, K, mode, epilogue): at most 1024 x 1152 x 512, none square
    "qkv_fwd": (512, 1152, 256, HK.MODE_BKM, HK.EPI_BF16_BIAS3),  # packed QKV, three biases
    "resid_fwd": (512, 384, 512, HK.MODE_BKM, HK.EPI_F32_RESID),
    "gelu_fwd": (512, 768, 256, HK.MODE_BKM, HK.EPI_GELU),  # with the pre-activation store
    "dx_bf16": (768, 384, 512, HK.MODE_NN, HK.EPI_BF16),
    "dw_fresh": (384, 768, 512, HK.MODE_AKM | HK.MODE_BKM, HK.EPI_F32_STORE),  # fresh=True: the z+ candidates too
}


@pytest.mark.parametrize("name", list(STEP_SHAPES))
def test_dispatcher_candidates_exact(K, name):
    """Every implementation ``gemm_dispatch`` would time for the problem gives the exact result.  ``blas16`` is by
    definition a bf16-output library GEMM plus one fp32 add pass: its product is the exact one rounded once to bf16,
    and it is held to exactly that."""
    from iit_amd.ops import gemm_dispatch as gd
    M, N, Kd, mode, epi = STEP_SHAPES[name]
    assert M <= 1024 and N <= 1152 and Kd <= 512 and M != N
    fresh = name == "dw_fresh"
    c = _case(K, mode, epi, M, N, Kd, 4242 + M + N, bias=name not in ("dx_bf16", "dw_fresh"))

    def cands(e):
        return gd._candidates(c.A, c.B, c.C, c.C2, M, N, Kd, c.kw["lda"], c.kw["ldb"], c.kw["ldc"], mode, e,
                              *(c.bias if e == epi else [None] * 3), c.resid, c.ldr, None, c.ldc2, c.bias_cols,
                              (0, 0, 0), None, None, "auto")

    calls = dict(cands(epi))
    assert "hip" in calls and "blas" in calls and sum(n.startswith("glds") for n in calls) >= 8, sorted(calls)
    if fresh:  # as gemm(fresh=True) builds them: zero C, then any accumulate candidate
        for n, f in cands(K.EPI_F32_ACC).items():
            calls["z+" + n] = lambda C, C2, C3, f=f: (C[:, :N].zero_(), f(C, C2, C3))
        assert any(n.startswith("z+glds") and "r" in n for n in calls) and any("k" in n for n in calls), sorted(calls)
    for n, f in calls.items():
        c.reset()
        f(c.C, c.C2, None)
        c.check(f"candidate {n}", bf16_product=n.endswith("blas16"), zeroed=n.startswith("z+"))
