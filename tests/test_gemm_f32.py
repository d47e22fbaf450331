"""Element-wise tests of the exact-fp32 MFMA GEMM (csrc/gemm_f32.hip): every tile x layout x epilogue, with and
without bias, on the three exact operand families of tests/gemm_f32_util.py (compared bitwise; the exactness
conditions are checked on the CPU in tests/test_gemm_f32_ref.py), deterministic split-K including empty trailing
splits, and standard-normal operands against float64 with the bound of ``gemm_f32_util.bad_real``.

Every operand and output has its own padded leading dimension (a multiple of 4); fp32 outputs and every operand's
padding are pre-filled with NaN and the padding must keep its bits.
"""
from types import SimpleNamespace

import pytest
import torch

import gemm_exact_util as U
import gemm_f32_util as F
from iit_amd.ops import hip_kernels as HK

pytestmark = pytest.mark.gpu
dev = "cuda"
TILES = sorted(HK.GEMM_F32_TILES)
EPI_BIAS = [(HK.EPI_F32_STORE, False), (HK.EPI_F32_STORE, True), (HK.EPI_F32_RESID, False), (HK.EPI_F32_RESID, True),
            (HK.EPI_F32_ACC, False)]
# (M, N, K): one tile, ragged edges, 2 x 2 and more tiles of either size; every K of gemm_f32_util.K_USED.
# 11 sizes and 4 families per case: the (case, family) pairs walk through all of them
SIZES = [(1, 1, 1), (17, 65, 3), (64, 64, 32), (65, 17, 33), (130, 130, 64), (64, 130, 96), (130, 65, 257),
         (65, 64, 1024), (1, 130, 257), (130, 1, 33), (17, 17, 1024)]
assert {s[2] for s in SIZES} == set(F.K_USED)


@pytest.fixture(scope="module")
def K():
    HK.lib()
    old = HK.CHECK_BOUNDS
    HK.CHECK_BOUNDS = True  # host-side extent check of every raw-pointer operand before each launch
    yield HK
    HK.CHECK_BOUNDS = old


def _first(bad):
    return tuple(int(v) for v in bad.nonzero()[0])


def _case(K, family, mode, epi, M, N, Kd, seed, bias=True):
    """One problem ``C = A @ B (+ epilogue)`` with operands in the layout of ``mode``, NaN-padded, and its checks."""
    akm, bkm = bool(mode & K.MODE_AKM), bool(mode & K.MODE_BKM)
    lda, ldb, ldc, ldr = F.lds([M if akm else Kd, N if bkm else Kd, N, N])
    a, b = F.operands(family, M, N, Kd, seed, dev)
    real = family == F.REAL
    c = SimpleNamespace(M=M, N=N, K=Kd, family=family)
    c.A = U.padded(a.t() if akm else a, lda)
    c.B = U.padded(b if bkm else b.t(), ldb)
    g = torch.Generator().manual_seed(seed + 1)

    def extra(shape, amax):
        if real:
            return torch.randn(shape, generator=g).to(dev)
        return torch.randint(-amax, amax + 1, shape, generator=g).float().to(dev)

    init = extra((M, N), U.ADD_MAX) if epi == K.EPI_F32_ACC else None
    c.bias = extra((N,), U.BIAS_MAX) if bias and epi != K.EPI_F32_ACC else None
    resid = extra((M, N), U.ADD_MAX) if epi == K.EPI_F32_RESID else None
    c.resid = None if resid is None else U.padded(resid, ldr)
    c.C, c.C0 = U.out_buffer(M, N, ldc, torch.float32, dev, init)
    c.kw = dict(M=M, N=N, K=Kd, lda=lda, ldb=ldb, ldc=ldc, mode=mode, epi=epi, bias=c.bias, resid=c.resid,
                ldr=ldr if resid is not None else 0)
    if real:
        ref, mag = F.real_reference(a, b, c.bias, resid if resid is not None else init)
    else:
        ref = U.exact_mm(a, b)
        for t in (c.bias, resid, init):
            if t is not None:
                ref = ref + t

    def run(tile, splits=1):
        c.C.copy_(c.C0)
        assert K.gemm_f32_ok(c.A, c.B, c.C, tile=tile, splits=splits, **c.kw), (tile, splits, c.kw)
        K.gemm_f32(c.A, c.B, c.C, tile=tile, splits=splits, **c.kw)
        torch.cuda.synchronize()
        return c.C[:, :N].clone()

    def check(tag, splits=1):
        got = c.C[:, :N]
        if real:
            ratio = F.real_ratio(got, ref, mag, Kd, splits)
            print(f"{tag}: worst |got - ref| / bound = {ratio.max().item():.4f}")
            bad = F.bad_real(got, ref, mag, Kd, splits)
        else:
            bad = U.bad_f32(got, ref)
        assert not bad.any(), (f"{tag}: {int(bad.sum())} of {bad.numel()} elements wrong, first at {_first(bad)}: "
                               f"got {got[bad][:4].tolist()}, reference {ref[bad][:4].tolist()}")
        assert U.padding_touched(c.C, c.C0, N) == 0, f"{tag}: padding of C written"

    c.run, c.check = run, check
    return c


@pytest.mark.parametrize("epi,bias", EPI_BIAS)
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("tile", TILES)
def test_every_tile_mode_epilogue(K, tile, mode, epi, bias):
    ci = (TILES.index(tile) * 4 + mode) * len(EPI_BIAS) + EPI_BIAS.index((epi, bias))
    for fi, family in enumerate(F.EXACT):
        M, N, Kd = SIZES[(ci * len(F.EXACT) + fi) % len(SIZES)]
        c = _case(K, family, mode, epi, M, N, Kd, seed=1000 + 10 * ci + fi, bias=bias)
        c.run(tile)
        c.check(f"tile {tile} mode {mode} epi {epi} bias {bias} {family} {M}x{N}x{Kd}")


def test_sizes_cover_every_tile():
    """The walk of ``test_every_tile_mode_epilogue`` gives every tile every size and every family every K."""
    per_tile = {t: set() for t in TILES}
    per_family = {f: set() for f in F.EXACT}
    for ci in range(len(TILES) * 4 * len(EPI_BIAS)):
        for fi, family in enumerate(F.EXACT):
            s = SIZES[(ci * len(F.EXACT) + fi) % len(SIZES)]
            per_tile[TILES[ci // (4 * len(EPI_BIAS))]].add(s)
            per_family[family].add(s[2])
    assert all(v == set(SIZES) for v in per_tile.values())
    assert all(v == set(F.K_USED) for v in per_family.values())


# K = 33 with 7 (and 64) splits: the K range of a split is a whole K-tile, so all but two splits are empty
SPLIT_SIZES = [(65, 130, 33), (130, 65, 257), (17, 64, 1024), (64, 17, 96)]


@pytest.mark.parametrize("splits", [2, 3, 7, 64])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("tile", TILES)
def test_split_k(K, tile, mode, splits):
    ci = (TILES.index(tile) * 4 + mode) * 4 + [2, 3, 7, 64].index(splits)
    for si, (M, N, Kd) in enumerate(SPLIT_SIZES):
        epi, bias = EPI_BIAS[(ci + si) % len(EPI_BIAS)]
        family = F.EXACT[(ci + si) % len(F.EXACT)]
        tag = f"tile {tile} mode {mode} epi {epi} bias {bias} {family} {M}x{N}x{Kd} splits {splits}"
        c = _case(K, family, mode, epi, M, N, Kd, seed=5000 + 10 * ci + si, bias=bias)
        one = c.run(tile, 1)
        c.check(tag + " (unsplit)")
        first = c.run(tile, splits)
        c.check(tag)
        again = c.run(tile, splits)
        assert not U.bad_bits(again, first).any(), f"{tag}: two identical launches differ"
        assert not U.bad_bits(first, one).any(), f"{tag}: differs from the unsplit launch"


def test_splits_1_and_7_agree_on_every_epilogue(K):
    for tile in TILES:
        for i, (epi, bias) in enumerate(EPI_BIAS):
            c = _case(K, F.EXACT[1 + i % 3], 2, epi, 65, 130, 257, seed=7000 + i, bias=bias)
            one, seven = c.run(tile, 1), c.run(tile, 7)
            c.check(f"tile {tile} epi {epi} splits 7")
            assert not U.bad_bits(seven, one).any(), (tile, epi, bias)


@pytest.mark.parametrize("splits", [1, 4])
@pytest.mark.parametrize("Kd", F.K_REAL)
@pytest.mark.parametrize("mode", [0, 2, 3])
@pytest.mark.parametrize("tile", TILES)
def test_real_valued_against_float64(K, tile, mode, Kd, splits):
    for epi, bias in ((K.EPI_F32_RESID, True), (K.EPI_F32_ACC, False)):
        c = _case(K, F.REAL, mode, epi, 65, 130, Kd, seed=9000 + mode + Kd, bias=bias)
        first = c.run(tile, splits)
        c.check(f"real tile {tile} mode {mode} epi {epi} K {Kd} splits {splits}", splits)
        assert not U.bad_bits(c.run(tile, splits), first).any(), "two identical launches differ"


def test_refusals(K):
    """A leading dimension of 6, a pointer offset by 4 bytes and a bf16 operand are refused, and ``gemm_f32`` raises
    for them without launching (C keeps its NaN prefill)."""
    M = N = Kd = 8
    a = torch.ones(M * 8 + 4, device=dev)
    b = torch.ones(N * 8 + 4, device=dev)
    C, C0 = U.out_buffer(M, N, 8, torch.float32, dev)
    good = dict(M=M, N=N, K=Kd, lda=8, ldb=8, ldc=8, mode=0, epi=K.EPI_F32_STORE)
    assert K.gemm_f32_ok(a, b, C, **good)
    bad_cases = {
        "lda 6": (a, b, dict(good, K=6, lda=6)),
        "ldb 6": (a, b, dict(good, K=6, ldb=6)),
        "A offset by 4 bytes": (a[1:], b, good),
        "B offset by 4 bytes": (a, b[1:], good),
        "bf16 A": (a.bfloat16(), b, good),
        "bf16 B": (a, b.bfloat16(), good),
        "65 splits": (a, b, dict(good, splits=65)),
        "unknown tile": (a, b, dict(good, tile=len(TILES))),
    }
    for name, (A, B, kw) in bad_cases.items():
        assert not K.gemm_f32_ok(A, B, C, **kw), name
        with pytest.raises(RuntimeError):
            K.gemm_f32(A, B, C, **kw)
    # the C entry point itself refuses too (an error code, no launch)
    rc = K.lib().iit_gemm_f32(a.data_ptr() + 4, b.data_ptr(), C.data_ptr(), None, None, None, 8, 8, 8, 0, M, N, Kd, 0,
                              K.EPI_F32_STORE, 0, 1, torch.cuda.current_stream().cuda_stream)
    assert rc != 0
    torch.cuda.synchronize()
    assert not U.bad_bits(C, C0).any(), "a refused problem wrote C"
    K.gemm_f32(a, b, C, **good)
    torch.cuda.synchronize()
    assert torch.equal(C, torch.full_like(C, float(Kd)))
