"""The fp32 block kernels on the GPU, element by element: the ``EPI_GELU`` / ``EPI_DGELU`` epilogues of
csrc/gemm_f32.hip and ``iit_ln_f32_fwd`` / ``iit_ln_f32_bwd`` / ``iit_dgelu_f32`` of csrc/block_f32.hip, against the
float64 references and bounds of tests/block_f32_util.py (proved on the CPU by tests/test_block_f32_ref.py).

GEMM epilogues: integer operands (``gemm_f32_util`` F1 scaled by 1/4, with a few one-hot rows of +-2^20), so every
accumulator -- split partials included -- is exact, ``pre = acc + bias`` is one IEEE addition that torch repeats, and
only the activation carries a bound.  The auxiliary matrix of ``EPI_DGELU`` is an input: reals over [-12, 12] and the
specials up to 2^40.
"""
import pytest
import torch

import block_f32_util as B
import gemm_exact_util as U
import gemm_f32_util as F

gpu = pytest.mark.gpu
dev = "cuda"
SHAPES = {0: (70, 76, 40), 1: (130, 132, 24)}  # partial tiles in both extents, a ragged last K-tile


@pytest.fixture(scope="module")
def K():
    from iit_amd.ops import hip_kernels
    hip_kernels.lib()
    return hip_kernels


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ================================================================================================ GEMM epilogues
def _operands(M, N, Kd, seed):
    """``a [M][K]`` (multiples of 1/4, |a| <= 3/4; rows 0..3 one-hot +-2^20), ``b [K][N]`` integers |b| <= 2."""
    a, b = F.operands(F.F1, M, N, Kd, seed)
    a = a * 0.25
    for r in range(min(4, M)):
        a[r] = 0.0
        a[r, r % Kd] = 2.0 ** 20 * (1 if r % 2 == 0 else -1)
    return a, b


def _layout(a, b, mode, K):
    akm, bkm = bool(mode & K.MODE_AKM), bool(mode & K.MODE_BKM)
    M, Kd = a.shape
    N = b.shape[1]
    lda, ldb, ldc, ldx = F.lds([M if akm else Kd, N if bkm else Kd, N, N])
    A = U.padded((a.t() if akm else a).contiguous().to(dev), lda)
    Bm = U.padded((b if bkm else b.t()).contiguous().to(dev), ldb)
    return A, Bm, dict(M=M, N=N, K=Kd, lda=lda, ldb=ldb, ldc=ldc, ldx=ldx, mode=mode)


@gpu
@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("tile", [0, 1])
def test_gemm_epi_gelu(K, tile, mode, splits):
    M, N, Kd = SHAPES[tile]
    a, b = _operands(M, N, Kd, 100 + tile)
    bias = (torch.randint(-64, 65, (N,), generator=B.gen(5)).float() / 64.0)
    A, Bm, kw = _layout(a, b, mode, K)
    C, C0 = U.out_buffer(M, N, kw["ldc"], torch.float32, dev)
    aux, aux0 = U.out_buffer(M, N, kw["ldx"], torch.float32, dev)
    kw.update(epi=K.EPI_GELU, bias=bias.to(dev), aux=aux, tile=tile, splits=splits)
    assert K.gemm_f32_ok(A, Bm, C, **kw)
    K.gemm_f32(A, Bm, C, **kw)
    torch.cuda.synchronize()
    pre = U.exact_mm(a, b) + bias  # exact accumulator, then the kernel's one addition
    assert pre.abs().max() >= 2.0 ** 20 and ((pre.abs() < 12).float().mean() > 0.85)
    assert not U.bad_bits(aux[:, :N].cpu(), pre).any()
    r = B.gelu_ref(pre)
    bad = B.bad_bound(C[:, :N].cpu(), r["y"], r["tol"])
    assert not bad.any(), (int(bad.sum()), tuple(int(v) for v in bad.nonzero()[0]))
    assert U.padding_touched(C, C0, N) == 0 and U.padding_touched(aux, aux0, N) == 0


@gpu
@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("tile", [0, 1])
def test_gemm_epi_dgelu(K, tile, mode, splits):
    M, N, Kd = SHAPES[tile]
    a, b = F.operands(F.F2, M, N, Kd, 200 + tile)
    A, Bm, kw = _layout(a, b, mode, K)
    pre = B.gelu_inputs(M * N, 6).view(M, N)
    aux = U.padded(pre.to(dev), kw["ldx"])
    aux0 = aux.clone()
    C, C0 = U.out_buffer(M, N, kw["ldc"], torch.float32, dev)
    kw.update(epi=K.EPI_DGELU, aux=aux, tile=tile, splits=splits)
    assert K.gemm_f32_ok(A, Bm, C, **kw)
    K.gemm_f32(A, Bm, C, **kw)
    torch.cuda.synchronize()
    acc = U.exact_mm(a, b)
    r = B.dgelu_ref(acc, pre)
    bad = B.bad_bound(C[:, :N].cpu(), r["y"], r["tol"])
    assert not bad.any(), (int(bad.sum()), tuple(int(v) for v in bad.nonzero()[0]))
    assert U.padding_touched(C, C0, N) == 0
    assert not U.bad_bits(aux, aux0).any()  # read only


@gpu
def test_gemm_aux_refusals(K):
    M = N = Kd = 8
    a = torch.ones(M, Kd, device=dev)
    C = torch.full((M, N), float("nan"), device=dev)
    auxbuf = torch.zeros(M * N + 8, device=dev)
    aux = auxbuf[:M * N].view(M, N)
    bias = torch.zeros(N, device=dev)
    good = dict(M=M, N=N, K=Kd, lda=8, ldb=8, ldc=8, mode=0, epi=K.EPI_GELU, aux=aux, ldx=8)
    assert K.gemm_f32_ok(a, a, C, **good) and K.gemm_f32_ok(a, a, C, **dict(good, epi=K.EPI_DGELU))
    bad_cases = {
        "missing aux": dict(good, aux=None),
        "missing aux, dgelu": dict(good, aux=None, epi=K.EPI_DGELU),
        "misaligned aux": dict(good, aux=auxbuf[1:M * N + 1].view(M, N)),
        "ldx < N": dict(good, ldx=4),
        "ldx % 4": dict(good, N=6, ldx=6),
        "bias with dgelu": dict(good, epi=K.EPI_DGELU, bias=bias),
    }
    for name, kw in bad_cases.items():
        assert not K.gemm_f32_ok(a, a, C, **kw), name
        with pytest.raises(RuntimeError):
            K.gemm_f32(a, a, C, **kw)
    # the C entry points refuse too (an error code, no launch); the older export still knows three epilogues only
    L = K.lib()
    rc = L.iit_gemm_f32_aux(a.data_ptr(), a.data_ptr(), C.data_ptr(), None, None, None, None, 8, 8, 8, 0, 8, M, N, Kd,
                            0, K.EPI_GELU, 0, 1, _stream())
    assert rc == 1  # hipErrorInvalidValue
    rc = L.iit_gemm_f32(a.data_ptr(), a.data_ptr(), C.data_ptr(), None, None, None, 8, 8, 8, 0, M, N, Kd, 0,
                        K.EPI_GELU, 0, 1, _stream())
    assert rc == 1
    assert not L.iit_gemm_f32_ok(a.data_ptr(), a.data_ptr(), C.data_ptr(), None, None, None, 8, 8, 8, 0, M, N, Kd, 0,
                                 K.EPI_DGELU, 0, 1)
    torch.cuda.synchronize()
    assert C.isnan().all()


# ================================================================================================ LayerNorm
LAYOUTS = ["packed", "odd_pitch", "offset_base"]


def _place(x, layout):
    """``x [T][d]`` on the GPU: packed, with an odd row pitch, or packed 4 bytes into a buffer (both scalar layouts)."""
    T, d = x.shape
    if layout == "packed":
        return B.strided_rows(x, d, 0, dev)
    if layout == "odd_pitch":
        return B.strided_rows(x, d + (2 if d % 2 else 3), 0, dev)
    return B.strided_rows(x, d, 1, dev)


def _ln_run(K, x, w, b, dy, eps, layout):
    T, d = x.shape
    xg, dyg = _place(x, layout), _place(dy, layout)
    yg, dxg = _place(torch.full((T, d), float("nan")), layout), _place(torch.full((T, d), float("nan")), layout)
    wg, bg = (None, None) if w is None else (w.to(dev), b.to(dev))
    mean, rstd = torch.full((T,), float("nan"), device=dev), torch.full((T,), float("nan"), device=dev)
    K.ln_f32_fwd(xg, wg, bg, yg, mean, rstd, eps)
    dw = db = None
    if w is not None:
        dw, db = torch.full((d,), float("nan"), device=dev), torch.full((d,), float("nan"), device=dev)
    K.ln_f32_bwd(dyg, xg, mean, rstd, wg, dxg, dw, db)
    torch.cuda.synchronize()
    out = {"y": yg.cpu(), "mean": mean.cpu(), "rstd": rstd.cpu(), "dx": dxg.cpu()}
    if w is not None:
        out.update(dw=dw.cpu(), db=db.cpu())
    for t in (yg, dxg):  # nothing written between the rows or before the base
        whole = torch.as_strided(t, (t.untyped_storage().nbytes() // 4,), (1,), 0)
        inside = torch.zeros_like(whole, dtype=torch.bool)
        torch.as_strided(inside, t.shape, t.stride(), t.storage_offset()).fill_(True)
        assert whole[~inside].isnan().all()
    return out


@gpu
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("d", B.LN_D)
def test_layer_norm_within_bounds(K, d, affine):
    assert K.ln_f32_part_rows() == B.PART_ROWS
    for T in B.LN_T:
        for family in B.LN_FAMILIES:
            x, w, b = B.ln_inputs(family, T, d, 10 * d + T, affine)
            dy = torch.randn(T, d, generator=B.gen(d + T)).float()
            ref = B.ln_fwd_ref(x, w, b, B.LN_EPS)
            for layout in LAYOUTS if family == "random" else LAYOUTS[:2]:
                got = _ln_run(K, x, w, b, dy, B.LN_EPS, layout)
                bad = B.ln_fwd_check(got, ref)
                bad.update(B.ln_bwd_check(got, B.ln_bwd_ref(dy, x, got["mean"], got["rstd"], w), affine))
                assert not any(v.any() for v in bad.values()), (T, family, layout,
                                                                {k: int(v.sum()) for k, v in bad.items()})


@gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("d", [64, 256])
def test_layer_norm_selector_case_is_bitwise_exact(K, d, layout):
    x, w, b, dy, ref = B.selector_case(37, d, d)
    got = _ln_run(K, x, w, b, dy, 0.0, layout)
    for k, v in ref.items():
        assert not B.bad_bits(got[k].contiguous(), v).any(), k


@gpu
@pytest.mark.parametrize("d", [68, 1023])
def test_layer_norm_affine_gradients_are_deterministic(K, d):
    """T spans four partial blocks, the last one ragged: within the bounds, the same bits in two runs and in a
    captured-graph replay."""
    T = 3 * B.PART_ROWS + 5
    x, w, b = B.ln_inputs("random", T, d, 7, True)
    dy = torch.randn(T, d, generator=B.gen(8)).float()
    first = _ln_run(K, x, w, b, dy, B.LN_EPS, "packed")
    bad = B.ln_bwd_check(first, B.ln_bwd_ref(dy, x, first["mean"], first["rstd"], w), True)
    assert not any(v.any() for v in bad.values()), {k: int(v.sum()) for k, v in bad.items()}
    second = _ln_run(K, x, w, b, dy, B.LN_EPS, "packed")
    for k in first:
        assert not B.bad_bits(first[k], second[k]).any(), k

    xg, dyg, wg, bg = (t.to(dev) for t in (x, dy, w, b))
    bufs = {k: torch.empty(s, device=dev) for k, s in dict(y=(T, d), dx=(T, d), mean=(T,), rstd=(T,), dw=(d,),
                                                           db=(d,)).items()}

    def launch():
        K.ln_f32_fwd(xg, wg, bg, bufs["y"], bufs["mean"], bufs["rstd"], B.LN_EPS)
        K.ln_f32_bwd(dyg, xg, bufs["mean"], bufs["rstd"], wg, bufs["dx"], bufs["dw"], bufs["db"])

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside capture
        launch()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for _ in range(2):
        for t in bufs.values():
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for k, t in bufs.items():
            assert not B.bad_bits(t.cpu(), first[k]).any(), k


@gpu
def test_layer_norm_refusals(K):
    x = torch.zeros(2, 4100, device=dev)
    v = torch.zeros(2, device=dev)
    with pytest.raises(ValueError):
        K.ln_f32_fwd(x, None, None, torch.empty_like(x), v, v.clone(), 1e-5)  # d > 4096
    x = torch.zeros(2, 8, device=dev)
    y = torch.full((2, 8), float("nan"), device=dev)
    w = torch.ones(8, device=dev)
    with pytest.raises(ValueError):
        K.ln_f32_fwd(x, w, None, y, v, v.clone(), 1e-5)  # w without b
    with pytest.raises(ValueError):
        K.ln_f32_bwd(x, x, v, v, None, y, w, w.clone())  # dw without w
    L = K.lib()
    p = x.data_ptr()
    assert L.iit_ln_f32_fwd(p, None, None, y.data_ptr(), v.data_ptr(), v.data_ptr(), 2, 4097, 4097, 4097, 1e-5,
                            _stream()) == 1
    assert L.iit_ln_f32_fwd(p, None, None, y.data_ptr(), v.data_ptr(), v.data_ptr(), 2, 8, 4, 8, 1e-5, _stream()) == 1
    assert L.iit_ln_f32_bwd(p, p, v.data_ptr(), v.data_ptr(), w.data_ptr(), y.data_ptr(), None, w.data_ptr(),
                            w.data_ptr(), 2, 8, 8, 8, 8, _stream()) == 1  # dw without the partial workspace
    assert L.iit_dgelu_f32(p, p, y.data_ptr(), 0, _stream()) == 1
    assert L.iit_dgelu_f32(p + 2, p, y.data_ptr(), 4, _stream()) == 1
    torch.cuda.synchronize()
    assert y.isnan().all()


# ================================================================================================ dgelu
@gpu
@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("n", B.DGELU_N)
def test_dgelu_f32(K, n, misaligned):
    pre = B.gelu_inputs(n, 11)
    g = (4.0 * torch.randn(n, generator=B.gen(12))).float()
    off = 1 if misaligned else 0

    def put(t):
        buf = torch.full((n + 9,), float("nan"), device=dev)
        buf[off:off + n] = t.to(dev)
        return buf, buf[off:off + n]

    (_, gg), (_, pg) = put(g), put(pre)
    obuf, og = put(torch.full((n,), float("nan")))
    K.dgelu_f32(gg, pg, og)
    torch.cuda.synchronize()
    r = B.dgelu_ref(g, pre)
    bad = B.bad_bound(og.cpu(), r["y"], r["tol"])
    assert not bad.any(), (int(bad.sum()), int(bad.nonzero()[0]))
    assert obuf[:off].isnan().all() and obuf[off + n:].isnan().all()
