"""The exact-fp32 convolution kernels (csrc/conv_f32.hip) element by element on the GPU: all three passes, both tiles,
the exact families bitwise and ``REAL`` inside its bound (helpers and references: tests/conv_f32_util.py, checked on the
CPU by tests/test_conv_f32_ref.py).  Every output buffer is pre-filled with NaN and sits between guard bands that must
come back untouched."""
import pytest
import torch

import conv_f32_util as C

pytestmark = pytest.mark.gpu

GUARD = 64  # floats either side of every buffer (a multiple of 4: the payload stays 16-byte aligned)
SENTINEL = -777.25


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from iit_amd.ops import hip_kernels
    hip_kernels.lib()
    return hip_kernels


def _banded(n, fill=None, offset=0):
    """(whole buffer, payload view of n floats starting ``offset`` floats past the aligned position)."""
    buf = torch.full((n + 2 * GUARD + 4,), SENTINEL, dtype=torch.float32, device="cuda")
    pay = buf[GUARD + offset:GUARD + offset + n]
    if fill is not None:
        pay.copy_(fill.reshape(-1)) if isinstance(fill, torch.Tensor) else pay.fill_(fill)
    return buf, pay


def _guards_intact(buf, n, offset=0):
    lo, hi = buf[:GUARD + offset], buf[GUARD + offset + n:]
    return bool((lo == SENTINEL).all() and (hi == SENTINEL).all())


def run_pass(K, pass_, shape, x, w, dy, tile=0, splits=1, offset=0):
    """The pass on the GPU from CPU tensors: ``[M][N]`` result on the CPU.  Inputs and output are banded; the output is
    NaN before the launch and fully written after it."""
    M, N, _ = C.mnk(pass_, shape)
    g = C.geom(shape)
    bx, dx_ = _banded(x.numel(), x if pass_ != C.DGRAD else float("nan"), offset)
    bw, dw_ = _banded(w.numel(), w if pass_ != C.WGRAD else float("nan"), offset)
    by, dy_ = _banded(dy.numel(), dy if pass_ != C.FWD else float("nan"), offset)
    if pass_ == C.FWD:
        K.conv_f32_fwd(dx_, dw_, dy_, g, tile, splits)
        out = dy_
    elif pass_ == C.DGRAD:
        K.conv_f32_dgrad(dy_, dw_, dx_, g, tile, splits)
        out = dx_
    else:
        K.conv_f32_wgrad(dx_, dy_, dw_, g, tile, splits)
        out = dw_
    torch.cuda.synchronize()
    for buf, t in ((bx, x), (bw, w), (by, dy)):
        assert _guards_intact(buf, t.numel(), offset), "a guard band was written"
    for pay, t, written in ((dx_, x, pass_ == C.DGRAD), (dw_, w, pass_ == C.WGRAD), (dy_, dy, pass_ == C.FWD)):
        if not written:
            assert torch.equal(pay.cpu(), t.reshape(-1)), "an input was modified"
    assert out.numel() == M * N
    return out.cpu().reshape(M, N)


def _check(K, family, pass_, shape, tile, splits=1, offset=0):
    x, w, dy = C.tensors(family, pass_, shape)
    ref, mag = C.expected(family, pass_, shape)
    got = run_pass(K, pass_, shape, x, w, dy, tile, splits, offset)
    assert not got.isnan().any(), "an output element was not written"
    wrong = C.bad(family, got, ref, mag, C.mnk(pass_, shape)[2], splits)
    assert not wrong.any(), (family, pass_, shape, tile, splits, int(wrong.sum()), wrong.nonzero()[:4].tolist())
    return got


@pytest.mark.parametrize("pass_", C.PASSES)
@pytest.mark.parametrize("shape", list(C.SHAPES), ids=lambda s: "x".join(map(str, s)))
def test_every_pass_tile_and_family(K, shape, pass_):
    for tile in C.TILES:
        for family in C.FAMILIES:
            got = _check(K, family, pass_, shape, tile)
            if pass_ == C.DGRAD and family == C.F1 and shape[5] == 1 and shape[6] == 2:
                # rows and columns of dX that no forward window reads are written, with +0
                N, H, W, Cin = shape[:4]
                odd = got.reshape(N, H, W, Cin)[:, 1::2]
                assert torch.equal(odd, torch.zeros_like(odd)) and not torch.signbit(odd).any()


@pytest.mark.parametrize("pass_", C.PASSES)
def test_plan_agrees_with_the_utility(K, pass_):
    for shape in C.SHAPES:
        for tile, (bm, bn, bk) in C.TILES.items():
            for splits in (1, 3):
                pl = K.conv_f32_plan(pass_, C.geom(shape), tile, splits)
                M, N, Kd = C.mnk(pass_, shape)
                assert (pl["M"], pl["N"], pl["K"]) == (M, N, Kd)
                assert pl["k_per_split"] == -(-(-(-Kd // splits)) // bk) * bk
                assert pl["grid_x"] == -(-M // bm) * -(-N // bn)
                assert pl["vector"] == int(C.vector_path(pass_, shape))


@pytest.mark.parametrize("pass_", C.PASSES)
def test_misaligned_base_takes_the_scalar_path_with_equal_bits(K, pass_):
    shape = (2, 5, 7, 8, 12, 3, 1, 1)
    assert C.vector_path(pass_, shape)
    for family in (C.F2, C.REAL):
        for tile in C.TILES:
            aligned = _check(K, family, pass_, shape, tile)
            shifted = _check(K, family, pass_, shape, tile, offset=1)  # every base one float past 16-byte alignment
            assert torch.equal(aligned.view(torch.int32), shifted.view(torch.int32))


@pytest.mark.parametrize("pass_", C.PASSES)
def test_split_k(K, pass_):
    shape = C.SPLIT_SHAPE
    Kd = C.mnk(pass_, shape)[2]
    for tile, (_, _, bk) in C.TILES.items():
        empty_last = -(-Kd // bk) + 1  # k_per_split = one K-tile: the last split starts at or past K
        assert empty_last <= 64
        pl = K.conv_f32_plan(pass_, C.geom(shape), tile, empty_last)
        assert (empty_last - 1) * pl["k_per_split"] >= Kd
        for family in C.FAMILIES:
            base = None
            for splits in (1, 2, 3, empty_last):
                got = _check(K, family, pass_, shape, tile, splits)
                if family in C.EXACT:  # exact sums do not depend on where the chain is cut
                    base = got if base is None else base
                    assert torch.equal(got.view(torch.int32), base.view(torch.int32)), (family, tile, splits)


def test_weight_gradient_pixel_counts_off_the_k_tile(K):
    seen = set()
    for shape in C.SHAPES:
        P = C.mnk(C.WGRAD, shape)[2]
        for tile, (_, _, bk) in C.TILES.items():
            if P % bk:
                seen.add(tile)
                _check(K, C.F2, C.WGRAD, shape, tile, splits=2)
    assert seen == set(C.TILES)


def test_graph_replay_equals_eager(K):
    shape = C.SPLIT_SHAPE
    g = C.geom(shape)
    x, w, dy = (t.cuda() for t in C.tensors(C.REAL, C.FWD, shape))
    outs = {}

    def run(tag):
        y, dx, dw = torch.empty_like(dy), torch.empty_like(x), torch.empty_like(w)
        K.conv_f32_fwd(x, w, y, g, 0, 2)
        K.conv_f32_dgrad(dy, w, dx, g, 1, 3)
        K.conv_f32_wgrad(x, dy, dw, g, 0, 2)
        outs[tag] = (y, dx, dw)

    run("eager")
    torch.cuda.synchronize()
    eager = [t.clone() for t in outs["eager"]]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run("warm")
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run("graph")
    for _ in range(2):
        for t in outs["graph"]:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(outs["graph"], eager):
            assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_refusals_raise_without_a_launch(K):
    shape = (2, 6, 6, 4, 8, 3, 2, 1)
    N, H, W, Cin, OH, OW, Cout, k, s, pad = C.geom(shape)
    x, w, dy = (t.cuda() for t in C.tensors(C.F1, C.FWD, shape))
    y = torch.full_like(dy, float("nan"))
    good = (N, H, W, Cin, OH, OW, Cout, k, s, pad)
    K.conv_f32_fwd(x, w, y, good)  # the base case is accepted
    torch.cuda.synchronize()
    assert not y.isnan().any()

    def geom(**kw):
        d = dict(N=N, H=H, W=W, Cin=Cin, OH=OH, OW=OW, Cout=Cout, k=k, s=s, pad=pad)
        d.update(kw)
        return tuple(d[n] for n in ("N", "H", "W", "Cin", "OH", "OW", "Cout", "k", "s", "pad"))

    bad = [(geom(k=8), 0, 1), (geom(k=0), 0, 1), (geom(s=3), 0, 1), (geom(s=0), 0, 1), (geom(pad=3), 0, 1),
           (geom(pad=-1), 0, 1), (geom(OH=OH + 1), 0, 1), (geom(OW=OW - 1), 0, 1), (geom(N=0), 0, 1),
           (geom(Cin=0), 0, 1), (geom(Cout=0), 0, 1), (geom(H=0), 0, 1), (good, 2, 1), (good, -1, 1), (good, 0, 0),
           (good, 0, 65),
           # an extent product beyond int: 2^15 x 2^8 x 2^8 x 2^4 input elements (OH, OW as the formula gives them)
           (geom(N=1 << 15, H=256, W=256, Cin=16, OH=128, OW=128), 0, 1),
           (geom(Cout=1 << 20, Cin=1 << 10), 0, 1)]
    for g, tile, splits in bad:
        y.fill_(float("nan"))
        dx, dw = torch.full_like(x, float("nan")), torch.full_like(w, float("nan"))
        for call in (lambda: K.conv_f32_fwd(x, w, y, g, tile, splits),
                     lambda: K.conv_f32_dgrad(dy, w, dx, g, tile, splits),
                     lambda: K.conv_f32_wgrad(x, dy, dw, g, tile, splits)):
            with pytest.raises(RuntimeError):
                call()
        torch.cuda.synchronize()
        assert y.isnan().all() and dx.isnan().all() and dw.isnan().all(), (g, tile, splits)
    with pytest.raises(RuntimeError):  # not fp32
        K.conv_f32_fwd(x.double(), w, y, good)
    with pytest.raises(RuntimeError):  # not on the GPU
        K.conv_f32_fwd(x.cpu(), w, y, good)
    # pointer refusals, on the pure-host check alone (no launch is attempted with made-up addresses)
    ok = K.lib().iit_conv_f32_ok
    a = x.data_ptr()
    for p in C.PASSES:
        assert ok(p, a, a, a, None, *good, 0, 1) == 1
        assert ok(p, None, a, a, None, *good, 0, 1) == 0 and ok(p, a, None, a, None, *good, 0, 1) == 0
        assert ok(p, a, a, None, None, *good, 0, 1) == 0
        assert ok(p, a + 2, a, a, None, *good, 0, 1) == 0 and ok(p, a, a + 1, a, None, *good, 0, 1) == 0
        assert ok(p, a, a, a + 3, None, *good, 0, 1) == 0
        assert ok(p, a + 4, a + 4, a + 4, None, *good, 0, 1) == 1  # 4-byte alignment is enough
        assert ok(p, a, a, a, None, *good, 0, 2) == 0  # splits without a workspace
        assert ok(p, a, a, a, a + 4, *good, 0, 2) == 0  # ... or with a misaligned one
        assert ok(p, a, a, a, a + 16, *good, 0, 2) == 1
