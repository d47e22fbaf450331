"""The LN forward launch that also prefetches (``iit_ln_fwd_pf``, csrc/layer_norm.hip): the extra workgroups in front of
the row blocks only read, so ``y``, ``y32``, ``mean`` and ``rstd`` must keep every bit they have without them, and the
prefetched buffers must keep theirs.

Shapes: the smallest that reach each path of the kernel -- d = 768 (vector layout, N = 3), d = 64 (N = 1), d = 100
(scalar layout), T = 5 (a partial last block) and T = 64, one paired row-select launch (S = 4, Tb = 8, T = 16, positions
0 and 2 spliced) and one launch with the fp32 twin.  Ranges: none, one and two; 64 B, 4 KiB + 64 B and 1 MiB + 128 B;
a null pointer with a length; 0 and 8 workgroups, the default density, and more workgroups than a range has granules.
Every range is the front of a larger allocation.  (That the reads stay inside a range is a property of
``prefetch_part``, csrc/prefetch.h: every granule start is below ``bytes``; no case here looks for an access outside.)
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

dev = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
EPS = 1e-5
KB4, MB1 = 4096 + 64, 2 ** 20 + 128

# (id, T, d, affine, (pos_mask, S, Tb) or None, fp32 twin)
SHAPES = [
    ("d768", 64, 768, True, None, False),
    ("d768-T5", 5, 768, False, None, False),
    ("d64", 64, 64, True, None, False),
    ("d100-T5", 5, 100, True, None, False),
    ("rowsel", 16, 64, True, (0b0101, 4, 8), False),
    ("twin", 64, 768, True, None, True),
]
# (id, bytes of range 0 or None, bytes of range 1 or None, workgroups or None = the default density)
RANGES = [
    ("one-64B-w8", 64, None, 8),  # one granule, eight workgroups
    ("one-4K-w0", KB4, None, 0),  # no workgroups: the row grid alone
    ("one-1M-w8", MB1, None, 8),
    ("two-1M-4K-w8", MB1, KB4, 8),
    ("two-4K-64B-w100", KB4, 64, 100),  # more workgroups than the 65 + 1 granules
    ("two-1M-1M-density", MB1, MB1, None),
]


@pytest.fixture(scope="module")
def K():
    from iit_amd.ops import hip_kernels
    hip_kernels.lib()
    return hip_kernels


@pytest.fixture(scope="module")
def pool():
    """Two allocations larger than any range taken from their fronts, and their copies."""
    g = torch.Generator().manual_seed(5)
    bufs = [torch.randint(0, 256, (MB1 + 4096,), dtype=torch.uint8, generator=g).to(dev) for _ in range(2)]
    return bufs, [b.clone() for b in bufs]


def _inputs(T, d, affine):
    g = torch.Generator().manual_seed(1000 * d + T)
    x = (torch.randn(T, d, generator=g) * 2 + 0.5).to(dev)
    w = (1 + 0.1 * torch.randn(d, generator=g)).to(dev) if affine else None
    b = (0.1 * torch.randn(d, generator=g)).to(dev) if affine else None
    return x, w, b


def _run(K, shape, launch):
    """One forward into fresh outputs; ``launch(args, sel, y32)`` does the call.  Returns the outputs as integers."""
    _, T, d, affine, sel, twin = shape
    x, w, b = _inputs(T, d, affine)
    y = torch.zeros(T, d, dtype=BF16, device=dev)
    y32 = torch.zeros(T, d, dtype=F32, device=dev) if twin else None
    mean, rstd = torch.zeros(T, device=dev), torch.zeros(T, device=dev)
    launch((x, w, b, y, y32, mean, rstd, T, d), sel)
    torch.cuda.synchronize()
    out = {"y": y.view(torch.int16), "mean": mean.view(torch.int32), "rstd": rstd.view(torch.int32)}
    if twin:
        out["y32"] = y32.view(torch.int32)
    return out


def _wrapper(K, **kw):
    def launch(a, sel):
        x, w, b, y, y32, mean, rstd, T, d = a
        if sel is not None:
            K.ln_fwd_sel(x, w, b, y, mean, rstd, T, d, EPS, *sel, **kw)
        elif y32 is not None:
            assert K.ln_fwd_twin(x, w, b, y, y32, mean, rstd, T, d, EPS, **kw)
        else:
            K.ln_fwd(x, w, b, y, mean, rstd, T, d, EPS, **kw)
    return launch


@pytest.fixture(scope="module")
def plain(K):
    """The outputs of each shape without a prefetch, computed once."""
    return {s[0]: _run(K, s, _wrapper(K)) for s in SHAPES}


def _same(got, ref):
    assert got.keys() == ref.keys()
    for name in ref:
        assert torch.equal(got[name], ref[name]), name


@pytest.mark.parametrize("rng", RANGES, ids=[r[0] for r in RANGES])
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_ln_fwd_prefetch_keeps_every_bit(K, pool, plain, shape, rng):
    bufs, copies = pool
    _, n0, n1, wgs = rng
    ts = [bufs[i][:n] for i, n in enumerate((n0, n1)) if n is not None]
    args = K._ln_prefetch_args(ts, wgs)
    if wgs == 0:
        assert args == (None, 0, None, 0, 0)
    else:
        want = wgs if wgs is not None else K.prefetch_wgs(n0 + (n1 or 0), K._PF_PER_MB)
        assert args[1] == n0 and args[3] == (n1 or 0) and args[4] == want > 0
    _same(_run(K, shape, _wrapper(K, prefetch=ts, pf_wgs=wgs)), plain[shape[0]])
    assert all(torch.equal(b, c) for b, c in zip(bufs, copies))


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_ln_fwd_prefetch_null_pointer_with_length(K, pool, plain, shape):
    """A null first range with a length is no range: the second one alone is read."""
    bufs, copies = pool

    def launch(a, sel):
        x, w, b, y, y32, mean, rstd, T, d = a
        pos_mask, S, Tb = sel or (0, 1, 0)
        K._check(K.lib().iit_ln_fwd_pf(K._p(x), K._p(w), K._p(b), K._p(y), K._p(y32), K._p(mean), K._p(rstd), T, d, EPS,
                                       pos_mask, S, Tb, None, KB4, K._p(bufs[1]), KB4, 8, K._stream()), "ln_fwd_pf")
    _same(_run(K, shape, launch), plain[shape[0]])
    assert all(torch.equal(b, c) for b, c in zip(bufs, copies))


def test_ln_fwd_export_without_ranges_is_the_plain_launch(K, plain):
    """``iit_ln_fwd`` keeps its signature and forwards with an empty prefetch."""
    def launch(a, sel):
        x, w, b, y, y32, mean, rstd, T, d = a
        K._check(K.lib().iit_ln_fwd(K._p(x), K._p(w), K._p(b), K._p(y), K._p(y32), K._p(mean), K._p(rstd), T, d, EPS,
                                    0, 1, 0, K._stream()), "ln_fwd")
    _same(_run(K, SHAPES[0], launch), plain[SHAPES[0][0]])
