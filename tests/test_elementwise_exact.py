"""Element-wise tests of the element-wise and copy kernels of csrc/kernels.hip on the GPU (``gelu_fwd_kernel`` /
``gelu_fwd_scalar_kernel``, ``dgelu_kernel``, ``add_bf16_kernel``, ``shadow_refresh_kernel``, ``zero_chunks_kernel``,
``zero_ranges_kernel``) against the references and bounds of tests/misc_exact_util.py (proved on the CPU by
tests/test_misc_exact_ref.py).

GELU: the input of every case is EVERY finite bf16 value with |x| <= 2^40 (filled up to 21 x 2048 = 6144 x 7 elements),
through the vector and the scalar forward of both forms and both bodies of the derivative, with dpost = 1, -1 and a
random bf16; the scalar forward is forced by N = 7, by a row stride that is no multiple of 8 and by a misaligned base.
``add_bf16``, ``shadow_refresh`` and the zeroing kernels are compared bit for bit, every output buffer whole, so that
a write outside the target shows.

Measured on an MI355X: 49 cases, 49 passed, none skipped, 2.5 s for the module; the slowest case is the first (0.24 s,
one-time initialisation), every other case 0.01 s or less.  Worst errors through the kernels, in units of the bound:
gelu_new 0.983 (x = -1.30), its derivative 0.971, erf GELU 0.971, its derivative 0.965 -- the bf16 store takes nearly
all of each bound; the erf forward differs from the rounded exact value by at most 0.45 E |x| (x = -4.44) where the
bound allows (ERF_K + 1.4) E |x| = 5.4 E |x|.  Before the stand-alone gelu_new kernels were moved to ``gelu_new_f``, all
five ``test_gelu_fwd[*-new]`` cases failed: 159 inputs from x = -9.94 to -3.98, the worst 255 times the bound at
x = -4.97 (the ``1 - 2 rcp(exp(2u) + 1)`` form).  As a check of the module itself, a library whose transposed
``shadow_refresh`` writes ``tile[i][tx]`` failed ``test_shadow_refresh`` in the descriptors 31 x 33, 32 x 32, 33 x 65
and 545 x 929 (991, 992, 2075 and 490066 bad elements; 1 x 1 cannot show it), in no plain one.
"""
import numpy as np
import pytest
import torch

import misc_exact_util as X

pytestmark = pytest.mark.gpu

dev = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
_CACHE = {}


@pytest.fixture(scope="module")
def K():
    from iit_amd.ops import hip_kernels
    hip_kernels.lib()
    old = hip_kernels.CHECK_BOUNDS
    hip_kernels.CHECK_BOUNDS = True
    yield hip_kernels
    hip_kernels.CHECK_BOUNDS = old


def _x() -> torch.Tensor:
    if "x" not in _CACHE:
        _CACHE["x"] = X.gelu_inputs()
    return _CACHE["x"]


def _gelu_ref(kind: str) -> dict:
    """The float64 reference of the shared input, computed once per form and left unchanged."""
    if kind not in _CACHE:
        _CACHE[kind] = X.gelu_ref(_x(), kind)
    return _CACHE[kind]


def _report(what, bad, x, got, ref, tol):
    """Worst error in units of the bound, and the first bad inputs, for the assertion message."""
    ratio = ((got.double() - ref).abs() / tol).reshape(-1)
    worst = int(torch.nan_to_num(ratio, nan=float("inf")).argmax())
    xs = x[bad].float()
    return (f"{what}: {int(bad.sum())} bad; worst {float(ratio[worst]):.3g} x bound at "
            f"x = {float(x.reshape(-1)[worst])}; bad x from {float(xs.min())} to {float(xs.max())}")


# ================================================================================================ GELU
# layout -> (M, N, ldp, ldo, base offset of pre in elements)
GELU_LAYOUTS = {"vec": (21, 2048, 2048, 2048, 0), "vec_pad": (21, 2048, 2056, 2064, 0), "n7": (6144, 7, 7, 7, 0),
                "ld_odd": (21, 2048, 2052, 2048, 0), "misaligned": (21, 2048, 2048, 2048, 1)}


@pytest.mark.parametrize("kind", X.GELU_KINDS)
@pytest.mark.parametrize("layout", sorted(GELU_LAYOUTS))
def test_gelu_fwd(K, layout, kind):
    M, N, ldp, ldo, off = GELU_LAYOUTS[layout]
    x = _x().view(M, N)
    pre = X.strided(x.to(dev), ldp, off, dev)
    obuf = X.filled((M * ldo + 8,), BF16, dev)
    out = obuf[:M * ldo].view(M, ldo)[:, :N]
    vec = N % 8 == 0 and ldp % 8 == 0 and ldo % 8 == 0 and pre.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    assert vec == layout.startswith("vec")
    K.gelu_fwd(pre, out, M, N, erf=kind == "erf")
    torch.cuda.synchronize()
    ref = _gelu_ref(kind)
    got = out.cpu()
    y, tol = ref["y"].view(M, N), ref["tol"].view(M, N)
    bad = X.bad_bound(got, y, tol)
    assert not int(bad.sum()), _report(f"gelu_{kind}[{layout}]", bad, x, got, y, tol)
    whole = obuf.cpu()
    keep = torch.ones(M * ldo + 8, dtype=torch.bool)
    keep[:M * ldo].view(M, ldo)[:, :N] = False
    assert bool((whole[keep].float() == X.BF16_FILL).all()), "written outside [M, N]"


@pytest.mark.parametrize("kind", X.GELU_KINDS)
@pytest.mark.parametrize("dpost", ["one", "minus_one", "random"])
@pytest.mark.parametrize("body", ["8", "tail"])
def test_dgelu(K, body, dpost, kind):
    """n % 8 == 0 (16-byte body) and n % 8 == 1 (scalar body: the same inputs and one more)."""
    x = _x() if body == "8" else torch.cat([_x(), torch.tensor([0.5], dtype=BF16)])
    n = x.numel()
    g = {"one": torch.ones(n), "minus_one": -torch.ones(n), "random": torch.randn(n, generator=X.gen(3))}[dpost]
    g = g.bfloat16()
    obuf = X.filled((n + 8,), BF16, dev)
    K.dgelu(g.to(dev), x.to(dev), obuf[:n], erf=kind == "erf")
    torch.cuda.synchronize()
    ref = X.dgelu_ref(g, x, kind)
    whole = obuf.cpu()
    bad = X.bad_bound(whole[:n], ref["y"], ref["tol"])
    assert not int(bad.sum()), _report(f"dgelu_{kind}[{body}]", bad, x, whole[:n], ref["y"], ref["tol"])
    assert bool((whole[n:].float() == X.BF16_FILL).all())


# ================================================================================================ add_bf16
@pytest.mark.parametrize("bias", ["bias", "none", "misaligned_bias"])
@pytest.mark.parametrize("alias", [False, True], ids=["separate", "in_place"])
@pytest.mark.parametrize("M,N,ld", [(3, 8, 8), (5, 264, 272), (3, 7, 7), (4, 770, 770)])
def test_add_bf16(K, M, N, ld, alias, bias):
    g = X.gen(M * N)
    base = (100.0 * torch.randn(M, N, generator=g)).float()
    y = torch.randn(M, N, generator=g).bfloat16()
    bs = None if bias == "none" else (1e-3 * torch.randn(N, generator=g)).float()
    base_v = X.strided(base.to(dev), ld, 0, dev)
    y_v = X.strided(y.to(dev), ld, 0, dev)
    bias_v = None
    if bs is not None:
        off = 1 if bias == "misaligned_bias" else 0
        bias_v = X.filled((N + 8,), F32, dev)[off:off + N]
        bias_v.copy_(bs)
    if alias:
        out_v, obuf = base_v, None
    else:
        obuf = X.filled((M * ld + 8,), F32, dev)
        out_v = obuf[:M * ld].view(M, ld)[:, :N]
    K.add_bf16(out_v, ld, base_v, ld, y_v, ld, bias_v, M, N)
    torch.cuda.synchronize()
    ref = X.add_bf16_ref(base, y, bs)
    assert not int(X.bad_bits(out_v.cpu(), ref).sum())
    if obuf is not None:
        whole = obuf.cpu()
        keep = torch.ones(M * ld + 8, dtype=torch.bool)
        keep[:M * ld].view(M, ld)[:, :N] = False
        assert bool(torch.isnan(whole[keep]).all()), "written outside [M, N]"
        assert not int(X.bad_bits(base_v.cpu(), base).sum())


# ================================================================================================ shadow_refresh
# (heads, rows, cols, ld, transpose, source offset in floats, source head gap, destination head gap)
SHADOW_CASES = [
    (1, 3, 8, 8, 0, 0, 0, 0),
    (1, 5, 7, 7, 0, 0, 0, 0),
    (1, 4, 10, 12, 0, 0, 0, 0),      # even rows: float4 body + 2-column tail; odd rows: unaligned source rows
    (1, 3, 9, 9, 0, 1, 0, 0),        # unaligned source: the per-row fallback
    (3, 4, 8, 8, 0, 0, 8, 16),       # head strides
    (1, 3, 8, 16, 0, 0, 0, 0),       # ld > cols
    (2, 515, 4, 4, 0, 0, 0, 0),      # heads * rows = 1030 > 512 blocks: the stride loop
    (1, 1, 1, 1, 1, 0, 0, 0),
    (1, 31, 33, 31, 1, 0, 0, 0),
    (1, 32, 32, 32, 1, 0, 0, 0),
    (1, 33, 65, 40, 1, 0, 0, 0),     # ld > rows
    (1, 545, 929, 552, 1, 0, 0, 0),  # 18 x 30 = 540 tiles > 512 blocks
]


def test_shadow_refresh(K):
    """Every case of SHADOW_CASES as one descriptor of ONE launch."""
    entries, keep = [], []
    for i, (heads, rows, cols, ld, tr, soff, sgap, dgap) in enumerate(SHADOW_CASES):
        src = torch.randn(heads, rows, cols, generator=X.gen(i))
        shs = rows * cols + sgap
        sbuf = X.filled((soff + heads * shs + 4,), F32, dev)
        for h in range(heads):
            sbuf[soff + h * shs:soff + h * shs + rows * cols].copy_(src[h].reshape(-1))
        dhs = rows * ld + dgap
        n_dst = (cols * ld if tr else heads * dhs) + 8
        dst0 = X.filled((n_dst,), BF16)
        dst = dst0.to(dev)
        entries.append((sbuf.data_ptr() + 4 * soff, dst.data_ptr(), rows, cols, ld, tr, heads, shs, dhs))
        keep.append((sbuf, dst, X.shadow_expected(dst0, src, ld, bool(tr), dhs)))
    descs = K.make_shadow_descs(entries, dev)
    K.shadow_refresh(descs, len(entries))
    torch.cuda.synchronize()
    bad = {i: int(X.bad_bits(dst.cpu(), want).sum()) for i, (_, dst, want) in enumerate(keep)}
    assert not any(bad.values()), {SHADOW_CASES[i]: n for i, n in bad.items() if n}


# ================================================================================================ zeroing
def _zero_buffer():
    ranges, n = X.zero_ranges_table()
    buf0 = torch.randn(n, generator=X.gen(8)).float()
    buf0[buf0 == 0] = 1.0
    return ranges, buf0


def test_zero_chunks(K):
    """A device table of (start, len): every length of ZERO_LENS at all four start alignments, one block each."""
    ranges, buf0 = _zero_buffer()
    buf = buf0.to(dev)
    chunks = torch.tensor(ranges, dtype=torch.int64).reshape(-1).to(dev)
    K.zero_chunks(buf, chunks, len(ranges))
    torch.cuda.synchronize()
    assert not int(X.bad_bits(buf.cpu(), X.zero_expected(buf0, ranges)).sum())


def test_zero_ranges(K):
    """The same ranges by value (65536 floats = four chunks of 16384)."""
    ranges, buf0 = _zero_buffer()
    buf = buf0.to(dev)
    K.zero_ranges(buf, np.array([a for a, _ in ranges]), np.array([n for _, n in ranges]))
    torch.cuda.synchronize()
    assert not int(X.bad_bits(buf.cpu(), X.zero_expected(buf0, ranges)).sum())
