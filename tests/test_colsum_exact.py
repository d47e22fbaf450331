"""Element-wise tests of the column-sum kernels of csrc/kernels.hip on the GPU (``colsum_kernel``,
``colsum_vec_kernel`` through ``hip_kernels.colsum_accum`` and ``colsum_multi_kernel`` through
``hip_kernels.colsum_multi``) against the float64 sums and bounds of tests/misc_exact_util.py (proved on the CPU by
tests/test_misc_exact_ref.py).

Every case adds into a prefilled output whose spare tail must keep its bits, and runs on the ``exact`` family
(integers: bitwise the float64 sum, so a dropped or doubled row shows) and the ``random`` one (``(T + 3) E`` bound).
Pad columns of ``ld > N`` hold NaN / the bf16 sentinel, so a read past N shows.  The three large cases pick T and N from
the rows-per-block loop of ``iit_colsum_accum`` (R = 64, 128, 256, T % R != 0) and take their float64 reference on
the device, one family each.

Measured on an MI355X: 83 cases, 83 passed, none skipped, 3.2 s for the module; the slowest cases are the first (0.3 s,
one-time initialisation) and R = 64 (0.17 s), every other case 0.01 s or less.  As a check of the module itself, a
library whose ``colsum_block`` starts its row loop at ``t0 + rg + 8`` failed all 8 cases of ``test_colsum_multi``; the
other 75 cases, which do not run ``colsum_multi_kernel``, passed.
"""
import pytest
import torch

import misc_exact_util as X

pytestmark = pytest.mark.gpu

dev = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
CPT = {F32: 4, BF16: 8}
T_MULTI = [1, 127, 128, 129, 300]


@pytest.fixture(scope="module")
def K():
    from iit_amd.ops import hip_kernels
    hip_kernels.lib()
    old = hip_kernels.CHECK_BOUNDS
    hip_kernels.CHECK_BOUNDS = True
    yield hip_kernels
    hip_kernels.CHECK_BOUNDS = old


def _out(family, N, seed):
    """Prefilled output [N] inside a buffer with 4 spare floats; returns (device view, device buffer, host prefill)."""
    pre = torch.cat([X.operand(family, (N,), F32, seed, 1), X.filled((4,), F32)])
    buf = pre.to(dev)
    return buf[:N], buf, pre


def _check(x_host, out_buf, pre, family, N):
    ref = X.colsum_ref(x_host, pre[:N])
    got = out_buf.cpu()
    bad = int(X.bad_sum(got[:N], ref["out"], ref["tol"], family).sum())
    assert not bad, bad
    assert not int(X.bad_bits(got[N:], pre[N:]).sum()), "written past N"


def _accum_case(K, T, N, dtype, family, ld, offset=0, vec=None):
    x = X.operand(family, (T, N), dtype, T * 1000 + N, T + 1)
    view = X.strided(x.to(dev), ld, offset, dev)
    if vec is not None:
        assert K.colsum_vec_ok(view, ld, torch.empty(0, dtype=F32), N) == vec
    out, buf, pre = _out(family, N, N)
    K.colsum_accum(view, ld, out, T, N)
    torch.cuda.synchronize()
    _check(x, buf, pre, family, N)


@pytest.mark.parametrize("family", X.FAMILIES)
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 130])
def test_colsum_scalar(K, N, dtype, family):
    """``colsum_kernel``: ld = N + 1 keeps every N, also 64, off the vector path."""
    for T in (1, 63, 64, 65, 129):
        _accum_case(K, T, N, dtype, family, ld=N + 1, vec=False)


@pytest.mark.parametrize("family", X.FAMILIES)
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_colsum_scalar_misaligned(K, dtype, family):
    """N = ld = 64 on a view offset by one element: only the base address takes it off the vector path."""
    for T in (1, 65):
        _accum_case(K, T, 64, dtype, family, ld=64, offset=1, vec=False)


VEC_N = [(BF16, n) for n in (8, 248, 256, 264)] + [(F32, n) for n in (4, 124, 128, 132)]


@pytest.mark.parametrize("family", X.FAMILIES)
@pytest.mark.parametrize("layout", ["dense", "padded", "column_offset"])
@pytest.mark.parametrize("dtype,N", VEC_N, ids=[f"{'bf16' if d == BF16 else 'f32'}-{n}" for d, n in VEC_N])
def test_colsum_vec(K, dtype, N, layout, family):
    """``colsum_vec_kernel`` (R = 32 at these sizes): dense rows, ld = N + 16 bytes of sentinel, and a view that starts
    16 bytes into every row of a wider matrix."""
    cpt = CPT[dtype]
    for T in (1, 7, 8, 9, 31, 32, 33, 257):
        if layout == "column_offset":
            x = X.operand(family, (T, N), dtype, T * 1000 + N, T + 1)
            wide = X.filled((T, N + 2 * cpt), dtype, dev)
            view = wide[:, cpt:cpt + N]
            view.copy_(x)
            assert K.colsum_vec_ok(view, N + 2 * cpt, torch.empty(0, dtype=F32), N)
            out, buf, pre = _out(family, N, N)
            K.colsum_accum(view, N + 2 * cpt, out, T, N)
            torch.cuda.synchronize()
            _check(x, buf, pre, family, N)
        else:
            _accum_case(K, T, N, dtype, family, ld=N if layout == "dense" else N + cpt, vec=True)


def _rows_per_block(T: int, N: int) -> int:
    """The R that iit_colsum_accum picks for a bf16 operand."""
    gx = (N + 255) // 256
    R = 256
    while R > 32 and gx * ((T + R - 1) // R) < 1024:
        R >>= 1
    return R


@pytest.mark.parametrize("R,T,family", [(64, 1990, "exact"), (128, 3970, "random"), (256, 7940, "exact")])
def test_colsum_vec_rows_per_block(K, R, T, family):
    N = 8192
    assert _rows_per_block(T, N) == R and T % R != 0
    if family == "exact":
        assert (T + 1) * 64 < 2 ** 24
        x = torch.randint(-64, 65, (T, N), device=dev, generator=torch.Generator(dev).manual_seed(R)).to(BF16)
    else:
        x = torch.randn(T, N, device=dev, generator=torch.Generator(dev).manual_seed(R)).to(BF16)
    out, buf, pre = _out(family, N, R)
    K.colsum_accum(x, N, out, T, N)
    torch.cuda.synchronize()
    ref = X.colsum_ref(x, pre[:N].to(dev))
    got = buf.cpu()
    assert not int(X.bad_sum(got[:N], ref["out"].cpu(), ref["tol"].cpu(), family).sum())
    assert not int(X.bad_bits(got[N:], pre[N:]).sum())


@pytest.mark.parametrize("family", X.FAMILIES)
@pytest.mark.parametrize("n_items", [1, 2, 32, 33])
def test_colsum_multi(K, n_items, family):
    """One call (two launches at 33 items: CS_MAX = 32): fp32 and bf16 items mixed, T around R = 128, another N per
    item, item 1 (0 when alone) with ld > N over a sentinel pad."""
    items, hosts = [], []
    for i in range(n_items):
        dtype = F32 if i % 3 == 1 else BF16
        cpt = CPT[dtype]
        T = T_MULTI[i % len(T_MULTI)]
        N = cpt * (1 + (7 * i) % 40)  # 8 ... 320 (bf16), 4 ... 160 (fp32): one or two column blocks
        ld = N + cpt if i == min(1, n_items - 1) else N
        x = X.operand(family, (T, N), dtype, 100 * i + T, T + 1)
        view = X.strided(x.to(dev), ld, 0, dev)
        out, buf, pre = _out(family, N, i)
        assert K.colsum_vec_ok(view, ld, out, N)
        items.append((view, ld, out, T, N))
        hosts.append((x, buf, pre, N))
    K.colsum_multi(items)
    torch.cuda.synchronize()
    for x, buf, pre, N in hosts:
        _check(x, buf, pre, family, N)
