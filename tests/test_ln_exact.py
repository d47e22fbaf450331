"""Element-wise layer-norm tests on the GPU: every LN kernel of csrc/layer_norm.hip, forward and backward, against the
float64 reference and the derived bounds of tests/kern_exact_util.py (proved on the CPU by
tests/test_kern_exact_ref.py).

* forward (``ln_fwd``, ``ln_fwd_twin``): every ``d`` at both ends of each vector (W = 4, N = 1 .. 16) and scalar
  (W = 1, N = 4 .. 64) instantiation, a misaligned view that sends a ``d % 4 == 0`` row to the scalar kernels, T = 1, 3, 5,
  9 (partial last workgroup), four operand families, with and without affine parameters; d = 4097 / 4100 refused;
* backward (``ln_bwd`` fused-partials and plain paths, ``ln_bwd_xh16``): fp32 / bf16 dy, dres, dx16, accumulate, dy2
  (in-kernel and summed by the wrapper), prefilled dw / db; the long-row-count cases of the partial reduce and of the
  two ``ln_dwdb`` kernels;
* row select (``ln_fwd_sel`` / ``ln_bwd_sel``) with S = 3 and S = 64 (bits 0 and S - 1).

Every output has four spare rows prefilled with NaN / the bf16 sentinel that must keep their bits; a case passes only
with no element outside its bound.

Measured on an MI355X: 344 cases, 344 passed, none skipped, 3.8 s for the module; the slowest case is the first
launch (0.13 s), every other case below 0.1 s.  As a check of the module itself, a library whose vector forward kernel
divides the variance by d - 1 failed all 68 vector-``d`` cases of ``test_ln_fwd`` (d = 4096 included, where the change
is 1.2e-4 of rstd) and the 8 vector cases of ``test_ln_row_select``, and none of the scalar-kernel cases.
"""
import pytest
import torch

import kern_exact_util as X

pytestmark = pytest.mark.gpu

dev = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
SPARE = 4
# (d, view offset in floats)
D_CASES = [(d, 0) for d in X.LN_D_VEC + X.LN_D_SCALAR] + [(516, 1)]


@pytest.fixture(scope="module")
def K():
    from iit_amd.ops import hip_kernels
    hip_kernels.lib()
    old = hip_kernels.CHECK_BOUNDS
    hip_kernels.CHECK_BOUNDS = True
    yield hip_kernels
    hip_kernels.CHECK_BOUNDS = old


def _count(bad: dict) -> dict:
    return {n: int(m.sum()) for n, m in bad.items() if int(m.sum())}


def _dev(t, off: int = 0):
    """``t`` on the GPU; ``off`` floats past a 16-byte boundary (the storage covers exactly the view)."""
    if t is None:
        return None
    if not off:
        return t.contiguous().to(dev, copy=True)
    buf = torch.empty(off + t.numel(), dtype=t.dtype, device=dev)
    view = buf[off:].view(t.shape)
    view.copy_(t)
    return view


def _out(T: int, d: int, dtype, init=None):
    """[T + SPARE, d] output prefilled with NaN / the sentinel (``init`` in the first T rows) and a copy of it."""
    buf = X.filled((T + SPARE, d) if d else (T + SPARE,), dtype, dev)
    if init is not None:
        buf[:T] = init.to(dev)
    return buf, buf.clone()


def _spare_kept(*pairs, T: int) -> int:
    return sum(int(X.bad_bits(buf[T:], pre[T:]).sum()) for buf, pre in pairs)


def run_fwd(K, x, w, b, T, d, sel=None):
    """``ln_fwd`` (or ``ln_fwd_sel`` with ``sel`` = (mask, S, Tb)) into prefilled buffers; checks the spare rows."""
    (y, y0), (mean, m0), (rstd, r0) = _out(T, d, BF16), _out(T, 0, F32), _out(T, 0, F32)
    if sel is None:
        K.ln_fwd(x, w, b, y, mean, rstd, T, d, X.LN_EPS)
    else:
        K.ln_fwd_sel(x, w, b, y, mean, rstd, T, d, X.LN_EPS, *sel)
    torch.cuda.synchronize()
    assert _spare_kept((y, y0), (mean, m0), (rstd, r0), T=T) == 0
    return {"y": y[:T], "mean": mean[:T], "rstd": rstd[:T]}


def _cpu(got: dict) -> dict:
    return {k: (None if v is None else v.cpu()) for k, v in got.items()}


# ================================================================================================ forward
@pytest.mark.parametrize("T", X.LN_T)
@pytest.mark.parametrize("d,off", D_CASES)
def test_ln_fwd(K, d, off, T):
    vector = d % 4 == 0 and not off
    for family, affine in [("random", True), ("random", False), ("offset", True), ("lowvar", False),
                           ("lowvar", True), ("balanced", True)]:
        x, w, b = X.ln_inputs(family, T, d, seed=31 * d + T, affine=affine)
        ref = X.ln_fwd_ref(x, w, b, X.LN_EPS)
        xd, wd, bd = _dev(x, off), _dev(w), _dev(b)
        got = run_fwd(K, xd, wd, bd, T, d)
        bad = _count(X.ln_fwd_check(_cpu(got), ref))
        assert not bad, (family, affine, bad)
        if family == "balanced" and d % 2 == 0:
            assert not int(X.bad_balanced(got["y"].cpu(), x).sum()), family
        # the twin entry point: same bits, plus the fp32 image of y; refused (nothing written) off the vector layout
        (y, y0), (y32, y320), (mean, m0), (rstd, r0) = _out(T, d, BF16), _out(T, d, F32), _out(T, 0, F32), _out(T, 0, F32)
        ok = K.ln_fwd_twin(xd, wd, bd, y, y32, mean, rstd, T, d, X.LN_EPS)
        torch.cuda.synchronize()
        assert ok == vector
        if vector:
            assert _spare_kept((y, y0), (y32, y320), (mean, m0), (rstd, r0), T=T) == 0
            assert not int(X.bad_bits(y32[:T], y[:T].float()).sum())
            for n, t in (("y", y), ("mean", mean), ("rstd", rstd)):
                assert not int(X.bad_bits(t[:T], got[n]).sum()), n
        else:
            assert _spare_kept((y, y0), (y32, y320), (mean, m0), (rstd, r0), T=0) == 0


@pytest.mark.parametrize("d", [4097, 4100])
def test_ln_refuses_wide_rows(K, d):
    T = 3
    x, w, b = X.ln_inputs("random", T, d, seed=d)
    xd, wd, bd = _dev(x), _dev(w), _dev(b)
    (y, y0), (mean, m0), (rstd, r0), (y32, y320) = _out(T, d, BF16), _out(T, 0, F32), _out(T, 0, F32), _out(T, d, F32)
    with pytest.raises(RuntimeError):
        K.ln_fwd(xd, wd, bd, y, mean, rstd, T, d, X.LN_EPS)
    assert K.ln_fwd_twin(xd, wd, bd, y, y32, mean, rstd, T, d, X.LN_EPS) is False
    i = X.ln_bwd_inputs(T, d, seed=d, bf16_dy=False)
    (dx, dx0), (dx16, dx160) = _out(T, d, F32), _out(T, d, BF16)
    dw, db = _dev(i["dw0"]), _dev(i["db0"])
    ones = torch.ones(T + SPARE, device=dev)
    with pytest.raises(RuntimeError):
        K.ln_bwd(_dev(i["dy"]), xd, ones, ones, wd, dx, dw, db, T, d, dx16=dx16)
    torch.cuda.synchronize()
    assert _spare_kept((y, y0), (mean, m0), (rstd, r0), (y32, y320), (dx, dx0), (dx16, dx160), T=0) == 0
    assert torch.equal(dw.cpu(), i["dw0"]) and torch.equal(db.cpu(), i["db0"])


# ================================================================================================ backward
def run_bwd(K, i, x, mean32, rstd32, w, T, d, *, off=0, want_dw=True, dres=False, dx16=False, acc=False, dy2=False,
            sel=None, xh16=False):
    """One backward launch into prefilled buffers.  Returns (got on the CPU, float64 reference)."""
    dyd, xd, wd = _dev(i["dy"], 0), _dev(x, off), _dev(w)
    md, rd = _dev(torch.cat([mean32, torch.full((SPARE,), X.NAN)])), _dev(torch.cat([rstd32, torch.full((SPARE,), X.NAN)]))
    dx, dx_pre = _out(T, d, F32, i["dx0"] if acc else None)
    d16, d16_pre = _out(T, d, BF16) if dx16 else (None, None)
    dres_d = _dev(i["dres"]) if dres else None
    dy2_d = _dev(i["dy2"]) if dy2 else None
    dw = db = None
    if want_dw:
        dw, db = _dev(i["dw0"]), _dev(i["db0"])
    dead = None
    if xh16:
        K.ln_bwd_xh16(dyd, xd, rd, dx, T, d, dres=dres_d, dx16=d16)
    elif sel is not None:
        mask, S = sel
        dead = X.sel_dead(T, S, mask)
        K.ln_bwd_sel(dyd, xd, md, rd, wd, dx, dw, db, T, d, mask, S, dres=dres_d, dx16=d16)
    else:
        K.ln_bwd(dyd, xd, md, rd, wd, dx, dw, db, T, d, accumulate=acc, dres=dres_d, dx16=d16, dy2=dy2_d)
    torch.cuda.synchronize()
    pairs = [(dx, dx_pre)] + ([(d16, d16_pre)] if dx16 else [])
    assert _spare_kept(*pairs, T=T) == 0
    if dx16:
        assert not int(X.bad_bits(d16[:T], dx[:T].bfloat16()).sum()), "dx16 is not the bf16 rounding of dx"
    ref = X.ln_bwd_ref(i["dy"], x, mean32, rstd32, w, dres=i["dres"] if dres else None, dx0=i["dx0"] if acc else None,
                       dy2=i["dy2"] if dy2 else None, dw0=i["dw0"] if want_dw else None,
                       db0=i["db0"] if want_dw else None, dead=dead, xh16=xh16)
    got = {"dx": dx[:T].cpu(), "dw": None if dw is None else dw.cpu(), "db": None if db is None else db.cpu()}
    return got, ref


# (affine, bf16 dy, dres, dx16, accumulate, dy2, fused partials allowed, operand family)
BWD_VARIANTS = [
    (True, False, True, True, False, False, True, "random"),
    (True, True, False, False, True, True, True, "offset"),
    (False, False, True, False, True, False, True, "random"),
    (False, True, False, True, False, False, True, "lowvar"),
    (True, True, True, True, False, True, False, "random"),
    (True, False, False, False, True, False, False, "offset"),
]


@pytest.mark.parametrize("T", X.LN_T)
@pytest.mark.parametrize("d,off", D_CASES)
def test_ln_bwd(K, monkeypatch, d, off, T):
    for affine, bf16_dy, dres, dx16, acc, dy2, fused, family in BWD_VARIANTS:
        monkeypatch.setenv("IIT_LN_FUSED_DWDB", "1" if fused else "0")
        x, w, b = X.ln_inputs(family, T, d, seed=17 * d + T, affine=affine)
        f = X.ln_fwd_ref(x, w, b, X.LN_EPS)
        i = X.ln_bwd_inputs(T, d, seed=d + T, bf16_dy=bf16_dy)
        got, ref = run_bwd(K, i, x, f["mean"].float(), f["rstd"].float(), w, T, d, off=off, want_dw=affine, dres=dres,
                           dx16=dx16, acc=acc, dy2=dy2)
        bad = _count(X.ln_bwd_check(got, ref))
        assert not bad, ((affine, bf16_dy, dres, dx16, acc, dy2, fused, family), bad)


@pytest.mark.parametrize("T", X.LN_T)
@pytest.mark.parametrize("d", X.LN_D_VEC)
def test_ln_bwd_xh16(K, d, T):
    """The bf16-xhat backward: the reference takes the stored bf16 xhat as its exact input."""
    for bf16_dy, dres, dx16 in [(True, True, True), (False, False, False)]:
        x, _, _ = X.ln_inputs("random", T, d, seed=d + 3 * T, affine=False)
        f = X.ln_fwd_ref(x, None, None, X.LN_EPS)
        xh = f["y"].float().bfloat16()
        i = X.ln_bwd_inputs(T, d, seed=d + T, bf16_dy=bf16_dy)
        got, ref = run_bwd(K, i, xh, f["mean"].float(), f["rstd"].float(), None, T, d, want_dw=False, dres=dres,
                           dx16=dx16, xh16=True)
        bad = _count(X.ln_bwd_check(got, ref))
        assert not bad, ((bf16_dy, dres, dx16), bad)


def _long(K, T, d, bf16_dy, dres=True):
    x, w, b = X.ln_inputs("random", T, d, seed=T + d)
    f = X.ln_fwd_ref(x, w, b, X.LN_EPS)
    i = X.ln_bwd_inputs(T, d, seed=T, bf16_dy=bf16_dy)
    got, ref = run_bwd(K, i, x, f["mean"].float(), f["rstd"].float(), w, T, d, dres=dres, dx16=True)
    bad = _count(X.ln_bwd_check(got, ref))
    assert not bad, bad


@pytest.mark.parametrize("bf16_dy", [False, True])
@pytest.mark.parametrize("T", [149, 1021])
@pytest.mark.parametrize("d", [8, 16])
def test_ln_bwd_long(K, monkeypatch, d, T, bf16_dy):
    """The partial reduce of the fused backward: 38 partial rows in G = 4 groups (T = 149: two four-wide passes and
    a remainder of two per group) and 256 in G = 32 (T = 1021)."""
    monkeypatch.setenv("IIT_LN_FUSED_DWDB", "1")
    _long(K, T, d, bf16_dy)


@pytest.mark.parametrize("bf16_dy", [False, True])
@pytest.mark.parametrize("T", [33, 65, 257])
@pytest.mark.parametrize("d,fused", [(16, False), (8, False), (1028, True)])
def test_ln_dwdb_vec(K, monkeypatch, d, fused, T, bf16_dy):
    """``ln_dwdb_vec_kernel``: without the fused path, and at d > 1024 where the fused path does not apply."""
    monkeypatch.setenv("IIT_LN_FUSED_DWDB", "1" if fused else "0")
    _long(K, T, d, bf16_dy)


@pytest.mark.parametrize("bf16_dy", [False, True])
def test_ln_dwdb_scalar(K, monkeypatch, bf16_dy):
    """``ln_dwdb_kernel`` (d % 4 != 0) over two 256-row blocks."""
    monkeypatch.setenv("IIT_LN_FUSED_DWDB", "1")
    _long(K, 257, 130, bf16_dy)


# ================================================================================================ row select
SEL_CASES = [(3, 3, 0b101, 260), (3, 4, 0b101, 255), (3, 4, 0b001, 2052), (3, 3, 0b100, 4095),
             (64, 64, (1 << 63) | (1 << 17) | 1, 8), (64, 64, (1 << 63) | 1, 6), (64, 64, 1 << 63, 16)]


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("S,Tb,mask,d", SEL_CASES)
def test_ln_row_select(K, monkeypatch, S, Tb, mask, d, fused):
    monkeypatch.setenv("IIT_LN_FUSED_DWDB", "1" if fused else "0")
    T = 2 * Tb
    x, w, b = X.ln_inputs("random", T, d, seed=S + d)
    xd, wd, bd = _dev(x), _dev(w), _dev(b)
    plain = run_fwd(K, xd, wd, bd, T, d)
    got = run_fwd(K, xd, wd, bd, T, d, sel=(mask, S, Tb))
    dead = X.sel_dead(Tb, S, mask)
    assert int(dead.sum()) and not bool(dead.all())
    rows = torch.arange(T)
    src = rows.clone()
    src[:Tb][dead] += Tb  # a masked base row shows the kernel's own result for row + Tb
    for n in ("y", "mean", "rstd"):
        assert not int(X.bad_bits(got[n], plain[n][src.to(dev)]).sum()), n
    assert not _count(X.ln_fwd_check(_cpu(plain), X.ln_fwd_ref(x, w, b, X.LN_EPS)))
    # backward over the base rows
    for dres, bf16_dy in [(True, False), (False, True)]:
        i = X.ln_bwd_inputs(Tb, d, seed=S + d, bf16_dy=bf16_dy)
        f = X.ln_fwd_ref(x[:Tb], w, b, X.LN_EPS)
        g, ref = run_bwd(K, i, x[:Tb], f["mean"].float(), f["rstd"].float(), w, Tb, d, dres=dres, dx16=True,
                         sel=(mask, S))
        bad = _count(X.ln_bwd_check(g, ref))
        assert not bad, (dres, bad)
        if dres:
            assert not int(X.bad_bits(g["dx"][dead], i["dres"][dead]).sum()), "a masked row's dx is not dres bit for bit"
        else:  # (the fused kernel writes -0.0 under a negative weight: 0 * w enters the combination)
            assert bool((g["dx"][dead] == 0).all()), "a masked row's dx is not zero"
