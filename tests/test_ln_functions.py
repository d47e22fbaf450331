"""The six layer-norm autograd Functions of iit_amd/ops/hip_ops.py against the ``hip_kernels`` wrappers they sit on.

Each Function is a thin layer over ``ln_fwd`` / ``ln_fwd_twin`` / ``ln_fwd_sel`` and ``ln_bwd`` / ``ln_bwd_xh16`` /
``ln_bwd_sel``, whose arithmetic tests/test_ln_exact.py proves element by element, so nothing here needs a tolerance
of its own:

* the outputs have the bits the matching forward wrapper writes for the same flattened rows; the fp32 twin is
  ``y.float()``; a ``*Pair*`` class puts the full-row tensors in ``box`` and returns their base slice;
* the gradient of ``x`` has the bits of the ``dx`` the matching backward wrapper writes for the same ``dy``, with the
  passed-through gradient as ``dres`` (Fork classes) or the fp32 output's gradient as ``dy2`` (Twin classes); an fp32
  ``x`` gets the ``_iit_bf16`` twin ``dx.bfloat16()``, a bf16 ``x`` gets ``dx.to(bf16)``;
* ``w.grad`` / ``b.grad`` lie inside ``tol_dw`` / ``tol_db`` of ``kern_exact_util.ln_bwd_ref`` (the order of the
  atomics is free: no bit claim);
* with one output unused the other path still gives the wrapper's bits; the autograd engine rejects a gradient tuple
  of the wrong length, and the early returns (no gradient at all) are called directly.

Shapes: 2 base + 2 source sequences of S = 3 (6 base rows, 12 paired rows: a partial last workgroup), d = 8 (fused
vector path), 130 (scalar fallback), 1028 (vector path without the fused affine gradients), with and without affine
parameters (without them ``LayerNormForkFn`` at d = 8 and 1028 reads the bf16 xhat), ``pos_mask`` 0b101 for
``LayerNormPairFn``.

Measured on an MI355X: 91 cases, 91 passed, none skipped, 3.8 s for the module; the slowest case is the first launch
(1.2 s), every other case below 0.1 s.
"""
import functools
import types

import pytest
import torch

import kern_exact_util as X

pytestmark = pytest.mark.gpu

dev = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
NB, S = 2, 3  # base sequences (as many source sequences), positions
T = NB * S
T2 = 2 * T
D = [8, 130, 1028]
MASK = 0b101


@pytest.fixture(scope="module")
def K():
    from iit_amd.ops import hip_kernels
    hip_kernels.lib()
    return hip_kernels


@pytest.fixture(scope="module")
def O():
    from iit_amd.ops import hip_ops
    return hip_ops


class _Tap(torch.autograd.Function):
    """Identity in front of the Function under test: its backward is handed the gradient tensor the LN backward
    returned, attributes included -- the way the next backward of a model receives it."""

    @staticmethod
    def forward(ctx, x, seen):
        ctx.seen = seen
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        ctx.seen.append(g)
        return g, None


@functools.lru_cache(maxsize=None)
def _inputs(d: int, affine: bool) -> dict:
    """One set of operands per (d, affine), shared by every test and left unchanged."""
    x, w, b = X.ln_inputs("random", T2, d, seed=7 * d + affine, affine=affine)
    i = X.ln_bwd_inputs(T, d, seed=d, bf16_dy=True)
    out = {"x": x, "w": w, "b": b, "dy": i["dy"], "dpass": i["dres"], "dy32": i["dy2"]}
    return {k: (None if v is None else v.to(dev)) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _fwd_ref(K, d: int, affine: bool, rows: int, kind: str) -> dict:
    """What the forward wrapper writes for the first ``rows`` rows: ``kind`` = plain / twin / sel."""
    i = _inputs(d, affine)
    x = i["x"][:rows].contiguous()
    y = torch.empty(rows, d, dtype=BF16, device=dev)
    mean, rstd = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
    out = {"x": x, "y": y, "mean": mean, "rstd": rstd}
    if kind == "twin":
        y32 = torch.empty(rows, d, device=dev)
        if K.ln_fwd_twin(x, i["w"], i["b"], y, y32, mean, rstd, rows, d, X.LN_EPS):
            out["y32"] = y32
        else:
            assert d % 4, "the twin kernel refused a vector-layout row"
    if kind == "sel":
        K.ln_fwd_sel(x, i["w"], i["b"], y, mean, rstd, rows, d, X.LN_EPS, MASK, S, rows // 2)
    elif "y32" not in out:
        K.ln_fwd(x, i["w"], i["b"], y, mean, rstd, rows, d, X.LN_EPS)
    torch.cuda.synchronize()
    return out


def _params(d: int, affine: bool):
    i = _inputs(d, affine)
    if not affine:
        return None, None
    return torch.nn.Parameter(i["w"].clone()), torch.nn.Parameter(i["b"].clone())


def _same(got, ref, what):
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    n = int(X.bad_bits(got, ref).sum())
    assert not n, f"{what}: {n} elements differ from the wrapper's bits"


def _check_fwd(y, f, rows=None, y32=None):
    lead = y.shape[:-1]
    _same(y, f["y"][:rows].view(*lead, -1), "y")
    if y32 is not None:
        _same(y32, y.float(), "y32 against y.float()")
        if "y32" in f:
            _same(y32, f["y32"][:rows].view(*lead, -1), "y32")


def _check_bwd(K, seen, w, b, f, d, affine, in_dtype, *, dy, dres=None, dy2=None, sel=False, xh16=False):
    """The gradient the Function returned for ``x`` against the backward wrapper on the base rows of ``f``."""
    i = _inputs(d, affine)
    x, mean, rstd = f["x"][:T], f["mean"][:T], f["rstd"][:T]
    dx = torch.empty(T, d, device=dev)
    dx16 = torch.empty(T, d, dtype=BF16, device=dev) if in_dtype == F32 else None
    dw = torch.zeros(d, device=dev) if affine else None
    db = torch.zeros(d, device=dev) if affine else None
    dy = dy.reshape(T, d)
    dres = None if dres is None else dres.reshape(T, d)
    dy2 = None if dy2 is None else dy2.reshape(T, d)
    if xh16:
        K.ln_bwd_xh16(dy, f["y"][:T], rstd, dx, T, d, dres=dres, dx16=dx16)
    elif sel:
        K.ln_bwd_sel(dy, x, mean, rstd, i["w"], dx, dw, db, T, d, MASK, S, dres=dres, dx16=dx16)
    else:
        K.ln_bwd(dy, x, mean, rstd, i["w"], dx, dw, db, T, d, dres=dres, dx16=dx16, dy2=dy2)
    torch.cuda.synchronize()
    assert len(seen) == 1
    g = seen[0]
    if in_dtype == F32:
        _same(g, dx.view(NB, S, d), "dx")
        twin = getattr(g, "_iit_bf16", None)
        assert twin is not None and twin[0] == g.data_ptr() and twin[1] == g._version
        _same(twin[2].view(T, d), dx.bfloat16(), "the bf16 twin of dx")
    else:
        _same(g, dx.view(NB, S, d).to(BF16), "dx in bf16")
    if affine:
        cpu = lambda t: None if t is None else t.cpu()  # noqa: E731
        ref = X.ln_bwd_ref(cpu(dy), cpu(x), cpu(mean), cpu(rstd), cpu(i["w"]), dres=cpu(dres), dy2=cpu(dy2),
                           dead=X.sel_dead(T, S, MASK) if sel else None)
        bad = X.ln_bwd_check({"dx": dx.cpu(), "dw": w.grad.cpu(), "db": b.grad.cpu()}, ref)
        bad = {n: int(m.sum()) for n, m in bad.items() if int(m.sum())}
        assert not bad, bad


def _x(d, affine, in_dtype, seen):
    """(leaf, tapped view of it) of the base rows in ``in_dtype``."""
    leaf = _inputs(d, affine)["x"][:T].view(NB, S, d).to(in_dtype, copy=True).requires_grad_(True)
    return leaf, _Tap.apply(leaf, seen)


def _x_full(d, affine):
    return _inputs(d, affine)["x"].view(2 * NB, S, d)


@functools.lru_cache(maxsize=None)
def _bf16_ref(K, d: int, affine: bool) -> dict:
    """``_fwd_ref`` of the bf16-rounded base rows (the unpaired Functions widen a bf16 input first)."""
    i = _inputs(d, affine)
    x = i["x"][:T].to(BF16).float().contiguous()
    y = torch.empty(T, d, dtype=BF16, device=dev)
    mean, rstd = torch.empty(T, device=dev), torch.empty(T, device=dev)
    K.ln_fwd(x, i["w"], i["b"], y, mean, rstd, T, d, X.LN_EPS)
    torch.cuda.synchronize()
    return {"x": x, "y": y, "mean": mean, "rstd": rstd}


CASES = [(d, affine) for d in D for affine in (True, False)]


# ================================================================================================ unpaired
@pytest.mark.parametrize("in_dtype", [F32, BF16])
@pytest.mark.parametrize("d,affine", CASES)
def test_layer_norm_fn(K, O, d, affine, in_dtype):
    i = _inputs(d, affine)
    f = _fwd_ref(K, d, affine, T, "plain") if in_dtype == F32 else _bf16_ref(K, d, affine)
    seen = []
    _, x = _x(d, affine, in_dtype, seen)
    w, b = _params(d, affine)
    y = O.LayerNormFn.apply(x, w, b, X.LN_EPS)
    _check_fwd(y, f)
    y.backward(i["dy"].view_as(y))
    _check_bwd(K, seen, w, b, f, d, affine, in_dtype, dy=i["dy"])


@pytest.mark.parametrize("use", ["both", "dy", "dy32"])
@pytest.mark.parametrize("d,affine", CASES)
def test_layer_norm_twin_fn(K, O, d, affine, use):
    i = _inputs(d, affine)
    f = _fwd_ref(K, d, affine, T, "twin")
    seen = []
    _, x = _x(d, affine, F32, seen)
    w, b = _params(d, affine)
    y, y32 = O.LayerNormTwinFn.apply(x, w, b, X.LN_EPS)
    _check_fwd(y, f, y32=y32)
    dy, dy32 = i["dy"].view_as(y), i["dy32"].view_as(y32)
    if use == "both":
        torch.autograd.backward([y, y32], [dy, dy32])
        _check_bwd(K, seen, w, b, f, d, affine, F32, dy=i["dy"], dy2=i["dy32"])
    elif use == "dy":
        y.backward(dy)
        _check_bwd(K, seen, w, b, f, d, affine, F32, dy=i["dy"])
    else:
        y32.backward(dy32)
        _check_bwd(K, seen, w, b, f, d, affine, F32, dy=i["dy32"])


@pytest.mark.parametrize("in_dtype,use", [(F32, "both"), (F32, "dy"), (F32, "dpass"), (BF16, "both")])
@pytest.mark.parametrize("d,affine", CASES)
def test_layer_norm_fork_fn(K, O, d, affine, in_dtype, use):
    i = _inputs(d, affine)
    f = _fwd_ref(K, d, affine, T, "plain") if in_dtype == F32 else _bf16_ref(K, d, affine)
    seen = []
    leaf, x = _x(d, affine, in_dtype, seen)
    w, b = _params(d, affine)
    y, xpass = O.LayerNormForkFn.apply(x, w, b, X.LN_EPS)
    _check_fwd(y, f)
    _same(xpass, leaf.detach(), "the passthrough")
    dy, dpass = i["dy"].view_as(y), i["dpass"].view_as(y).to(in_dtype)
    xh16 = not affine and d % 4 == 0
    if use == "both":
        torch.autograd.backward([y, xpass], [dy, dpass])
        _check_bwd(K, seen, w, b, f, d, affine, in_dtype, dy=i["dy"], dres=dpass.float(), xh16=xh16)
    elif use == "dy":
        y.backward(dy)
        _check_bwd(K, seen, w, b, f, d, affine, in_dtype, dy=i["dy"], xh16=xh16)
    else:  # only the passthrough is used: its gradient goes through untouched and the parameters get none
        xpass.backward(dpass)
        assert len(seen) == 1
        _same(seen[0], dpass, "the passthrough gradient")
        assert w is None or (w.grad is None and b.grad is None)


# ================================================================================================ paired
@pytest.mark.parametrize("use", ["both", "dy"])
@pytest.mark.parametrize("d,affine", CASES)
def test_layer_norm_fork_pair_fn(K, O, d, affine, use):
    i = _inputs(d, affine)
    f = _fwd_ref(K, d, affine, T2, "plain")
    seen = []
    leaf, x = _x(d, affine, F32, seen)
    w, b = _params(d, affine)
    box = []
    y, xpass = O.LayerNormForkPairFn.apply(x, w, b, X.LN_EPS, _x_full(d, affine), box)
    assert len(box) == 1
    _check_fwd(box[0], f)
    _check_fwd(y, f, rows=T)
    _same(xpass, leaf.detach(), "the passthrough")
    xh16 = not affine and d % 4 == 0
    if use == "both":
        torch.autograd.backward([y, xpass], [i["dy"].view_as(y), i["dpass"].view_as(y)])
        _check_bwd(K, seen, w, b, f, d, affine, F32, dy=i["dy"], dres=i["dpass"], xh16=xh16)
    else:
        y.backward(i["dy"].view_as(y))
        _check_bwd(K, seen, w, b, f, d, affine, F32, dy=i["dy"], xh16=xh16)


@pytest.mark.parametrize("use", ["both", "dy32"])
@pytest.mark.parametrize("d,affine", CASES)
def test_layer_norm_pair_twin_fn(K, O, d, affine, use):
    i = _inputs(d, affine)
    f = _fwd_ref(K, d, affine, T2, "twin")
    seen = []
    _, x = _x(d, affine, F32, seen)
    w, b = _params(d, affine)
    box = []
    y, y32 = O.LayerNormPairTwinFn.apply(x, w, b, X.LN_EPS, _x_full(d, affine), box)
    assert len(box) == 1 and len(box[0]) == 2
    _check_fwd(box[0][0], f, y32=box[0][1])
    _check_fwd(y, f, rows=T, y32=y32)
    if use == "both":
        torch.autograd.backward([y, y32], [i["dy"].view_as(y), i["dy32"].view_as(y32)])
        _check_bwd(K, seen, w, b, f, d, affine, F32, dy=i["dy"], dy2=i["dy32"])
    else:
        y32.backward(i["dy32"].view_as(y32))
        _check_bwd(K, seen, w, b, f, d, affine, F32, dy=i["dy32"])


@pytest.mark.parametrize("mask", [0, MASK])
@pytest.mark.parametrize("d,affine", CASES)
def test_layer_norm_pair_fn(K, O, d, affine, mask):
    i = _inputs(d, affine)
    f = _fwd_ref(K, d, affine, T2, "sel" if mask else "plain")
    seen = []
    _, x = _x(d, affine, F32, seen)
    w, b = _params(d, affine)
    box = []
    y = O.LayerNormPairFn.apply(x, w, b, X.LN_EPS, _x_full(d, affine), box, mask)
    assert len(box) == 1
    _check_fwd(box[0], f)
    _check_fwd(y, f, rows=T)
    y.backward(i["dy"].view_as(y))
    _check_bwd(K, seen, w, b, f, d, affine, F32, dy=i["dy"], sel=bool(mask))


# ================================================================================================ no gradient at all
def test_early_returns(O):
    """With no output gradient the backward returns before it touches ``ctx``: one None per forward input (the
    passthrough's gradient first for the Fork classes).  The engine never makes these calls with every gradient
    missing, so they are made directly."""
    ctx = types.SimpleNamespace(sel=(0, S))
    g = torch.zeros(1)
    assert O.LayerNormFn.backward(ctx, None) == (None,) * 4
    assert O.LayerNormTwinFn.backward(ctx, None, None) == (None,) * 4
    assert O.LayerNormPairTwinFn.backward(ctx, None, None) == (None,) * 6
    assert O.LayerNormPairFn.backward(ctx, None) == (None,) * 7
    assert O.LayerNormPairFn.backward(types.SimpleNamespace(sel=(MASK, S)), None) == (None,) * 7
    for cls, n in ((O.LayerNormForkFn, 4), (O.LayerNormForkPairFn, 6)):
        out = cls.backward(ctx, None, g)
        assert len(out) == n and out[0] is g and out[1:] == (None,) * (n - 1)
        assert cls.backward(ctx, None, None) == (None,) * n
