"""The nine projection autograd Functions of iit_amd/ops/hip_ops.py, addressed directly: ``QKVFn``, ``LinearFn``,
``UnembedFn``, ``MLPInFn``, ``MLPOutGeluFn`` and the paired ``QKVPairFn``, ``LinearPairFn``, ``MLPInPairFn``,
``MLPOutGeluPairFn``.

Operands are the small integers of tests/gemm_exact_util.py (|activation| <= 3, |weight| <= 2, |bias| <= 5,
|residual| <= 50; |x|, |W_in| <= 1 where a pre-activation has to be exact in bf16), so every product sum is exact in
fp32 whatever tile, split or launch the dispatcher picks -- the longest reductions are K = 3HD = 384 (at most 2304,
twice that after two accumulated backwards) and K = 1027 (at most 12324), far below 2^24 (asserted below, on the
CPU, when the module is collected) -- and results are compared bitwise
(``bad_f32`` / ``bad_bf16`` against ``exact_mm``) with no decision pinned.  The two GELU epilogues are held to
``bad_gelu`` / ``bad_dgelu``.  Where an operand is not integer-valued -- the ``dgelu``-produced ``dpre`` of
``MLPInFn``'s ``gpost`` path, and the column sums of ``MLPOutGeluFn``'s DGELU output (the ``b_in`` gradient) -- the
older ``norm_ratio < 1e-2`` applies.

Parameters: a one-block ``HookedTransformer`` on the ``hip`` backend with integer matrices and biases, once with plain
parameters (copy-mode shadow, gradients through ``_grad_slot``) and once under the flat arena as ``make_optimizer``
builds it (mirror-mode shadow, claimed stores, packed QKV gradient and bias, norm slots).  d_model 128, 2 heads of 64,
d_mlp 256, vocabulary 1027; 2 base + 2 source sequences of S = 64 (128 base rows) and S = 3 (6 base rows).

Every case runs two accumulating backwards (the gradients hold the value, then twice the value) and, under the arena,
a third after ``zero_grad`` (the claimed store), with a ``grad_hooks`` listener (each parameter once per backward, biases
before weights) and in three modes: the dispatcher's own choice, ``gemm_dispatch.DUAL`` off (the serial branch), and
the dual launch forced through ``gemm_dispatch.FORCE`` for the pair keys a warm-up created, where a spy on
``hip_kernels.gemm_dual`` sees one launch per backward whose ``prefetch`` is the previous registration.

Measured on an MI355X: 277 cases, 277 passed, none skipped, 8.9 s for the module (9.3 s on the commit before the
Functions shared their forwards and their weight-gradient tail, which passes it unchanged); the slowest case is the
first (1.9 s: the in-process timing of its GEMM candidates), every other case below 0.75 s.
"""
import types

import pytest
import torch

import gemm_exact_util as X

pytestmark = pytest.mark.gpu

dev = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
D, H, DH, DM, V = 128, 2, 64, 256, 1027
HD = H * DH
NB = 2  # base sequences (as many source sequences)
SEQS = [64, 3]
RATIO = 1e-2  # the norm_ratio bound of the older tolerance tests
# the largest |value| of any exact comparison: a reduction over K of |a| |b| products, twice for the second accumulated
# backward, plus bias and residual (UnembedFn's "both" gradient is the sum of two: |g| <= 2 A_MAX)
for _k, _a, _b in ((3 * HD, X.A_MAX, X.B_MAX), (V, 2 * X.A_MAX, X.B_MAX), (NB * 64, X.A_MAX, 2 * X.A_MAX),
                   (DM, X.A_MAX, X.B_MAX), (D, X.A_MAX, X.B_MAX)):
    assert 2 * _k * _a * _b + X.BIAS_MAX + X.ADD_MAX < 2 ** 24


# ================================================================================================ model and operands
_MODELS = {}


def _model(setup: str):
    """The one-block model of ``setup`` ("plain" / "arena") with integer parameters; built once per set-up."""
    if setup in _MODELS:
        return _MODELS[setup]
    from iit_amd.models.config import gpt2_config_dict
    from iit_amd.models.transformer import HookedTransformer
    cfg = gpt2_config_dict()
    cfg.update(n_layers=1, d_model=D, n_heads=H, d_head=DH, d_mlp=DM, d_vocab=V, d_vocab_out=V, n_ctx=64,
               device="cuda:0", dtype=BF16)
    m = HookedTransformer(cfg)
    m.set_op_backend("hip")
    a, mlp, ue = m.blocks[0].attn, m.blocks[0].mlp, m.unembed
    ranges = [(a.W_Q, X.B_MAX), (a.W_K, X.B_MAX), (a.W_V, X.B_MAX), (a.W_O, X.B_MAX), (mlp.W_in, X.UNIT_MAX),
              (mlp.W_out, X.B_MAX), (ue.W_U, X.B_MAX), (a.b_Q, X.BIAS_MAX), (a.b_K, X.BIAS_MAX), (a.b_V, X.BIAS_MAX),
              (a.b_O, X.BIAS_MAX), (mlp.b_in, X.BIAS_MAX), (mlp.b_out, X.BIAS_MAX), (ue.b_U, X.BIAS_MAX)]
    with torch.no_grad():
        for i, (p, hi) in enumerate(ranges):
            p.copy_(X.ints(p.shape, -hi, hi, seed=100 + i, device=dev))
    m.mark_weights_changed()
    flat = None
    if setup == "arena":
        from iit_amd.engine.flat import FlatParams
        flat = FlatParams(m, with_bf16_shadow=getattr(m, "wants_bf16_shadow", False))
        flat.norm_fuse = True  # what make_optimizer sets for one process
    ops = m.ops()
    ops.begin_forward()
    assert ops.shadow.mode == ("mirror" if flat is not None else "copy")
    _MODELS[setup] = types.SimpleNamespace(m=m, ops=ops, flat=flat, attn=a, mlp=mlp, ue=ue, L=ops.shadow.layers[0],
                                           qkv_bias16=ops.shadow.biases[0])
    return _MODELS[setup]


def _ints(shape, hi, seed, dtype=BF16):
    return X.ints(shape, -hi, hi, seed=seed, device=dev).to(dtype)


def _acts(S, width, seed, hi=X.A_MAX, dtype=BF16):
    """(base rows [NB, S, width], full rows [2 NB, S, width]): the base rows are the first half of the full ones."""
    full = _ints((2 * NB, S, width), hi, seed, dtype)
    return full[:NB], full


def _bad(mask) -> int:
    return int(mask.sum())


def _f32_is(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    n = _bad(X.bad_f32(got, ref))
    assert not n, f"{what}: {n} of {got.numel()} fp32 elements differ from the exact result"


def _bf16_is(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    n = _bad(X.bad_bf16(got, ref))
    assert not n, f"{what}: {n} of {got.numel()} bf16 elements differ from the exact result rounded once"


def _close(got, ref, what):
    r = X.norm_ratio(got, ref)
    print(f"{what}: norm ratio {r:.3e}")
    assert r < RATIO, (what, r)


class _Tap(torch.autograd.Function):
    """Identity in front of the Function under test: its backward is handed the gradient tensor that Function
    returned, attributes included -- the way the next backward of a model receives it."""

    @staticmethod
    def forward(ctx, x, seen):
        ctx.seen = seen
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        ctx.seen.append(g)
        return g, None


# ================================================================================================ the driver
@pytest.fixture(params=["plain-auto", "plain-serial", "plain-dual", "arena-auto", "arena-serial", "arena-dual"])
def env(request, monkeypatch):
    from iit_amd.engine import grad_hooks
    from iit_amd.ops import gemm_dispatch, hip_kernels, hip_ops
    hip_kernels.lib()
    setup, mode = request.param.split("-")
    e = _model(setup)
    e.ops.begin_forward()
    notified, duals = [], []
    listener = grad_hooks.add_listener(lambda p: notified.append(id(p)))
    real_dual = hip_kernels.gemm_dual

    def spy(*a, **kw):
        if "prefetch" in kw:  # the launch of gemm_pair itself (the candidates it times pass none)
            duals.append(kw["prefetch"])
        return real_dual(*a, **kw)

    monkeypatch.setattr(hip_kernels, "gemm_dual", spy)
    if mode == "serial":
        monkeypatch.setattr(gemm_dispatch, "DUAL", False)
    yield types.SimpleNamespace(e=e, setup=setup, mode=mode, O=hip_ops, G=gemm_dispatch, K=hip_kernels,
                                notified=notified, duals=duals, monkeypatch=monkeypatch)
    grad_hooks.remove_listener(listener)


def _reset_grads(e):
    if e.flat is None:
        for p in e.m.parameters():
            p.grad = None
    else:  # every gradient a zeroed arena view: the first backward accumulates
        e.flat.zero_grad()
        e.flat.grad.zero_()
        e.flat.rebind_grads()
        if e.flat.gsq is not None:
            e.flat.gsq.zero_()


def _drive(env, one_pass, params, order, dual_expected, one_pair=True):
    """Run ``one_pass(scale, check)`` -- forward, checks of the outputs, backward, checks of the input gradients and,
    with ``scale`` s, of every parameter gradient against s times its value -- for two accumulating backwards and,
    under the arena, a third after ``zero_grad``.  ``params``: the parameters the Function writes; ``order``: the
    notifications of one backward; ``dual_expected``: a dual launch covers the pair; ``one_pair``: the backward
    runs one pair, whose prefetch is then the sentinel registered before the forward."""
    e, O, G = env.e, env.O, env.G
    sentinel = (torch.zeros(64, dtype=BF16, device=dev), torch.zeros(64, dtype=BF16, device=dev))

    def sequence(check):
        _reset_grads(e)
        for step, scale in enumerate((1, 2, 1) if e.flat is not None else (1, 2)):
            if step == 2:
                e.flat.zero_grad()  # claimed slots are now None: this backward stores
            O._PF_SEQ.clear()
            O._PF_ON[0] = True
            O._PF_SEQ.append(sentinel)
            del env.notified[:], env.duals[:]
            one_pass(scale, check)
            torch.cuda.synchronize()
            if not check:
                continue
            assert env.notified == [id(p) for p in order], "notifications of one backward"
            if env.mode == "serial" or not dual_expected:
                assert not env.duals
            elif not one_pair:
                pass
            elif env.mode == "dual":
                assert len(env.duals) == 1 and env.duals[0] is sentinel, "one dual launch, prefetching the sentinel"
            else:
                assert all(pf is sentinel for pf in env.duals)
            if step == 2 and e.flat._norm_covered:  # the store added the gradients' sums of squares
                want = sum(float(p.grad.double().pow(2).sum()) for p in params
                           if e.flat.index[id(p)] in e.flat._norm_covered)
                got = float(e.flat.gsq.double().sum())
                assert abs(got - want) <= 1e-4 * want, (got, want)

    if env.mode == "dual" and one_pair:
        pairs = []
        real_pair = O.gemm_pair
        with env.monkeypatch.context() as mp:
            mp.setattr(O, "gemm_pair", lambda x, w, prefetch=None: (pairs.append((x, w)),
                                                                    real_pair(x, w, prefetch=prefetch))[1])
            sequence(False)  # the warm-up: every pair key of the sequence is decided
        names = None
        for x, w in pairs:
            c = list(G._dual_candidates(x, w, x["C"], w["C"], x.get("colsum"), w.get("bsum"), w.get("gsq"))) \
                if G._dual_eligible(x, w) else []
            names = c if names is None else [n for n in names if n in c]
        assert bool(names) == dual_expected, (names, dual_expected)
        if names:
            for key in G.DUAL_DECISIONS:
                env.monkeypatch.setitem(G.FORCE, key, names[0])
    sequence(True)


def _registered(O, saved, w):
    """The forward registered its saved base rows and its weight for the prefetch of the pair before it."""
    x2, ww = O._PF_SEQ[-1]
    assert len(O._PF_SEQ) == 2 and ww is w
    assert (x2.data_ptr(), x2.shape, x2.stride()) == (saved.data_ptr(), saved.shape, saved.stride())


def _wgrad(x2, g2):
    return X.exact_mm(x2.float().t(), g2.float())


# ================================================================================================ QKV
@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("S", SEQS)
def test_qkv(env, S, paired):
    e, O, a = env.e, env.O, env.e.attn
    T = NB * S
    xb, xf = _acts(S, D, seed=1)
    rows = xf if paired else xb
    Wp = torch.cat([W.detach().permute(1, 0, 2).reshape(D, HD) for W in (a.W_Q, a.W_K, a.W_V)], dim=1)
    bp = torch.cat([b.detach().reshape(HD) for b in (a.b_Q, a.b_K, a.b_V)])
    ref = (X.exact_mm(rows.reshape(-1, D).float(), Wp) + bp).view(-1, S, 3, H, DH)
    g = _ints((NB, S, 3, H, DH), X.A_MAX, seed=2)
    g2, x2 = g.view(T, 3 * HD), xb.reshape(T, D)
    ref_dx = X.exact_mm(g2.float(), Wp.t()).view(NB, S, D)
    ref_dW = _wgrad(x2, g2).view(D, 3, H, DH).permute(1, 2, 0, 3)  # [3][H][d][dh]
    ref_db = g2.float().sum(0).view(3, H, DH)
    Ws, bs = (a.W_Q, a.W_K, a.W_V), (a.b_Q, a.b_K, a.b_V)

    def one_pass(scale, check):
        leaf = xb.clone().requires_grad_(True)
        args = (leaf, e.L, e.qkv_bias16) + Ws + bs
        if paired:
            box = []
            out = O.QKVPairFn.apply(*args, xf, box)
        else:
            out = O.QKVFn.apply(*args)
        if check:
            if paired:
                assert len(box) == 1 and box[0].shape == (2 * NB, S, 3, H, DH)
                _bf16_is(box[0], ref, "box")
                assert out.data_ptr() == box[0].data_ptr() and out.shape == (NB, S, 3, H, DH)
            _bf16_is(out, ref[:NB], "qkv")
            _registered(O, out.grad_fn.saved_tensors[0], e.L["qkv"])
        out.backward(g)
        if check:
            _bf16_is(leaf.grad, ref_dx, "dx")
            for i in range(3):
                _f32_is(Ws[i].grad, scale * ref_dW[i], "dW_" + "QKV"[i])
                _f32_is(bs[i].grad, scale * ref_db[i], "db_" + "QKV"[i])

    # plain parameters are not one packed [d][3HD] matrix: the scatter epilogue, no pair
    _drive(env, one_pass, Ws + bs, bs + Ws, dual_expected=S == 64 and env.setup == "arena")


# ================================================================================================ linear
LINEAR = [("bf16", False, BF16), ("resid", False, BF16), ("f32", False, F32), ("bf16", True, BF16),
          ("resid", True, BF16), ("bf16-nox", False, BF16)]


@pytest.mark.parametrize("kind,paired,x_dtype", LINEAR)
@pytest.mark.parametrize("S", SEQS)
def test_linear(env, S, kind, paired, x_dtype):
    """``bf16``: the attention output projection (a 3-D weight whose gradient is reshaped); ``resid`` / ``f32``: the
    MLP output matrix (K = 256); ``f32`` with an fp32 input (the cast of dx); ``nox``: no input gradient, the weight
    gradient alone."""
    e, O = env.e, env.O
    nox = kind.endswith("-nox")
    kind = kind.split("-")[0]
    T = NB * S
    if kind == "bf16":
        W, b, w, Kd = e.attn.W_O, e.attn.b_O, e.L["o"], HD
    else:
        W, b, w, Kd = e.mlp.W_out, e.mlp.b_out, e.L["out"], DM
    W2 = W.detach().reshape(Kd, D)
    xb, xf = _acts(S, Kd, seed=3, dtype=x_dtype)
    rb, rf = _acts(S, D, seed=4, hi=X.ADD_MAX, dtype=F32)
    rows = xf if paired else xb
    ref = (X.exact_mm(rows.reshape(-1, Kd).float(), W2) + b.detach()).view(-1, S, D)
    if kind == "resid":
        ref = ref + (rf if paired else rb)
    g = _ints((NB, S, D), X.A_MAX, seed=5, dtype=BF16 if kind == "bf16" else F32)
    g2, x2 = g.view(T, D), xb.reshape(T, Kd)
    ref_dx = X.exact_mm(g2.float(), W2.t()).view(NB, S, Kd)
    ref_dW, ref_db = _wgrad(x2, g2).view_as(W), g2.float().sum(0)

    def one_pass(scale, check):
        leaf = xb.clone().requires_grad_(not nox)
        res = rb.clone().requires_grad_(True) if kind == "resid" else None
        if paired:
            box = []
            out = O.LinearPairFn.apply(leaf, W, b, w, D, res, kind, xf, rf if kind == "resid" else None, box)
        else:
            out = O.LinearFn.apply(leaf, W, b, w, D, res, kind)
        if check:
            same = _bf16_is if kind == "bf16" else _f32_is
            if paired:
                assert len(box) == 1
                same(box[0], ref, "box")
                assert out.data_ptr() == box[0].data_ptr()
            same(out, ref[:NB], "out")
            assert out.shape == (NB, S, D) and out.stride(-2) == O._pad8(D)
            _registered(O, out.grad_fn.saved_tensors[0], w)
        out.backward(g)
        if check:
            if nox:
                assert leaf.grad is None
            elif x_dtype == BF16:
                _bf16_is(leaf.grad, ref_dx, "dx")
            else:  # the bf16 result, cast to the input's dtype
                _f32_is(leaf.grad, ref_dx.bfloat16().float(), "dx")
            if res is not None:
                _f32_is(res.grad, g, "the residual's gradient")
            _f32_is(W.grad, scale * ref_dW, "dW")
            _f32_is(b.grad, scale * ref_db, "db")

    _drive(env, one_pass, (W, b), (b, W), dual_expected=S == 64 and not nox)


@pytest.mark.parametrize("use", ["handle", "both"])
@pytest.mark.parametrize("S", SEQS)
def test_unembed(env, S, use):
    """Vocabulary 1027: padded fp32 rows, the ragged GEMMs, and the split-K fp32 input gradient (K >= 1024), which is
    never paired.  The gradient arrives through the bf16 handle, or through the handle and the logits."""
    e, O, W, b = env.e, env.O, env.e.ue.W_U, env.e.ue.b_U
    T = NB * S
    sh = e.ops.shadow
    assert sh.Vp == 1032 and O.K._tiling(T, D, V, True)[1] > 1
    xb, _ = _acts(S, D, seed=6)
    x2 = xb.reshape(T, D)
    ref = (X.exact_mm(x2.float(), W.detach()) + b.detach()).view(NB, S, V)
    gh = _ints((NB, S, V), X.A_MAX, seed=7)
    gl = _ints((NB, S, V), X.A_MAX, seed=8, dtype=F32)
    g2 = (gh.float() + (gl if use == "both" else 0)).view(T, V)
    ref_dx = X.exact_mm(g2, W.detach().t()).view(NB, S, D)
    ref_dW, ref_db = _wgrad(x2, g2), g2.sum(0)

    def one_pass(scale, check):
        leaf = xb.clone().requires_grad_(True)
        logits, handle = O.UnembedFn.apply(leaf, W, b, sh.U, sh.Vp)
        if check:
            _f32_is(logits, ref, "logits")
            assert logits.stride(-2) == sh.Vp and handle.shape == logits.shape and handle.dtype == BF16
            assert handle.stride() == (0, 0, 0) and handle.requires_grad
            _registered(O, logits.grad_fn.saved_tensors[0], sh.U)
        if use == "both":
            torch.autograd.backward([logits, handle], [gl, gh])
        else:
            handle.backward(gh)
        if check:
            _bf16_is(leaf.grad, ref_dx, "dx")
            _f32_is(W.grad, scale * ref_dW, "dW")
            _f32_is(b.grad, scale * ref_db, "db")

    _drive(env, one_pass, (W, b), (b, W), dual_expected=False)


# ================================================================================================ MLP in
def _spec(S):
    from iit_amd.core.index import Ix
    from iit_amd.ops.splice import patch_spec
    index = Ix[:, 1, 8:24]
    spec = patch_spec(index, (NB, S, DM))
    assert spec is not None
    return index.as_index, spec


MLP_IN = [(False, False, "both", False), (False, True, "gpost", False), (False, False, "gpre", False),
          (True, False, "both", False), (True, True, "gpre", False), (True, False, "both", True),
          (True, False, "gpost", True)]


@pytest.mark.parametrize("paired,erf,use,spliced", MLP_IN)
@pytest.mark.parametrize("S", SEQS)
def test_mlp_in(env, S, paired, erf, use, spliced):
    e, O, W, b, w = env.e, env.O, env.e.mlp.W_in, env.e.mlp.b_in, env.e.L["in"]
    T = NB * S
    xb, xf = _acts(S, D, seed=9, hi=X.UNIT_MAX)
    rows = xf if paired else xb
    pre = (X.exact_mm(rows.reshape(-1, D).float(), W.detach()) + b.detach()).view(-1, S, DM)
    assert float(pre.abs().max()) <= 256  # exact in bf16
    act = pre.clone()  # what ``post`` is the GELU of: the spliced elements take the source rows' value
    idx, spec = _spec(S) if spliced else (None, None)
    if spliced:
        act[:NB][idx] = pre[NB:][idx]
    gpre = _ints((NB, S, DM), X.A_MAX, seed=10) if use != "gpost" else None
    gpost = _ints((NB, S, DM), X.A_MAX, seed=11) if use != "gpre" else None
    x2 = xb.reshape(T, D)
    dpre = torch.zeros(NB, S, DM, dtype=torch.float64, device=dev)
    if gpost is not None:
        dpre = gpost.double() * X.dgelu64(pre[:NB], erf)
        if spliced:
            dpre[idx] = 0.0
    if gpre is not None:
        dpre = dpre + gpre.double()
    d2 = dpre.view(T, DM)
    ref_dx = (d2 @ W.detach().double().t()).view(NB, S, D)
    ref_dW, ref_db = x2.double().t() @ d2, d2.sum(0)
    exact = gpost is None  # an integer dpre: bitwise

    def one_pass(scale, check):
        leaf = xb.clone().requires_grad_(True)
        if paired:
            box = []
            p, q = O.MLPInPairFn.apply(leaf, W, b, w, erf, xf, spec, box)
        else:
            p, q = O.MLPInFn.apply(leaf, W, b, w, erf)
        if check:
            if paired:
                assert len(box) == 1 and len(box[0]) == 2
                _bf16_is(box[0][0], pre, "box pre")
                assert not _bad(X.bad_gelu(box[0][1], act, erf)), "box post"
                assert p.data_ptr() == box[0][0].data_ptr() and q.data_ptr() == box[0][1].data_ptr()
                if spliced:
                    assert not _bad(X.bad_bits(box[0][1][:NB][idx], box[0][1][NB:][idx])), "the spliced elements"
            _bf16_is(p, pre[:NB], "pre")
            assert not _bad(X.bad_gelu(q, act[:NB], erf)), "post"
            saved = p.grad_fn.saved_tensors
            _registered(O, saved[0], w)
            assert saved[1].data_ptr() == p.data_ptr() and saved[1].shape == (T, DM)
        outs, gs = zip(*[(t, gt) for t, gt in ((p, gpre), (q, gpost)) if gt is not None])
        torch.autograd.backward(outs, gs)
        if check:
            if exact:
                _bf16_is(leaf.grad, ref_dx.float(), "dx")
                _f32_is(W.grad, scale * ref_dW.float(), "dW")
                _f32_is(b.grad, scale * ref_db.float(), "db")
            else:
                _close(leaf.grad, ref_dx, "dx")
                _close(W.grad, scale * ref_dW, "dW")
                _close(b.grad, scale * ref_db, "db")

    _drive(env, one_pass, (W, b), (b, W), dual_expected=S == 64)


# ================================================================================================ MLP out
@pytest.mark.parametrize("paired,erf,nox", [(False, False, False), (False, True, False), (True, False, False),
                                            (True, True, False), (False, False, True)])
@pytest.mark.parametrize("S", SEQS)
def test_mlp_out_gelu(env, S, paired, erf, nox):
    """``pre`` and ``post`` are independent integers here (``post`` enters as data).  ``nox``: ``pre`` needs no
    gradient, the weight gradient runs alone."""
    e, O, mlp, w = env.e, env.O, env.e.mlp, env.e.L["out"]
    W, b, b_in = mlp.W_out, mlp.b_out, mlp.b_in
    T = NB * S
    pb, _ = _acts(S, DM, seed=12)
    qb, qf = _acts(S, DM, seed=13)
    rb, rf = _acts(S, D, seed=14, hi=X.ADD_MAX, dtype=F32)
    rows = qf if paired else qb
    ref = (X.exact_mm(rows.reshape(-1, DM).float(), W.detach()) + b.detach()).view(-1, S, D) + (rf if paired else rb)
    g = _ints((NB, S, D), X.A_MAX, seed=15, dtype=F32)
    g2 = g.view(T, D)
    s = X.exact_mm(g2, W.detach().t()).view(NB, S, DM)
    ref_dW, ref_db = _wgrad(qb.reshape(T, DM), g2), g2.sum(0)
    ref_dbin = (s.double() * X.dgelu64(pb, erf)).view(T, DM).sum(0)

    def one_pass(scale, check):
        seen = []
        leaf = pb.clone().requires_grad_(not nox)
        res = rb.clone().requires_grad_(True)
        pre = leaf if nox else _Tap.apply(leaf, seen)
        if paired:
            box = []
            out = O.MLPOutGeluPairFn.apply(pre, qb, W, b, w, D, res, b_in, erf, qf, rf, box)
        else:
            out = O.MLPOutGeluFn.apply(pre, qb, W, b, w, D, res, b_in, erf)
        if check:
            if paired:
                assert len(box) == 1
                _f32_is(box[0], ref, "box")
                assert out.data_ptr() == box[0].data_ptr()
            _f32_is(out, ref[:NB], "out")
            saved = out.grad_fn.saved_tensors
            _registered(O, saved[0], w)
            assert saved[0].data_ptr() == rows.data_ptr() and saved[1].shape == (T, DM)
        out.backward(g)
        if check:
            _f32_is(res.grad, g, "the residual's gradient")
            _f32_is(W.grad, scale * ref_dW, "dW")
            _f32_is(b.grad, scale * ref_db, "db")
            if nox:
                assert leaf.grad is None and (b_in.grad is None or not bool(b_in.grad.any()))
            else:
                (dpre,) = seen
                assert not _bad(X.bad_dgelu(dpre, s, pb, erf)), "dpre"
                assert dpre._iit_bias_sum == (dpre.data_ptr(), dpre._version, id(b_in))
                _close(b_in.grad, scale * ref_dbin, "db_in")

    # DGELU_ERF is no dual epilogue: the erf pair runs serially
    _drive(env, one_pass, (W, b, b_in), (b, W), dual_expected=S == 64 and not erf and not nox)


@pytest.mark.parametrize("S", SEQS)
def test_mlp_chain_bias_once(env, S):
    """``HipOps.mlp_gelu_residual``: MLPOutGeluFn's DGELU epilogue sums ``b_in``'s gradient and tags ``dpre``, so
    MLPInFn adds no second column sum; it still reports ``b_in``, before ``W_in``."""
    e, mlp = env.e, env.e.mlp
    T = NB * S
    xb, _ = _acts(S, D, seed=16, hi=X.UNIT_MAX)
    rb, _ = _acts(S, D, seed=17, hi=X.ADD_MAX, dtype=F32)
    g = _ints((NB, S, D), X.A_MAX, seed=18, dtype=F32)
    pre = (X.exact_mm(xb.reshape(T, D).float(), mlp.W_in.detach()) + mlp.b_in.detach())
    s = X.exact_mm(g.view(T, D), mlp.W_out.detach().t())
    ref_dbin = (s.double() * X.dgelu64(pre, False)).sum(0)

    def one_pass(scale, check):
        leaf = xb.clone().requires_grad_(True)
        out = e.ops.mlp_gelu_residual(leaf, mlp.W_in, mlp.b_in, mlp.W_out, mlp.b_out, rb)
        out.backward(g)
        if check:
            _close(mlp.b_in.grad, scale * ref_dbin, "db_in")

    params = (mlp.W_out, mlp.b_out, mlp.W_in, mlp.b_in)
    _drive(env, one_pass, params, (mlp.b_out, mlp.W_out, mlp.b_in, mlp.W_in), dual_expected=S == 64, one_pair=False)


# ================================================================================================ no gradient at all
def test_early_returns():
    """With no output gradient the backward returns before it touches ``ctx``: one None per forward input.  The
    engine never makes these calls with every gradient missing, so they are made directly."""
    from iit_amd.ops import hip_ops as O
    ctx = types.SimpleNamespace()
    assert O.QKVFn.backward(ctx, None) == (None,) * 9
    assert O.QKVPairFn.backward(ctx, None) == (None,) * 11
    assert O.LinearFn.backward(ctx, None) == (None,) * 7
    assert O.LinearPairFn.backward(ctx, None) == (None,) * 10
    assert O.UnembedFn.backward(ctx, None, None) == (None,) * 5
    assert O.MLPInFn.backward(ctx, None, None) == (None,) * 5
    assert O.MLPInPairFn.backward(ctx, None, None) == (None,) * 8
    assert O.MLPOutGeluFn.backward(ctx, None) == (None,) * 9
    assert O.MLPOutGeluPairFn.backward(ctx, None) == (None,) * 12
