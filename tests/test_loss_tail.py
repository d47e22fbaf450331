"""The loss tail of a training phase: last-position unembed -> cross-entropy -> their backward.

When the logits come from the fp32 unembed and nothing observes their fp32 gradient, the cross-entropy backward
writes only the bf16 gradient the unembed backward GEMMs read (``ce_bwd16``), handed over through the unembed's
bf16 gradient handle instead of an fp32 [rows][vocab] tensor.  Checked here:

* the bf16-only kernel against the existing kernel's ``out16``, bit for bit, with zeroed row pads and nothing
  written outside its rows -- aligned (vector loads) and unaligned logits rows, vocabularies that are no multiple of 8;
* every other reader still gets the exact fp32 gradient: a tensor hook on the logits, ``retain_grad``, logits of
  another producer; a second autograd consumer of the logits has its gradient summed with the cross-entropy's;
* a two-layer model's train step gives the same parameter gradients through the bf16-only tail as through the fp32
  path run with single (non-dual) GEMM launches, within the per-parameter bound of tests/test_headline_parity.py.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"
SENT = 7.0


def _pad8(n):
    return (n + 7) // 8 * 8


@pytest.fixture(scope="module")
def K():
    from iit_amd.ops import hip_kernels
    hip_kernels.lib()
    return hip_kernels


def _ce_case(K, R, V, ld):
    """fp32 logits [R][ld] (pads NaN), labels (one at the last column), lse from ce_fwd."""
    g = torch.Generator(device="cpu").manual_seed(100 * V + ld)
    store = torch.full((R, ld), float("nan"))
    store[:, :V] = torch.randn(R, V, generator=g) * 3
    logits = store.to(dev)
    labels = torch.randint(0, V, (R,), generator=g)
    labels[-1] = V - 1
    labels = labels.to(dev)
    loss, lse = torch.empty(R, device=dev), torch.empty(R, device=dev)
    K.ce_fwd(logits, ld, labels, loss, lse, None, R, V)
    return logits, labels, lse


@pytest.mark.parametrize("V", [209, 1025])
@pytest.mark.parametrize("aligned", [True, False])
def test_ce_bwd16_equals_twin_bitwise(K, V, aligned):
    R, ldo = 3, _pad8(V)
    ld = ldo if aligned else V  # V odd: rows 1.. start off a 16-byte boundary -> the scalar-load kernel
    logits, labels, lse = _ce_case(K, R, V, ld)
    gs = torch.full((1,), 0.625, device=dev)
    out = torch.full((R, ldo), SENT, device=dev)
    twin = torch.full((R, ldo), SENT, dtype=torch.bfloat16, device=dev)
    K.ce_bwd(logits, ld, labels, lse, gs, 1.0 / R, out, ldo, R, V, out16=twin)
    # rows [1, 1 + R) of a sentinel-filled [R + 2][ldo] buffer: the rows before and after must survive
    whole = torch.full((R + 2, ldo), SENT, dtype=torch.bfloat16, device=dev)
    K.ce_bwd16(logits, ld, labels, lse, gs, 1.0 / R, whole[1:1 + R], ldo, R, V)
    got = whole[1:1 + R]
    assert torch.equal(got.view(torch.int16), twin.view(torch.int16))
    assert got[:, V:].abs().max() == 0 and torch.isfinite(got.float()).all()
    assert (whole[0] == SENT).all() and (whole[-1] == SENT).all()
    p = logits[:, :V].double().softmax(-1)
    ref = (p - torch.nn.functional.one_hot(labels, V)) * 0.625 / R
    # bf16 rounding (2^-9 of the value) of a softmax whose exponent x - lse (|.| < 32) carries a few fp32 ulps of
    # error (__logf, the online sum, the subtraction: under 8 ulp(16) = 2^-16, relative to p)
    assert ((got[:, :V].double() - ref).abs() <= 2.0 ** -8 * ref.abs() + 2.0 ** -16 * p * 0.625 / R).all()


def test_ce_bwd16_rejects_unpadded_output(K):
    logits, labels, lse = _ce_case(K, 3, 209, 216)
    out = torch.empty(3, 209, dtype=torch.bfloat16, device=dev)
    with pytest.raises(RuntimeError):
        K.ce_bwd16(logits, 216, labels, lse, torch.ones(1, device=dev), 1.0 / 3, out, 209, 3, 209)


# ---------------------------------------------------------------------------------------------- autograd routing
def _unembed_setup(V, T=16, d=128):
    """(ops, x, W_U, b_U): a tiny hip-backend model's unembed and a bf16 last-position activation."""
    from iit_amd.models.transformer import HookedTransformer
    cfg = dict(n_layers=2, d_model=d, n_heads=4, d_head=32, d_mlp=4 * d, n_ctx=32, act_fn="gelu_new", d_vocab=V,
               normalization_type="LN", device=dev, initializer_range=0.05, dtype=torch.bfloat16)
    torch.manual_seed(0)
    model = HookedTransformer(cfg)
    model.set_op_backend("hip")
    return model


def _tail(model, x, labels, observe=None, extra=None):
    """Gradients (x, W_U, b_U) of ``cross_entropy(unembed(x))`` (+ ``extra(logits)``)."""
    from iit_amd.ops import cross_entropy
    ops = model.ops()
    ops.begin_forward()  # binds the bf16 shadow of W_U, as every model forward does
    assert ops.shadow.U is not None
    model.zero_grad(set_to_none=True)
    flat = getattr(model, "_flat_params", None)
    x = x.detach().clone().requires_grad_(True)
    logits = ops.unembed(x, model.unembed.W_U, model.unembed.b_U)
    if observe is not None:
        observe(logits)
    loss = cross_entropy(logits, labels)
    if extra is not None:
        loss = loss + extra(logits)
    loss.backward()
    if flat is not None:
        flat.rebind_grads(zero_missing=True)
    return (x.grad.float().clone(), model.unembed.W_U.grad.float().clone(), model.unembed.b_U.grad.float().clone(),
            loss.detach().clone())


@pytest.mark.parametrize("V", [209, 1025])
def test_tail_routes_and_keeps_fp32_for_observers(V, monkeypatch):
    from iit_amd.ops import cross_entropy as cross_entropy_
    from iit_amd.ops import hip_ops
    model = _unembed_setup(V)
    R = 3
    torch.manual_seed(V)
    x = torch.randn(R, 128, device=dev).bfloat16()
    labels = torch.randint(0, V, (R,), device=dev)
    calls = {"16": 0, "32": 0}
    k16, k32 = hip_ops.K.ce_bwd16, hip_ops.K.ce_bwd

    def spy16(*a, **k):
        calls["16"] += 1
        return k16(*a, **k)

    def spy32(*a, **k):
        calls["32"] += 1
        return k32(*a, **k)

    monkeypatch.setattr(hip_ops.K, "ce_bwd16", spy16)
    monkeypatch.setattr(hip_ops.K, "ce_bwd", spy32)

    fused = _tail(model, x, labels)
    assert calls == {"16": 1, "32": 0}
    monkeypatch.setenv("IIT_CE_BF16_ONLY", "0")
    plain = _tail(model, x, labels)
    assert calls == {"16": 1, "32": 1}
    monkeypatch.delenv("IIT_CE_BF16_ONLY")
    # the same bf16 operand reaches the same GEMMs: equal up to the order of atomic fp32 partial sums (split-K over
    # the V terms of dX, the R rows of the column sums): terms * 2^-24 relative to the largest element
    assert torch.equal(fused[3], plain[3])
    for a, b, terms in zip(fused[:3], plain[:3], (V, R, R)):
        print("fused vs plain max diff", float((a - b).abs().max()), "of", float(b.abs().max()))
        assert (a - b).abs().max() <= terms * 2.0 ** -24 * b.abs().max()

    # a tensor hook on the logits sees the exact fp32 gradient (and the result is the plain path's)
    seen = []
    hooked = _tail(model, x, labels, observe=lambda lg: lg.register_hook(lambda g: seen.append(g.clone())))
    assert calls == {"16": 1, "32": 2}
    assert len(seen) == 1 and seen[0].dtype == torch.float32 and seen[0].shape == (R, V)
    lg = model.ops().unembed(x, model.unembed.W_U, model.unembed.b_U).detach()
    p = lg.double().softmax(-1)
    ref = (p - torch.nn.functional.one_hot(labels, V)) / R
    # fp32 throughout: the exponent x - lse (|.| < 32) carries under 8 ulp(16) = 2^-16 of error, relative to p; the
    # subtraction of the one-hot, the two multiplications and 1 / R round the value itself (4 x 2^-24 of |value|)
    assert ((seen[0].double() - ref).abs() <= 2.0 ** -16 * p / R + 2.0 ** -22 * ref.abs() + 1e-12).all()
    assert (hooked[1] - plain[1]).abs().max() <= R * 2.0 ** -24 * plain[1].abs().max()

    # retain_grad is an observer too
    kept = []
    _tail(model, x, labels, observe=lambda t: (t.retain_grad(), kept.append(t)))
    assert calls == {"16": 1, "32": 3}
    assert kept[0].grad is not None and kept[0].grad.dtype == torch.float32
    assert torch.equal(kept[0].grad, seen[0])

    # a second autograd consumer of the logits: its fp32 gradient is summed with the cross-entropy's bf16 one
    both = _tail(model, x, labels, extra=lambda t: 1e-3 * t.float().pow(2).mean())
    assert calls == {"16": 2, "32": 3}
    monkeypatch.setenv("IIT_CE_BF16_ONLY", "0")
    both_plain = _tail(model, x, labels, extra=lambda t: 1e-3 * t.float().pow(2).mean())
    monkeypatch.delenv("IIT_CE_BF16_ONLY")
    assert calls == {"16": 2, "32": 4}
    for a, b in zip(both[:3], both_plain[:3]):
        # the GEMM operand is bf16(g_other + float(bf16(g_ce))) instead of bf16(g_other + g_ce): elementwise within
        # 2^-8 (one extra bf16 rounding and a possible flip of the last one).  The results are linear in it, with
        # well-conditioned random factors (3 x 128 activations, 128 x V weights: condition number under 4)
        print("two consumers, rel diff", float((a - b).norm() / b.norm()))
        assert (a - b).norm() <= 2.0 ** -6 * b.norm()

    # a second cross-entropy on the same logits: the handle carries one bf16 gradient, the other stays fp32
    ops = model.ops()
    lg3 = ops.unembed(x.detach().clone().requires_grad_(True), model.unembed.W_U, model.unembed.b_U)
    (cross_entropy_(lg3, labels) + cross_entropy_(lg3, (labels + 1) % V)).backward()
    assert calls == {"16": 3, "32": 5}

    # logits of another producer (no tag): fp32 path
    from iit_amd.ops import cross_entropy
    other = lg.clone().requires_grad_(True)
    cross_entropy(other, labels).backward()
    assert calls == {"16": 3, "32": 6}
    assert torch.equal(other.grad, seen[0])

    # an in-place change of the logits invalidates the tag (version check)
    model.zero_grad(set_to_none=True)
    lg2 = model.ops().unembed(x.detach().clone().requires_grad_(True), model.unembed.W_U, model.unembed.b_U)
    assert hip_ops._grad16_handle(lg2) is not None
    with torch.no_grad():
        assert hip_ops._grad16_handle(lg2) is None
    lg2.detach().mul_(1.0)  # shares the version counter
    assert hip_ops._grad16_handle(lg2) is None


def test_tiny_model_train_step_same_gradients(monkeypatch):
    """Whole backward of a two-layer model from last-position logits: bf16-only tail with the default GEMM launches
    vs the fp32 gradient path with single launches (no dual dX + dW)."""
    from iit_amd.engine.plan import RunPlan
    from iit_amd.ops import cross_entropy, gemm_dispatch
    V = 1025
    model = _unembed_setup(V)
    torch.manual_seed(1)
    tok = torch.randint(0, V, (8, 16), device=dev)
    labels = torch.randint(0, V, (8,), device=dev)

    def grads():
        model.zero_grad(set_to_none=True)
        loss = cross_entropy(model(tok, plan=RunPlan(logits="last")), labels)
        loss.backward()
        flat = getattr(model, "_flat_params", None)
        if flat is not None:
            flat.rebind_grads(zero_missing=True)
        return loss.detach().clone(), {n: p.grad.detach().float().clone() for n, p in model.named_parameters()
                                       if p.grad is not None}

    lf, gf = grads()
    monkeypatch.setenv("IIT_CE_BF16_ONLY", "0")
    monkeypatch.setattr(gemm_dispatch, "DUAL", False)
    lr, gr = grads()
    assert torch.equal(lf, lr)
    assert gf.keys() == gr.keys() and "unembed.W_U" in gf
    big = max(float(g.norm()) for g in gr.values())
    for n in gr:
        if float(gr[n].norm()) < 1e-3 * big:  # zero in exact arithmetic (b_K): noise on both sides
            assert float(gf[n].norm()) < 1e-2 * big, n
            continue
        err = float((gf[n] - gr[n]).norm() / gr[n].norm())
        assert err < 0.03, (n, err)  # tests/test_headline_parity.py's per-parameter bound


def test_every_phase_of_an_ioi_step_takes_the_bf16_only_tail(monkeypatch):
    """IIT, strict and behaviour phase of one ``IOI_ModelPair`` train step all end in ``ce_bwd16``: none of them hands
    the loss a re-wrapped view of the logits (which would drop the gradient handle)."""
    from iit_amd.data.iit_dataset import IITDataset
    from iit_amd.model_pairs import IOI_ModelPair
    from iit_amd.models.config import gpt2_config_dict
    from iit_amd.models.transformer import HookedTransformer
    from iit_amd.ops import hip_ops
    from iit_amd.tasks.ioi import make_ioi_corr, make_ioi_dataset_and_hl
    torch.manual_seed(0)
    cfg = gpt2_config_dict()
    cfg.update(n_layers=6, d_model=128, n_heads=4, d_head=32, d_mlp=512, device=dev, dtype=torch.bfloat16)
    ll = HookedTransformer(cfg)
    ll.set_op_backend("hip")
    ds, hl = make_ioi_dataset_and_hl(64, ll, device=torch.device(dev))
    train = IITDataset(ds, ds, seed=0, device=torch.device(dev))
    pair = IOI_ModelPair(hl, ll, make_ioi_corr(6), training_args={"batch_size": 32, "lr": 1e-3, "lr_scheduler": None})
    opt = pair.make_optimizer(1e-3)
    base, abl = next(iter(train.make_loader(32, 0)))
    calls = {"16": 0, "32": 0}
    k16, k32 = hip_ops.K.ce_bwd16, hip_ops.K.ce_bwd
    monkeypatch.setattr(hip_ops.K, "ce_bwd16", lambda *a, **k: (calls.__setitem__("16", calls["16"] + 1), k16(*a, **k)))
    monkeypatch.setattr(hip_ops.K, "ce_bwd", lambda *a, **k: (calls.__setitem__("32", calls["32"] + 1), k32(*a, **k)))
    out = pair.run_train_step(base, abl, pair.loss_fn, opt)
    torch.cuda.synchronize()
    assert all(float(v) == float(v) for v in out.values()), out
    assert calls == {"16": 3, "32": 0}, calls
