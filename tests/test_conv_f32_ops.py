"""``iit_amd.ops.conv_f32`` on the GPU: :class:`ConvF32Fn` bitwise against float64 autograd of ``F.conv2d`` on exact
integer data (F1- and F2-style tensors through all three passes at once, F3 pass by pass), and ResNet-18 with the
``hip32`` convolution backend against the library path and a float64 oracle.

The model criterion is the one of tests/test_hip32_ops.py, for the reason given there: per tensor (the logits and every
parameter gradient of ``logits.logsumexp(-1).sum()``) ``e = max|t - oracle| / max|oracle|`` and
``e_hip32 <= 4 e_torch + 2^-20``.

ReLU and max-pool make the gradient discontinuous, so the test first asserts, on the float64 oracle alone, how far the
oracle stays from every kink: every ReLU input has ``|v| >= MARGIN max|v|`` of its tensor, and in every pooling window
whose maximum is positive the top two values differ by at least as much of the pooled tensor's ``max|v|``.  ``MARGIN``
is 2^-17, not the 2^-12 first asked for, which no seed can reach: the model has about 190 000 roughly normal ReLU inputs
whose largest is about 4.5 sigma (65 536 in the stem alone), so about 150 of them fall below 2^-12 of it in every draw;
over seeds 0..299 the best margin is 2^-16.46 (seed 175, the one used here).  A pooling window whose maximum is 0 holds
only zeros of the ReLU before it (and the -inf padding); its tie passes no gradient whichever element takes it, since the
ReLU's derivative there is 0, so such windows are exempt.  A margin of 1.1e-5 is of the size of the fp32 errors this
test records (1e-5 to 9e-5 of a tensor's maximum), so it does not prove that no fp32 path crosses a kink; what keeps
the comparison from failing at random is that both fp32 runs are repeatable: the fixture runs them with the BatchNorm
statistics' fixed-order reduction (``IIT_BN_REDUCE=two``), under which the whole model is bit-identical run to run on
either backend (:func:`test_backend_torch_is_the_path_from_before_the_import` checks that), so a pass is a pass on
every run.

The measured ``(e_hip32, e_torch)`` pairs are printed, and written to the file ``IIT_CONV_F32_PARITY_OUT`` names when it
is set (``profiles/conv_f32_parity.txt`` was made that way).
"""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as TF
from torch import nn

import conv_f32_util as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, MARGIN = 175, 2.0 ** -17
OPS_SHAPES = ((2, 5, 7, 8, 12, 3, 1, 1), (2, 6, 6, 4, 8, 3, 2, 1), (2, 12, 12, 3, 8, 7, 2, 3))
# (|x|, |w|, |dy|) bounds of the two integer families: every sum of the three passes stays below 2^24 (asserted)
INT_FAMILIES = {"F1": (3, 2, 3), "F2": (4095, 3, 3)}


@pytest.fixture(scope="module")
def cf():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from iit_amd.ops import conv_f32
    yield conv_f32
    conv_f32.set_backend("torch")


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("family", list(INT_FAMILIES))
@pytest.mark.parametrize("shape", OPS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_function_is_bitwise_float64_autograd(cf, shape, family):
    N, H, W, Cin, Cout, k, s, pad = shape
    OH, OW = C.out_hw(shape)
    bx, bw, bdy = INT_FAMILIES[family]
    assert max(bx * bw * k * k * max(Cin, Cout), bx * bdy * N * OH * OW, bdy * bw * k * k * Cout) < 2 ** 24
    g = torch.Generator().manual_seed(11)
    x = torch.randint(-bx, bx + 1, (N, Cin, H, W), generator=g).float()
    w = torch.randint(-bw, bw + 1, (Cout, Cin, k, k), generator=g).float()
    dy = torch.randint(-bdy, bdy + 1, (N, Cout, OH, OW), generator=g).float()
    x64, w64 = x.double().requires_grad_(), w.double().requires_grad_()
    y64 = TF.conv2d(x64, w64, stride=s, padding=pad)
    y64.backward(dy.double())
    for dense_dy in (False, True):
        xg, wg = _cl(x.cuda()).requires_grad_(), _cl(w.cuda()).requires_grad_()
        before = dict(cf.calls)
        y = cf.ConvF32Fn.apply(xg, wg, (k, s, pad))
        dyg = dy.cuda()  # NCHW-contiguous: not the layout the kernels read
        if dense_dy:
            dyg = _cl(dyg)
        else:
            assert dyg.numel() == 1 or not cf.nhwc_dense(dyg)
        y.backward(dyg)
        torch.cuda.synchronize()
        delta = {n: cf.calls[n] - before.get(n, 0) for n in ("fwd", "dgrad", "wgrad", "dy_copy")}
        assert delta == {"fwd": 1, "dgrad": 1, "wgrad": 1, "dy_copy": 0 if dense_dy else 1}
        assert y.shape == y64.shape and cf.nhwc_dense(y) and cf.nhwc_dense(wg.grad) and wg.grad.shape == w.shape
        for got, want in ((y, y64), (xg.grad, x64.grad), (wg.grad, w64.grad)):
            assert torch.equal(got.detach().cpu().view(torch.int32), want.detach().float().view(torch.int32))
    # the stem's case: no input gradient asked, no dgrad run
    xg, wg = _cl(x.cuda()), _cl(w.cuda()).requires_grad_()
    before = cf.calls["dgrad"]
    cf.ConvF32Fn.apply(xg, wg, (k, s, pad)).backward(_cl(dy.cuda()))
    assert cf.calls["dgrad"] == before
    assert torch.equal(wg.grad.cpu(), w64.grad.float())


@pytest.mark.parametrize("pass_", C.PASSES)
@pytest.mark.parametrize("shape", OPS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_function_is_bitwise_float64_autograd_on_f3(cf, shape, pass_):
    """The sparse 22-bit family, which a bf16 hi + lo split cannot hold.  Its wide operand sits where one pass's
    reduction meets it at most three times, so one set of tensors cannot serve all three passes: each pass runs on its
    own ``conv_f32_util.tensors(F3, pass, shape)`` and only that pass's result is asked for."""
    N, H, W, Cin, Cout, k, s, pad = shape
    x, w, dy = (t.permute(0, 3, 1, 2) for t in C.tensors(C.F3, pass_, shape))  # NHWC memory, [N, C, H, W] views
    assert C.worst_sum(C.F3, pass_, shape) < 2 ** 24
    x64 = x.double().requires_grad_(pass_ == C.DGRAD)
    w64 = w.double().requires_grad_(pass_ == C.WGRAD)
    y64 = TF.conv2d(x64, w64, stride=s, padding=pad)
    xg = x.cuda().requires_grad_(pass_ == C.DGRAD)
    wg = w.cuda().requires_grad_(pass_ == C.WGRAD)
    assert cf.nhwc_dense(xg) and cf.nhwc_dense(wg)
    before = dict(cf.calls)
    y = cf.ConvF32Fn.apply(xg, wg, (k, s, pad))
    if pass_ == C.FWD:
        got, want, ran = y, y64, {"fwd": 1}
    else:
        y64.backward(dy.double())
        y.backward(dy.cuda())
        got, want = (xg.grad, x64.grad) if pass_ == C.DGRAD else (wg.grad, w64.grad)
        ran = {"fwd": 1, "dgrad": 1} if pass_ == C.DGRAD else {"fwd": 1, "wgrad": 1}
    torch.cuda.synchronize()
    assert {n: v - before.get(n, 0) for n, v in cf.calls.items() if v != before.get(n, 0)} == ran
    assert want.abs().max() > 2 ** 16  # the wide operands reached the result
    assert torch.equal(got.detach().cpu().view(torch.int32), want.detach().float().view(torch.int32))


# ------------------------------------------------------------------------------ ResNet-18
def _model_and_input():
    from iit_amd.models.resnet import resnet18
    torch.manual_seed(SEED)
    return resnet18(), torch.randn(4, 3, 32, 32)


def _run(model, x):
    model.train()
    model.zero_grad(set_to_none=True)
    logits = model(x)
    logits.logsumexp(-1).sum().backward()
    out = {"logits": logits.detach().cpu()}
    out.update({n: p.grad.detach().cpu().contiguous() for n, p in model.named_parameters()})
    return out


def _oracle_margins(model64, x64):
    """(smallest |v| / max|v| over the ReLU inputs, smallest top-two gap / max|v| over the pooling windows with a
    positive maximum) of the float64 oracle."""
    relu, pool, hooks = [], [], []
    for mod in model64.modules():
        if isinstance(mod, nn.ReLU):
            hooks.append(mod.register_forward_pre_hook(lambda _m, a: relu.append(a[0].detach().clone())))
        if isinstance(mod, nn.MaxPool2d):
            hooks.append(mod.register_forward_pre_hook(lambda _m, a: pool.append(a[0].detach().clone())))
    model64.train()
    model64(x64)
    for h in hooks:
        h.remove()
    assert len(relu) == 17 and len(pool) == 1
    rm = min((v.abs().min() / v.abs().max()).item() for v in relu)
    v = pool[0]
    win = TF.unfold(TF.pad(v, (1, 1, 1, 1), value=float("-inf")), 3, stride=2).reshape(v.shape[0], v.shape[1], 9, -1)
    top = win.topk(2, dim=2).values
    gap = top[:, :, 0] - top[:, :, 1]
    return rm, (gap[top[:, :, 0] > 0].min() / v.abs().max()).item()


@pytest.fixture(scope="module")
def parity(cf):
    import copy
    model, x = _model_and_input()
    oracle = copy.deepcopy(model).double()
    margins = _oracle_margins(copy.deepcopy(oracle), x.double())
    res = {"margins": margins, "oracle": _run(oracle, x.double())}
    gpu = model.cuda().to(memory_format=torch.channels_last)
    xg = x.cuda()
    saved = os.environ.get("IIT_BN_REDUCE")
    os.environ["IIT_BN_REDUCE"] = "two"  # fixed-order BatchNorm statistics: both runs repeat bit for bit
    try:
        for name in ("torch", "hip32"):
            cf.set_backend(name)
            cf.calls.clear()
            res[name] = _run(gpu, xg)
            res[name + "_calls"] = dict(cf.calls)
    finally:
        cf.set_backend("torch")
        if saved is None:
            del os.environ["IIT_BN_REDUCE"]
        else:
            os.environ["IIT_BN_REDUCE"] = saved
    return res


def test_oracle_is_away_from_every_kink(parity):
    relu_margin, pool_margin = parity["margins"]
    print(f"ReLU margin 2^{torch.tensor(relu_margin).log2():.2f}, pooling margin 2^{torch.tensor(pool_margin).log2():.2f}")
    assert relu_margin >= MARGIN and pool_margin >= MARGIN


def _err(t, oracle):
    return ((t.double() - oracle).abs().max() / oracle.abs().max()).item()


def test_model_matches_float64_as_well_as_the_library_path(parity):
    o, t, h = parity["oracle"], parity["torch"], parity["hip32"]
    assert set(o) == set(t) == set(h) and len(o) == 63
    lines, failed = [], []
    for name in o:
        e_t, e_h = _err(t[name], o[name]), _err(h[name], o[name])
        lines.append(f"{name:40s} e_hip32 {e_h:.3e}  e_torch {e_t:.3e}")
        if not e_h <= 4 * e_t + 2.0 ** -20:
            failed.append(lines[-1])
    print("\n".join(lines))
    dest = os.environ.get("IIT_CONV_F32_PARITY_OUT")
    if dest:
        with open(dest, "w") as f:
            f.write("\n".join(lines) + "\n")
    assert not failed, "\n".join(failed)


def test_every_convolution_ran_on_the_kernels(parity):
    # the stem, 16 block convolutions and 3 downsamples; no input gradient for the stem; no fallback, no copy
    assert parity["hip32_calls"] == {"fwd": 20, "dgrad": 19, "wgrad": 20}
    assert parity["torch_calls"] == {}


CHILD = r"""
import sys, torch
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import test_conv_f32_ops as T
torch.backends.cudnn.deterministic = True
model, x = T._model_and_input()
gpu, xg = model.cuda().to(memory_format=torch.channels_last), x.cuda()
assert "iit_amd.ops.conv_f32" not in sys.modules
before = T._run(gpu, xg)
assert "iit_amd.ops.conv_f32" not in sys.modules
from iit_amd.ops import conv_f32
assert conv_f32.backend() == "torch" and dict(conv_f32.calls) == {{}}
conv_f32.set_backend("hip32")
first, second = T._run(gpu, xg), T._run(gpu, xg)
assert dict(conv_f32.calls) == {{"fwd": 40, "dgrad": 38, "wgrad": 40}}, dict(conv_f32.calls)
for n in first:  # the kernels repeat themselves bit for bit through the whole model
    assert torch.equal(first[n], second[n]), ("hip32", n)
conv_f32.set_backend("torch")
conv_f32.calls.clear()
after = T._run(gpu, xg)
assert dict(conv_f32.calls) == {{}}, dict(conv_f32.calls)
assert set(before) == set(after) == set(first) and len(before) == 63
for n in before:
    assert torch.equal(before[n], after[n]), ("torch", n)
print("backend torch unchanged")
"""


def test_backend_torch_is_the_path_from_before_the_import(cf):
    """One fresh process, whole ResNet-18 (logits and all 62 parameter gradients): a run before ``conv_f32`` is
    imported, two ``hip32`` runs that must equal each other bit for bit, and a ``torch`` run after switching back that
    must equal the first bit for bit and leave the counters empty.  The process runs with ``IIT_BN_REDUCE=two``: the
    fused BatchNorm's default statistics are summed with fp32 atomics and repeat on neither backend, its fixed-order
    two-level reduction does."""
    code = CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    env = dict(os.environ, IIT_BN_REDUCE="two")
    run = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "backend torch unchanged" in run.stdout
