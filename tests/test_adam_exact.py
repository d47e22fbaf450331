"""Element-wise tests of the fused clip + Adam pass on the GPU (``sumsq_span_kernel`` + ``adam_span_kernel`` of
csrc/kernels.hip through ``FusedAdam.step`` / ``hip_kernels.adam_step``) against the float64 Adam and the derived
bounds of tests/kern_exact_util.py (proved on the CPU by tests/test_kern_exact_ref.py).

Every case is ONE step from a chosen state: p, g, both moments and the device step counter (t - 1) are written, one
step runs, and p', m', v' are compared element by element.  The arena is a tiny ModuleDict whose restricted embedding
cuts it into spans of 1, 255, 256, 257, 1023, 1024 and 1025 (= 1024 + 1) float4 groups, with a Linear whose sizes are
no multiple of 4.  Always checked: the bf16 mirror is bitwise the rounding of the new weights over the spans, every
element outside the spans keeps its bits in the weights, both moments and the mirror, and the step counter is t.

Measured on an MI355X: 28 cases, 28 passed, none skipped, 4.4 s for the module; the slowest case is the first step
(1.6 s, one-time initialisation), every other case 0.03 s or less.  ``powf``: the worst error measured through the
kernel is 0.508 ulps of beta^t (beta = 0.9, t = 3; the method and every figure are in tests/kern_exact_util.py), so
the bounds use ``POW_K`` = 1.02.  As a check of the module itself, a library with eps inside the square root of the
denominator failed all ten tiny-gradient cases of ``test_adam_step`` and three of the random ones (t = 1 and 10000).
"""
import pytest
import torch

import kern_exact_util as X

pytestmark = pytest.mark.gpu

dev = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
CLIP_BELOW = {"random": 1.0, "tiny": 1e-9}  # below the gradient norm (about 124, and 1e-6 + 1.2e-10)


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


class Arena:
    """The model, its arena with the bf16 mirror and the restricted embedding, and a FusedAdam over it."""

    def __init__(self, wd=0.0, nan_guard=True, lr=X.ADAM_HYPER["lr"]):
        from iit_amd.engine.flat import FlatParams
        from iit_amd.ops.optim import FusedAdam
        self.model = X.adam_model().to(dev)
        self.flat = FlatParams(self.model, with_bf16_shadow=True)
        assert self.flat.restrict_rows(self.model["emb"].weight, X.adam_live_rows())
        h = X.ADAM_HYPER
        self.hyper = dict(lr=lr, b1=h["b1"], b2=h["b2"], eps=h["eps"], wd=wd)
        self.opt = FusedAdam(self.flat, lr=lr, betas=(h["b1"], h["b2"]), eps=h["eps"], weight_decay=wd,
                             nan_guard=nan_guard)
        # weight decay lifts the restriction (FusedAdam._validate_restriction): every row is then inside a span
        self.param, self.active = X.adam_masks(self.flat, restricted=wd == 0.0)
        self.n = self.flat.numel

    def load(self, st: dict, t: int):
        self.flat.data.copy_(st["p"])
        self.flat.grad.copy_(st["g"])
        self.opt.exp_avg.copy_(st["m"])
        self.opt.exp_avg_sq.copy_(st["v"])
        self.opt._step_dev.fill_(t - 1)
        self.flat.shadow.fill_(X.BF16_FILL)

    def read(self) -> dict:
        torch.cuda.synchronize()
        return {"p": self.flat.data.cpu(), "m": self.opt.exp_avg.cpu(), "v": self.opt.exp_avg_sq.cpu(),
                "mirror": self.flat.shadow.cpu(), "t": int(self.opt._step_dev.item())}

    def check(self, got: dict, st: dict, t: int, clip, **over):
        """``got`` against one reference step from ``st``; returns nothing, asserts."""
        ref = X.adam_ref(st["p"], st["g"], st["m"], st["v"], t, **dict(self.hyper, **over), clip=clip,
                         active=self.active)
        bad = _count(X.adam_check(got, ref, self.active))
        assert not bad, bad
        off = ~self.active
        for k in ("p", "m", "v"):
            assert not int(X.bad_bits(got[k][off], st[k][off]).sum()), k
        assert bool((got["mirror"][off].float() == X.BF16_FILL).all())
        assert got["t"] == t


def _unchanged(got: dict, st: dict) -> bool:
    return all(not int(X.bad_bits(got[k], st[k]).sum()) for k in ("p", "m", "v")) and \
        bool((got["mirror"].float() == X.BF16_FILL).all())


@pytest.mark.parametrize("wd", [0.0, 0.1])
@pytest.mark.parametrize("t", X.ADAM_T)
@pytest.mark.parametrize("family", ["random", "tiny"])
def test_adam_step(K, family, t, wd):
    """No clip, a clip far above the norm (bit-identical to no clip: the coefficient is exactly 1), a clip below it."""
    a = Arena(wd=wd)
    st = X.adam_state(family, a.n, a.active, seed=t, param=a.param)
    res = {}
    for clip in (None, 1e6, CLIP_BELOW[family]):
        a.load(st, t)
        a.opt.step(clip_norm=clip)
        res[clip] = a.read()
        a.check(res[clip], st, t, clip)
    for k in ("p", "m", "v", "mirror"):
        assert not int(X.bad_bits(res[None][k], res[1e6][k]).sum()), k
    assert a.opt.skipped_steps == 0
    assert bool(a.flat._inactive) == (wd == 0.0)


@pytest.mark.parametrize("clip", [None, 1.0])
def test_adam_without_guard_is_bitwise_the_guarded_step(K, clip):
    res = []
    for guard in (True, False):
        a = Arena(nan_guard=guard)
        st = X.adam_state("random", a.n, a.active, seed=5, param=a.param)
        a.load(st, 3)
        a.opt.step(clip_norm=clip)
        res.append(a.read())
        a.check(res[-1], st, 3, clip)
    for k in ("p", "m", "v", "mirror"):
        assert not int(X.bad_bits(res[0][k], res[1][k]).sum()), k


@pytest.mark.parametrize("clip", [None, 1.0])
@pytest.mark.parametrize("what", ["inf", "nan"])
def test_adam_skips_a_non_finite_gradient(K, what, clip):
    """One inf / NaN among the gradients: weights, both moments, the mirror and the step counter keep their bits, the
    skip is counted, and the next finite step runs with the unchanged t."""
    a = Arena()
    t = 3
    st = X.adam_state(what, a.n, a.active, seed=9, param=a.param)
    assert int((~torch.isfinite(st["g"])).sum()) == 1
    a.load(st, t)
    a.opt.step(clip_norm=clip)
    got = a.read()
    assert _unchanged(got, st) and got["t"] == t - 1
    assert a.opt.skipped_steps == 1
    good = dict(st, g=X.adam_state("random", a.n, a.active, seed=9, param=a.param)["g"])
    a.flat.grad.copy_(good["g"])
    a.opt.step(clip_norm=clip)
    a.check(a.read(), good, t, clip)
    assert a.opt.skipped_steps == 1


def test_adam_learning_rate_change_eager(K):
    a = Arena()
    st = X.adam_state("random", a.n, a.active, seed=4, param=a.param)
    for lr in (1e-3, 2e-3):
        a.opt.param_groups[0]["lr"] = lr
        a.load(st, 2)
        a.opt.step(clip_norm=1.0)
        a.check(a.read(), st, 2, 1.0, lr=lr)


def test_adam_learning_rate_change_reaches_a_captured_step(K):
    """One capture, two replays: the second after ``param_groups`` changed and ``sync_hyper()`` copied the device
    hyper-parameter block."""
    a = Arena()
    st = X.adam_state("random", a.n, a.active, seed=6, param=a.param)
    a.load(st, 2)
    a.opt.step(clip_norm=1.0)  # eager warm-up: span table, norm partials and the hyper block exist before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    a.load(st, 2)
    with torch.cuda.graph(graph):
        a.opt.step(clip_norm=1.0)
    for lr in (1e-3, 2e-3):
        a.opt.param_groups[0]["lr"] = lr
        a.opt.sync_hyper()
        a.load(st, 2)
        graph.replay()
        a.check(a.read(), st, 2, 1.0, lr=lr)
