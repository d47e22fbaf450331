"""Element-wise tests of ``sumsq_2d_kernel``, of the ZeRO-1 entry points ``iit_sumsq_spans`` / ``iit_adam_spans``
(``sumsq_span_kernel`` + ``adam_span_kernel<true, 2>`` over a span table whose gradient / moment offsets differ from
the parameter offsets) in a single process, and of ``kl_rows_kernel`` on the GPU, against the references and bounds of
tests/misc_exact_util.py (proved on the CPU by tests/test_misc_exact_ref.py).

The span test uses a hand-built table over a small arena and a separate shard buffer: spans of 1, 255, 256, 257 and
1024 float4 groups with gaps between them in both.  Checked: the norm partials against the float64 sum of squares,
p', m', v' against ``adam_ref``, the bf16 mirror bitwise, every element outside the spans bit-unchanged in all five
buffers, the step counter, and the non-finite guard.

Measured on an MI355X: 37 cases, 37 passed, none skipped, 2.7 s for the module; the slowest case is the first (0.2 s,
one-time initialisation), every other case 0.02 s or less.  (No mutated library was run against this module; the CPU
module shows the ``start4`` / ``local4`` mix-up, a dropped element and a touched idle slot flagged.)
"""
import types

import pytest
import torch

import kern_exact_util as KX
import misc_exact_util as X

pytestmark = pytest.mark.gpu

dev = "cuda"
F32, BF16 = torch.float32, torch.bfloat16


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


# ================================================================================================ sumsq_2d
@pytest.mark.parametrize("family", X.FAMILIES)
@pytest.mark.parametrize("M,N,ld", [(1, 1, 1), (3, 2047, 2050), (3, 2048, 2048), (2, 2049, 2049), (5, 4100, 4104),
                                    (2100, 8, 8)])
def test_sumsq_2d(K, M, N, ld, family):
    """One chunk and more, the ragged last chunk, ld > N over a NaN pad, and 2100 items over 2048 blocks (the
    grid-stride loop); slots at index >= the block count keep their prefill bits."""
    if family == "exact":
        lim = X.sumsq_lim(M, N)
        c = X.int_operand((M, N), F32, M + N, 1, lim=lim)
        g0 = torch.randint(0, lim * lim + 1, (64,), generator=X.gen(N)).float()
    else:
        c = torch.randn(M, N, generator=X.gen(M + N))
        g0 = torch.rand(64, generator=X.gen(N))
    pre = torch.cat([g0, X.filled((4,), F32)])
    gsq = pre.to(dev)
    K.sumsq_2d(X.strided(c.to(dev), ld, 0, dev), ld, M, N, gsq)
    torch.cuda.synchronize()
    ref = X.sumsq_ref(c, g0)
    got = gsq.cpu()
    bad = X.bad_sum(got[:64], ref["gsq"], ref["tol"], family, g0, ref["n"])
    assert not int(bad.sum()), (int(bad.sum()), bad.nonzero().view(-1)[:8])
    assert not int(X.bad_bits(got[64:], pre[64:]).sum())
    assert int((ref["n"] == 0).sum()) == max(0, 64 - min(2048, M * ((N + 2047) // 2048)))


# ================================================================================================ spans
class Shard:
    """Arena (weights + bf16 mirror) and shard (gradient + both moments) buffers on the device with the span table."""

    def __init__(self, K):
        self.K = K
        self.spans, self.an, self.sn = X.span_table()
        self.table = X.span_bytes(self.spans).to(dev)
        assert X.SPAN_DTYPE.itemsize == K.lib().iit_adam_span_size()
        self.mirror0 = X.filled((self.an,), BF16)
        self.part = torch.empty(1024, dtype=F32, device=dev)
        self.total = torch.zeros(1, dtype=F32, device=dev)
        self.step = torch.zeros(1, dtype=torch.int32, device=dev)
        self.skipped = torch.zeros(1, dtype=torch.int32, device=dev)

    def run(self, st, t, clip, hyper, do_norm, guard, hyper_dev=False):
        d = {k: v.to(dev) for k, v in st.items()}
        mirror = self.mirror0.to(dev)
        self.step.fill_(t - 1)
        self.part.fill_(float("nan"))
        self.total.fill_(float("nan"))
        K = self.K
        K.sumsq_spans(d["g"], self.table, len(self.spans), self.part, self.step, do_norm)
        if do_norm:
            torch.sum(self.part, dim=0, keepdim=True, out=self.total)
        flat = types.SimpleNamespace(data=d["p"], shadow=mirror)
        h = dict(lr=hyper["lr"], b1=hyper["b1"], b2=hyper["b2"], eps=hyper["eps"], wd=hyper.get("wd", 0.0))
        hd = None
        if hyper_dev:  # the device block overrides the scalars: pass wrong scalars
            hd = torch.tensor([h["lr"], h["b1"], h["b2"], h["eps"], h["wd"]], dtype=F32, device=dev)
            h = dict(lr=1.0, b1=0.5, b2=0.5, eps=1.0, wd=0.5)
        K.adam_spans(flat, d["g"], d["m"], d["v"], self.table, len(self.spans), self.total, self.step,
                     clip_norm=clip, skipped=self.skipped if guard else None, hyper=hd, **h)
        torch.cuda.synchronize()
        got = {k: v.cpu() for k, v in d.items()}
        got.update(mirror=mirror.cpu(), part=self.part.cpu(), t=int(self.step.item()), skipped=int(self.skipped.item()))
        return got


@pytest.mark.parametrize("hyper_dev", [False, True], ids=["scalars", "device_hyper"])
@pytest.mark.parametrize("mode", ["no_norm", "guard_only", "clip_above", "clip_below"])
@pytest.mark.parametrize("t", [1, 10])
def test_adam_spans(K, t, mode, hyper_dev):
    sh = Shard(K)
    st = X.span_state(sh.an, sh.sn, seed=t)
    clip = {"no_norm": None, "guard_only": None, "clip_above": 1e6, "clip_below": 1.0}[mode]
    do_norm = mode != "no_norm"
    hyper = dict(KX.ADAM_HYPER, wd=0.1 if t == 10 else 0.0)
    got = sh.run(st, t, clip, hyper, do_norm, guard=mode != "no_norm", hyper_dev=hyper_dev)
    ref = X.span_ref(st, sh.spans, t, clip, hyper)
    bad = _count(X.span_check(got, st, ref, sh.spans, sh.mirror0))
    assert not bad, bad
    assert got["t"] == t and got["skipped"] == 0
    if do_norm:  # every one of the 1024 partials written, their sum the squared norm
        assert bool(torch.isfinite(got["part"]).all())
        ssq = float(ref["ssq"])
        assert abs(float(got["part"].double().sum()) - ssq) <= KX.NSQ * X.E * ssq
    else:
        assert bool(torch.isnan(got["part"]).all())


@pytest.mark.parametrize("what", ["nan", "inf"])
def test_adam_spans_skips_a_non_finite_gradient(K, what):
    sh = Shard(K)
    st = X.span_state(sh.an, sh.sn, seed=3)
    ia, il = X.span_index(sh.spans)
    st["g"][il[il.numel() // 2]] = float(what)
    got = sh.run(st, 4, 1.0, KX.ADAM_HYPER, True, guard=True)
    for k in ("p", "g", "m", "v"):
        assert not int(X.bad_bits(got[k], st[k]).sum()), k
    assert not int(X.bad_bits(got["mirror"], sh.mirror0).sum())
    assert got["t"] == 3 and got["skipped"] == 1


def test_adam_spans_ignores_a_nan_outside_the_spans(K):
    """A NaN in a gap of the shard gradient is outside every span: the norm and the step must not see it."""
    sh = Shard(K)
    st = X.span_state(sh.an, sh.sn, seed=5)
    ia, il = X.span_index(sh.spans)
    gap = torch.ones(sh.sn, dtype=torch.bool)
    gap[il] = False
    st["g"][gap] = float("nan")
    got = sh.run(st, 2, 1.0, KX.ADAM_HYPER, True, guard=True)
    ref = X.span_ref(st, sh.spans, 2, 1.0, KX.ADAM_HYPER)
    assert not _count(X.span_check(got, st, ref, sh.spans, sh.mirror0))
    assert got["t"] == 2 and got["skipped"] == 0


# ================================================================================================ kl_rows
@pytest.mark.parametrize("V", X.KL_V)
def test_kl_rows(K, V):
    """R = 5 rows (normal logits, a pmf, -inf logits where b = 0, an all -inf row, a pmf with zeros where b = 0) with
    lda, ldb > V over a NaN pad."""
    a, b, cols = X.kl_inputs(V, V)
    got = K.kl_rows(X.strided(a.to(dev), V + 3, 0, dev), X.strided(b.to(dev), V + 5, 0, dev)).cpu()
    ref = X.kl_ref(a, b)
    bad = X.kl_check(got, ref, cols)
    assert not int(bad.sum()), (bad, got, ref["out"])
    assert float(got[3, 1]) == float("-inf") and float(got[3, 2]) == 0.0 and float(got[3, 3]) == 0.0
    assert bool(torch.isfinite(got[2, 2])) and bool(torch.isfinite(got[4, 2:]).all())
