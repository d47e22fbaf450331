"""The forward weight prefetch around the kernel (tests/test_ln_prefetch.py has the kernel itself):

* ``hip_kernels.prefetch_wgs``, the (bytes, density) -> workgroup count rule, on the CPU;
* a dual dX + dW launch with and without its prefetch workgroups, whose ``Prefetch`` / ``prefetch_part`` now live in
  csrc/prefetch.h: bitwise-equal dX and dW;
* the switch ``IIT_FWD_PREFETCH`` on a two-layer model: 1 hands every LN1 / LN2 launch its block's weights, 0 none,
  and the logits of the two runs are bitwise equal.  The parameter gradients are compared the way
  tests/test_headline_parity.py compares two engines, per parameter by relative norm with the parameters whose
  gradient is zero in exact arithmetic bounded against the largest one -- but at 1e-4 instead of its 3e-2: the two
  runs here differ only in the arrival order of fp32 atomic sums (bias / LN affine / embedding gradients over
  B S = 128 rows), each of which moves a sum by at most 128 * 2^-24 = 7.6e-6 of its sum of magnitudes, and a sum of
  signed terms is rarely below a tenth of that sum.
"""
import pytest
import torch

gpu = pytest.mark.gpu
dev = "cuda"


# ------------------------------------------------------------------------------ workgroup count (CPU)
def test_prefetch_wgs_rule():
    from iit_amd.ops.hip_kernels import prefetch_wgs
    for per_mb in (8, 16, 32):
        assert prefetch_wgs(0, per_mb) == 0 and prefetch_wgs(63, per_mb) == 0 and prefetch_wgs(-64, per_mb) == 0
        assert prefetch_wgs(64, per_mb) == 1
        last = 0
        for nbytes in sorted(list(range(64, 8192, 64)) + [2 ** k for k in range(13, 31)] + [9 * 2 ** 20 + 64]):
            n = prefetch_wgs(nbytes, per_mb)
            assert last <= n <= min(nbytes // 64, 1024), (nbytes, per_mb, n)  # monotone, never above the granules
            last = n
        assert prefetch_wgs(2 ** 20, per_mb) == per_mb and prefetch_wgs(2 ** 30, per_mb) == 1024
    assert prefetch_wgs(2 ** 20, 0) == 0 and prefetch_wgs(2 ** 20, -1) == 0
    # GPT-2-small: LN1 reads W_QKV + W_O (3.5 + 1.2 MB), LN2 W_in + W_out (4.7 + 4.7 MB)
    assert prefetch_wgs(768 * 2304 * 2 + 768 * 768 * 2, 16) == 72 and prefetch_wgs(2 * 768 * 3072 * 2, 16) == 144


# ------------------------------------------------------------------------------ dual launch
@gpu
def test_dual_launch_with_prefetch_keeps_every_bit(monkeypatch):
    from iit_amd.ops import hip_kernels as K
    K.lib()
    T, KIN, NOUT = 256, 128, 128
    g = torch.Generator().manual_seed(3)
    x = torch.randn(T, KIN, generator=g).to(dev).bfloat16()
    dy = (torch.randn(T, NOUT, generator=g) / 4).to(dev).bfloat16()
    w = (torch.randn(KIN, NOUT, generator=g) / 8).to(dev).bfloat16()
    big = torch.randint(0, 256, (2 ** 20 + 4096,), dtype=torch.uint8, generator=g).to(dev)
    big0 = big.clone()
    monkeypatch.setattr(K, "_PF_PER_MB", 8.0)  # 8 workgroups for the 1 MiB range
    assert K._prefetch_args((big[:2 ** 20],)) == (big.data_ptr(), 2 ** 20, None, 0, 8)
    outs = []
    for prefetch in (None, (big[:2 ** 20],)):
        gW = torch.zeros(KIN, NOUT, device=dev)
        dX = torch.zeros(T, KIN, device=dev, dtype=torch.bfloat16)
        ws = dict(A=x, B=dy, C=gW, M=KIN, N=NOUT, K=T, lda=KIN, ldb=NOUT, ldc=NOUT, epi=K.EPI_F32_STORE)
        xs = dict(A=dy, B=w, C=dX, M=T, N=KIN, K=NOUT, lda=NOUT, ldb=NOUT, ldc=KIN, epi=K.EPI_BF16)
        tiles = [(wt, xt) for wt in range(5) for xt in range(4) if K.gemm_dual_ok(ws, xs, wt, xt)]
        assert tiles
        K.gemm_dual(ws, xs, *tiles[0], prefetch=prefetch)  # one K pass per tile, plain stores: repeatable
        torch.cuda.synchronize()
        outs.append((gW.view(torch.int32), dX.view(torch.int16)))
    torch.testing.assert_close(outs[0][0].view(torch.float32), x.float().t() @ dy.float(), rtol=1e-4, atol=2e-3)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(big, big0)


# ------------------------------------------------------------------------------ the switch, on a model
CFG = dict(n_layers=2, d_model=64, n_heads=4, d_head=16, d_mlp=256, d_vocab=97, n_ctx=16, act_fn="gelu_new",
           normalization_type="LN")


def _fwd_bwd(monkeypatch, switch: str):
    from iit_amd.models.transformer import HookedTransformer
    from iit_amd.ops import hip_kernels as K
    monkeypatch.setenv("IIT_FWD_PREFETCH", switch)
    torch.manual_seed(0)
    m = HookedTransformer(dict(CFG, device=dev, dtype=torch.bfloat16, init_weights=True))
    m.set_op_backend("hip")
    tok = torch.randint(0, 97, (8, 16), generator=torch.Generator().manual_seed(2)).to(dev)
    launches = []  # (bytes of range 0, bytes of range 1, workgroups) of every LN forward launch
    real = K._ln_prefetch_args

    def spy(prefetch, wgs):
        args = real(prefetch, wgs)
        launches.append((args[1], args[3], args[4]))
        return args
    monkeypatch.setattr(K, "_ln_prefetch_args", spy)
    logits = m(tok)
    logits.float().logsumexp(-1).sum().backward()
    torch.cuda.synchronize()
    monkeypatch.setattr(K, "_ln_prefetch_args", real)
    return logits.detach(), {n: p.grad.detach().float() for n, p in m.named_parameters()}, launches


@gpu
def test_switch_hands_the_norms_their_weights_and_changes_no_logit(monkeypatch):
    from iit_amd.ops.hip_kernels import _PF_PER_MB, prefetch_wgs
    logits1, grads1, on = _fwd_bwd(monkeypatch, "1")
    logits0, grads0, off = _fwd_bwd(monkeypatch, "0")
    d, dm = CFG["d_model"], CFG["d_mlp"]
    ln1 = (d * 3 * d * 2, d * d * 2, prefetch_wgs(d * 3 * d * 2 + d * d * 2, _PF_PER_MB))
    ln2 = (d * dm * 2, dm * d * 2, prefetch_wgs(2 * d * dm * 2, _PF_PER_MB))
    assert [a for a in on if a[2]] == [ln1, ln2] * CFG["n_layers"], on
    assert off and not any(a[2] for a in off), off
    assert torch.equal(logits1.view(torch.int16), logits0.view(torch.int16))
    big = max(float(g.norm()) for g in grads0.values())
    assert big > 0
    for n, g0 in grads0.items():
        diff = float((grads1[n] - g0).norm())
        scale = max(float(g0.norm()), 1e-3 * big)  # (b_K and friends: zero in exact arithmetic)
        assert diff <= 1e-4 * scale, (n, diff, float(g0.norm()), big)
