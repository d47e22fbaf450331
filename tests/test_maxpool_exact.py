"""Element-wise tests of the 3x3 / stride-2 / padding-1 max pool of csrc/bn_nhwc.hip (``maxpool3s2_fwd_kernel`` /
``maxpool3s2_bwd_kernel``, bf16 and fp32) on the GPU against the references of tests/bn_exact_util.py (proved on the
CPU by tests/test_bn_exact_ref.py).

Forward: ``y`` bitwise (any NaN equals any NaN) and every argmax byte equal to the reference tap, against torch's CPU
pool with indices and against the independent tap scan, on H, W from 1 to 12 (windows clipped on every side, more than
256 threads with a partial last workgroup), random data, integer ties with both zeros, and NaN / +-inf / whole windows
of -inf / a NaN followed by a larger finite value.  Backward: on the forward's bytes and on hand-built bytes (every
value 0 .. 8, taps that point outside the image, and bytes no tap has), ``dx`` bitwise the fp32 sum in ascending
(kh, kw) order rounded once; every input element no window chose exactly +0.  ``C = 12`` and an ``idx`` view offset by
one byte are refused before any launch (``iit_maxpool3s2_fwd`` / ``_bwd`` check ``C % 8`` and the alignment first).

Measured on an MI355X: 41 cases, 41 passed, none skipped, 2.5 s for the module run on its own (every comparison is
bitwise, so there is no error figure to record); the slowest case is the first (0.2 s, one-time initialisation).  A
library whose scan takes ``>=`` instead of ``>`` failed 18 of the 30 forward cases (every ``ties`` and ``specials`` id
with more than one element per window, and two ``random`` bf16 ids where equal values occur).
"""
import pytest
import torch

import bn_exact_util as X

pytestmark = pytest.mark.gpu

dev = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
DT = {"bf16": BF16, "f32": F32}
CL = torch.channels_last


@pytest.fixture(scope="module")
def K():
    from iit_amd.ops import hip_kernels
    hip_kernels.lib()
    old = hip_kernels.CHECK_BOUNDS
    hip_kernels.CHECK_BOUNDS = True
    yield hip_kernels
    hip_kernels.CHECK_BOUNDS = old


def _nhwc(t: torch.Tensor) -> torch.Tensor:
    """NCHW values -> a channels-last tensor on the device (its memory is [N][H][W][C])."""
    return t.to(dev).contiguous(memory_format=CL)


def _bwd(K, dy, tap, shape):
    """dx [N, C, H, W] (on the host, NCHW) of the kernel for NCHW ``dy`` and tap bytes [N, C, OH, OW]."""
    N, C, H, W = shape
    idx = tap.permute(0, 2, 3, 1).contiguous().to(dev)  # [N][OH][OW][C] bytes
    dx = _nhwc(X.filled(shape, dy.dtype))
    K.maxpool3s2_bwd(_nhwc(dy), idx, dx, N, H, W, C)
    torch.cuda.synchronize()
    return dx.cpu().contiguous()


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("family", X.POOL_FAMILIES)
@pytest.mark.parametrize("shape", X.POOL_SHAPES, ids=["x".join(map(str, s)) for s in X.POOL_SHAPES])
def test_maxpool_fwd_bwd(K, shape, family, dt):
    dtype = DT[dt]
    N, C, H, W = shape
    OH, OW = X.pool_out(H, W)
    x = X.pool_x(family, shape, dtype, H * W + C)
    y = _nhwc(X.filled((N, C, OH, OW), dtype))
    idx = torch.full((N, OH, OW, C), 77, dtype=torch.uint8, device=dev)
    K.maxpool3s2_fwd(_nhwc(x), y, idx, N, H, W, C)
    torch.cuda.synchronize()
    got_y = y.cpu().contiguous()
    got_t = idx.cpu().permute(0, 3, 1, 2).contiguous()
    for name, (ry, rt) in (("torch", X.pool_ref_torch(x)), ("scan", X.pool_ref_scan(x))):
        assert not int(X.bad_pool_y(got_y, ry).sum()), (name, "y")
        assert torch.equal(got_t, rt), (name, "tap", int((got_t != rt).sum()))
    dy = torch.randn(N, C, OH, OW, generator=X.gen(H + W)).to(dtype)
    dx = _bwd(K, dy, got_t, shape)
    ref = X.pool_bwd_emul(dy, got_t, H, W)
    assert not int(X.bad_bits(dx, ref).sum())
    ih = 2 * torch.arange(OH).view(1, 1, OH, 1) - 1 + (got_t // 3).long()
    iw = 2 * torch.arange(OW).view(1, 1, 1, OW) - 1 + (got_t % 3).long()
    chosen = torch.zeros(N, C, H * W, dtype=torch.bool).scatter_(2, (ih * W + iw).view(N, C, -1),
                                                                 torch.ones(N, C, OH * OW, dtype=torch.bool))
    zero = X.bad_bits(dx, torch.zeros_like(dx)).view(N, C, -1)
    assert not int((zero & ~chosen).sum()), "an element no window chose is not +0"


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("shape", X.POOL_SHAPES, ids=["x".join(map(str, s)) for s in X.POOL_SHAPES])
def test_maxpool_bwd_hand_built(K, shape, dt):
    """Bytes the forward would not write: every value 0 .. 8 at random (taps outside the image included: no input
    element gathers them), 9 and 255 (no tap: nothing gathered), and one tap everywhere (four windows meet in an
    element when tap 4 is the centre: up to four additions in order)."""
    dtype = DT[dt]
    N, C, H, W = shape
    OH, OW = X.pool_out(H, W)
    g = X.gen(H * W)
    dy = torch.randn(N, C, OH, OW, generator=g).to(dtype)
    taps = [torch.randint(0, 9, (N, C, OH, OW), generator=g).to(torch.uint8),
            torch.where(torch.rand(N, C, OH, OW, generator=g) < 0.5, 9, 255).to(torch.uint8)]
    taps += [torch.full((N, C, OH, OW), t, dtype=torch.uint8) for t in (0, 4, 8)]
    for tap in taps:
        dx = _bwd(K, dy, tap, shape)
        assert not int(X.bad_bits(dx, X.pool_bwd_emul(dy, tap, H, W)).sum()), int(tap.view(-1)[0])
    assert not int(X.bad_bits(_bwd(K, dy, taps[1], shape), torch.zeros(shape, dtype=dtype)).sum())


def test_maxpool_refusals(K, monkeypatch):
    """``C = 12`` (C % 8) and an ``idx`` view offset by one byte return before any launch: the outputs keep their
    prefill."""
    monkeypatch.setattr(K, "CHECK_BOUNDS", False)  # the native refusal, not the Python-side assertion
    N, H, W = 1, 4, 4
    for C, off in ((12, 0), (16, 1)):
        x = torch.zeros(N * H * W * C, dtype=BF16, device=dev)
        y = X.filled((N * 2 * 2 * C,), BF16, dev)
        idx = torch.full((N * 2 * 2 * C + 8,), 77, dtype=torch.uint8, device=dev)
        dx = X.filled((N * H * W * C,), BF16, dev)
        with pytest.raises(RuntimeError):
            K.maxpool3s2_fwd(x, y, idx[off:], N, H, W, C)
        with pytest.raises(RuntimeError):
            K.maxpool3s2_bwd(y, idx[off:], dx, N, H, W, C)
        torch.cuda.synchronize()
        assert not int(X.bad_bits(y, X.filled(tuple(y.shape), BF16, dev)).sum())
        assert not int(X.bad_bits(dx, X.filled(tuple(dx.shape), BF16, dev)).sum())
        assert bool((idx == 77).all())

