"""``hip32``: an opt-in op backend that runs an fp32 model's projections on the exact-fp32 MFMA GEMM
(``csrc/gemm_f32.hip``, :func:`iit_amd.ops.hip_kernels.gemm_f32`).

:class:`HipF32Ops` is :class:`~iit_amd.ops.torch_ops.TorchOps` in fp32 with ``lin`` (and through it ``mlp_in``,
``mlp_out``, ``unembed``), ``qkv`` and ``o_proj`` replaced; attention, LayerNorm, GELU, the loss and the optimizer
stay where the fp32 torch path has them.  Gradients are returned to autograd exactly as ``x @ W`` returns them
(no direct arena accumulation).  The backend is never chosen automatically: ``select_ops(model, "hip32")`` or
``model.set_op_backend("hip32")``.

``hip32x`` (:class:`HipF32XOps`) is ``hip32`` plus attention on the exact-fp32 MFMA kernel of
``csrc/attn_fp32.hip`` (:class:`AttentionF32Fn`), opt-in in the same way.

``hip32n`` (:class:`HipF32NOps`) is ``hip32x`` plus the rest of a GPT-2-family block: LayerNorm on
``csrc/block_f32.hip`` (:class:`LayerNormF32Fn`), ``gelu_new`` in the W_in GEMM's epilogue (:class:`MlpInF32Fn`),
its derivative in the ``dY W_out^T`` GEMM's epilogue (:class:`MlpGeluResidualF32Fn`) and both residual adds in the
projections' epilogues (``LinearF32Fn``'s ``resid``).  Opt-in in the same way.

``hip32p`` (:class:`HipF32POps`) is ``hip32n`` plus the paired forward: an interchange intervention runs as one
forward of 2B rows up to its deepest site (``HookedTransformer.run_paired``), with the ``hook_z`` splice in the store of
``csrc/attn_fp32.hip``'s paired forward, its gradient mask in the staging of the masked backward, and an
``mlp.hook_post`` splice as a sparse copy (``iit_sparse_pair_f32``).  Opt-in in the same way.
"""
from __future__ import annotations

import torch

from . import hip_kernels as K
from .hip_ops import Paired, PairSpliceFn, _one, pair_specs
from .splice import PatchSpec, patch_spec
from .torch_ops import TorchOps, act_fn


def _up4(n: int) -> int:
    return (n + 3) // 4 * 4


def _operand(t: torch.Tensor) -> torch.Tensor:
    """``t [rows][cols]`` as the kernel takes it -- unit column stride, a row pitch that is a multiple of 4 elements,
    a 16-byte aligned base -- copying into a padded buffer only when ``t`` is not already so."""
    rows, cols = t.shape
    if (t.dtype == torch.float32 and t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.stride(0) >= cols
            and t.data_ptr() % 16 == 0):
        return t
    buf = torch.empty(rows, _up4(cols), dtype=torch.float32, device=t.device)[:, :cols]
    buf.copy_(t)
    return buf


def _out(rows: int, cols: int, device) -> torch.Tensor:
    """Uninitialised fp32 ``[rows][cols]`` output whose row pitch is a multiple of 4 elements."""
    return torch.empty(rows, _up4(cols), dtype=torch.float32, device=device)[:, :cols]


def _tile(M: int, N: int) -> int:
    """The 128 x 128 tile once its tiles alone give every CU a workgroup and neither extent leaves half of it
    empty, else 64 x 64 (a stated policy)."""
    return 1 if min(M, N) >= 128 and ((M + 127) // 128) * ((N + 127) // 128) >= K.N_CU else 0


def _gemm(A, B, C, M, N, Kd, mode, epi=K.EPI_F32_STORE, bias=None, resid=None, aux=None):
    tile = _tile(M, N)
    K.gemm_f32(A, B, C, M=M, N=N, K=Kd, lda=A.stride(0), ldb=B.stride(0), ldc=C.stride(0), mode=mode, epi=epi,
               bias=bias, resid=resid, ldr=0 if resid is None else resid.stride(0), tile=tile,
               splits=K.gemm_f32_splits(M, N, Kd, tile), aux=aux, ldx=0 if aux is None else aux.stride(0))


def _forward(x2, W2, b, r2=None):
    """``x2 [T][K] @ W2 [K][N] (+ b) (+ r2)``: one mode-2 GEMM, bias and residual in its epilogue."""
    T, Kd = x2.shape
    N = W2.shape[1]
    y = _out(T, N, x2.device)
    _gemm(x2, W2, y, T, N, Kd, K.MODE_BKM, K.EPI_F32_STORE if r2 is None else K.EPI_F32_RESID, b, r2)
    return y


def _backward(x2, W2, dy2, need_x: bool, need_w: bool):
    """``(dX = dY W^T`` by a mode-0 GEMM, ``dW = X^T dY`` by a mode-3 GEMM); W2 ``[K][N]`` serves both as stored."""
    T, Kd = x2.shape
    N = W2.shape[1]
    dx = dw = None
    if need_x:
        dx = _out(T, Kd, x2.device)
        _gemm(dy2, W2, dx, T, Kd, N, K.MODE_NN)
    if need_w:
        dw = _out(Kd, N, x2.device)
        _gemm(x2, dy2, dw, Kd, N, T, K.MODE_AKM | K.MODE_BKM)
    return dx, dw


def weight_ok(x2: torch.Tensor, W2: torch.Tensor) -> bool:
    """Whether ``x2 @ W2`` can take the kernel: fp32 on the GPU, a 2-D weight with unit column stride that passes
    ``gemm_f32_ok`` (aligned base, row pitch a multiple of 4).  ``x2`` is an operand as :func:`_operand` returns it
    and also stands in for the output, which the function allocates aligned."""
    if not (x2.is_cuda and W2.is_cuda and x2.dtype == torch.float32 and W2.dtype == torch.float32 and W2.dim() == 2
            and W2.stride(1) == 1 and x2.shape[0] > 0):
        return False
    return K.gemm_f32_ok(x2, W2, x2, M=x2.shape[0], N=W2.shape[1], K=x2.shape[1], lda=x2.stride(0),
                         ldb=W2.stride(0), ldc=_up4(W2.shape[1]), mode=K.MODE_BKM, epi=K.EPI_F32_STORE)


class LinearF32Fn(torch.autograd.Function):
    """``y = x @ W2 (+ b) (+ resid)`` for fp32 ``x [..., K]`` and a weight ``W2 [K][N]`` with unit column stride (any
    aligned row pitch: the arena's padded ``W_U`` is taken as stored).  The backward returns ``dX``, ``dW``,
    ``db = colsum(dY)`` (``sum(0)``: a fixed-order reduction) and ``dresid = dY`` to autograd."""

    @staticmethod
    def forward(ctx, x, W2, b, resid=None):
        Kd, N = W2.shape
        lead = x.shape[:-1]
        x2 = _operand(x.reshape(-1, Kd))
        r2 = None if resid is None else _operand(resid.reshape(-1, N))
        ctx.save_for_backward(x2, W2)
        ctx.lead, ctx.has_b, ctx.has_r = lead, b is not None, resid is not None
        return _forward(x2, W2, b, r2).view(*lead, N)

    @staticmethod
    def backward(ctx, dy):
        x2, W2 = ctx.saved_tensors
        Kd, N = W2.shape
        dy2 = _operand(dy.reshape(-1, N))
        dx, dw = _backward(x2, W2, dy2, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        db = dy2.sum(0) if ctx.has_b and ctx.needs_input_grad[2] else None
        dr = dy if ctx.has_r and ctx.needs_input_grad[3] else None
        return None if dx is None else dx.view(*ctx.lead, Kd), dw, db, dr


class QKVF32Fn(torch.autograd.Function):
    """The packed QKV projection: ``W_Q | W_K | W_V`` in the arena layout of ``qkv_arena_groups`` are one
    ``[d][(H + 2 H_kv) dh]`` matrix, so the three projections are one GEMM, and so are their input gradient and
    their weight gradient; the three weight (bias) gradients are strided views of one ``[d][N]`` (``[N]``) buffer."""

    @staticmethod
    def forward(ctx, x, W_Q, W_K, W_V, b_Q, b_K, b_V):
        H, d, dh = W_Q.shape
        Hkv = W_K.shape[0]
        N = (H + 2 * Hkv) * dh
        Wp = W_Q.detach().as_strided((d, N), (N, 1))
        bp = b_Q.detach().as_strided((N,), (1,))
        lead = x.shape[:-1]
        x2 = _operand(x.reshape(-1, d))
        ctx.save_for_backward(x2, Wp)
        ctx.lead, ctx.dims = lead, (H, Hkv, dh)
        y = _forward(x2, Wp, bp).view(*lead, N)
        return (y[..., :H * dh].view(*lead, H, dh), y[..., H * dh:(H + Hkv) * dh].view(*lead, Hkv, dh),
                y[..., (H + Hkv) * dh:].view(*lead, Hkv, dh))

    @staticmethod
    def backward(ctx, dq, dk, dv):
        x2, Wp = ctx.saved_tensors
        H, Hkv, dh = ctx.dims
        d, N = Wp.shape
        T = x2.shape[0]
        dy2 = _out(T, N, x2.device)
        c0 = 0
        for g, n in zip((dq, dk, dv), (H * dh, Hkv * dh, Hkv * dh)):
            if g is None:
                dy2[:, c0:c0 + n].zero_()
            else:
                dy2[:, c0:c0 + n].copy_(g.reshape(T, n))
            c0 += n
        need = ctx.needs_input_grad
        dx, dw = _backward(x2, Wp, dy2, need[0], any(need[1:4]))
        gw = [None] * 3
        gb = [None] * 3
        spans = ((0, H), (H, Hkv), (H + Hkv, Hkv))
        if dw is not None:
            dw3 = dw.view(d, H + 2 * Hkv, dh)
            gw = [dw3[:, c:c + n].permute(1, 0, 2) if need[1 + i] else None for i, (c, n) in enumerate(spans)]
        if any(need[4:7]):
            db = dy2.sum(0).view(H + 2 * Hkv, dh)
            gb = [db[c:c + n] if need[4 + i] else None for i, (c, n) in enumerate(spans)]
        return (None if dx is None else dx.view(*ctx.lead, d), *gw, *gb)


def _same_storage(*ts) -> bool:
    p = ts[0].untyped_storage().data_ptr()
    return all(t.untyped_storage().data_ptr() == p for t in ts)


def packed_qkv(W_Q, W_K, W_V, b_Q, b_K, b_V) -> bool:
    """Whether the six parameters have the packed arena layout of ``qkv_arena_groups``: weights ``[H][d][dh]`` with
    strides ``(dh, N, 1)`` at adjacent offsets of one buffer, biases packed contiguously in the same order."""
    if W_Q.dim() != 3 or any(b is None for b in (b_Q, b_K, b_V)):
        return False
    H, d, dh = W_Q.shape
    Hkv = W_K.shape[0]
    N = (H + 2 * Hkv) * dh
    ws, bs = (W_Q, W_K, W_V), (b_Q, b_K, b_V)
    if W_K.shape != (Hkv, d, dh) or W_V.shape != (Hkv, d, dh) or any(w.stride() != (dh, N, 1) for w in ws):
        return False
    if b_Q.shape != (H, dh) or b_K.shape != (Hkv, dh) or b_V.shape != (Hkv, dh) or not all(
            b.is_contiguous() for b in bs):
        return False
    if not (_same_storage(*ws) and _same_storage(*bs)):
        return False
    offs = (0, H * dh * 4, (H + Hkv) * dh * 4)
    return all(w.data_ptr() == W_Q.data_ptr() + o and b.data_ptr() == b_Q.data_ptr() + o
               for w, b, o in zip(ws, bs, offs))


class HipF32Ops(TorchOps):
    """fp32 :class:`TorchOps` whose projections run on ``csrc/gemm_f32.hip``.  ``calls`` counts, per op, the calls
    that took the kernel (``"qkv"``, ``"o_proj"``, ``"mlp_in"``, ``"mlp_out"``, ``"unembed"``, ``"lin"``) and those
    that fell back to the inherited torch op (``"<op>_fallback"``)."""
    name = "hip32"
    fused = False
    calls: dict = {}

    def __init__(self):
        super().__init__(torch.float32)

    @classmethod
    def _count(cls, op: str) -> None:
        cls.calls[op] = cls.calls.get(op, 0) + 1

    def _lin(self, op: str, x, W, b):
        Wv = self.w(W)
        bv = None if b is None else self.w(b)
        if Wv.dim() == 2 and x.dtype == torch.float32 and x.is_cuda and x.numel() > 0 \
                and (bv is None or (bv.dim() == 1 and bv.dtype == torch.float32 and bv.is_contiguous())):
            x2 = _operand(x.detach().reshape(-1, x.shape[-1]))
            if not weight_ok(x2, Wv) and Wv.is_cuda and Wv.dtype == torch.float32:
                # a weight outside the arena whose rows are no multiple of 4 long (W_U [d][97]): a padded copy per
                # call (differentiable, so dW reaches the parameter); the arena stores such rows padded already
                Wv = _operand(Wv)
            if weight_ok(x2, Wv):
                self._count(op)
                return LinearF32Fn.apply(x, Wv, bv)
        self._count(op + "_fallback")
        y = x @ Wv
        return y if bv is None else y + bv

    def lin(self, x, W, b=None):
        return self._lin("lin", x, W, b)

    def qkv(self, x, W_Q, W_K, W_V, b_Q, b_K, b_V):
        ps = (W_Q, W_K, W_V, b_Q, b_K, b_V)
        if x.is_cuda and x.dtype == torch.float32 and x.numel() > 0 and all(
                p is not None and p.dtype == torch.float32 and self.w(p) is p for p in ps) and packed_qkv(*ps):
            H, d, dh = W_Q.shape
            N = (H + 2 * W_K.shape[0]) * dh
            if weight_ok(_operand(x.detach().reshape(-1, d)), W_Q.detach().as_strided((d, N), (N, 1))):
                self._count("qkv")
                return QKVF32Fn.apply(x, *ps)
        self._count("qkv_fallback")
        return TorchOps.qkv(self, x, *ps)

    def o_proj(self, z, W_O, b_O):
        Wv = self.w(W_O)
        if Wv.dim() == 3 and Wv.is_contiguous():
            H, dh, d = Wv.shape
            return self._lin("o_proj", z.reshape(*z.shape[:-2], H * dh), Wv.view(H * dh, d), b_O)
        self._count("o_proj_fallback")
        return TorchOps.o_proj(self, z, W_O, b_O)

    def mlp_in(self, x, W_in, b_in, act: str, hook_pre=None):
        pre = self._lin("mlp_in", x, W_in, b_in)
        if hook_pre is not None:
            pre = hook_pre(pre)
        return pre, act_fn(act)(pre)

    def mlp_out(self, post, W_out, b_out):
        return self._lin("mlp_out", post, W_out, b_out)

    def unembed(self, x, W_U, b_U):
        return self._lin("unembed", x, W_U, b_U)


def _unit_last(t: torch.Tensor) -> torch.Tensor:
    return t if t.stride(-1) == 1 or t.shape[-1] == 1 else t.contiguous()


class AttentionF32Fn(torch.autograd.Function):
    """``z = softmax(scale q k^T (causal mask)) v`` for fp32 q, k, v ``[B][S][H][dh]`` on ``csrc/attn_fp32.hip``
    (``S <= 64``, ``dh <= 64``).  The operands are taken as stored (the q / k / v views of ``QKVF32Fn``'s packed
    output are the normal case); only one whose last stride is not 1 is copied.  q, k, v and the row log-sum-exp are
    saved; the backward is one launch that recomputes P and writes dq, dk, dv."""

    @staticmethod
    def forward(ctx, q, k, v, causal: bool, scale: float):
        q, k, v = (_unit_last(t.detach()) for t in (q, k, v))
        B, S, H, dh = q.shape
        z = torch.empty(B, S, H, dh, dtype=torch.float32, device=q.device)
        lse = torch.empty(B, H, S, dtype=torch.float32, device=q.device)
        K.attn_f32_fwd(q, k, v, z, lse, scale, causal)
        ctx.save_for_backward(q, k, v, lse)
        ctx.causal, ctx.scale = bool(causal), float(scale)
        return z

    @staticmethod
    def backward(ctx, dz):
        q, k, v, lse = ctx.saved_tensors
        dq, dk, dv = (torch.empty(q.shape, dtype=torch.float32, device=q.device) for _ in range(3))
        K.attn_f32_bwd(q, k, v, _unit_last(dz), lse, dq, dk, dv, ctx.scale, ctx.causal)
        need = ctx.needs_input_grad
        return dq if need[0] else None, dk if need[1] else None, dv if need[2] else None, None, None


class HipF32XOps(HipF32Ops):
    """:class:`HipF32Ops` with attention on ``csrc/attn_fp32.hip`` as well.  ``calls`` (its own dictionary, not
    ``HipF32Ops.calls``) also counts ``"attention"`` (the kernel ran) and ``"attention_fallback"`` (the inherited
    torch op: S or dh above 64, a non-fp32 or CPU operand, or the hooks / masked fill that ``compute_z`` passes on
    when a score or pattern hook is live or the fill is not ``-inf``).  ``native_attention`` tells
    ``Attention.compute_z`` to call ``attention`` instead of ``TorchOps.attention``."""
    name = "hip32x"
    fused = False
    native_attention = True
    calls: dict = {}

    def attention(self, q, k, v, causal: bool, attn_scale: float, **kw):
        if not kw and K.attn_f32_ok(q, k, v):
            self._count("attention")
            return AttentionF32Fn.apply(q, k, v, causal, 1.0 / attn_scale)
        self._count("attention_fallback")
        return TorchOps.attention(self, q, k, v, causal, attn_scale, **kw)


def _rows(t: torch.Tensor, d: int) -> torch.Tensor:
    """``t [..., d]`` as the rows ``[T][d]`` the LayerNorm kernels take: as stored when the last stride is 1 and the
    row pitch covers the row, else copied once."""
    t2 = t.reshape(-1, d)
    if (d == 1 or t2.stride(1) == 1) and (t2.shape[0] == 1 or t2.stride(0) >= d) and t2.dtype == torch.float32:
        return t2
    return t2.float().contiguous()


class LayerNormF32Fn(torch.autograd.Function):
    """``y = (x - mean) / sqrt(var + eps) (* w + b)`` over the last dimension of fp32 ``x`` on ``csrc/block_f32.hip``
    (``d <= 4096``; ``w`` and ``b`` both or neither).  ``x`` and the row statistics are saved; the backward is one
    ``ln_f32_bwd`` call that returns ``dx``, ``dw`` and ``db`` to autograd (no atomics: the affine gradients are
    per-block partials added in block order)."""

    @staticmethod
    def forward(ctx, x, w, b, eps: float):
        d = x.shape[-1]
        x2 = _rows(x.detach(), d)
        T = x2.shape[0]
        y = torch.empty(T, d, dtype=torch.float32, device=x.device)
        mean = torch.empty(T, dtype=torch.float32, device=x.device)
        rstd = torch.empty(T, dtype=torch.float32, device=x.device)
        wd = None if w is None else w.detach()
        K.ln_f32_fwd(x2, wd, None if b is None else b.detach(), y, mean, rstd, eps)
        ctx.save_for_backward(x2, mean, rstd, wd)
        ctx.shape = x.shape
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        x2, mean, rstd, w = ctx.saved_tensors
        T, d = x2.shape
        dx = torch.empty(T, d, dtype=torch.float32, device=x2.device)
        dw = db = None
        if w is not None and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]):
            dw, db = torch.empty(d, dtype=torch.float32, device=x2.device), torch.empty(
                d, dtype=torch.float32, device=x2.device)
        K.ln_f32_bwd(_rows(dy, d), x2, mean, rstd, w, dx, dw, db)
        need = ctx.needs_input_grad
        return (dx.view(ctx.shape) if need[0] else None, dw if need[1] else None, db if need[2] else None, None)


def _mlp_in_forward(x2, W_in, b_in):
    """``(pre, post)`` ``[T][d_mlp]`` (contiguous: ``d_mlp % 4 == 0``) of one ``EPI_GELU`` GEMM."""
    T, Kd = x2.shape
    N = W_in.shape[1]
    pre = torch.empty(T, N, dtype=torch.float32, device=x2.device)
    post = torch.empty(T, N, dtype=torch.float32, device=x2.device)
    _gemm(x2, W_in, post, T, N, Kd, K.MODE_BKM, K.EPI_GELU, b_in, aux=pre)
    return pre, post


class MlpInF32Fn(torch.autograd.Function):
    """``post = gelu_new(x @ W_in (+ b_in))``: one GEMM whose epilogue stores the pre-activation beside the result
    (``d_mlp % 4 == 0``).  ``pre`` is kept for the backward and not returned: ``dpre = dpost * gelu_new'(pre)``
    (``dgelu_f32``), then ``LinearF32Fn``'s two GEMMs and ``db_in = dpre.sum(0)``."""

    @staticmethod
    def forward(ctx, x, W_in, b_in):
        Kd, N = W_in.shape
        x2 = _operand(x.detach().reshape(-1, Kd))
        pre, post = _mlp_in_forward(x2, W_in.detach(), None if b_in is None else b_in.detach())
        ctx.save_for_backward(x2, W_in.detach(), pre)
        ctx.lead, ctx.has_b = x.shape[:-1], b_in is not None
        return post.view(*ctx.lead, N)

    @staticmethod
    def backward(ctx, dpost):
        x2, W_in, pre = ctx.saved_tensors
        Kd, N = W_in.shape
        dpre = torch.empty_like(pre)
        K.dgelu_f32(dpost.reshape(-1, N).contiguous(), pre, dpre)
        dx, dw = _backward(x2, W_in, dpre, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        db = dpre.sum(0) if ctx.has_b and ctx.needs_input_grad[2] else None
        return None if dx is None else dx.view(*ctx.lead, Kd), dw, db


class MlpGeluResidualF32Fn(torch.autograd.Function):
    """``resid + gelu_new(x @ W_in + b_in) @ W_out + b_out``: an ``EPI_GELU`` GEMM and an ``EPI_F32_RESID`` GEMM
    (``d_mlp % 4 == 0``).  Backward: ``dpre`` out of one ``EPI_DGELU`` GEMM (``dY W_out^T`` with ``aux = pre``),
    ``dW_out = post^T dY``, ``db_out = dY.sum(0)``, ``dW_in = x^T dpre``, ``db_in = dpre.sum(0)``,
    ``dx = dpre W_in^T`` and ``dresid = dY``, all returned to autograd."""

    @staticmethod
    def forward(ctx, x, W_in, b_in, W_out, b_out, resid):
        d, dm = W_in.shape
        n_out = W_out.shape[1]
        x2 = _operand(x.detach().reshape(-1, d))
        r2 = _operand(resid.detach().reshape(-1, n_out))
        W_in, W_out = W_in.detach(), W_out.detach()
        pre, post = _mlp_in_forward(x2, W_in, None if b_in is None else b_in.detach())
        y = _forward(post, W_out, None if b_out is None else b_out.detach(), r2)
        ctx.save_for_backward(x2, W_in, W_out, pre, post)
        ctx.lead, ctx.has_b = x.shape[:-1], (b_in is not None, b_out is not None)
        return y.view(*resid.shape[:-1], n_out)

    @staticmethod
    def backward(ctx, dy):
        x2, W_in, W_out, pre, post = ctx.saved_tensors
        d, dm = W_in.shape
        n_out = W_out.shape[1]
        T = x2.shape[0]
        need = ctx.needs_input_grad
        dy2 = _operand(dy.reshape(-1, n_out))
        dpre = torch.empty_like(pre)
        _gemm(dy2, W_out, dpre, T, dm, n_out, K.MODE_NN, K.EPI_DGELU, aux=pre)
        dw_out = None
        if need[3]:
            dw_out = _out(dm, n_out, x2.device)
            _gemm(post, dy2, dw_out, dm, n_out, T, K.MODE_AKM | K.MODE_BKM)
        db_out = dy2.sum(0) if ctx.has_b[1] and need[4] else None
        dx, dw_in = _backward(x2, W_in, dpre, need[0], need[1])
        db_in = dpre.sum(0) if ctx.has_b[0] and need[2] else None
        return (None if dx is None else dx.view(*ctx.lead, d), dw_in, db_in, dw_out, db_out,
                dy if need[5] else None)


_GELU_NEW = ("gelu_new", "gelu_fast", "gelu_pytorch_tanh")


class HipF32NOps(HipF32XOps):
    """:class:`HipF32XOps` with the rest of a GPT-2-family block on the repo's kernels when no hook inside the op is
    live: LayerNorm (``native_layer_norm`` tells ``LayerNormSite.run`` to call ``layer_norm``), ``gelu_new`` and its
    derivative in GEMM epilogues, the two residual adds in the projections' epilogues (``fuses_residual``).
    ``calls`` (its own dictionary) also counts ``"layer_norm"`` / ``"layer_norm_fallback"`` and ``"mlp_fused"`` /
    ``"mlp_fused_fallback"``; the residual projections count under ``"o_proj"`` / ``"mlp_out"``."""
    name = "hip32n"
    fused = False
    native_layer_norm = True
    fuses_residual = True
    calls: dict = {}

    def _param(self, p) -> bool:
        return p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and self.w(p) is p

    def layer_norm(self, x, w, b, eps, **kw):
        if not kw and K.ln_f32_ok(x) and (w is None) == (b is None) and (
                w is None or (self._param(w) and self._param(b) and w.shape == b.shape == x.shape[-1:])):
            self._count("layer_norm")
            return LayerNormF32Fn.apply(x, w, b, eps)
        self._count("layer_norm_fallback")
        return TorchOps.layer_norm(self, x, w, b, eps, **kw)

    def _lin_resid(self, op: str, x, W, b, resid):
        """``resid + x @ W (+ b)`` by ``LinearF32Fn``'s residual epilogue under the conditions of ``_lin``; None when
        they do not hold (the caller composes the fallback, which counts itself)."""
        Wv = self.w(W)
        bv = None if b is None else self.w(b)
        if not (Wv.dim() == 2 and x.dtype == torch.float32 and x.is_cuda and x.numel() > 0
                and resid.dtype == torch.float32 and resid.is_cuda and resid.shape[:-1] == x.shape[:-1]
                and resid.shape[-1] == Wv.shape[1]
                and (bv is None or (bv.dim() == 1 and bv.dtype == torch.float32 and bv.is_contiguous()))):
            return None
        if not weight_ok(_operand(x.detach().reshape(-1, x.shape[-1])), Wv):
            return None
        self._count(op)
        return LinearF32Fn.apply(x, Wv, bv, resid)

    def o_proj_residual(self, z, W_O, b_O, resid):
        Wv = self.w(W_O)
        if Wv.dim() == 3 and Wv.is_contiguous():
            H, dh, d = Wv.shape
            out = self._lin_resid("o_proj", z.reshape(*z.shape[:-2], H * dh), Wv.view(H * dh, d), b_O, resid)
            if out is not None:
                return out
        return self.residual(resid, self.o_proj(z, W_O, b_O))

    def mlp_out_residual(self, post, W_out, b_out, resid):
        out = self._lin_resid("mlp_out", post, W_out, b_out, resid)
        return out if out is not None else self.residual(resid, self.mlp_out(post, W_out, b_out))

    def _mlp_in_ok(self, x, W_in, b_in) -> bool:
        if not (x.is_cuda and x.dtype == torch.float32 and x.numel() > 0 and W_in.dim() == 2 and W_in.shape[1] % 4 == 0
                and self.w(W_in) is W_in and (b_in is None or (b_in.dim() == 1 and self._param(b_in)))):
            return False
        return weight_ok(_operand(x.detach().reshape(-1, x.shape[-1])), W_in)

    def mlp_in(self, x, W_in, b_in, act: str, hook_pre=None):
        """With no ``hook_pre`` and an act of the ``gelu_new`` family (``d_mlp % 4 == 0``): :class:`MlpInF32Fn`, and
        ``(None, post)`` is returned -- every caller that passes no ``hook_pre`` discards the first element, and
        the pre-activation stays inside the function for its backward.  Anything else: the inherited method."""
        if hook_pre is None and act in _GELU_NEW and self._mlp_in_ok(x, W_in, b_in):
            self._count("mlp_in")
            return None, MlpInF32Fn.apply(x, W_in, b_in)
        return super().mlp_in(x, W_in, b_in, act, hook_pre=hook_pre)

    def mlp_gelu_residual(self, x, W_in, b_in, W_out, b_out, resid):
        """The whole ``gelu_new`` MLP and its residual add (:class:`MlpGeluResidualF32Fn`) when both weights pass
        ``weight_ok``; else ``mlp_in`` and ``mlp_out_residual`` composed."""
        if self._mlp_in_ok(x, W_in, b_in) and W_out.dim() == 2 and self.w(W_out) is W_out and W_out.is_cuda \
                and W_out.dtype == torch.float32 and (b_out is None or (b_out.dim() == 1 and self._param(b_out))) \
                and resid.is_cuda and resid.dtype == torch.float32 and resid.shape[:-1] == x.shape[:-1] \
                and resid.shape[-1] == W_out.shape[1]:
            # post is allocated aligned and contiguous [T][d_mlp]: W_out itself stands in for it and for the output
            if W_out.stride(1) == 1 and W_out.shape[0] == W_in.shape[1] and K.gemm_f32_ok(
                    W_out, W_out, W_out, M=x.numel() // x.shape[-1], N=W_out.shape[1], K=W_in.shape[1],
                    lda=W_in.shape[1], ldb=W_out.stride(0), ldc=_up4(W_out.shape[1]), mode=K.MODE_BKM,
                    epi=K.EPI_F32_STORE):
                self._count("mlp_fused")
                return MlpGeluResidualF32Fn.apply(x, W_in, b_in, W_out, b_out, resid)
        self._count("mlp_fused_fallback")
        _, post = self.mlp_in(x, W_in, b_in, "gelu_new")
        return self.mlp_out_residual(post, W_out, b_out, resid)


# ------------------------------------------------------------------------------ hip32p: paired source + base rows
# Each paired Function derives from the unpaired one: the forward runs the same kernel once over the 2B / 2T rows
# (rows [0, B) base, [B, 2B) source), returns the base rows, puts the full result in ``box`` and saves base-row slices
# only, so the backward is the unpaired backward on the tensors the unpaired forward would have saved.


def _base_rows(x: torch.Tensor) -> int:
    return x.numel() // x.shape[-1]


class LayerNormF32PairFn(LayerNormF32Fn):
    @staticmethod
    def forward(ctx, x, w, b, eps, x_full, box):
        d = x.shape[-1]
        x2 = _rows(x_full.detach(), d)
        T2, T = x2.shape[0], _base_rows(x)
        y = torch.empty(T2, d, dtype=torch.float32, device=x.device)
        mean = torch.empty(T2, dtype=torch.float32, device=x.device)
        rstd = torch.empty(T2, dtype=torch.float32, device=x.device)
        wd = None if w is None else w.detach()
        K.ln_f32_fwd(x2, wd, None if b is None else b.detach(), y, mean, rstd, eps)
        ctx.save_for_backward(x2[:T], mean[:T], rstd[:T], wd)
        ctx.shape = x.shape
        yf = y.view(x_full.shape)
        box.append(yf)
        return yf[:x.shape[0]]

    @staticmethod
    def backward(ctx, dy):
        return LayerNormF32Fn.backward(ctx, dy) + (None, None)


class QKVF32PairFn(QKVF32Fn):
    @staticmethod
    def forward(ctx, x, W_Q, W_K, W_V, b_Q, b_K, b_V, x_full, box):
        H, d, dh = W_Q.shape
        Hkv = W_K.shape[0]
        N = (H + 2 * Hkv) * dh
        Wp = W_Q.detach().as_strided((d, N), (N, 1))
        bp = b_Q.detach().as_strided((N,), (1,))
        x2 = _operand(x_full.detach().reshape(-1, d))
        ctx.save_for_backward(x2[:_base_rows(x)], Wp)
        ctx.lead, ctx.dims = x.shape[:-1], (H, Hkv, dh)
        lead = x_full.shape[:-1]
        yf = _forward(x2, Wp, bp).view(*lead, N)
        box.append((yf[..., :H * dh].view(*lead, H, dh), yf[..., H * dh:(H + Hkv) * dh].view(*lead, Hkv, dh),
                    yf[..., (H + Hkv) * dh:].view(*lead, Hkv, dh)))
        return tuple(t[:x.shape[0]] for t in box[0])

    @staticmethod
    def backward(ctx, dq, dk, dv):
        return QKVF32Fn.backward(ctx, dq, dk, dv) + (None, None)


class AttentionF32PairFn(AttentionF32Fn):
    """Attention over the 2B rows.  ``spec`` (a ``PatchSpec`` over the base ``[B][S][H][dh]``, or None): the
    interchange splice of ``hook_z`` in the kernel's store (``attn_f32_fwd_pair``), and its gradient mask in the
    staging of dO (``attn_f32_bwd_masked``).  Without one: the plain forward and the plain backward."""

    @staticmethod
    def forward(ctx, q, k, v, causal, scale, spec, q_full, k_full, v_full, box):
        qf, kf, vf = (_unit_last(t.detach()) for t in (q_full, k_full, v_full))
        B2, S, H, dh = qf.shape
        B = q.shape[0]
        z = torch.empty(B2, S, H, dh, dtype=torch.float32, device=q.device)
        lse = torch.empty(B2, H, S, dtype=torch.float32, device=q.device)
        if spec is None:
            K.attn_f32_fwd(qf, kf, vf, z, lse, scale, causal)
        else:
            K.attn_f32_fwd_pair(qf, kf, vf, z, lse, scale, causal, spec)
        ctx.save_for_backward(qf[:B], kf[:B], vf[:B], lse[:B])
        ctx.causal, ctx.scale, ctx.spec = bool(causal), float(scale), spec
        box.append(z)
        return z[:B]

    @staticmethod
    def backward(ctx, dz):
        if ctx.spec is None:
            return AttentionF32Fn.backward(ctx, dz) + (None,) * 5
        q, k, v, lse = ctx.saved_tensors
        dq, dk, dv = (torch.empty(q.shape, dtype=torch.float32, device=q.device) for _ in range(3))
        K.attn_f32_bwd_masked(q, k, v, _unit_last(dz), lse, dq, dk, dv, ctx.scale, ctx.causal, ctx.spec)
        need = ctx.needs_input_grad
        return (dq if need[0] else None, dk if need[1] else None, dv if need[2] else None) + (None,) * 7


class LinearF32PairFn(LinearF32Fn):
    @staticmethod
    def forward(ctx, x, W2, b, resid, x_full, resid_full, box):
        Kd, N = W2.shape
        x2 = _operand(x_full.detach().reshape(-1, Kd))
        r2 = None if resid_full is None else _operand(resid_full.detach().reshape(-1, N))
        ctx.save_for_backward(x2[:_base_rows(x)], W2)
        ctx.lead, ctx.has_b, ctx.has_r = x.shape[:-1], b is not None, resid is not None
        yf = _forward(x2, W2, b, r2).view(*x_full.shape[:-1], N)
        box.append(yf)
        return yf[:x.shape[0]]

    @staticmethod
    def backward(ctx, dy):
        return LinearF32Fn.backward(ctx, dy) + (None, None, None)


class MlpInF32PairFn(MlpInF32Fn):
    """``spec`` (a ``PatchSpec`` over the base ``[B][S][d_mlp]``, or None): the interchange splice of
    ``mlp.hook_post`` inside the op -- ``sparse_pair_f32`` copies the selected elements of the source half into the
    base half right after the GEMM, and zeroes them in ``dpost`` before the dgelu."""

    @staticmethod
    def forward(ctx, x, W_in, b_in, x_full, spec, box):
        Kd, N = W_in.shape
        x2 = _operand(x_full.detach().reshape(-1, Kd))
        T = _base_rows(x)
        pre, post = _mlp_in_forward(x2, W_in.detach(), None if b_in is None else b_in.detach())
        if spec is not None:
            K.sparse_pair_f32(post, T, N, spec, 0)
        ctx.save_for_backward(x2[:T], W_in.detach(), pre[:T])
        ctx.lead, ctx.has_b, ctx.spec = x.shape[:-1], b_in is not None, spec
        pf = post.view(*x_full.shape[:-1], N)
        box.append(pf)
        return pf[:x.shape[0]]

    @staticmethod
    def backward(ctx, dpost):
        if ctx.spec is not None:
            N = dpost.shape[-1]
            dpost = dpost.reshape(-1, N).clone(memory_format=torch.contiguous_format)
            K.sparse_pair_f32(dpost, dpost.shape[0], N, ctx.spec, 1)
        return MlpInF32Fn.backward(ctx, dpost) + (None, None, None)


class MlpGeluResidualF32PairFn(MlpGeluResidualF32Fn):
    @staticmethod
    def forward(ctx, x, W_in, b_in, W_out, b_out, resid, x_full, resid_full, box):
        d, dm = W_in.shape
        n_out = W_out.shape[1]
        x2 = _operand(x_full.detach().reshape(-1, d))
        r2 = _operand(resid_full.detach().reshape(-1, n_out))
        W_in, W_out = W_in.detach(), W_out.detach()
        T = _base_rows(x)
        pre, post = _mlp_in_forward(x2, W_in, None if b_in is None else b_in.detach())
        y = _forward(post, W_out, None if b_out is None else b_out.detach(), r2)
        ctx.save_for_backward(x2[:T], W_in, W_out, pre[:T], post[:T])
        ctx.lead, ctx.has_b = x.shape[:-1], (b_in is not None, b_out is not None)
        yf = y.view(*resid_full.shape[:-1], n_out)
        box.append(yf)
        return yf[:resid.shape[0]]

    @staticmethod
    def backward(ctx, dy):
        return MlpGeluResidualF32Fn.backward(ctx, dy) + (None, None, None)


def _heads_spec(heads, shape):
    """The ``PatchSpec`` over ``shape = (B, S, H, dh)`` that selects whole heads (none for an empty list)."""
    runs = []
    for h in sorted(set(int(h) for h in heads)):
        if runs and runs[-1][1] == h:
            runs[-1] = (runs[-1][0], h + 1)
        else:
            runs.append((h, h + 1))
    if len(runs) > 8:
        return None
    return PatchSpec([(n, runs if i == 2 else [(0, n)], 0) for i, n in enumerate(shape)])


class HipF32POps(HipF32NOps):
    """:class:`HipF32NOps` with the paired forward: an interchange intervention as one forward of 2B rows up to the
    deepest site (``HookedTransformer.run_paired`` / ``TransformerBlock.forward_paired``, the protocol of
    ``HipOps``), on the fp32 kernels.  The ``hook_z`` splice and its gradient mask run inside the attention kernels
    (``csrc/attn_fp32.hip`` ``iit_attn_f32_fwd_pair`` / ``iit_attn_f32_bwd_masked``), an ``mlp.hook_post`` splice as
    one thread per selected element (``iit_sparse_pair_f32``).  Everything else is ``hip32n``.  ``calls`` (its own
    dictionary) also counts the paired ops (``"pair_embed"``, ``"pair_layer_norm"``, ``"pair_qkv"``,
    ``"pair_attention"``, ``"pair_o_proj"``, ``"pair_mlp_in"``, ``"pair_mlp_fused"``, ``"pair_mlp_out"``,
    ``"pair_splice"``) and ``"paired_fallback"``: a ``run_paired`` that ``pair_model_ok`` sent back to the two
    forwards before any paired op ran."""
    name = "hip32p"
    fused = False
    supports_pairs = True
    calls: dict = {}

    # -- the parts of the protocol that only the bf16 backend needs
    def begin_forward(self):
        pass

    def fwd_prefetch(self, *Ws):
        return None

    def layer_norm(self, x, w, b, eps, prefetch=None, **kw):
        return super().layer_norm(x, w, b, eps, **kw)

    def qkv(self, x, W_Q, W_K, W_V, b_Q, b_K, b_V):
        q, k, v = super().qkv(x, W_Q, W_K, W_V, b_Q, b_K, b_V)
        q._iit_kv = (k, v)  # for attention_dual, which is handed q alone
        return q, k, v

    def pair_heads_ok(self, S: int, dh: int) -> bool:
        return 1 <= S <= K.ATTN_F32_MAX_S and 1 <= dh <= K.ATTN_F32_MAX_DH

    def pair_model_ok(self, model, tokens) -> bool:
        """Whether ``model`` can run paired on this backend: fp32 on the GPU, S <= 64, d_head <= 64,
        ``d_mlp % 4 == 0``, QKV packed in an arena, the ``-inf`` masked fill.  Counts a refusal as
        ``"paired_fallback"``."""
        cfg = model.cfg
        ok = (cfg.dtype == torch.float32 and model.embed.W_E.is_cuda and model.embed.W_E.dtype == torch.float32
              and tokens.dim() == 2 and self.pair_heads_ok(tokens.shape[1], cfg.d_head)
              and (cfg.attn_only or cfg.d_mlp % 4 == 0) and cfg.d_model % 4 == 0)
        for blk in model.blocks if ok else ():
            a = blk.attn
            ps = (a.W_Q, a.W_K, a.W_V, a.b_Q, a.b_K, a.b_V)
            lns = [ln for ln in (blk.ln1, None if cfg.attn_only else blk.ln2) if ln is not None and ln.w is not None]
            if not (all(p is not None and p.is_cuda and p.dtype == torch.float32 and self.w(p) is p for p in ps)
                    and packed_qkv(*ps) and a.ignore_value() == float("-inf") and a.W_O.is_contiguous()
                    and all(ln.b is not None and self._param(ln.w) and self._param(ln.b) for ln in lns)):
                ok = False
                break
        if not ok:
            self._count("paired_fallback")
        return ok

    # -- paired ops
    def pair_embed_pos(self, tokens, src_tokens, W_E, W_pos):
        B, S = tokens.shape
        self._count("pair_embed")
        base = self.residual(self.embed(tokens, W_E), self.pos_embed(B, S, W_pos))
        with torch.no_grad():
            src = self.residual(self.embed(src_tokens, W_E), self.pos_embed(B, S, W_pos))
            full = torch.cat([base.detach(), src])
        return Paired(base, full)

    def pair_layer_norm_fork(self, p, w, b, eps, prefetch=None):
        self._count("pair_layer_norm")
        y, yf = _one(LayerNormF32PairFn, p.base, w, b, eps, p.full)
        return Paired(y, yf), p

    def pair_qkv(self, p, W_Q, W_K, W_V, b_Q, b_K, b_V):
        self._count("pair_qkv")
        base, full = _one(QKVF32PairFn, p.base, W_Q, W_K, W_V, b_Q, b_K, b_V, p.full)
        return tuple(Paired(b_, f) for b_, f in zip(base, full))

    def _pair_attention(self, qkv, causal, attn_scale, spec):
        q, k, v = qkv
        self._count("pair_attention")
        z, zf = _one(AttentionF32PairFn, q.base, k.base, v.base, causal, 1.0 / attn_scale, spec, q.full, k.full,
                     v.full)
        return Paired(z, zf)

    def pair_attention(self, qkv, causal: bool, attn_scale: float, heads=None):
        """Attention over paired rows; ``heads``: the base rows of these heads take the source rows' z."""
        spec = None
        if heads:
            B2, S, H, dh = qkv[0].full.shape
            spec = _heads_spec(heads, (B2 // 2, S, H, dh))
            if spec is None:
                raise RuntimeError(f"hip32p: the head list {list(heads)} needs more than 8 ranges")
        return self._pair_attention(qkv, causal, attn_scale, spec)

    def pair_attention_spliced(self, qkv, causal: bool, attn_scale: float, index):
        """Attention over paired rows with ``hook_z[index]`` of the base rows taken from the source rows in the
        kernel's store; None when the range table cannot express ``index`` (the caller splices in a pass)."""
        B2, S, H, dh = qkv[0].full.shape
        spec = patch_spec(index, (B2 // 2, S, H, dh))
        if spec is None or [d[0] for d in spec.dims] != [B2 // 2, S, H, dh]:
            return None
        return self._pair_attention(qkv, causal, attn_scale, spec)

    def attention_dual(self, q, causal: bool, attn_scale: float) -> torch.Tensor:
        """No-grad attention of the source rows behind ``q`` (``qkv``'s output), copied into both halves of a
        ``[2B][S][H][dh]`` tensor: the z of a whole-layer ``hook_z`` splice."""
        k, v = q._iit_kv
        z = self.attention(q, k, v, causal, attn_scale)
        return torch.cat([z, z])

    def pair_splice(self, p, index):
        if not p.full.is_contiguous():
            return None
        specs = pair_specs(index, tuple(p.base.shape))
        if specs is None:
            return None
        self._count("pair_splice")
        out, full = _one(PairSpliceFn, p.base, p.full, specs[0], specs[1])
        return Paired(out, full)

    def pair_o_proj_residual(self, z, W_O, b_O, resid):
        H, dh, d = W_O.shape
        self._count("pair_o_proj")
        out, full = _one(LinearF32PairFn, z.base.reshape(*z.base.shape[:-2], H * dh), W_O.view(H * dh, d), b_O,
                         resid.base, z.full.reshape(*z.full.shape[:-2], H * dh), resid.full)
        return Paired(out, full)

    def pair_mlp_in(self, x, W_in, b_in, erf: bool = False, index=None):
        """Paired W_in + gelu_new.  ``index`` (optional): an ``mlp.hook_post`` splice applied inside the op; None
        when the range table cannot express it (the caller then splices in a pass)."""
        spec = None
        if index is not None:
            spec = patch_spec(index, tuple(x.base.shape[:-1]) + (W_in.shape[1],))
            if spec is None:
                return None
        self._count("pair_mlp_in")
        post, pf = _one(MlpInF32PairFn, x.base, W_in, b_in, x.full, spec)
        return None, Paired(post, pf)

    def pair_mlp_out_residual(self, post, W_out, b_out, resid):
        self._count("pair_mlp_out")
        out, full = _one(LinearF32PairFn, post.base, W_out, b_out, resid.base, post.full, resid.full)
        return Paired(out, full)

    def pair_mlp_gelu_residual(self, x, W_in, b_in, W_out, b_out, resid, erf: bool = False):
        self._count("pair_mlp_fused")
        out, full = _one(MlpGeluResidualF32PairFn, x.base, W_in, b_in, W_out, b_out, resid.base, x.full, resid.full)
        return Paired(out, full)


_OPS = {}


def _get(cls, model):
    if model.cfg.dtype != torch.float32:
        raise RuntimeError(f"{cls.name} op backend computes in fp32; the model's dtype is {model.cfg.dtype}")
    K.lib()
    if cls not in _OPS:
        _OPS[cls] = cls()
    return _OPS[cls]


def get_hip32_ops(model) -> HipF32Ops:
    """The backend for an fp32 model on a GPU; raises when the kernel library cannot be loaded (no fallback)."""
    return _get(HipF32Ops, model)


def get_hip32x_ops(model) -> HipF32XOps:
    """``hip32x`` under the same rules as :func:`get_hip32_ops`."""
    return _get(HipF32XOps, model)


def get_hip32n_ops(model) -> HipF32NOps:
    """``hip32n`` under the same rules as :func:`get_hip32_ops`."""
    return _get(HipF32NOps, model)


def get_hip32p_ops(model) -> HipF32POps:
    """``hip32p`` under the same rules as :func:`get_hip32_ops`."""
    return _get(HipF32POps, model)
