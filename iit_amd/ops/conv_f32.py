"""Opt-in fp32 convolutions on the exact-fp32 implicit-GEMM kernels (``csrc/conv_f32.hip``).

``set_backend("hip32")`` makes :class:`iit_amd.models.resnet.Conv2d` run every convolution :func:`covered` accepts --
fp32, channels-last, square ``1 <= k <= 7``, stride 1 or 2, no bias, dilation or groups -- through
:class:`ConvF32Fn`: forward, input gradient and weight gradient on the kernels, gradients handed to autograd as
``F.conv2d`` hands them (``dW`` a channels-last ``[Cout, Cin, k, k]`` tensor; no direct arena stores).  The default
backend is ``"torch"`` and nothing ever selects ``"hip32"`` automatically.  ``calls`` counts what ran and why a
convolution fell back.
"""
from __future__ import annotations

import functools
from collections import Counter

import torch

from . import hip_kernels as K
from .hip32_ops import _tile as gemm_f32_tile  # the fp32 GEMM's stated tile policy: the convolutions follow it

BACKENDS = ("torch", "hip32")
_backend = "torch"
# fwd / dgrad / wgrad: kernel passes run; dy_copy: output gradients re-laid to dense channels-last first;
# fallback_layout / fallback_geometry / fallback_dtype: convolutions ``covered`` refused, by reason
calls: Counter = Counter()


def backend() -> str:
    return _backend


def set_backend(name: str) -> None:
    """``"torch"`` (the default) or ``"hip32"``; the latter raises when the kernel library is not built."""
    global _backend
    if name not in BACKENDS:
        raise ValueError(f"conv_f32 backend {name!r}: one of {BACKENDS}")
    if name == "hip32" and not (K.available() and hasattr(K.lib(), "iit_conv_f32_fwd")):
        raise RuntimeError("conv_f32 backend 'hip32' needs the built kernel library (iit_amd/_native/libiit_hip.so)")
    _backend = name


def nhwc_dense(t: torch.Tensor) -> bool:
    """Whether the memory of a 4-D ``[N, C, H, W]`` tensor is the dense ``[N][H][W][C]`` array: every dimension longer
    than 1 has exactly the channels-last stride (strides of length-1 dimensions address nothing, so a 1 x 1 kernel's
    weight and a 1 x 1 activation, which are the same memory in both formats, pass whichever way they are labelled)."""
    if t.dim() != 4:
        return False
    n, c, h, w = t.shape
    want = (h * w * c, 1, w * c, c)
    return all(size == 1 or have == exp for size, have, exp in zip(t.shape, t.stride(), want))


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def geometry(conv):
    """``(k, s, pad)`` of a convolution module the kernels' geometry list may hold, else None."""
    k, s, pad, dil = _pair(conv.kernel_size), _pair(conv.stride), conv.padding, _pair(conv.dilation)
    if isinstance(pad, str) or conv.bias is not None or conv.groups != 1 or dil != (1, 1) or \
            conv.padding_mode != "zeros" or getattr(conv, "transposed", False):
        return None
    pad = _pair(pad)
    if k[0] != k[1] or s[0] != s[1] or pad[0] != pad[1]:
        return None
    if not (1 <= k[0] <= 7 and s[0] in (1, 2) and 0 <= pad[0] < k[0]):
        return None
    return k[0], s[0], pad[0]


def _geom(x, w, ksp):
    n, cin, h, wd = x.shape
    return K.conv_f32_geom(n, h, wd, cin, w.shape[0], *ksp)


def covered(x: torch.Tensor, conv) -> bool:
    """Whether ``conv(x)`` runs on the fp32 kernels; a refusal is counted by reason in ``calls``."""
    w = conv.weight
    ksp = geometry(conv)
    if ksp is None or x.dim() != 4 or w.dim() != 4 or x.shape[1] != w.shape[1] or \
            min(x.shape[2], x.shape[3]) + 2 * ksp[2] < ksp[0]:
        calls["fallback_geometry"] += 1
        return False
    # the weight's layout is checked on its own: a 1 x 1 activation is channels-last whatever its weight is
    if not nhwc_dense(x) or not nhwc_dense(w):
        calls["fallback_layout"] += 1
        return False
    if not (x.is_cuda and w.is_cuda and x.dtype == torch.float32 and w.dtype == torch.float32):
        calls["fallback_dtype"] += 1
        return False
    # fp32 tensors are non-null and 4-byte aligned, which is all the library asks of the pointers: what is left of
    # its check is the geometry, asked once per geometry (the launch wrappers repeat the full check)
    if x.numel() == 0 or not _geometry_ok(_geom(x, w, ksp)):
        calls["fallback_geometry"] += 1
        return False
    return True


@functools.lru_cache(maxsize=None)
def _geometry_ok(g) -> bool:
    return K.conv_f32_plan(K.CONV_F32_FWD, g) is not None


@functools.lru_cache(maxsize=None)
def policy(pass_: int, g):
    """(tile, splits) of one pass: ``hip32_ops._tile`` and ``gemm_f32_splits`` on the pass's GEMM extents as the
    library states them -- the stated policies of the fp32 GEMM, not a tuned table.  Cached per (pass, geometry)."""
    pl = K.conv_f32_plan(pass_, g)
    if pl is None:
        raise RuntimeError(f"conv_f32: unsupported geometry {tuple(g)}")
    tile = gemm_f32_tile(pl["M"], pl["N"])
    return tile, K.gemm_f32_splits(pl["M"], pl["N"], pl["K"], tile)


def _empty_nhwc(shape, device):
    return torch.empty(shape, dtype=torch.float32, device=device, memory_format=torch.channels_last)


class ConvF32Fn(torch.autograd.Function):
    """``conv2d(x, W)`` for dense channels-last fp32 ``x [N, Cin, H, W]`` and ``W [Cout, Cin, k, k]``;
    ``geom = (k, s, pad)``.  The input gradient runs only when the input needs one, the weight gradient only when
    ``W`` does."""

    @staticmethod
    def forward(ctx, x, w, geom):
        g = _geom(x, w, geom)
        y = _empty_nhwc((g[0], g[6], g[4], g[5]), x.device)
        K.conv_f32_fwd(x, w, y, g, *policy(K.CONV_F32_FWD, g))
        calls["fwd"] += 1
        ctx.save_for_backward(x, w)
        ctx.g = g
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        g = ctx.g
        if dy.dtype != torch.float32 or not nhwc_dense(dy):
            dy = _empty_nhwc(dy.shape, dy.device).copy_(dy)
            calls["dy_copy"] += 1
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = _empty_nhwc(x.shape, x.device)
            K.conv_f32_dgrad(dy, w, dx, g, *policy(K.CONV_F32_DGRAD, g))
            calls["dgrad"] += 1
        if ctx.needs_input_grad[1]:
            dw = _empty_nhwc(w.shape, w.device)
            K.conv_f32_wgrad(x, dy, dw, g, *policy(K.CONV_F32_WGRAD, g))
            calls["wgrad"] += 1
        return dx, dw, None


def conv(x: torch.Tensor, conv_m) -> torch.Tensor:
    """``conv_m(x)`` on the kernels; the caller has checked :func:`covered`."""
    return ConvF32Fn.apply(x, conv_m.weight, geometry(conv_m))
