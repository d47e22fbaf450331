"""Op backends for the native LL models.

* ``torch`` – :class:`TorchOps`, reference semantics, any device / dtype (oracle).
* ``hip``   – :class:`iit_amd.ops.hip_ops.HipOps`, hand-written gfx950 kernels
  (bf16 activations, fp32 accumulation / residual stream / master weights).
* ``hip32`` – :class:`iit_amd.ops.hip32_ops.HipF32Ops`, ``TorchOps`` in fp32 with the
  projections on the exact-fp32 MFMA GEMM (``csrc/gemm_f32.hip``).  Opt-in only:
  ``backend=None`` never selects it; on a CPU model or without the extension it raises.
* ``hip32x`` – :class:`iit_amd.ops.hip32_ops.HipF32XOps`, ``hip32`` with attention on the
  exact-fp32 MFMA kernel (``csrc/attn_fp32.hip``, S <= 64 and d_head <= 64; the torch op
  otherwise and whenever a score / pattern hook is live).  Opt-in under ``hip32``'s rules.
* ``hip32n`` – :class:`iit_amd.ops.hip32_ops.HipF32NOps`, ``hip32x`` with the rest of a GPT-2-family
  block on the repo's kernels when no hook inside the op is live: LayerNorm (``csrc/block_f32.hip``),
  ``gelu_new`` and its derivative in ``gemm_f32`` epilogues, both residual adds in the projections'
  epilogues.  Opt-in under ``hip32``'s rules.
* ``hip32p`` – :class:`iit_amd.ops.hip32_ops.HipF32POps`, ``hip32n`` with the paired forward: an interchange
  intervention is one forward of 2B rows up to its deepest site (``HookedTransformer.run_paired``), the ``hook_z``
  splice and its gradient mask inside the fp32 attention kernels, an ``mlp.hook_post`` splice as a sparse copy.
  Models it does not cover (QKV outside an arena, S or d_head above 64, ``d_mlp % 4 != 0``) run the two forwards.
  Opt-in under ``hip32``'s rules.

``select_ops(model, backend)`` picks per call: ``backend=None`` means "hip when
the model lives on a GPU and computes in bf16, else torch".  Asking for ``hip``
explicitly on a GPU when the extension is not built raises (no silent fallback).
"""
from __future__ import annotations

from typing import Optional

import torch

from .torch_ops import TorchOps, gelu_new

_TORCH_OPS_CACHE = {}


def _torch_ops(dtype):
    ops = _TORCH_OPS_CACHE.get(dtype)
    if ops is None:
        ops = _TORCH_OPS_CACHE[dtype] = TorchOps(dtype)
    return ops


def hip_supported(cfg) -> bool:
    """Architectures the fused HIP backend implements (GPT-2 family and BERT encoders); others run TorchOps on
    the GPU (bf16 compute, library GEMMs) until their kernels exist (RMSNorm / rotary / SwiGLU / GQA)."""
    return (cfg.positional_embedding_type == "standard" and cfg.normalization_type in ("LN", "LNPre", None)
            and not cfg.gated_mlp and (cfg.n_key_value_heads in (None, cfg.n_heads))
            and not cfg.parallel_attn_mlp and not cfg.final_rms
            and cfg.act_fn in ("gelu_new", "gelu_fast", "gelu_pytorch_tanh", "gelu", "relu"))


def select_ops(model, backend: Optional[str] = None):
    cfg = model.cfg
    dtype = cfg.dtype
    on_gpu = next(model.parameters()).is_cuda
    if backend is None:
        from .. import config as _config
        env = _config.backend()
        backend = "hip" if (on_gpu and dtype == torch.bfloat16 and env == "hip" and hip_supported(cfg)) else "torch"
    if backend == "torch":
        return _torch_ops(dtype)
    if backend == "hip":
        if not on_gpu:
            raise RuntimeError("hip op backend requires the model on a GPU")
        from .hip_ops import get_hip_ops
        return get_hip_ops(model)
    if backend in ("hip32", "hip32x", "hip32n", "hip32p"):  # opt-in only: ``backend=None`` never selects them
        if not on_gpu:
            raise RuntimeError(f"{backend} op backend requires the model on a GPU")
        from .hip32_ops import get_hip32_ops, get_hip32n_ops, get_hip32p_ops, get_hip32x_ops
        return {"hip32": get_hip32_ops, "hip32x": get_hip32x_ops, "hip32n": get_hip32n_ops,
                "hip32p": get_hip32p_ops}[backend](model)
    raise ValueError(f"unknown op backend {backend}")


def cross_entropy(logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """Mean CE with index targets; fused HIP kernel on GPU (fp32 logits, any row stride)."""
    if logits.is_cuda and logits.dim() == 2 and not target.dtype.is_floating_point:
        from .hip_ops import cross_entropy as _hip_ce
        return _hip_ce(logits, target)
    return torch.nn.functional.cross_entropy(logits.float(), target)
