"""GEMM dispatch: hand-written MFMA kernel (fused epilogues) vs hipBLASLt, autotuned per shape.

Every GEMM of the engine goes through :func:`gemm`.  Implementations:

* ``hip``  - ``csrc/gemm.hip``: MFMA 16x16x32 bf16 with the epilogue fused
  (bias, packed-QKV bias, fp32 residual add, bias+gelu_new, dgelu, fp32
  accumulate into the gradient arena, head-blocked QKV gradient scatter);
* ``blas`` - hipBLASLt through ``torch.mm`` / ``torch.addmm`` for the product and
  separate elementwise passes for whatever the BLAS epilogue cannot express;
* ``blas16`` - for fp32 residual / accumulate epilogues: bf16-output library GEMM
  + one fused ``add_bf16`` pass.

``IIT_GEMM=auto`` (default) times every candidate once per (shape, layout,
epilogue) -- as a captured graph of back-to-back calls, i.e. device time only --
outside graph capture and keeps the fastest; ``IIT_GEMM=hip|blas|blas16`` force one.  The
decisions are recorded in :data:`DECISIONS` (``report()`` prints them) so profiles
can say which GEMMs ran on hand-written MFMA code.
"""
from __future__ import annotations

import os
import re
from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F

from . import hip_kernels as K

POLICY = os.environ.get("IIT_GEMM", "auto")
DECISIONS: Dict[Tuple, Tuple[str, Dict[str, float]]] = {}
# in-context tuning (scripts/tune_gemm_in_situ.py): per problem key a forced candidate, and a list that receives
# (key, candidate, start event, end event) for every GEMM launched while it is set
FORCE: Dict[Tuple, str] = {}
TIMING = None
BF16, F32 = torch.bfloat16, torch.float32
_BLAS_OK = {}
_BLAS_SELECTED = False


def select_graph_safe_blas() -> None:
    """Optionally route torch's library GEMMs through rocBLAS instead of hipBLASLt (``IIT_BLAS=rocblas``).

    Both replay correctly from captured HIP graphs in our tests (``tests/test_graphs.py``,
    ``scripts/diag_graphs.py``: graph and eager losses agree phase by phase until fp32-atomic
    noise, amplified by Adam, makes any two runs -- eager or not -- drift apart); hipBLASLt is
    ~2 % faster on the IOI step, so it stays the default."""
    global _BLAS_SELECTED
    if _BLAS_SELECTED or not torch.cuda.is_available():
        return
    _BLAS_SELECTED = True
    if os.environ.get("IIT_BLAS", "lt") != "rocblas":
        return
    try:
        torch.backends.cuda.preferred_blas_library("cublas")
    except Exception as e:  # pragma: no cover - older torch
        print(f"[iit] could not select rocBLAS ({e})")


_TUNED_CSV = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuned", "tunableop_gfx950.csv")
_TUNABLE_DONE = False


def enable_tuned_library_gemms() -> bool:
    """Load the shipped TunableOp table (``ops/tuned/tunableop_gfx950.csv``): the fastest hipBLASLt / rocBLAS
    solution per library-GEMM shape of the engine's workloads, found by PyTorch TunableOp's exhaustive search on
    an MI355X (``scripts/gpu_tunableop.sh``).  The table carries validators (PyTorch / HIP / hipBLASLt / rocBLAS
    versions, gfx arch); TunableOp ignores it on any mismatch, and shapes not in it take the library default.
    Tuning itself stays off (it cannot run inside graph capture).  ``IIT_TUNABLEOP=0`` disables."""
    global _TUNABLE_DONE
    if _TUNABLE_DONE:
        return True
    _TUNABLE_DONE = True
    if os.environ.get("IIT_TUNABLEOP", "1") == "0" or not torch.cuda.is_available() or not os.path.exists(_TUNED_CSV):
        return False
    if os.environ.get("PYTORCH_TUNABLEOP_ENABLED") is not None:  # the user drives TunableOp themselves
        return False
    try:
        import tempfile
        from torch.cuda import tunable
        tunable.enable(True)
        tunable.tuning_enable(False)
        tunable.set_filename(os.path.join(tempfile.gettempdir(), "iit_tunableop_results%d.csv"))
        return bool(tunable.read_file(_TUNED_CSV))
    except Exception as e:  # pragma: no cover - older torch
        print(f"[iit] TunableOp table not loaded ({e})")
        return False


def deterministic() -> bool:
    """Run-to-run reproducible GEMMs: ``IIT_DETERMINISTIC=1`` or ``torch.use_deterministic_algorithms(True)``.

    The split-K candidates (fp32 atomics into the output: the weight-gradient accumulate tiles) sum their partial
    products in arrival order, so two runs can differ in the last bits.  In deterministic mode the
    dispatcher drops them and every candidate has a fixed reduction order.  The reduction split-K candidates
    (``glds*r*``: partial tiles summed in split order by the last-arriving workgroup) are deterministic and stay."""
    return os.environ.get("IIT_DETERMINISTIC", "0") == "1" or torch.are_deterministic_algorithms_enabled()


def _as(t, rows, cols, ld, dtype=None):
    v = torch.as_strided(t, (rows, cols), (ld, 1))
    return v if dtype is None or v.dtype == dtype else v.to(dtype)


def _operands(A, B, M, N, Kd, lda, ldb, mode):
    if mode & K.MODE_AKM:
        a = _as(A, Kd, M, lda).t()
    else:
        a = _as(A, M, Kd, lda)
    if mode & K.MODE_BKM:
        b = _as(B, Kd, N, ldb)
    else:
        b = _as(B, N, Kd, ldb).t()
    if a.dtype != BF16:
        a = a.to(BF16)
    if b.dtype != BF16:
        b = b.to(BF16)
    return a, b


def _mm_f32(a, b):
    # (the capability flags are per device type: a CPU call that lacks ``out_dtype`` must not send the GPU's fp32
    # GEMMs to the fallback below, which rounds the product to bf16 -- tests/test_gemm_exact.py found exactly that)
    if _BLAS_OK.get(("out_dtype", a.device.type), True):
        try:
            return torch.mm(a, b, out_dtype=F32)
        except (RuntimeError, TypeError):
            _BLAS_OK[("out_dtype", a.device.type)] = False
    return torch.mm(a, b).float()


def _mm_f32_into(c, a, b) -> None:
    """c = a @ b (bf16 operands, fp32 output written straight into ``c``: beta = 0, no read of ``c``)."""
    if _BLAS_OK.get(("mm_out_dtype", a.device.type), True) and c.is_contiguous():
        try:
            torch.mm(a, b, out_dtype=F32, out=c)
            return
        except (RuntimeError, TypeError):
            _BLAS_OK[("mm_out_dtype", a.device.type)] = False
    c.copy_(_mm_f32(a, b))


def _addmm_f32(c, base, a, b) -> None:
    """c = base + a @ b with bf16 operands, fp32 accumulate/output, in one hipBLASLt call when supported
    (``base`` may alias ``c``: the accumulate-into-gradient case)."""
    if _BLAS_OK.get(("addmm_dtype", a.device.type), True):
        try:
            torch.addmm(base, a, b, out_dtype=F32, out=c)
            return
        except (RuntimeError, TypeError):
            _BLAS_OK[("addmm_dtype", a.device.type)] = False
    if base is c:
        c.add_(_mm_f32(a, b))
    else:
        torch.add(base, _mm_f32(a, b), out=c)


def wgrad_into(c, x2, g2, store: bool, params=(), bsum=None) -> None:
    """Weight gradient ``c (+)= x2^T @ g2`` (x2 [T, K_in], g2 [T, N] bf16; c [K_in, N] fp32, unit column stride):
    ``store`` writes it (beta = 0, a lazily-zeroed slot), else accumulates.  On the GPU the dispatcher measures the
    LDS-DMA kernel's fp32-store / -accumulate epilogues (and its deterministic reduction split) against hipBLASLt
    per shape -- on the Llama-3-8B weight gradients the repo's kernel wins (profiles/llama3_8b_gemm_study_r3.txt).
    ``params``: the arena parameters whose complete gradient a store writes -- the GEMM then also adds its sum of
    squares into the arena's fused-norm slots (``FlatParams.norm_cover``), so the optimizer's clip does not read
    these gradients again (the torch op backend's share of the fused norm; the HIP backend does the same).
    ``bsum`` (fp32 [N], optional): += the column sums of ``g2`` -- the bias gradient of the layer -- from the B
    fragments the LDS-DMA kernel already holds (a column-sum pass after a library GEMM)."""
    T, Kin = x2.shape
    N = g2.shape[1]
    ok = (c.is_cuda and x2.dtype == BF16 and g2.dtype == BF16 and c.dtype == F32 and x2.stride(1) == 1
          and g2.stride(1) == 1 and c.stride(-1) == 1 and c.dim() == 2 and POLICY in ("auto", "glds"))
    if ok:
        gsq = None
        flat = getattr(params[0], "_iit_flat", None) if params else None
        if flat is not None:
            flat.norm_intent(*params)
            gsq = flat.norm_cover(*params) if store else None
        gemm(x2, g2, c, M=Kin, N=N, K=T, lda=x2.stride(0), ldb=g2.stride(0), ldc=c.stride(0),
             mode=K.MODE_AKM | K.MODE_BKM, epi=K.EPI_F32_STORE if store else K.EPI_F32_ACC, fresh=store, gsq=gsq,
             bsum=bsum)
        return
    if store:
        _mm_f32_into(c, x2.t(), g2)
    else:
        _addmm_f32(c, c, x2.t(), g2)
    if bsum is not None:
        bsum.add_(g2.float().sum(0))


def _gelu_into(pre, out, erf: bool = False) -> None:
    if pre.is_cuda and pre.dtype == BF16 and out.dtype == BF16 and pre.dim() == 2:
        K.gelu_fwd(pre, out, pre.shape[0], pre.shape[1], erf=erf)
    else:
        torch._C._nn.gelu(pre, approximate="none" if erf else "tanh", out=out)


def _blas(A, B, C, M, N, Kd, lda, ldb, ldc, mode, epi, C2, C3, bias0, bias1, bias2, resid, ldr, aux, ldc2, bias_cols,
          qkv, blas_bias=None):
    a, b = _operands(A, B, M, N, Kd, lda, ldb, mode)
    if epi in (K.EPI_BF16, K.EPI_BF16_BIAS3):
        c = _as(C, M, N, ldc)
        if blas_bias is not None:
            bias = blas_bias
        elif epi == K.EPI_BF16_BIAS3:
            bias = torch.cat([bias0.reshape(-1)[:N], bias1.reshape(-1), bias2.reshape(-1)]).to(BF16)
        else:
            bias = None if bias0 is None else bias0.reshape(-1)[:N].to(BF16)
        if bias is None:
            torch.mm(a, b, out=c)
        else:
            torch.addmm(bias, a, b, out=c)
    elif epi == K.EPI_F32_RESID:
        c = _as(C, M, N, ldc)
        _addmm_f32(c, _as(resid, M, N, ldr), a, b)
        if bias0 is not None:
            c.add_(bias0.reshape(-1)[:N])
    elif epi in (K.EPI_GELU, K.EPI_GELU_ERF):
        # (C2 None: an inference forward that keeps no pre-activation -- a scratch for the library path)
        pre = _as(C2, M, N, ldc2) if C2 is not None else torch.empty(M, N, dtype=BF16, device=A.device)
        torch.addmm(bias0.reshape(-1)[:N].to(BF16), a, b, out=pre)
        _gelu_into(pre, _as(C, M, N, ldc), erf=epi == K.EPI_GELU_ERF)
    elif epi in (K.EPI_DGELU, K.EPI_DGELU_ERF):
        tmp = torch.mm(a, b)
        K.dgelu(tmp, _as(aux, M, N, ldc2).contiguous(), _as(C, M, N, ldc), erf=epi == K.EPI_DGELU_ERF)
    elif epi == K.EPI_F32_ACC:
        c = _as(C, M, N, ldc)
        _addmm_f32(c, c, a, b)
    elif epi == K.EPI_F32_STORE:
        c = _as(C, M, N, ldc)
        if bias0 is not None:
            _addmm_f32(c, bias0.reshape(-1)[:N].float(), a, b)
        else:
            _mm_f32_into(c, a, b)
    else:
        raise NotImplementedError(epi)


def _blas_supported(epi, C) -> bool:
    if epi == K.EPI_F32_ACC_QKV:
        return False
    if epi in (K.EPI_DGELU, K.EPI_DGELU_ERF):
        return True
    return True


def _scratch(t, rows, ld):
    """Dense stand-in output for timing (``t`` may be a strided view into a larger buffer)."""
    if t is None:
        return None
    return torch.zeros(rows * ld, dtype=t.dtype, device=t.device)


def _time(fn, reps: int = 10) -> float:
    """GPU time per call in microseconds.

    Candidates are timed as a captured graph of ``reps`` back-to-back calls, so the
    number reflects device time only (training steps run as graph replays, where
    host launch overhead is gone); if capture fails the eager loop is timed."""
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    try:
        from ..engine.graphs import _CaptureGC
        g = torch.cuda.CUDAGraph()
        with _CaptureGC(collect=False), torch.cuda.graph(g, capture_error_mode="thread_local"):
            for _ in range(reps):
                fn()
        g.replay()
        s.record()
        g.replay()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / reps * 1e3
    except Exception:
        torch.cuda.synchronize()
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / reps * 1e3


def _blas16(A, B, C, M, N, Kd, lda, ldb, ldc, mode, epi, bias0, resid, ldr):
    """fp32-output epilogues as a bf16-output library GEMM + one fused ``add_bf16`` pass
    (hipBLASLt's bf16-in/fp32-out kernels are markedly slower than its bf16-out ones on gfx950)."""
    a, b = _operands(A, B, M, N, Kd, lda, ldb, mode)
    y = torch.mm(a, b)
    bias = None if bias0 is None else bias0.reshape(-1)[:N].float().contiguous()
    if epi == K.EPI_F32_RESID:
        K.add_bf16(C, ldc, resid, ldr, y, N, bias, M, N)
    else:  # EPI_F32_ACC: C += y
        K.add_bf16(C, ldc, C, ldc, y, N, None, M, N)


_BLAS16_EPIS = (K.EPI_F32_RESID, K.EPI_F32_ACC)


# diagnostics: ``IIT_GEMM_EXCLUDE`` = comma-separated regular expressions of candidate names the dispatcher must not
# offer (shipped decisions naming one are re-measured among the rest); "hip" always stays.  A pattern with "@" is
# matched against ``name@repr(problem key)`` (one call site only).  ``IIT_GEMM_TRACE=1`` prints each problem key's
# choice once.
_EXCLUDE = [re.compile(x) for x in os.environ.get("IIT_GEMM_EXCLUDE", "").split(";" if ";" in
                                                                                 os.environ.get("IIT_GEMM_EXCLUDE", "")
                                                                                 else ",") if x]
_TRACE = os.environ.get("IIT_GEMM_TRACE", "0") == "1"
_TAIL_LIBRARY = os.environ.get("IIT_GEMM_TAIL_LIBRARY", "0") == "1"
_TRACED = set()


def _excluded(name: str, key=None) -> bool:
    if name == "hip":
        return False
    tagged = f"{name}@{key!r}"
    return any(r.fullmatch(tagged) if "@" in r.pattern else r.fullmatch(name) for r in _EXCLUDE)


def _candidates(A, B, C, C2, M, N, Kd, lda, ldb, ldc, mode, epi, bias0, bias1, bias2, resid, ldr, aux, ldc2,
                bias_cols, qkv, splits, blas_bias, policy, csum_box=None):
    """name -> f(c, c2, c3) for every implementation that covers the problem.

    ``csum_box`` ([fp32 tensor] or None): every candidate also adds the column sums of its (bf16) output into
    ``csum_box[0]`` -- fused in the LDS-DMA kernel's DGELU epilogue, a column-sum pass after the others."""
    calls = _candidates_plain(A, B, C, C2, M, N, Kd, lda, ldb, ldc, mode, epi, bias0, bias1, bias2, resid, ldr, aux,
                              ldc2, bias_cols, qkv, splits, blas_bias, policy, csum_box)
    if _EXCLUDE:
        calls = {n: f for n, f in calls.items() if not _excluded(n)}
    if csum_box is not None:
        for name in list(calls):
            if not name.startswith("glds"):
                calls[name] = lambda c=C, c2=C2, c3=None, f=calls[name]: (  # noqa: E731
                    f(c, c2, c3), K_.colsum_accum(c, ldc, csum_box[0], M, N))
    return calls


def _candidates_plain(A, B, C, C2, M, N, Kd, lda, ldb, ldc, mode, epi, bias0, bias1, bias2, resid, ldr, aux, ldc2,
                      bias_cols, qkv, splits, blas_bias, policy, csum_box):
    det = deterministic()
    if det:
        splits = 1
    hip_call = lambda c=C, c2=C2, c3=None: K_.gemm(  # noqa: E731
        A, B, c, M=M, N=N, K=Kd, lda=lda, ldb=ldb, ldc=ldc, mode=mode, epi=epi, C2=c2, C3=c3, bias0=bias0,
        bias1=bias1, bias2=bias2, resid=resid, ldr=ldr, aux=aux, ldc2=ldc2, bias_cols=bias_cols, qkv=qkv,
        splits=splits)
    calls = {"hip": hip_call}
    if not _blas_supported(epi, C):
        return calls
    calls["blas"] = lambda c=C, c2=C2, c3=None: _blas(A, B, c, M, N, Kd, lda, ldb, ldc, mode, epi, c2, c3,  # noqa
                                                     bias0, bias1, bias2, resid, ldr, aux, ldc2, bias_cols, qkv,
                                                     blas_bias)
    if policy in ("auto", "glds") and A.is_cuda:
        split_opts = (1,)
        if epi == K_.EPI_F32_ACC and (M // 64) * (N // 64) < 1024 and not det:
            split_opts = (1, 2, 4, 8, 16) if (M // 64) * (N // 64) < 64 else (1, 2, 4)
        dg = epi in (K_.EPI_DGELU, K_.EPI_DGELU_ERF)  # the LDS-DMA kernel reads pre through its C2 operand
        for tile in K_.GLDS_DISPATCH_TILES:
            for sp in split_opts:
                if K_.gemm_glds_ok(A, B, C, M=M, N=N, K=Kd, lda=lda, ldb=ldb, ldc=ldc, mode=mode, epi=epi,
                                   C2=aux if dg else C2, resid=resid, ldc2=ldc2, ldr=ldr, bias_cols=bias_cols,
                                   tile=tile, splits=sp):
                    calls[f"glds{tile}" + (f"k{sp}" if sp > 1 else "")] = \
                        lambda c=C, c2=C2, c3=None, t=tile, sp=sp, bs=None, sq=None: K_.gemm_glds(  # noqa: E731
                            A, B, c, M=M, N=N, K=Kd, lda=lda, ldb=ldb, ldc=ldc, mode=mode, epi=epi,
                            C2=aux if dg else c2, bias0=bias0, bias1=bias1, bias2=bias2, resid=resid, ldc2=ldc2,
                            ldr=ldr, bias_cols=bias_cols, tile=t, splits=sp,
                            csum=csum_box[0] if csum_box is not None else None, bsum=bs, gsq=sq)
            # the weight gradients (X^T dY, reduction over the tokens) also get the deterministic reduction split:
            # larger tiles per CU (fewer operand bytes per flop) without fp32 atomics; they only run in backward
            # passes, which are serial on one stream
            # ... and so do the long-K fp32 residual GEMMs (W_out's forward, K = d_mlp: [T][768] outputs are too few
            # big tiles for 256 CUs; the last-arriving split adds bias + residual once)
            if (mode == 3 and epi in (K_.EPI_F32_ACC, K_.EPI_F32_STORE)) or \
                    (mode == 2 and epi == K_.EPI_F32_RESID and Kd >= 2048 and bias_cols == 0):
                for sp in (2, 4):
                    if Kd // sp < 256 or not K_.gemm_glds_ok(A, B, C, M=M, N=N, K=Kd, lda=lda, ldb=ldb, ldc=ldc,
                                                             mode=mode, epi=epi, resid=resid, ldr=ldr, tile=tile,
                                                             splits=sp, reduce=True):
                        continue
                    calls[f"glds{tile}r{sp}"] = lambda c=C, c2=C2, c3=None, t=tile, sp=sp, bs=None, sq=None: \
                        K_.gemm_glds(A, B, c, M=M, N=N, K=Kd, lda=lda, ldb=ldb, ldc=ldc, mode=mode, epi=epi,  # noqa
                                     bias0=bias0, resid=resid, ldr=ldr, tile=t, splits=sp, reduce=True, bsum=bs,
                                     gsq=sq)
        # a ragged N (the vocabulary-sized unembed forward and weight gradient) whole, in ONE launch on the
        # edge-capable tiles (csrc/gemm_edge.hip) -- a candidate beside the bulk + tail split of _ragged_split
        if N % 128 and mode in (2, 3) and C2 is None and resid is None and aux is None and bias1 is None \
                and csum_box is None:
            for tile in K_.GLDS_EDGE_TILES:
                if K_.gemm_glds_edge_ok(A, B, C, M=M, N=N, K=Kd, lda=lda, ldb=ldb, ldc=ldc, mode=mode, epi=epi,
                                        bias0=bias0, tile=tile):
                    calls[f"glds{tile}e"] = lambda c=C, c2=C2, c3=None, t=tile, bs=None, sq=None: \
                        K_.gemm_glds_edge(A, B, c, M=M, N=N, K=Kd, lda=lda, ldb=ldb, ldc=ldc, mode=mode, epi=epi,  # noqa
                                          bias0=bias0, tile=t, bsum=bs, gsq=sq)
    if epi in _BLAS16_EPIS:
        calls["blas16"] = lambda c=C, c2=C2, c3=None: _blas16(A, B, c, M, N, Kd, lda, ldb, ldc, mode, epi,  # noqa
                                                             bias0, resid, ldr)
    # (an "init C with bias / residual, then split-K atomics" candidate for the few-tile fp32 stores -- the
    # last-position final block, ragged vocab tails -- made the gradients of the paired, last-position forward vary
    # from run to run by up to 0.1 (scripts/diag_uninit_poison.py --keys: excluding it at the one problem key that
    # chose it, (32, 128, 512) residual, made every configuration bit-stable) at no measurable gain (16,022 vs 16,019
    # pairs/s without it, profiles/split_store_removal_r4.txt): removed from the offered candidates.  VERDICT r4 #3:
    # it is reinstated behind the test-only switch ``IIT_GEMM_SPLIT_STORE`` for the root-cause experiment
    # (profiles/split_store_rootcause_r5.txt): "1" the removed candidate as it was, "nosplit" the same init followed by
    # ONE non-split accumulate launch, "sync" a device synchronisation between the init and the split-K launch.)
    # "atomic1": the init + ONE launch whose epilogue still adds with fp32 atomics (one adder per element);
    # ``IIT_GEMM_SPLIT_STORE_KEY=M,N,K`` restricts the switch to one problem shape.
    mode_ss = _SPLIT_STORE
    if _SPLIT_STORE_KEY and (M, N, Kd) != _SPLIT_STORE_KEY:
        mode_ss = ""
    if (mode_ss and not det and epi in (K_.EPI_F32_STORE, K_.EPI_F32_RESID) and A.is_cuda and mode in (0, 2, 3)
            and Kd >= 256 and Kd % 64 == 0 and ((M + 63) // 64) * ((N + 63) // 64) < 64):
        sp = 1 if mode_ss in ("nosplit", "atomic1") else min(16, Kd // 64)

        def split_store(c=C, c2=C2, c3=None):
            cv = _as(c, M, N, ldc)
            b = None if bias0 is None else bias0.reshape(-1)[:N].float()
            if epi == K_.EPI_F32_RESID:
                r = _as(resid, M, N, ldr)
                if b is None:
                    cv.copy_(r)
                else:
                    torch.add(r, b, out=cv)
            elif b is not None:
                cv.copy_(b.expand(M, N))
            else:
                cv.zero_()
            if mode_ss == "sync" and not torch.cuda.is_current_stream_capturing():
                torch.cuda.synchronize()
            K_.gemm(A, B, c, M=M, N=N, K=Kd, lda=lda, ldb=ldb, ldc=ldc, mode=mode, epi=K_.EPI_F32_ACC, splits=sp,
                    atomic=mode_ss == "atomic1")

        calls["s+hip"] = split_store
    return calls


_SPLIT_STORE = os.environ.get("IIT_GEMM_SPLIT_STORE", "")  # test-only (see _candidates_plain)
# ``IIT_GEMM_FREEZE=1``: no in-process timing at all -- every problem key must be in the shipped decision table (or
# already decided / synchronised), else the GEMM raises: run-to-run and rank-to-rank identical kernel choice
_FREEZE = os.environ.get("IIT_GEMM_FREEZE", "0") == "1"


def _frozen_miss(key) -> None:
    if _FREEZE:
        raise RuntimeError(f"IIT_GEMM_FREEZE=1: GEMM problem {key!r} is not in the decision table "
                           f"({os.environ.get('IIT_GEMM_TABLE', _TABLE_PATH)}); export one with IIT_GEMM_TABLE_EXPORT")
_SPLIT_STORE_KEY = tuple(int(x) for x in os.environ.get("IIT_GEMM_SPLIT_STORE_KEY", "").split(",") if x) or None


def _shift(t, off: int):
    """1-D view of ``t``'s storage starting ``off`` elements after ``t``'s first element (operand sub-blocks for
    the raw-pointer kernels; the library path re-strides it with ``_as``)."""
    if t is None:
        return None
    n = t.untyped_storage().nbytes() // t.element_size() - t.storage_offset() - off
    return torch.as_strided(t, (n,), (1,), t.storage_offset() + off)


RAGGED = {}  # ragged problem key -> (split wins, whole time, [bulk time, tail time])


EDGE: Dict[Tuple, str] = {}  # ragged problem key -> "glds{tile}e" ("" = none): the shipped whole-problem edge choice


def _edge_whole(rkey) -> Optional[str]:
    """The shipped choice ``glds{tile}e`` for a ragged problem that the table otherwise splits ("edge" section of the
    decision table: measured faster than bulk + tail, profiles/loss_tail_ab.txt), or None."""
    name = EDGE.get(rkey)
    if name is None:
        name = EDGE[rkey] = _edge_table().get(repr(rkey), "")
    if not name or re.fullmatch(r"glds\d+e", name) is None or _excluded(name, rkey):
        return None
    return name


def _ragged_split(A, B, C, *, M, N, K, lda, ldb, mode, epi, C2, bias0, resid, aux, bsum=None, gsq=None):
    """Problem pieces ``[kwargs, ...]`` for a GEMM whose N (any column-wise epilogue) or K (fp32 accumulate) is
    large but not tile-aligned: a bulk of N // 128 * 128 columns (resp. K // 1024 * 1024 reduction steps, so
    split-K factors up to 16 divide it) plus the remainder.  None when the problem is aligned or small."""
    if epi in (K_.EPI_BF16, K_.EPI_F32_STORE, K_.EPI_F32_ACC) and N >= 4096 and N % 128:
        n0 = N // 128 * 128
        boff = n0 if mode & K_.MODE_BKM else n0 * ldb
        return [dict(A=A, B=B, C=C, M=M, N=n0, K=K, C2=C2, bias0=bias0, resid=resid, aux=aux, bsum=bsum, gsq=gsq),
                dict(A=A, B=_shift(B, boff), C=_shift(C, n0), M=M, N=N - n0, K=K, C2=_shift(C2, n0),
                     bias0=_shift(bias0, n0), resid=_shift(resid, n0), aux=_shift(aux, n0), bsum=_shift(bsum, n0),
                     gsq=gsq)]
    if epi == K_.EPI_F32_ACC and K >= 16384 and K % 1024:
        k0 = K // 1024 * 1024
        aoff = k0 * lda if mode & K_.MODE_AKM else k0
        boff = k0 * ldb if mode & K_.MODE_BKM else k0
        return [dict(A=A, B=B, C=C, M=M, N=N, K=k0, C2=C2, bias0=bias0, resid=resid, aux=aux, bsum=bsum, gsq=gsq),
                dict(A=_shift(A, aoff), B=_shift(B, boff), C=C, M=M, N=N, K=K - k0, C2=C2, bias0=None,
                     resid=resid, aux=aux, bsum=bsum, gsq=gsq)]
    return None


def gemm(A, B, C, *, M, N, K: int, lda, ldb, ldc, mode=0, epi=0, C2=None, C3=None, bias0=None, bias1=None,
         bias2=None, resid=None, ldr=0, aux=None, ldc2=0, bias_cols=0, qkv=(0, 0, 0), splits=None, blas_bias=None,
         fresh: bool = False, colsum=None, bsum=None, gsq=None, _decide_only: bool = False,
         _no_split: bool = False, _tail: bool = False):
    """``C = A @ B`` (+ epilogue) on the fastest measured implementation for this problem:

    * ``hip``    -- the hand-written MFMA kernel with the epilogue fused;
    * ``glds*``  -- the LDS-DMA MFMA kernel, per tile (and split-K for accumulate epilogues);
    * ``blas``   -- hipBLASLt (``torch.mm`` / ``addmm``; fp32-output variants for fp32 epilogues);
    * ``blas16`` -- (fp32 residual / accumulate epilogues) hipBLASLt bf16 output + the fused
      :func:`iit_amd.ops.hip_kernels.add_bf16` pass.

    ``fresh`` (with ``EPI_F32_STORE``): ``C`` holds garbage (a lazily zeroed gradient slot), so besides
    storing, "zero ``C`` then accumulate" is also correct -- the split-K accumulate tiles compete too
    (``z+`` candidates, the memset included in their time).
    ``blas_bias``: optional ready-made bf16 bias row (e.g. a view of the arena's bf16 mirror) for the
    library path, saving its per-call concatenate/cast.
    ``colsum`` (``EPI_DGELU`` only): fp32 [N] that also receives the column sums of the bf16 output (the MLP
    input-bias gradient), fused into the LDS-DMA kernel's epilogue or as a pass after the other candidates.

    ``bsum`` (weight gradients, mode 3: ``B`` is dY [K][N]): fp32 [N] that also receives ``colsum(B)`` -- the bias
    gradient of the layer -- fused into the LDS-DMA kernel's main loop (the B fragments already in registers are
    summed on the VALU), or as a column-sum pass after any other implementation.  It does not enter the decision.
    ``gsq`` (``EPI_F32_STORE``: a weight gradient stored complete): fp32 [64] slots that also receive the sum of squares
    of the stored gradient (its share of the clip's global norm, ``FlatParams.norm_cover``) -- in the LDS-DMA kernel's
    epilogue, or as a pass over ``C`` after any other implementation; not part of the decision either.

    Ragged problems (the vocabulary-sized unembed GEMMs: N or K = 50257) are split into a tile-aligned bulk, which
    the LDS-DMA kernel can serve, and a narrow tail (see :func:`_ragged_split`) -- or, for a ragged N with a k-major
    B, run whole on the ragged-N variant of that kernel (``glds{tile}e``, csrc/gemm_edge.hip): a candidate of the
    whole problem when the choice is measured, the table's "edge" section when it is shipped.

    Returns the name of the implementation that ran when the choice was measured (else None)."""
    Kd = K
    if not _BLAS_SELECTED:
        select_graph_safe_blas()
        enable_tuned_library_gemms()
    policy = POLICY
    if policy in ("auto", "glds") and A.is_cuda and qkv[0] == 0 and colsum is None and not _no_split:
        parts = _ragged_split(A, B, C, M=M, N=N, K=K, lda=lda, ldb=ldb, mode=mode, epi=epi, C2=C2, bias0=bias0,
                              resid=resid, aux=aux, bsum=bsum, gsq=gsq)
        if parts is not None:
            bulk, tail = parts

            def run(kw, decide=False, tail=False):
                kw = dict(kw)
                return gemm(kw.pop("A"), kw.pop("B"), kw.pop("C"), lda=lda, ldb=ldb, ldc=ldc, mode=mode, epi=epi,
                            ldr=ldr, ldc2=ldc2, blas_bias=None, fresh=fresh, _decide_only=decide, _tail=tail, **kw)

            rkey = (M, N, K, mode, epi, bias0 is not None, fresh, deterministic())
            split = RAGGED.get(rkey)
            if split is None:  # the shipped split-or-whole choice (then bulk and tail take their own table entries)
                shipped = _ragged_table().get(repr(rkey))
                if shipped is not None:
                    split = RAGGED[rkey] = (bool(shipped), float("nan"), [])
            if split is None and _FREEZE:  # no timing: the tile-aligned bulk + tail (both keys must be in the table)
                split = RAGGED[rkey] = (True, float("nan"), [])
            if split is None and not torch.cuda.is_current_stream_capturing():
                # the split is one more candidate: bulk + tail against the whole problem, each at its best
                whole = gemm(A, B, C, M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc, mode=mode, epi=epi, C2=C2, C3=C3,
                             bias0=bias0, bias1=bias1, bias2=bias2, resid=resid, ldr=ldr, aux=aux, ldc2=ldc2,
                             bias_cols=bias_cols, qkv=qkv, splits=splits, blas_bias=blas_bias, fresh=fresh,
                             bsum=bsum, gsq=gsq, _decide_only=True, _no_split=True)
                pieces = [run(bulk, True), run(tail, True, True)]
                split = RAGGED[rkey] = (None not in pieces and whole is not None and sum(pieces) < whole,
                                        whole, pieces)
            if split is not None and split[0]:
                # bulk + tail, or -- where the table's "edge" section names an edge-capable tile for this problem -- the
                # whole ragged problem in ONE launch of the ragged-N kernel (csrc/gemm_edge.hip).  The split stays the
                # fallback (no entry, an operand the variant does not cover) and the IIT_GEMM_TAIL_LIBRARY path.
                edge = None if _TAIL_LIBRARY else _edge_whole(rkey)
                if edge is not None and C2 is None and resid is None and aux is None and bias1 is None:
                    tile = int(edge[4:-1])
                    ekw = dict(M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc, mode=mode, epi=epi, bias0=bias0, tile=tile)
                    if K_.gemm_glds_edge_ok(A, B, C, **ekw):
                        K_.gemm_glds_edge(A, B, C, bsum=bsum, gsq=gsq, **ekw)
                        return edge
                choice = run(bulk)
                run(tail, tail=True)
                return choice
    fresh = fresh and epi == K_.EPI_F32_STORE and bias0 is None
    assert colsum is None or epi in (K_.EPI_DGELU, K_.EPI_DGELU_ERF), "fused column sums need a DGELU epilogue"
    box = [colsum] if colsum is not None else None
    args = (A, B, C, C2, M, N, Kd, lda, ldb, ldc, mode, epi, bias0, bias1, bias2, resid, ldr, aux, ldc2, bias_cols,
            qkv, splits, blas_bias, policy)
    calls = _candidates(*args, csum_box=box)
    if _tail and not _TAIL_LIBRARY:
        # the narrow remainder of a ragged split (81 vocabulary columns / reduction steps) stays on the repo's kernels:
        # hipBLASLt wins it by ~1-2 us in isolation, the headline step is the same within +-0.2 % either way
        # (profiles/unembed_tail_r4s2.txt), and the step then holds no library GEMM at all;
        # IIT_GEMM_TAIL_LIBRARY=1 restores the library candidates
        calls = {n: f for n, f in calls.items() if not n.startswith("blas")}
    hip_call = calls["hip"]
    if _decide_only and (policy != "auto" or (len(calls) == 1 and not _tail)):
        return None  # nothing to measure: a forced policy or a single candidate (a tail's time is still needed)
    if bsum is not None or gsq is not None:
        assert bsum is None or mode == 3, "fused bias sums are the column sums of a weight gradient's dY"
        assert gsq is None or epi == K_.EPI_F32_STORE, "fused norm sums are of a stored gradient"
        # every path below ends in _run: the sums fused in the LDS-DMA kernel, else passes after the GEMM
        def _run(name):
            if name.startswith("glds"):
                calls[name](C, C2, C3, bs=bsum, sq=gsq)
            else:
                calls[name](C, C2, C3)
                if bsum is not None:
                    K_.colsum_accum(B, ldb, bsum, Kd, N)
                if gsq is not None:
                    K_.sumsq_2d(C, ldc, M, N, gsq)
            return name
    else:
        def _run(name):
            calls[name](C, C2, C3)
            return name
    if policy == "hip" or (len(calls) == 1 and not _decide_only):
        _run("hip")
        return None
    if fresh:
        acc = _candidates(A, B, C, C2, M, N, Kd, lda, ldb, ldc, mode, K_.EPI_F32_ACC, None, None, None, resid, ldr,
                          aux, ldc2, bias_cols, qkv, None, blas_bias, policy)
        for name, f in acc.items():
            if _tail and not _TAIL_LIBRARY and name.startswith("blas"):
                continue
            calls["z+" + name] = lambda c=C, c2=C2, c3=None, f=f: (_as(c, M, N, ldc).zero_(), f(c, c2, c3))
    if policy == "glds":
        glds = [k for k in calls if k.startswith("glds")]
        _run(glds[0] if glds else "hip")
        return None
    if policy in calls:
        _run(policy)
        return None
    # the last key field marks the variant: a fresh store (EPI_F32_STORE) or fused column sums (EPI_DGELU)
    key = (M, N, Kd, mode, epi, bias0 is not None, fresh or (colsum is not None), deterministic())
    if _EXCLUDE:
        calls = {n: f for n, f in calls.items() if not _excluded(n, key)}
    choice = DECISIONS.get(key)
    if choice is None:
        shipped = None if _decide_only else _table().get(repr(key))  # ragged bulk/tail splits compare real times
        if shipped in calls:
            choice = DECISIONS[key] = (shipped, {shipped: float("nan")})
    if choice is None:
        if torch.cuda.is_current_stream_capturing():
            if _decide_only:
                return None
            _run("hip")
            return None
        _frozen_miss(key)
        # time on scratch outputs so accumulate epilogues (and column sums) do not corrupt C
        sc = _scratch(C, M, max(ldc, N))
        sc2 = _scratch(C2, M, max(ldc2, N))
        sc3 = _scratch(C3, M, max(ldc, N))
        if box is not None:
            box[0] = torch.zeros_like(colsum)
        timed = calls
        if bsum is not None or gsq is not None:  # candidates timed with their fused sums or passes, into scratch
            sc_bs = torch.zeros_like(bsum) if bsum is not None else None
            sc_sq = torch.zeros_like(gsq) if gsq is not None else None

            def _passes(c):
                if sc_bs is not None:
                    K_.colsum_accum(B, ldb, sc_bs, Kd, N)
                if sc_sq is not None:
                    K_.sumsq_2d(c, ldc, M, N, sc_sq)

            timed = {name: (lambda c, c2, c3, f=f: f(c, c2, c3, bs=sc_bs, sq=sc_sq)) if name.startswith("glds") else
                     (lambda c, c2, c3, f=f: (f(c, c2, c3), _passes(c)))
                     for name, f in calls.items()}
        try:
            times = {name: min(_time(lambda f=f: f(sc, sc2, sc3)) for _ in range(2)) for name, f in timed.items()}
            # the closest contenders are re-timed with more repetitions: near-ties (a few %) between tiles are
            # otherwise decided by timing noise
            for name in sorted(times, key=times.get)[:3] if len(times) > 1 else ():
                f = timed[name]
                times[name] = min(_time(lambda f=f: f(sc, sc2, sc3), reps=30) for _ in range(3))
        finally:
            if box is not None:
                box[0] = colsum
        best = min(times, key=times.get)
        choice = DECISIONS[key] = (best, times)
    if _decide_only:  # the measured time of the best implementation; nothing runs on C
        return choice[1][choice[0]]
    name = FORCE.get(key, choice[0])
    if name not in calls:
        name = choice[0]
    if _SPLIT_STORE and "s+hip" in calls:  # the test-only switch forces the reinstated candidate where it applies
        name = "s+hip"
    if _TRACE and key not in _TRACED:
        _TRACED.add(key)
        print(f"[gemm] {key!r} -> {name}", flush=True)
    if TIMING is not None:
        s_ev, e_ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s_ev.record()
        _run(name)
        e_ev.record()
        TIMING.append((key, name, s_ev, e_ev))
        return name
    return _run(name)


K_ = K  # the kernel module (``K`` is shadowed by the reduction-size keyword above)

# ------------------------------------------------------------------------------ dX + dW in one launch
DUAL = os.environ.get("IIT_GEMM_DUAL", "1") != "0"
DUAL_DECISIONS: Dict[Tuple, Tuple[str, Dict[str, float]]] = {}
_DUAL_X_EPIS = (K.EPI_BF16, K.EPI_DGELU)
_DUAL_W_EPIS = (K.EPI_F32_STORE, K.EPI_F32_ACC)


def _dual_eligible(x: dict, w: dict) -> bool:
    return (DUAL and POLICY == "auto" and x["A"].is_cuda and x.get("mode", 0) == 0 and x.get("epi", 0) in _DUAL_X_EPIS
            and w.get("mode") == (K.MODE_AKM | K.MODE_BKM) and w.get("epi") in _DUAL_W_EPIS
            and all(x.get(k) is None for k in ("bias0", "resid", "C2", "splits"))
            and all(w.get(k) is None for k in ("bias0", "resid", "C2", "splits", "aux", "colsum")))


def _dual_specs(x: dict, w: dict, xc, wc, csum, bsum=None, gsq=None):
    ws = dict(A=w["A"], B=w["B"], C=wc, M=w["M"], N=w["N"], K=w["K"], lda=w["lda"], ldb=w["ldb"], ldc=w["ldc"],
              epi=w["epi"], bsum=bsum, gsq=gsq)
    xs = dict(A=x["A"], B=x["B"], C=xc, C2=x.get("aux"), M=x["M"], N=x["N"], K=x["K"], lda=x["lda"], ldb=x["ldb"],
              ldc=x["ldc"], ldc2=x.get("ldc2", 0), epi=x["epi"], csum=csum)
    return ws, xs


def _dual_candidates(x: dict, w: dict, xc, wc, csum, bsum=None, gsq=None):
    """name -> f() for every dual configuration (dW tile, dX tile, dW K-split) that covers the pair."""
    ws, xs = _dual_specs(x, w, xc, wc, csum, bsum, gsq)
    det = deterministic()
    out = {}
    for wt in K.DUAL_W_TILES:
        for xt in K.DUAL_X_TILES:
            if not K.dual_family_ok(wt, xt):
                continue
            for sp, red in ((1, False), (2, True), (4, True), (8, True), (2, False), (4, False), (8, False)):
                if not red and sp > 1 and (w["epi"] != K.EPI_F32_ACC or det):
                    continue  # atomic split-K: accumulate only, never in deterministic mode
                if sp > 1 and w["K"] // sp < 256:
                    continue
                if K.gemm_dual_ok(ws, xs, wt, xt, sp, red) and not _excluded(
                        f"dual{wt}.{xt}" + (f"{'r' if red else 'k'}{sp}" if sp > 1 else "")):
                    out[f"dual{wt}.{xt}" + (f"{'r' if red else 'k'}{sp}" if sp > 1 else "")] = \
                        lambda wt=wt, xt=xt, sp=sp, red=red: K.gemm_dual(ws, xs, wt, xt, sp, red)
    return out


def gemm_pair(x: dict, w: dict, prefetch=None) -> Optional[str]:
    """A layer's input gradient ``x`` (mode 0: ``dX = dY W^T``, bf16 or DGELU epilogue) and weight gradient ``w``
    (mode 3: ``dW (+)= X^T dY``), given as :func:`gemm` keyword dicts.  They are independent, so besides running
    them one after the other (each on its own best implementation) they can share ONE launch on the dual kernel
    (``csrc/gemm_dual.hip``): the dispatcher times both options once per problem pair and keeps the faster.
    ``IIT_GEMM_DUAL=0`` disables the dual launch.  ``prefetch``: tensors (the next pair's cold operands) the dual
    launch reads into the caches from extra workgroups.  Returns the weight-gradient choice (for ``_settle_claim``)."""
    def serial():
        gemm(**x)
        return gemm(**w)

    if not _dual_eligible(x, w):
        return serial()
    fresh = bool(w.get("fresh")) and w["epi"] == K.EPI_F32_STORE
    key = ("dual", x["M"], x["N"], x["K"], x["epi"], x.get("colsum") is not None,
           w["M"], w["N"], w["K"], w["epi"], fresh, deterministic())
    choice = DUAL_DECISIONS.get(key)
    if choice is None:
        shipped = _table().get(repr(key))
        if shipped is not None and not _excluded(shipped):
            choice = DUAL_DECISIONS[key] = (shipped, {shipped: float("nan")})
    if choice is None:
        if torch.cuda.is_current_stream_capturing():
            return serial()
        _frozen_miss(key)
        # time on scratch outputs (accumulate epilogues and column sums must not touch the real ones)
        xc = _scratch(x["C"], x["M"], max(x["ldc"], x["N"]))
        wc = _scratch(w["C"], w["M"], max(w["ldc"], w["N"]))
        cs = torch.zeros_like(x["colsum"]) if x.get("colsum") is not None else None
        bs = torch.zeros_like(w["bsum"]) if w.get("bsum") is not None else None
        sq = torch.zeros_like(w["gsq"]) if w.get("gsq") is not None else None
        calls = _dual_candidates(x, w, xc, wc, cs, bs, sq)
        calls["serial"] = lambda: (gemm(**{**x, "C": xc, "colsum": cs}),
                                   gemm(**{**w, "C": wc, "bsum": bs, "gsq": sq}))
        times = {n: min(_time(f) for _ in range(2)) for n, f in calls.items()}
        for n in sorted(times, key=times.get)[:3] if len(times) > 1 else ():
            times[n] = min(_time(calls[n], reps=30) for _ in range(3))
        best = min(times, key=times.get)
        choice = DUAL_DECISIONS[key] = (best, times)
    name = FORCE.get(key, choice[0])
    cfg = _parse_dual(name)
    ws, xs = _dual_specs(x, w, x["C"], w["C"], x.get("colsum"), w.get("bsum"), w.get("gsq"))
    if cfg is None or not K.gemm_dual_ok(ws, xs, *cfg):
        name, cfg = "serial", None
    s_ev = e_ev = None
    if TIMING is not None:  # in-context tuning (scripts/tune_gemm_in_situ.py): the pair's span, serial included
        s_ev, e_ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s_ev.record()
    if cfg is None:
        res = serial()
    else:
        K.gemm_dual(ws, xs, *cfg, prefetch=prefetch)
        res = name
    if TIMING is not None:
        e_ev.record()
        TIMING.append((key, name, s_ev, e_ev))
    return res


def _parse_dual(name: str):
    """``dual{wtile}.{xtile}[r|k]{splits}`` -> (wtile, xtile, splits, reduce)."""
    import re
    m = re.fullmatch(r"dual(\d+)\.(\d+)(?:([rk])(\d+))?", name)
    if m is None:
        return None
    return int(m.group(1)), int(m.group(2)), int(m.group(4) or 1), m.group(3) == "r"

# Shipped decision table: the measured choice per problem key from an MI355X run (``export_table``), so a fresh
# process skips the autotuning of known shapes (the first training epoch / the bench warm-up).  Entries are only
# used when the named implementation is among the problem's candidates; anything else is measured as before.
# ``IIT_GEMM_TABLE=0`` disables it, ``IIT_GEMM_TABLE=<path>`` reads another file.
_TABLE_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuned", "gemm_decisions_gfx950.json")
_TABLE = None
_RAGGED_TABLE: Dict[str, bool] = {}
_EDGE_TABLE: Dict[str, str] = {}


def _edge_table() -> Dict[str, str]:
    """Shipped whole-problem edge choices (``"edge"`` section of the table) for ragged problems."""
    _table()
    return _EDGE_TABLE


def _ragged_table() -> Dict[str, bool]:
    """Shipped ragged-problem choices (``"ragged"`` section of the table): split into bulk + tail or not."""
    _table()
    return _RAGGED_TABLE


def _table() -> Dict[str, str]:
    global _TABLE
    if _TABLE is None:
        _TABLE = {}
        _RAGGED_TABLE.clear()
        _EDGE_TABLE.clear()
        path = os.environ.get("IIT_GEMM_TABLE", _TABLE_PATH)
        if path != "0" and os.path.exists(path) and torch.cuda.is_available():
            import json
            try:
                with open(path) as f:
                    data = json.load(f)
                arch = getattr(torch.cuda.get_device_properties(0), "gcnArchName", "").split(":")[0]
                if data.get("arch") == arch:  # decisions measured on this GPU architecture only
                    _TABLE = dict(data.get("decisions", {}))
                    _RAGGED_TABLE.update({k: bool(v) for k, v in data.get("ragged", {}).items()})
                    _EDGE_TABLE.update({k: str(v) for k, v in data.get("edge", {}).items()})
            except (OSError, ValueError) as e:  # pragma: no cover - a corrupt table only costs autotuning
                print(f"[iit] GEMM decision table not loaded ({e})")
    return _TABLE


def sync_decisions(group=None) -> int:
    """Make the GEMM decisions identical on every data-parallel rank.

    Each rank measures the shapes it meets on its own (a shape missing from the shipped table), so two ranks can
    time different winners.  At a point every rank reaches together -- before any HIP-graph capture of a
    data-parallel phase (:mod:`iit_amd.engine.graphs`), and at the bench's end of warm-up -- all ranks exchange their
    tables (one ``all_gather_object``) and adopt, per problem key, the choice of the LOWEST rank that measured it: a
    captured graph then holds the same kernel on every rank, and rank 0's choice is the job's.  Collective: every
    rank of ``group`` must call it.  Returns the number of local entries that changed."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return 0
    ws = dist.get_world_size(group)
    mine = {"gemm": dict(DECISIONS), "dual": dict(DUAL_DECISIONS), "ragged": dict(RAGGED)}
    every = [None] * ws
    dist.all_gather_object(every, mine, group=group)
    changed = 0
    for name, table in (("gemm", DECISIONS), ("dual", DUAL_DECISIONS), ("ragged", RAGGED)):
        merged = {}
        for r in reversed(range(ws)):  # lower ranks overwrite: the lowest rank that measured a key decides it
            merged.update(every[r][name])
        for k, v in merged.items():
            old = table.get(k)
            if old is None or old[0] != v[0]:
                changed += 1
            table[k] = v
    return changed


def export_table(path: str) -> int:
    """Write the measured decisions of this process (``DECISIONS``) as a decision table; returns the entry count."""
    import json
    dec = {repr(k): v[0] for k, v in DECISIONS.items()}
    dec.update({repr(k): v[0] for k, v in DUAL_DECISIONS.items()})
    ragged = {repr(k): bool(v[0]) for k, v in RAGGED.items() if v[0] is not None}
    arch = getattr(torch.cuda.get_device_properties(0), "gcnArchName", "").split(":")[0] \
        if torch.cuda.is_available() else None
    with open(path, "w") as f:
        json.dump({"arch": arch, "device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else None,
                   "decisions": dec, "ragged": ragged, "edge": {repr(k): v for k, v in EDGE.items() if v}}, f,
                  indent=0, sort_keys=True)
    return len(dec) + len(ragged)


def report() -> str:
    lines = [f"library fast paths: {dict(_BLAS_OK) or 'all available'}"]
    for (M, N, Kd, mode, epi, bias, fresh, _det), (c, times) in sorted(DECISIONS.items()):
        ts = "  ".join(f"{k} {v:8.1f}us" for k, v in times.items())
        lines.append(f"M={M:6d} N={N:6d} K={Kd:6d} mode={mode:2d} epi={epi}{'f' if fresh else ''} bias={int(bias)} "
                     f"-> {c:6s} {ts}")
    for (M, N, Kd, mode, epi, bias, fresh, _), (split, whole, pieces) in sorted(RAGGED.items()):
        lines.append(f"M={M:6d} N={N:6d} K={Kd:6d} mode={mode:2d} epi={epi}{'f' if fresh else ''} bias={int(bias)} "
                     f"-> {'bulk+tail' if split else 'whole'}  whole {whole}us  bulk+tail {pieces}us")
    for key, (c, times) in sorted(DUAL_DECISIONS.items()):
        ts = "  ".join(f"{k} {v:8.1f}us" for k, v in sorted(times.items(), key=lambda kv: kv[1])[:6])
        lines.append(f"pair dX {key[1:6]} dW {key[6:11]} -> {c}  {ts}")
    return "\n".join(lines)
