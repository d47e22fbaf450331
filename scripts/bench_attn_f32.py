"""Per-call timing of fp32 attention, forward + backward, at the shapes of the fp32 models: what the op costs today on
the fp32 torch path (``TorchOps.attention`` under autograd: two batched einsums with their permute copies, a divide,
a masked fill, softmax, the NaN scrub and a ``where``, and autograd's backward of each), the number an fp32 attention
kernel has to beat.  ``CANDIDATES`` is the list of implementations; ``GPU_CANDIDATES`` adds the fp32 MFMA kernel of
csrc/attn_fp32.hip (``AttentionF32Fn``) when the device is a GPU.

Each candidate's forward + backward is captured as a graph of ``--inner`` back-to-back calls; the graphs are replayed
alternately for ``--rounds`` rounds on one device and timed with device events.  The table gives the median and the
minimum microseconds per call, the ratio to the first candidate, and that time times the layers of the 6L model.
Without a GPU (``--device cpu``, tests) the calls run eagerly under a wall clock.

    python scripts/bench_attn_f32.py --out profiles/attn_f32_kernel_6l.txt
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, B, S, H, dh): the 6L/64d IOI model at the train_ioi.py batch, its paired size (base + source rows in one
# call), GPT-2-small's heads at the same batch
SHAPES = (("ioi-6l", 256, 16, 4, 16), ("ioi-6l paired", 512, 16, 4, 16), ("gpt2-small", 256, 16, 12, 64))
LAYERS_6L = 6


def torch_attention(q, k, v, causal: bool, scale: float):
    """``TorchOps.attention`` in fp32 as ``Attention.compute_z`` calls it on the torch backend (no hooks, -inf fill)."""
    from iit_amd.ops.torch_ops import TorchOps
    return TorchOps.attention(None, q, k, v, causal, 1.0 / scale)  # the op reads nothing from its backend object


def hip32x_attention(q, k, v, causal: bool, scale: float):
    """``AttentionF32Fn``: the fp32 MFMA kernels of csrc/attn_fp32.hip, as the ``hip32x`` backend calls them."""
    from iit_amd.ops.hip32_ops import AttentionF32Fn
    return AttentionF32Fn.apply(q, k, v, causal, scale)


CANDIDATES = {"torch": torch_attention}  # what runs on any device
GPU_CANDIDATES = {"hip32x": hip32x_attention}


def candidates(device) -> dict:
    """``CANDIDATES``, on a GPU followed by the kernels that need one."""
    return {**CANDIDATES, **GPU_CANDIDATES} if torch.device(device).type == "cuda" else dict(CANDIDATES)


def operands(B, S, H, dh, device, seed: int = 0):
    """Standard-normal fp32 q, k, v (requiring gradients) and dO, ``[B][S][H][dh]``."""
    g = torch.Generator().manual_seed(seed)
    q, k, v, do = (torch.randn(B, S, H, dh, generator=g).to(device) for _ in range(4))
    return [t.requires_grad_() for t in (q, k, v)], do


def step(fn, leaves, do, causal: bool, scale: float):
    """One forward + backward: (z, dq, dk, dv)."""
    z = fn(*leaves, causal, scale)
    return (z,) + tuple(torch.autograd.grad(z, leaves, do))


def measure(fns: dict, leaves, do, causal: bool, scale: float, inner: int, rounds: int) -> dict:
    """name -> {"median_us", "min_us", "out"} per call of ``step``; on a GPU as alternating captured graphs of
    ``inner`` calls timed with device events, else eagerly under ``perf_counter``."""
    cuda = do.is_cuda
    runs = {}
    keep = []  # every graph's leaves: a graph reads them at their addresses, so they live as long as the graphs do
    for name, fn in fns.items():
        if not cuda:
            out = step(fn, leaves, do, causal, scale)
            runs[name] = (lambda fn=fn: [step(fn, leaves, do, causal, scale) for _ in range(inner)], out)
            continue
        # Fresh leaves per candidate, first used in the warm-up on the side stream, and no earlier result kept, as
        # tests/test_hip32_ops.py captures its Function.  torch's autograd warns (input_buffer.cpp) that an
        # AccumulateGrad node kept alive from an earlier use on the default stream "may ... break CUDA graph capture";
        # a capture through such leaves did not survive here, and that warning is the supposed, not a proven, reason
        lv = [t.detach().clone().requires_grad_() for t in leaves]
        keep.append(lv)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):  # warm-up outside capture
            step(fn, lv, do, causal, scale)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(inner):
                out = step(fn, lv, do, causal, scale)
        graph.replay()
        torch.cuda.synchronize()
        runs[name] = (graph.replay, out)
    times = {name: [] for name in runs}
    for _ in range(rounds):
        for name, (run, _) in runs.items():
            if cuda:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                run()
                b.record()
                b.synchronize()
                times[name].append(a.elapsed_time(b) * 1e3 / inner)
            else:
                t0 = time.perf_counter()
                run()
                times[name].append((time.perf_counter() - t0) * 1e6 / inner)
    return {name: {"median_us": statistics.median(t), "min_us": min(t), "out": runs[name][1]}
            for name, t in times.items()}


def table(device, inner: int, rounds: int, shapes=SHAPES, fns=None) -> list:
    fns = fns or CANDIDATES
    where = torch.cuda.get_device_name() if torch.device(device).type == "cuda" else "cpu (eager, wall clock)"
    lines = [f"# {where}; fp32 attention forward + backward, causal, scale dh^-0.5; {inner} calls per graph, {rounds} "
             f"alternating rounds; microseconds per call (median / min); x{LAYERS_6L} = one pass over the 6L model",
             f"{'shape':<14} {'B':>4} {'S':>3} {'H':>3} {'dh':>3} {'candidate':<10} {'us per call':>15} {'ratio':>6} "
             f"{'x' + str(LAYERS_6L) + ' us':>8}"]
    for name, B, S, H, dh in shapes:
        leaves, do = operands(B, S, H, dh, device)
        res = measure(fns, leaves, do, True, dh ** -0.5, inner, rounds)
        first = next(iter(res.values()))["median_us"]
        for cand, r in res.items():
            lines.append(f"{name:<14} {B:>4} {S:>3} {H:>3} {dh:>3} {cand:<10} {r['median_us']:>8.1f}/{r['min_us']:>6.1f} "
                         f"{r['median_us'] / first:>6.2f} {LAYERS_6L * r['median_us']:>8.1f}")
    return lines


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=None)
    return ap.parse_args(argv)


def main(argv=None):
    args = parse(argv)
    if args.device == "cuda" and not torch.cuda.is_available():
        raise SystemExit("bench_attn_f32.py measures on a GPU; none is visible (--device cpu runs it eagerly)")
    text = "\n".join(table(args.device, args.inner, args.rounds, fns=candidates(args.device))) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
