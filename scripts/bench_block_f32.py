"""Per-call timing of the fp32 block glue, forward + backward, in the style of scripts/bench_attn_f32.py: LayerNorm
at ``[4096][64]`` and ``[4096][768]`` (``LayerNormF32Fn`` of csrc/block_f32.hip against ``TorchOps.layer_norm`` under
autograd) and the ``gelu_new`` MLP with its residual add at the 6L model's shape and at GPT-2-small's
(``MlpGeluResidualF32Fn`` against the ``hip32x`` composition: ``hip32`` GEMMs, torch ``gelu_new``, torch add).

Each candidate's forward + backward is captured as a graph of ``--inner`` back-to-back calls; the graphs are replayed
alternately for ``--rounds`` rounds on one device and timed with device events (median / minimum microseconds per call).

    python scripts/bench_block_f32.py --out profiles/block_f32_kernels.txt
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LN_SHAPES = (("ioi-6l", 4096, 64), ("gpt2-small", 4096, 768))  # (name, tokens, d_model): batch 256 x 16 positions
MLP_SHAPES = (("ioi-6l", 4096, 64, 256), ("gpt2-small", 4096, 768, 3072))  # (name, tokens, d_model, d_mlp)
EPS = 1e-5


def torch_layer_norm(x, w, b):
    """``TorchOps.layer_norm`` in fp32, what every backend but ``hip32n`` runs for an fp32 model."""
    from iit_amd.ops import _torch_ops
    return _torch_ops(torch.float32).layer_norm(x, w, b, EPS)


def hip32n_layer_norm(x, w, b):
    from iit_amd.ops.hip32_ops import LayerNormF32Fn
    return LayerNormF32Fn.apply(x, w, b, EPS)


def hip32x_mlp(x, W_in, b_in, W_out, b_out, resid):
    from iit_amd.ops.hip32_ops import LinearF32Fn
    from iit_amd.ops.torch_ops import gelu_new
    return resid + LinearF32Fn.apply(gelu_new(LinearF32Fn.apply(x, W_in, b_in)), W_out, b_out)


def hip32n_mlp(x, W_in, b_in, W_out, b_out, resid):
    from iit_amd.ops.hip32_ops import MlpGeluResidualF32Fn
    return MlpGeluResidualF32Fn.apply(x, W_in, b_in, W_out, b_out, resid)


def measure(fns: dict, operands, dy, inner: int, rounds: int) -> dict:
    """name -> (median, min) microseconds per forward + backward: alternating captured graphs of ``inner`` calls.
    Fresh leaves per candidate, first used on the side stream (see scripts/bench_attn_f32.py)."""
    runs = {}
    for name, fn in fns.items():
        lv = [t.detach().clone().requires_grad_() for t in operands]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):  # warm-up outside capture
            torch.autograd.grad(fn(*lv), lv, dy)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(inner):
                out = torch.autograd.grad(fn(*lv), lv, dy)
        graph.replay()
        torch.cuda.synchronize()
        runs[name] = (graph, out, lv)  # the graph reads the leaves at their addresses: they live as long as it does
    times = {name: [] for name in runs}
    for _ in range(rounds):
        for name, (graph, _, _) in runs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            graph.replay()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3 / inner)
    return {name: (statistics.median(t), min(t)) for name, t in times.items()}


def table(inner: int, rounds: int) -> list:
    dev = "cuda"
    g = torch.Generator().manual_seed(0)

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).to(dev)

    lines = [f"# {torch.cuda.get_device_name()}; fp32 forward + backward; {inner} calls per graph, {rounds} alternating "
             f"rounds; microseconds per call (median / min); ratio to the first candidate of the row group",
             f"{'op':<10} {'shape':<11} {'T':>5} {'d':>4} {'d_mlp':>5} {'candidate':<22} {'us per call':>15} {'ratio':>6}"]

    def emit(op, name, T, d, dm, res):
        first = next(iter(res.values()))[0]
        for cand, (med, mn) in res.items():
            lines.append(f"{op:<10} {name:<11} {T:>5} {d:>4} {dm:>5} {cand:<22} {med:>8.1f}/{mn:>6.1f} {med / first:>6.2f}")

    for name, T, d in LN_SHAPES:
        ops = [rnd(T, d), 1.0 + rnd(d, scale=0.1), rnd(d, scale=0.1)]
        emit("layer_norm", name, T, d, 0, measure({"torch (hip32x)": torch_layer_norm, "hip32n LayerNormF32Fn": hip32n_layer_norm},
                                                  ops, rnd(T, d), inner, rounds))
    for name, T, d, dm in MLP_SHAPES:
        ops = [rnd(T, d), rnd(d, dm, scale=d ** -0.5), rnd(dm, scale=0.1), rnd(dm, d, scale=dm ** -0.5),
               rnd(d, scale=0.1), rnd(T, d)]
        emit("mlp+resid", name, T, d, dm, measure({"hip32x composition": hip32x_mlp, "hip32n fused Fn": hip32n_mlp},
                                                  ops, rnd(T, d), inner, rounds))
    return lines


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=None)
    return ap.parse_args(argv)


def main(argv=None):
    args = parse(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_block_f32.py measures on a GPU; none is visible")
    text = "\n".join(table(args.inner, args.rounds)) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
