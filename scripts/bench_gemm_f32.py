"""Per-shape timing of the exact-fp32 MFMA GEMM (``csrc/gemm_f32.hip``) against fp32 ``torch.mm`` for the
projections of the 6L/64d IOI model at the ``train_ioi.py`` batch (256 prompts of 16 tokens; the unembed sees the
last position only): forward ``x @ W``, input gradient ``dY @ W^T`` and weight gradient ``X^T dY`` of each.

Both sides are captured graphs of ``--inner`` back-to-back products, replayed alternately for ``--rounds`` rounds on
one device and timed with device events; the table gives the median and the minimum microseconds per product, the
tile and split count the ``hip32`` policy picked, and the largest difference between the two results relative to the
largest result.  Needs a GPU; prints the table and writes it to ``--out`` when given.

    python scripts/bench_gemm_f32.py --out profiles/hip32_gemm_shapes.txt
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=256 * 16)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gemm_f32.py measures on a GPU; none is visible")
    from iit_amd.ops import hip32_ops as H32
    from iit_amd.ops import hip_kernels as K

    K.lib()
    dev = "cuda"
    T, B = args.tokens, args.batch
    layers = [("QKV", T, 64, 192), ("W_O", T, 64, 64), ("W_in", T, 64, 3072), ("W_out", T, 3072, 64),
              ("unembed (last position)", B, 64, 50257)]
    g = torch.Generator(device=dev).manual_seed(0)
    lines = [f"# {torch.cuda.get_device_name()}; tokens {T}, batch {B}; graphs of {args.inner} products, "
             f"{args.rounds} alternating rounds; microseconds per product (median / min)",
             f"{'layer':<24} {'pass':<4} {'M':>6} {'N':>6} {'K':>6} {'tile':>4} {'splits':>6} "
             f"{'gemm_f32 us':>15} {'torch.mm us':>15} {'ratio':>6} {'max rel diff':>12}"]

    def timed(graph):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / args.inner

    def capture(fn):
        fn()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(args.inner):
                out = fn()
        graph.replay()
        torch.cuda.synchronize()
        return graph, out

    for name, rows, kin, nout in layers:
        x = torch.randn(rows, kin, device=dev, generator=g)
        W = (torch.randn(kin, H32._up4(nout), device=dev, generator=g) * 0.1)[:, :nout]  # rows padded as in the arena
        dy = H32._out(rows, nout, dev).copy_(torch.randn(rows, nout, device=dev, generator=g))
        passes = [
            ("fwd", rows, nout, kin, lambda: H32._forward(x, W, None), lambda: torch.mm(x, W)),
            ("dX", rows, kin, nout, lambda: H32._backward(x, W, dy, True, False)[0], lambda: torch.mm(dy, W.t())),
            ("dW", kin, nout, rows, lambda: H32._backward(x, W, dy, False, True)[1], lambda: torch.mm(x.t(), dy)),
        ]
        for pname, M, N, Kd, ours, theirs in passes:
            tile = H32._tile(M, N)
            splits = K.gemm_f32_splits(M, N, Kd, tile)
            g_ours, y_ours = capture(ours)
            g_ref, y_ref = capture(theirs)
            diff = ((y_ours - y_ref).abs().max() / y_ref.abs().max()).item()
            t_ours, t_ref = [], []
            for _ in range(args.rounds):
                t_ours.append(timed(g_ours))
                t_ref.append(timed(g_ref))
            mo, mr = statistics.median(t_ours), statistics.median(t_ref)
            lines.append(f"{name:<24} {pname:<4} {M:>6} {N:>6} {Kd:>6} {tile:>4} {splits:>6} "
                         f"{mo:>8.1f}/{min(t_ours):>6.1f} {mr:>8.1f}/{min(t_ref):>6.1f} {mo / mr:>6.2f} {diff:>12.2e}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
