"""Per-call timing of the paired fp32 attention (csrc/attn_fp32.hip ``iit_attn_f32_fwd_pair`` +
``iit_attn_f32_bwd_masked``) against the composition it replaces in an interchange intervention on ``hook_z``: the
plain forward over the 2B rows, ``K.splice`` (source rows into the base rows), the gradient-mask splice and the plain
backward over the B base rows.  Shapes: the 6-layer IOI model's heads (B 256, S 16, H 4, dh 16) and GPT-2-small's
(B 256, S 16, H 12, dh 64); indexes: one head, and one position of every head.

Each candidate is captured as a graph of ``--inner`` back-to-back calls; the graphs are replayed alternately for
``--rounds`` rounds, and the whole measurement is taken twice (two runs), timed with device events (median / minimum
microseconds per forward + backward).

    python scripts/bench_attn_f32_pair.py --out profiles/attn_f32_pair_kernel.txt
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("ioi-6l", 256, 16, 4, 16), ("gpt2-small", 256, 16, 12, 64))  # (name, B, S, H, dh)


def candidates(B, S, H, dh, index):
    """name -> a function running one forward + backward on preallocated tensors."""
    from iit_amd.ops import hip_kernels as K
    from iit_amd.ops.hip_ops import pair_specs
    from iit_amd.ops.splice import patch_spec
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(2 * B, S, H, dh, generator=g).to(dev) for _ in range(3))
    dz = torch.randn(B, S, H, dh, generator=g).to(dev)
    z, z2 = torch.empty_like(q), torch.empty_like(q)
    lse = torch.empty(2 * B, H, S, device=dev)
    dzm = torch.empty_like(dz)
    grads = [torch.empty_like(dz) for _ in range(3)]
    scale = dh ** -0.5
    spec = patch_spec(index, (B, S, H, dh))
    pair_spec, base_spec = pair_specs(index, (B, S, H, dh))

    def composition():
        K.attn_f32_fwd(q, k, v, z, lse, scale, True)
        K.splice(z, z[B:], z2, z.numel(), pair_spec.ptr, True, 0)
        K.splice(dz, None, dzm, dz.numel(), base_spec.ptr, True, 1)
        K.attn_f32_bwd(q[:B], k[:B], v[:B], dzm, lse[:B], *grads, scale, True)

    def paired():
        K.attn_f32_fwd_pair(q, k, v, z, lse, scale, True, spec)
        K.attn_f32_bwd_masked(q[:B], k[:B], v[:B], dz, lse[:B], *grads, scale, True, spec)

    return {"fwd(2B) + splice + mask + bwd": composition, "fwd_pair + bwd_masked": paired}


def measure(fns: dict, inner: int, rounds: int) -> dict:
    runs = {}
    for name, fn in fns.items():
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):  # warm-up outside capture
            fn()
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(inner):
                fn()
        graph.replay()
        torch.cuda.synchronize()
        runs[name] = graph
    times = {name: [] for name in runs}
    for _ in range(rounds):
        for name, graph in runs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            graph.replay()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3 / inner)
    return {name: (statistics.median(t), min(t)) for name, t in times.items()}


def table(inner: int, rounds: int) -> list:
    from iit_amd.core.index import Ix
    lines = [f"# {torch.cuda.get_device_name()}; fp32 causal attention, forward + backward of an interchange "
             f"intervention on hook_z; {inner} calls per graph, {rounds} alternating rounds, two runs; microseconds "
             f"per call (median / min); ratio to the composition",
             f"{'run':>3} {'shape':<11} {'B':>4} {'S':>3} {'H':>3} {'dh':>3} {'index':<13} {'candidate':<30} "
             f"{'us per call':>15} {'ratio':>6}"]
    for run in (1, 2):
        for name, B, S, H, dh in SHAPES:
            for iname, index in (("one head", Ix[:, :, 1]), ("last position", Ix[:, -1])):
                res = measure(candidates(B, S, H, dh, index), inner, rounds)
                first = next(iter(res.values()))[0]
                for cand, (med, mn) in res.items():
                    lines.append(f"{run:>3} {name:<11} {B:>4} {S:>3} {H:>3} {dh:>3} {iname:<13} {cand:<30} "
                                 f"{med:>8.1f}/{mn:>6.1f} {med / first:>6.2f}")
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
        raise SystemExit("bench_attn_f32_pair.py measures on a GPU; none is visible")
    text = "\n".join(table(args.inner, args.rounds)) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
