"""Per-shape timing of the exact-fp32 implicit-GEMM convolutions (``csrc/conv_f32.hip``) against the library's fp32
convolutions at the shapes of ``train.py`` (MNIST-PVR, batch 256, channels-last ResNet-18): the stem, one 3 x 3
convolution of each layer, the three stride-2 3 x 3 convolutions and the three 1 x 1 downsamples; forward, input
gradient and weight gradient of each.

The kernel side is ``hip_kernels.conv_f32_fwd`` / ``_dgrad`` / ``_wgrad`` with the tile and split count of
``conv_f32.policy``; the library side is ``F.conv2d``, ``torch.nn.grad.conv2d_input`` and
``aten.convolution_backward`` (weight gradient only) on channels-last tensors with ``cudnn.benchmark`` off, which is
``train.py``'s default.  Both sides are captured graphs of ``--inner`` back-to-back calls, replayed alternately for
``--rounds`` rounds on one device and timed with device events; the table gives the median and the minimum
microseconds per call and the largest difference between the two results relative to the largest result.  Needs a
GPU; prints the table and writes it to ``--out`` when given.

    python scripts/bench_conv_f32.py --out profiles/conv_f32_kernels.txt
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name, H = W, Cin, Cout, k, s, pad
SHAPES = [("stem 7x7 s2", 56, 3, 64, 7, 2, 3), ("layer1 3x3", 14, 64, 64, 3, 1, 1), ("layer2 3x3", 7, 128, 128, 3, 1, 1),
          ("layer3 3x3", 4, 256, 256, 3, 1, 1), ("layer4 3x3", 2, 512, 512, 3, 1, 1),
          ("layer2 3x3 s2", 14, 64, 128, 3, 2, 1), ("layer3 3x3 s2", 7, 128, 256, 3, 2, 1),
          ("layer4 3x3 s2", 4, 256, 512, 3, 2, 1), ("layer2 down 1x1 s2", 14, 64, 128, 1, 2, 0),
          ("layer3 down 1x1 s2", 7, 128, 256, 1, 2, 0), ("layer4 down 1x1 s2", 4, 256, 512, 1, 2, 0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_conv_f32.py measures on a GPU; none is visible")
    from iit_amd.ops import conv_f32 as CF
    from iit_amd.ops import hip_kernels as K

    K.lib()
    torch.backends.cudnn.benchmark = False
    dev, B = "cuda", args.batch
    cl = torch.channels_last
    g = torch.Generator(device=dev).manual_seed(0)
    lines = [f"# {torch.cuda.get_device_name()}; batch {B}, channels-last fp32, cudnn.benchmark off; graphs of "
             f"{args.inner} calls, {args.rounds} alternating rounds; microseconds per call (median / min)",
             f"{'conv':<20} {'pass':<4} {'M':>7} {'N':>5} {'K':>6} {'tile':>4} {'splits':>6} "
             f"{'conv_f32 us':>17} {'library us':>17} {'ratio':>6} {'max rel diff':>12}"]

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

    for name, hw, cin, cout, k, s, pad in SHAPES:
        geom = K.conv_f32_geom(B, hw, hw, cin, cout, k, s, pad)
        oh = geom[4]
        x = torch.randn(B, cin, hw, hw, device=dev, generator=g).contiguous(memory_format=cl)
        w = (torch.randn(cout, cin, k, k, device=dev, generator=g) * 0.05).contiguous(memory_format=cl)
        dy = torch.randn(B, cout, oh, oh, device=dev, generator=g).contiguous(memory_format=cl)
        y, dx, dw = torch.empty_like(dy), torch.empty_like(x), torch.empty_like(w)

        def ours(pass_, fn, *ts):
            tile, splits = CF.policy(pass_, geom)

            def run():
                fn(*ts, geom, tile, splits)
                return ts[2]
            return tile, splits, run

        def lib_dw():
            return torch.ops.aten.convolution_backward(dy, x, w, None, [s, s], [pad, pad], [1, 1], False, [0, 0], 1,
                                                       [False, True, False])[1]

        passes = [("fwd", K.CONV_F32_FWD, ours(K.CONV_F32_FWD, K.conv_f32_fwd, x, w, y),
                   lambda: F.conv2d(x, w, stride=s, padding=pad)),
                  ("dX", K.CONV_F32_DGRAD, ours(K.CONV_F32_DGRAD, K.conv_f32_dgrad, dy, w, dx),
                   lambda: torch.nn.grad.conv2d_input(x.shape, w, dy, stride=s, padding=pad)),
                  ("dW", K.CONV_F32_WGRAD, ours(K.CONV_F32_WGRAD, K.conv_f32_wgrad, x, dy, dw), lib_dw)]
        for pname, pass_, (tile, splits, run), theirs in passes:
            pl = K.conv_f32_plan(pass_, geom, tile, splits)
            g_ours, y_ours = capture(run)
            g_ref, y_ref = capture(theirs)
            diff = ((y_ours - y_ref).abs().max() / y_ref.abs().max()).item()
            t_ours, t_ref = [], []
            for _ in range(args.rounds):
                t_ours.append(timed(g_ours))
                t_ref.append(timed(g_ref))
            mo, mr = statistics.median(t_ours), statistics.median(t_ref)
            lines.append(f"{name:<20} {pname:<4} {pl['M']:>7} {pl['N']:>5} {pl['K']:>6} {tile:>4} {splits:>6} "
                         f"{mo:>9.1f}/{min(t_ours):>7.1f} {mr:>9.1f}/{min(t_ref):>7.1f} {mo / mr:>6.2f} {diff:>12.2e}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
