"""``hip32p`` against ``hip32n`` on the 6-layer / 64-d IOI model in the training loop, by the recipe of
profiles/hip32n_6l_step.txt: ``scripts/time_to_iia.py --model ioi-6l --epochs 30 --fp32-backend {hip32n,hip32p}``
(``IOI_ModelPair.train`` as ``train_ioi.py`` runs it, phase graphs on), each run a fresh process, alternating hip32n,
hip32p, hip32n, hip32p in one session on one device.

Reported: the steady epoch (median epoch-to-epoch wall time, training + evaluation) of every run; the largest relative
difference of any metric of any epoch between the two backends and between the two runs of one backend; the
backend's call counters (that the paired ops ran, and no ``paired_fallback``); and the tile / split-K choice of every
forward GEMM at T and at 2T rows, which is where the two backends' bits could part.

    python scripts/bench_hip32p.py --out profiles/hip32p_6l_step.txt
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BACKENDS = ("hip32n", "hip32p")


def run_once(backend: str, epochs: int, timeout: int):
    """(record, per-epoch metric dicts) of one ``time_to_iia.py`` child process."""
    with tempfile.TemporaryDirectory() as tmp:
        dump = os.path.join(tmp, "epochs.jsonl")
        cmd = [sys.executable, os.path.join(ROOT, "scripts", "time_to_iia.py"), "--model", "ioi-6l", "--epochs",
               str(epochs), "--fp32-backend", backend, "--dump-epochs", dump]
        out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
        if out.returncode != 0:
            raise SystemExit(f"{' '.join(cmd)} exited with {out.returncode}\n{out.stdout[-4000:]}")
        rec = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
        with open(dump) as f:
            epochs_seen = [json.loads(ln) for ln in f]
    return rec, epochs_seen


def max_rel_diff(a, b) -> float:
    worst = 0.0
    assert len(a) == len(b)
    for ea, eb in zip(a, b):
        for k, va in ea.items():
            if k in ("epoch", "wall_s"):
                continue
            vb = eb[k]
            worst = max(worst, abs(va - vb) / max(abs(va), abs(vb), 1e-30) if va != vb else 0.0)
    return worst


def gemm_policy() -> list:
    """(tile, splits) of every forward GEMM of the model at T = 4096 and 2T = 8192 rows."""
    from iit_amd.ops import hip_kernels as K
    from iit_amd.ops.hip32_ops import _tile
    from iit_amd.models.config import gpt2_config_dict
    from iit_amd.tasks.ioi import ioi_cfg
    cfg = gpt2_config_dict()
    cfg.update(ioi_cfg)  # as time_to_iia.py builds the model: d_mlp stays GPT-2's
    d, H, dh, dm = cfg["d_model"], cfg["n_heads"], cfg["d_head"], cfg["d_mlp"]
    T = 256 * 16
    lines = []
    for name, N, Kd in (("qkv", 3 * H * dh, d), ("o_proj", d, H * dh), ("mlp_in", dm, d), ("mlp_out", d, dm)):
        got = [(_tile(M, N), K.gemm_f32_splits(M, N, Kd, _tile(M, N))) for M in (T, 2 * T)]
        lines.append(f"   {name:<8} N {N:>4} K {Kd:>4}: T rows tile {got[0][0]} splits {got[0][1]}; 2T rows tile "
                     f"{got[1][0]} splits {got[1][1]}{'' if got[0] == got[1] else '   <- differs'}")
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=400, help="seconds per child process")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    runs = {b: [] for b in BACKENDS}
    for _ in range(args.rounds):
        for b in BACKENDS:
            runs[b].append(run_once(b, args.epochs, args.timeout))
            print(b, runs[b][-1][0]["steady_s_per_epoch"], flush=True)

    device = runs["hip32n"][0][0]["device"]
    lines = [f"hip32p (hip32n plus the paired source + base forward) against hip32n on the 6L/64d IOI model (train_ioi.py "
             f"configuration: batch 256, 16 tokens, fp32), one {device}; the protocol of profiles/hip32n_6l_step.txt.",
             "",
             f"1. In the loop: scripts/time_to_iia.py --model ioi-6l --epochs {args.epochs} --fp32-backend "
             "{hip32n,hip32p} (graphs on), a fresh",
             "   process per run, alternating in one session; steady = median epoch-to-epoch wall time (training + "
             "evaluation).", ""]
    for r in range(args.rounds):
        for b in BACKENDS:
            lines.append(f"   run {r + 1} {b} steady {runs[b][r][0]['steady_s_per_epoch']:.3f} s/epoch")
    mean = {b: sum(x[0]["steady_s_per_epoch"] for x in runs[b]) / len(runs[b]) for b in BACKENDS}
    lines.append(f"   means: hip32n {mean['hip32n']:.3f}, hip32p {mean['hip32p']:.3f} s/epoch; hip32p / hip32n = "
                 f"{mean['hip32p'] / mean['hip32n']:.3f}.  No target was fixed in advance.")
    lines += ["", f"2. Epoch metrics, all {args.epochs} epochs, largest relative difference in any metric of any epoch:"]
    for b in BACKENDS:
        for r in range(1, args.rounds):
            lines.append(f"   {b} run 1 against {b} run {r + 1}: {max_rel_diff(runs[b][0][1], runs[b][r][1]):.1e}")
    lines.append(f"   hip32p against hip32n: {max_rel_diff(runs['hip32p'][0][1], runs['hip32n'][0][1]):.1e}")
    for e in sorted({0, min(10, args.epochs - 1), args.epochs - 1}):
        for b in BACKENDS:
            m = runs[b][0][1][e]
            lines.append(f"   epoch {e:>2} {b} " + " ".join(f"{v:.5f}" for k, v in m.items() if k not in ("epoch", "wall_s")))
    lines += ["", "3. Forward GEMM policy (hip32_ops._tile, hip_kernels.gemm_f32_splits) at T = 4096 and 2T = 8192 rows; "
              "the two backends'", "   bits can differ only where a line differs:"]
    lines += gemm_policy()
    lines += ["", "4. Call counters of the hip32p process (calls made while the phase graphs were captured and in eager "
              "evaluation):", "   " + json.dumps(runs["hip32p"][0][0].get("backend_calls"))]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
