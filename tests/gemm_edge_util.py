"""Helpers of the ragged-N GEMM tests (tests/test_gemm_edge.py on the GPU, tests/test_gemm_edge_ref.py on the CPU):
problem builders on the small-integer operands of tests/gemm_exact_util.py, laid out so that a stray read or write
shows, and the comparator of what a launch left behind.

Layout of every buffer: one flat allocation, NaN (or the bf16 sentinel) everywhere, the operand's rows at stride
``pad8(extent)`` (+ 8 for A) from its start, so the row pads ``[extent, ld)`` are NaN and the first bytes after the
last row's ``pad8(extent)`` columns belong to a NaN-filled neighbour inside the same allocation.
"""
import torch

import gemm_exact_util as U
from iit_amd.ops import hip_kernels as HK

F32, BF16 = torch.float32, torch.bfloat16
EDGE_TILES = {t: HK.GLDS_TILES[t] for t in HK.GLDS_EDGE_TILES}  # tile id -> (BM, BN); K-tiles of 64
BK = 64
N_REMAINDERS = (1, 7, 8, 9, 81)
MODE_BKM, MODE_3 = 2, 3
EPI_BF16, EPI_F32_ACC, EPI_F32_STORE = 0, 5, 7
TAIL = 64  # elements of NaN neighbour after every operand


def pad8(n: int) -> int:
    return (n + 7) // 8 * 8


def edge_shapes(tile: int):
    """(M, N, K) of every N-edge case of ``tile``: N = BN + r, 2 BN - 1; M = BM, 2 BM; K = 2 BK, 3 BK."""
    bm, bn = EDGE_TILES[tile]
    for n in [bn + r for r in N_REMAINDERS] + [2 * bn - 1]:
        for m in (bm, 2 * bm):
            for k in (2 * BK, 3 * BK):
                yield m, n, k


def _hosted(x: torch.Tensor, ld: int, dtype, fill) -> torch.Tensor:
    """``x`` as a [rows][cols] view (row stride ``ld``) of a flat ``fill``-filled buffer with a ``TAIL`` after it."""
    rows, cols = x.shape
    flat = torch.full(((rows - 1) * ld + pad8(cols) + TAIL,), fill, dtype=dtype, device=x.device)
    view = torch.as_strided(flat, (rows, cols), (ld, 1))
    view.copy_(x)
    return view


def make_case(mode: int, epi: int, M: int, N: int, Kd: int, seed: int, device):
    """One ragged-N problem: dict of operands, outputs (pre-filled), their prefills and the exact expectations."""
    a = U.ints((M, Kd), -U.A_MAX, U.A_MAX, seed, device)
    b = U.ints((Kd, N), -U.B_MAX, U.B_MAX, seed + 1, device)
    c = {"M": M, "N": N, "K": Kd, "mode": mode, "epi": epi}
    if mode == MODE_3:  # A [K][M] k-major
        c["lda"] = pad8(M) + 8
        c["A"] = _hosted(a.t().contiguous(), c["lda"], BF16, float("nan"))
    else:
        c["lda"] = Kd + 8
        c["A"] = _hosted(a, c["lda"], BF16, float("nan"))
    c["ldb"] = c["ldc"] = pad8(N)
    c["B"] = _hosted(b, c["ldb"], BF16, float("nan"))
    out_dtype = BF16 if epi == EPI_BF16 else F32
    fill = U.BF16_FILL if out_dtype == BF16 else U.F32_FILL
    # output: M rows of pad8(N) and one more row beyond the problem, all pre-filled
    c["Cbuf"] = torch.full(((M + 1) * c["ldc"] + TAIL,), fill, dtype=out_dtype, device=device)
    c["C"] = torch.as_strided(c["Cbuf"], (M, N), (c["ldc"], 1))
    exp = U.exact_mm(a, b)
    if epi == EPI_F32_ACC:
        init = U.ints((M, N), -U.ADD_MAX, U.ADD_MAX, seed + 2, device)
        c["C"].copy_(init)
        exp = exp + init
        c["bias0"] = None
    else:
        bias = U.ints((N,), -U.BIAS_MAX, U.BIAS_MAX, seed + 10, device)
        c["bias0"] = _hosted(bias[None], pad8(N), F32, float("nan"))[0]
        exp = exp + bias
    c["C0"] = c["Cbuf"].clone()
    c["exp"] = exp.bfloat16() if out_dtype == BF16 else exp
    c["bsum"] = c["gsq"] = None
    if mode == MODE_3:
        binit = U.ints((N,), -U.ADD_MAX, U.ADD_MAX, seed + 20, device)
        c["bsum_buf"] = torch.full((pad8(N) + TAIL,), float("nan"), device=device)
        c["bsum_buf"][:N] = binit
        c["bsum"] = c["bsum_buf"][:N]
        c["bsum0"] = c["bsum_buf"].clone()
        c["bsum_exp"] = binit + b.double().sum(0).float()
        if epi == EPI_F32_STORE:
            c["gsq"] = torch.zeros(64, device=device)
            c["gsq_exp"] = float(exp.double().pow(2).sum())
    return c


def check_case(c, tag="") -> list:
    """What is wrong with the outputs of ``c`` after a launch: a list of messages (empty: all exact).

    * the [M][N] result bitwise against the exact one (fp32), or against it rounded once (bf16);
    * every other element of the output allocation -- row pads [N, pad8(N)), the row beyond M, the neighbour --
      must hold its prefill bits;
    * ``bsum`` [0, N) exact (integer sums), its pads and neighbour untouched;
    * ``gsq``: the 64 slots sum to the exact sum of squares within M N 2^-24 relative (an fp32 sum of M N
      non-negative terms in any order); NaN -- a leaked pad -- fails."""
    M, N = c["M"], c["N"]
    errs = []
    got = c["C"]
    bad = U.bad_bits(got, c["exp"])
    if bad.any():
        i, j = (int(v) for v in bad.nonzero()[0])
        errs.append(f"{tag}: {int(bad.sum())} of {bad.numel()} elements wrong, first at ({i}, {j}): "
                    f"got {float(got[i, j])}, exact {float(c['exp'][i, j])}")
    keep = torch.ones_like(c["Cbuf"], dtype=torch.bool)
    torch.as_strided(keep, (M, N), (c["ldc"], 1)).fill_(False)
    touched = U.bad_bits(c["Cbuf"], c["C0"]) & keep
    if touched.any():
        at = int(touched.nonzero()[0])
        errs.append(f"{tag}: {int(touched.sum())} elements outside the [M][N] result written, first at row "
                    f"{at // c['ldc']} column {at % c['ldc']}")
    if c["bsum"] is not None:
        bad = U.bad_bits(c["bsum"], c["bsum_exp"])
        if bad.any():
            errs.append(f"{tag}: bsum wrong at column {int(bad.nonzero()[0])}")
        if U.bad_bits(c["bsum_buf"][N:], c["bsum0"][N:]).any():
            errs.append(f"{tag}: bsum written at or beyond column N")
    if c["gsq"] is not None:
        tot = float(c["gsq"].double().sum())
        if not abs(tot - c["gsq_exp"]) <= M * N * 2.0 ** -24 * c["gsq_exp"]:
            errs.append(f"{tag}: gsq {tot} vs exact {c['gsq_exp']}")
    return errs
