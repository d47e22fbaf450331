"""Helpers shared by the exact-fp32 GEMM tests (tests/test_gemm_f32.py on the GPU, tests/test_gemm_f32_ref.py on the
CPU): operand families, references, comparators and the wrong products a comparator must flag.

Three exact families.  Operands are integers exact in fp32 and every sum of products -- plus bias, residual and
initial C -- stays below 2^24, so the fp32 result does not depend on the order of the additions and is compared
bitwise.  Each family rejects a different shortcut:

* ``F1``: the small integers of tests/gemm_exact_util.py (exact even in bf16): indexing and epilogue mistakes.
* ``F2``: wide integers |a| <= 4095, |b| <= 3 (K <= 1024): 12-bit operands that bf16 (8 bits) cannot hold.
* ``F3`` / ``F3M``: sparse wide -- at most 3 nonzeros per row of A (``F3``) or per column of B (``F3M``) with
  magnitude below 2^22, the other operand in {-1, 0, 1}: 22-bit operands that a bf16 hi + lo split (16 bits)
  cannot hold either.

One real-valued family (``REAL``, standard-normal operands) is checked against float64 with the bound of
:func:`bad_real`.
"""
import torch

import gemm_exact_util as U

F1, F2, F3, F3M, REAL = "F1", "F2", "F3", "F3M", "REAL"
EXACT = (F1, F2, F3, F3M)
F2_A, F2_B = 4095, 3
F3_WIDE, F3_NNZ = (1 << 22) - 1, 3  # |wide| < 2^22, nonzeros per reduction
K_USED = (1, 3, 32, 33, 64, 96, 257, 1024)  # every reduction length the GPU module uses on the exact families
K_REAL = (64, 256)
LIMIT = 1 << 24  # integers up to here are exact in fp32


def worst_sum(family: str, K: int) -> int:
    """Largest |value| a partial or final sum of an epilogue can reach on ``family``."""
    extra = U.BIAS_MAX + 2 * U.ADD_MAX
    if family == F1:
        return U.A_MAX * U.B_MAX * K + extra
    if family == F2:
        return F2_A * F2_B * K + extra
    return F3_WIDE * min(F3_NNZ, K) + extra


def _sparse_wide(rows: int, K: int, g: torch.Generator) -> torch.Tensor:
    """[rows][K] with at most ``F3_NNZ`` nonzeros per row, each an integer of magnitude below 2^22."""
    vals = torch.randint(-F3_WIDE, F3_WIDE + 1, (rows, F3_NNZ), generator=g).float()
    cols = torch.randint(0, K, (rows, F3_NNZ), generator=g)
    return torch.zeros(rows, K).scatter_(1, cols, vals)


def operands(family: str, M: int, N: int, K: int, seed: int, device="cpu"):
    """``(a [M][K], b [K][N])`` in fp32, reproducible per seed (generated on the CPU, then moved)."""
    g = torch.Generator().manual_seed(seed)
    if family == F1:
        a = torch.randint(-U.A_MAX, U.A_MAX + 1, (M, K), generator=g).float()
        b = torch.randint(-U.B_MAX, U.B_MAX + 1, (K, N), generator=g).float()
    elif family == F2:
        a = torch.randint(-F2_A, F2_A + 1, (M, K), generator=g).float()
        b = torch.randint(-F2_B, F2_B + 1, (K, N), generator=g).float()
    elif family == F3:
        a = _sparse_wide(M, K, g)
        b = torch.randint(-1, 2, (K, N), generator=g).float()
    elif family == F3M:
        a = torch.randint(-1, 2, (M, K), generator=g).float()
        b = _sparse_wide(N, K, g).t().contiguous()
    elif family == REAL:
        a = torch.randn(M, K, generator=g)
        b = torch.randn(K, N, generator=g)
    else:
        raise ValueError(family)
    return a.to(device), b.to(device)


def lds(widths, step: int = 4):
    """One padded leading dimension per width: a multiple of ``step`` elements, all distinct."""
    out = []
    for i, w in enumerate(widths):
        ld = (w + step - 1) // step * step + step * (i + 1)
        while ld in out:
            ld += step * (len(widths) + 1)
        out.append(ld)
    return out


# ------------------------------------------------------------------------------ wrong products
def _bf(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).to(torch.float64)


def bf16_rounded_mm(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """The product a kernel computes that rounds its operands to bf16 while staging (exact sums)."""
    return (_bf(a) @ _bf(b)).float()


def bf16_split3_mm(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """The three-term bf16 split product ``hi hi + hi lo + lo hi`` (exact sums)."""
    ah, bh = _bf(a), _bf(b)
    al, bl = _bf(a.double() - ah), _bf(b.double() - bh)
    return (ah @ bh + ah @ bl + al @ bh).float()


# ------------------------------------------------------------------------------ the real-valued bound
def gamma(K: int, splits: int = 1) -> float:
    """``n u / (1 - n u)`` for a chain of ``n = K + splits + 2`` roundings (K products-and-adds, the split sums,
    bias and residual) at ``u = 2^-23``: twice the round-to-nearest unit, since an MFMA accumulator need not round
    to nearest."""
    n, u = K + splits + 2, 2.0 ** -23
    return n * u / (1.0 - n * u)


def real_reference(a, b, bias=None, resid=None):
    """float64 value and magnitude sum ``sum_k |a||b| + |bias| + |resid|`` of ``a @ b (+ bias) (+ resid)``."""
    ref = a.double() @ b.double()
    mag = a.double().abs() @ b.double().abs()
    for t in (bias, resid):
        if t is not None:
            ref = ref + t.double()
            mag = mag + t.double().abs()
    return ref, mag


def real_ratio(got, ref, mag, K: int, splits: int = 1) -> torch.Tensor:
    """``|got - ref| / (gamma mag)`` per element (<= 1 passes)."""
    return (got.double() - ref).abs() / (gamma(K, splits) * mag)


def bad_real(got, ref, mag, K: int, splits: int = 1) -> torch.Tensor:
    return ~((got.double() - ref).abs() <= gamma(K, splits) * mag)
