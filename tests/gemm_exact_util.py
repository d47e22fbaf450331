"""Helpers shared by the exact GEMM tests (tests/test_gemm_exact.py on the GPU, tests/test_gemm_exact_ref.py on the
CPU): small-integer operands, exact references, element-wise comparators and the perturbations they must flag.

Operands are small integers, exact in bf16, and every sum stays below 2^24, so the fp32 result of a GEMM does not
depend on the order of the additions: a wrong element is a wrong element, never rounding, and outputs are compared
bitwise.  Only the GELU epilogues need a bound, derived from the number formats (see :func:`bad_gelu`).
"""
import math

import torch

A_MAX, B_MAX = 3, 2  # |A| <= 3, |B| <= 2 (the operands of tests/test_split_k_exact.py)
UNIT_MAX = 1  # operands of the GELU cases: |pre| stays small enough to be exact in bf16
BIAS_MAX, ADD_MAX = 5, 50  # bias; residual and initial C
K_LIMIT = 1152  # the longest reduction any exact test uses (9 K-tiles of 128)
# every (|A| max, |B| max, K) family the GPU module uses: K-tiles of 64 / 128 times 1..9, the ragged K of the older
# kernel, the reduction lengths of the dual and dispatcher cases
K_USED = sorted(set([64 * n for n in range(1, 10)] + [128 * n for n in range(1, 10)] + [72, 192, 256, 320, 384, 512,
                                                                                         768, 1024]))
RANGES_USED = [(A_MAX, B_MAX), (UNIT_MAX, UNIT_MAX)]


def worst_sum(K: int, amax: int = A_MAX, bmax: int = B_MAX) -> int:
    """Largest |value| any epilogue can produce: the product sum plus bias, residual and initial C."""
    return amax * bmax * K + BIAS_MAX + 2 * ADD_MAX


def ints(shape, lo: int, hi: int, seed: int, device="cpu") -> torch.Tensor:
    """fp32 tensor of integers in [lo, hi] (inclusive), reproducible per (seed, device type)."""
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randint(lo, hi + 1, tuple(shape), device=device, generator=g).float()


def exact_mm(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a @ b in float64, returned as fp32 (exact for the integer operands above)."""
    return (a.double() @ b.double()).float()


_C = math.sqrt(2.0 / math.pi)


def gelu64(x: torch.Tensor, erf: bool) -> torch.Tensor:
    x = x.double()
    if erf:
        return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    return 0.5 * x * (1.0 + torch.tanh(_C * (x + 0.044715 * x ** 3)))


def dgelu64(x: torch.Tensor, erf: bool) -> torch.Tensor:
    x = x.double()
    if erf:
        return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    t = torch.tanh(_C * (x + 0.044715 * x ** 3))
    return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * _C * (1.0 + 3 * 0.044715 * x * x)


# ------------------------------------------------------------------------------ comparators: bool masks of bad elements
def bad_bits(got: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """Elements of ``got`` whose bit pattern differs from ``ref``'s (same dtype and shape; NaN == NaN bitwise)."""
    assert got.dtype == ref.dtype and got.shape == ref.shape, (got.dtype, ref.dtype, got.shape, ref.shape)
    it = {4: torch.int32, 2: torch.int16}[got.element_size()]
    return got.contiguous().view(it) != ref.contiguous().view(it)


def bad_f32(got: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """fp32 epilogues: bitwise against the exact result."""
    assert got.dtype == torch.float32
    return bad_bits(got, ref.float())


def bad_bf16(got: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """bf16 epilogues: bitwise against the exact result rounded once."""
    assert got.dtype == torch.bfloat16
    return bad_bits(got, ref.float().bfloat16())


def bad_gelu(got: torch.Tensor, pre: torch.Tensor, erf: bool) -> torch.Tensor:
    """GELU output against the float64 GELU of the exact pre-activation: |got - ref| <= 2^-7 |ref| + 2^-14 -- two bf16
    ulps (2^-8 each: the output rounding and one more for the kernel's fast exp / rcp) plus 8 fp32 ulps of
    ``1 + tanh`` (8 * 2^-24 * |x| / 2 <= 2^-14 for |x| <= 256)."""
    ref = gelu64(pre, erf)
    return ~((got.double() - ref).abs() <= 2.0 ** -7 * ref.abs() + 2.0 ** -14)


def bad_dgelu(got: torch.Tensor, s: torch.Tensor, pre: torch.Tensor, erf: bool) -> torch.Tensor:
    """DGELU output ``s * gelu'(pre)`` (``s`` the exact integer sum, ``pre`` the saved bf16 pre-activation) against
    float64: |got - ref| <= 2^-7 |ref| + 2^-14 max(1, |s|)."""
    ref = s.double() * dgelu64(pre, erf)
    return ~((got.double() - ref).abs() <= 2.0 ** -7 * ref.abs() + 2.0 ** -14 * s.double().abs().clamp(min=1.0))


def norm_ratio(got: torch.Tensor, ref: torch.Tensor) -> float:
    """The criterion of the older tolerance tests: ||got - ref|| / ||ref|| (they pass below 1e-2)."""
    return ((got.double() - ref.double()).norm() / ref.double().norm()).item()


# ------------------------------------------------------------------------------ padded buffers
F32_FILL = float("nan")  # prefill of fp32 outputs and of every operand's padding
BF16_FILL = -23168.0  # sentinel prefill of bf16 outputs (exact in bf16, outside every result's range)


def padded(x: torch.Tensor, ld: int, dtype=None, fill=F32_FILL) -> torch.Tensor:
    """[rows][ld] buffer holding ``x`` in its first columns and ``fill`` in the padding."""
    rows, cols = x.shape
    assert ld >= cols
    buf = torch.full((rows, ld), fill, dtype=dtype or x.dtype, device=x.device)
    buf[:, :cols] = x
    return buf


def out_buffer(rows: int, cols: int, ld: int, dtype, device, init=None):
    """Output buffer and its prefill: NaN (fp32) / the sentinel (bf16) everywhere, ``init`` (accumulate epilogues) in
    the first ``cols`` columns.  Returns (buffer, copy of the prefill)."""
    buf = torch.full((rows, ld), F32_FILL if dtype == torch.float32 else BF16_FILL, dtype=dtype, device=device)
    if init is not None:
        buf[:, :cols] = init
    return buf, buf.clone()


def padding_touched(buf: torch.Tensor, prefill: torch.Tensor, cols: int) -> int:
    """Number of padding elements (columns >= ``cols``) that no longer hold their prefill bits."""
    return int(bad_bits(buf[:, cols:], prefill[:, cols:]).sum())


# ------------------------------------------------------------------------------ perturbations a comparator must flag
def perturbations(a: torch.Tensor, b: torch.Tensor, bias: torch.Tensor, tile=(64, 64), at=None) -> dict:
    """Four wrong versions of ``a @ b + bias`` (the exact fp32 result): name -> tensor.

    * ``one_off``: one element (``at``, default the one of smallest magnitude) off by 1;
    * ``tiles_swapped``: output tiles (0, 0) and (1, 1) exchanged;
    * ``bias_shifted``: inside one 16 x 16 block, column c gets the bias of column c + 1;
    * ``k_slice_missing``: one 16 x 16 block lacks the products of one 32-deep K slice."""
    prod = exact_mm(a, b)
    ref = prod + bias
    bm, bn = tile
    out = {}
    p = ref.clone()
    if at is None:
        at = divmod(int(ref.abs().argmin()), ref.shape[1])
    p[at] += 1.0
    out["one_off"] = p
    p = ref.clone()
    p[:bm, :bn] = ref[bm:2 * bm, bn:2 * bn]
    p[bm:2 * bm, bn:2 * bn] = ref[:bm, :bn]
    out["tiles_swapped"] = p
    p = ref.clone()
    p[16:32, 32:48] = prod[16:32, 32:48] + bias[33:49]
    out["bias_shifted"] = p
    p = ref.clone()
    p[32:48, 16:32] -= exact_mm(a[32:48, 32:64], b[32:64, 16:32])
    out["k_slice_missing"] = p
    for name, t in out.items():
        assert not torch.equal(t, ref), name
    return out
