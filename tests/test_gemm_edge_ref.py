"""CPU side of the ragged-N GEMM tests: the exported edge plan (the kernels' own granule arithmetic, run on the host)
for every shape the GPU tests use, and the comparator of tests/gemm_edge_util.py against wrong results it must flag."""
import pytest
import torch

import gemm_edge_util as E
from iit_amd.ops import hip_kernels as HK


@pytest.fixture(scope="module")
def K():
    HK.lib()
    return HK


@pytest.mark.parametrize("tile", sorted(E.EDGE_TILES))
def test_edge_plan(K, tile):
    bm, bn = E.EDGE_TILES[tile]
    for M, N, Kd in list(E.edge_shapes(tile)) + [(256, 50257, 768), (768, 50257, 256)]:
        ld = E.pad8(N)
        for rows, elem in ((Kd, 2), (M, 4), (M, 2)):  # B (bf16, K rows), C (fp32 / bf16, M rows)
            p = K.gemm_edge_plan(rows, N, ld, elem, tile)
            assert p is not None
            tiles_n = (N + bn - 1) // bn
            assert p["tiles_n"] == tiles_n
            assert p["used"] == (N + 7) // 8 and p["used"] + p["redirected"] == tiles_n * bn // 8
            assert p["straddle"] == N % 8
            # nothing is touched beyond the last row's pad8(N) columns -- the last valid byte of the operand
            assert p["last_byte"] == p["valid_bytes"] == ((rows - 1) * ld + E.pad8(N)) * elem
    assert K.gemm_edge_plan(64, 129, 128, 2, tile) is None  # rows shorter than pad8(N)
    assert K.gemm_edge_plan(64, 129, 136, 2, 9) is None  # not an edge tile


def _wrong(c, what):
    """``c`` with the exact outputs in place, then one defect."""
    c["C"].copy_(c["exp"])
    c["bsum"].copy_(c["bsum_exp"])
    c["gsq"].zero_()
    c["gsq"][3] = c["gsq_exp"]
    M, N = c["M"], c["N"]
    if what == "edge_column":  # the last valid column of one row off by one
        c["C"][5, N - 1] += 1.0
    elif what == "unmasked_gsq":  # a pad column's NaN square summed in
        c["gsq"][7] = float("nan")
    elif what == "leaked_pad_nan":  # a B pad column reached a stored column
        c["C"][M - 1, N - 1] = float("nan")
    elif what == "pad_written":  # a store beyond column N
        c["Cbuf"][N] = 0.0
    elif what == "bsum_beyond":  # a column sum beyond N
        c["bsum_buf"][N] = 1.0
    return c


def test_comparator_flags_edge_defects():
    c = E.make_case(E.MODE_3, E.EPI_F32_STORE, 128, 129, 128, 3, "cpu")
    assert E.check_case(_wrong(c, "none")) == []
    for what in ("edge_column", "unmasked_gsq", "leaked_pad_nan", "pad_written", "bsum_beyond"):
        c = E.make_case(E.MODE_3, E.EPI_F32_STORE, 128, 129, 128, 3, "cpu")
        assert len(E.check_case(_wrong(c, what))) == 1, what
    # the bf16 epilogue: compared with the exact result rounded once
    c = E.make_case(E.MODE_BKM, E.EPI_BF16, 128, 135, 128, 4, "cpu")
    c["C"].copy_(c["exp"])
    assert E.check_case(c) == []
    c["C"][0, 134] = c["C"][0, 134] + 8.0
    assert len(E.check_case(c)) == 1
