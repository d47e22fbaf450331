"""scripts/bench_attn_f32.py: the per-call cost of fp32 attention forward + backward.  On the CPU the tool runs eagerly;
what it times must be attention -- its torch candidate's z, dq, dk, dv stay inside the fp32 bounds of
tests/attn_f32_util.py -- at the three shapes of the fp32 models."""
import importlib.util
import os

import pytest

import attn_f32_util as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("bench_attn_f32", os.path.join(ROOT, "scripts", "bench_attn_f32.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_shapes_are_those_of_the_fp32_models():
    T = _tool()
    assert [s[1:] for s in T.SHAPES] == [(256, 16, 4, 16), (512, 16, 4, 16), (256, 16, 12, 64)]
    assert "torch" in T.CANDIDATES and T.parse([]).inner == 20 and T.parse(["--device", "cpu"]).device == "cpu"


def test_the_timed_step_is_attention_forward_and_backward():
    T = _tool()
    B, S, H, dh = 3, 17, 3, 16
    scale = dh ** -0.5
    leaves, do = T.operands(B, S, H, dh, "cpu", seed=4)
    r = T.measure(T.CANDIDATES, leaves, do, True, scale, inner=2, rounds=3)["torch"]
    assert 0 < r["min_us"] <= r["median_us"]
    q, k, v = (t.detach() for t in leaves)
    ref = A.reference(q, k, v, do, True, scale)
    for n, got in zip(("z", "dq", "dk", "dv"), r["out"]):
        err = (got.double() - ref[n]).abs()
        assert bool((err <= 0.25 * ref["tol_" + n]).all()), n


def test_table_has_a_row_per_shape_and_candidate():
    T = _tool()
    lines = T.table("cpu", 1, 2, shapes=(("tiny", 2, 5, 2, 8),))
    assert len(lines) == 3 and lines[2].split()[:6] == ["tiny", "2", "5", "2", "8", "torch"]
    assert float(lines[2].split()[-2]) == 1.0  # the first candidate is the yardstick of the ratio column


@pytest.mark.gpu
def test_captured_graphs_time_the_same_attention():
    """The GPU path: each candidate's forward + backward captured once and replayed; the replayed outputs are
    attention within the same quarter of the bounds (an fp32 torch implementation uses a few hundredths)."""
    T = _tool()
    B, S, H, dh = 3, 17, 3, 16
    scale = dh ** -0.5
    leaves, do = T.operands(B, S, H, dh, "cuda", seed=4)
    r = T.measure(T.CANDIDATES, leaves, do, True, scale, inner=2, rounds=3)["torch"]
    assert 0 < r["min_us"] <= r["median_us"]
    q, k, v = (t.detach().cpu() for t in leaves)
    ref = A.reference(q, k, v, do.cpu(), True, scale)
    for n, got in zip(("z", "dq", "dk", "dv"), r["out"]):
        err = (got.double().cpu() - ref[n]).abs()
        assert bool((err <= 0.25 * ref["tol_" + n]).all()), n
