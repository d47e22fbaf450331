"""Kernels that only a launch-time environment variable selects (read once per process, so each needs a fresh one):
``IIT_LN_PART_R`` = 2 / 4 (``ln_bwd_part_kernel<*, *, 2 / 4>``), ``IIT_ADAM_NT`` = 0 (``adam_span_kernel<false,
4>``), ``IIT_ADAM_UNROLL`` = 1 / 2 (``adam_span_kernel<true, 1 / 2>``), ``IIT_EMBED_BWD_POS`` = 0 (the token-major
``embed_bwd_kernel``) and ``IIT_LLAMA_VEC`` = 0 (the scalar ``rms_dw_kernel``, and the per-pair ``rotary_kernel`` at
the shapes the vector kernel otherwise takes), and ``IIT_BN_ROWS`` = 0 with ``IIT_BN_GRID`` = 64 (the fused BatchNorm's
grid sized by a target of 64 workgroups instead of 8 rows per thread group, so small shapes take many rows per thread
through the unroll-by-4 loops and their remainders).  Five child processes, one at a time: the first three each with one
layer-norm and / or one Adam variable set (the third the embedding variable too) run the fused layer-norm backward and
row-select cases of tests/test_ln_exact.py, the single-step cases of tests/test_adam_exact.py and, in the third, the
embedding backward cases of tests/test_embed_exact.py; the fourth, with ``IIT_LLAMA_VEC=0``, runs the ``dw`` cases of
tests/test_rms_exact.py and all of tests/test_rotary_exact.py; the fifth, with ``IIT_BN_ROWS=0 IIT_BN_GRID=64``, runs
the statistics and backward cases of tests/test_bn_exact.py (``test_bn_stats``, the grid-cap case included: 257 rows
per thread there), whose bounds follow the variables through ``bn_exact_util.bn_plan``.  Each runs under its own time
limit; the loop ends at the first child that does not exit with 0, so nothing more starts on the GPU after a fault, an
abort or a timeout.  ``adam_span_kernel<false, 1 / 2>`` (both variables at once) is run by no test.

Measured on an MI355X: one case, passed, none skipped, 35.9 s -- five children of about 7 s each, most of it the start
of a fresh process (interpreter, torch, the first launch); the children select 164, 164, 94 (26 Adam and 68 embedding
backward cases), 126 (80 RMSNorm ``dw`` and 46 rotary cases in the fourth) and 22 cases (the 20 statistics ids and the
two grid-cap ids of tests/test_bn_exact.py in the fifth, 8.0 s on its own).
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LN = "(test_ln_bwd and not xh16) or row_select"
ADAM = "test_adam_step or guard or non_finite"
EMBED = "test_embed_bwd"
FILES = ["test_ln_exact.py", "test_adam_exact.py"]
VARIANTS = [({"IIT_LN_PART_R": "2", "IIT_ADAM_NT": "0"}, FILES, f"({LN}) or {ADAM}"),
            ({"IIT_LN_PART_R": "4", "IIT_ADAM_UNROLL": "1"}, FILES, f"({LN}) or {ADAM}"),
            ({"IIT_ADAM_UNROLL": "2", "IIT_EMBED_BWD_POS": "0"}, FILES + ["test_embed_exact.py"], f"{ADAM} or {EMBED}"),
            ({"IIT_LLAMA_VEC": "0"}, ["test_rms_exact.py", "test_rotary_exact.py"], "test_rms_dw or test_rotary"),
            ({"IIT_BN_ROWS": "0", "IIT_BN_GRID": "64"}, ["test_bn_exact.py"], "test_bn_stats")]
LIMIT_S = 240


def test_launch_time_variants():
    for env, files, expr in VARIANTS:
        cmd = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, "-m", "pytest", "-q", "-x", "-p",
               "no:cacheprovider"] + [os.path.join(HERE, f) for f in files] + ["-k", expr]
        res = subprocess.run(cmd, env=dict(os.environ, **env), cwd=os.path.dirname(HERE), stdout=subprocess.PIPE,
                             stderr=subprocess.STDOUT, text=True)
        tail = "\n".join(res.stdout.splitlines()[-25:])
        assert res.returncode == 0, f"{env}: exit status {res.returncode} (no further variant started)\n{tail}"
        assert " passed" in tail and "skipped" not in tail and "failed" not in tail, f"{env}\n{tail}"
