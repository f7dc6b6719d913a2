"""Scalar::kUnaryExpression of the C++ host layer (quickstep_amd/host): a Select projecting EXTRACT(YEAR), EXTRACT(MONTH),
SUBSTRING and EXTRACT(YEAR) * 100 + EXTRACT(MONTH) over a nullable date; Q8's shape SUM(CASE ..), SUM(volume) GROUP BY
EXTRACT(YEAR FROM o_orderdate) through AggregationStateSpec::group_by_scalars per block, over a run (which must stay on the run
path), as Select -> Aggregation, with the date dictionary-compressed (extracted from the dictionary, never decoded) and under
COLLISION_FREE; Q22's shape GROUP BY SUBSTRING(c_phone, 0, m) packed (m = 2) and interned (m = 3); NULL operands as NULL keys;
every refusal.  The C++ test is tests/cpp/unary_operator_test.cpp; pytest builds it (if needed) and runs it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINARY = os.path.join(ROOT, "tests", "cpp", "bin", "unary_operator_test")


def _ensure_built():
    if not os.path.exists(BINARY):
        subprocess.run(["make", "-C", os.path.join(ROOT, "quickstep_amd", "host")], check=True)


def test_unary_operators_refuse_to_run_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    _ensure_built()
    r = subprocess.run([BINARY], capture_output=True, text=True)
    assert r.returncode == 2 and "no CPU fallback" in r.stderr


@pytest.mark.gpu
def test_unary_expressions_through_the_operators():
    _ensure_built()
    r = subprocess.run([BINARY], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "[  PASSED  ]" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
