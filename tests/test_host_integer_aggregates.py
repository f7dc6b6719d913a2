"""AggregationStateSpec::integer_argument_arithmetic of the C++ host layer (quickstep_amd/host): aggregates over integer-typed
scalar expressions evaluated in integer arithmetic and typed like the reference's catalog types them.  The C++ test is
tests/cpp/integer_aggregate_operator_test.cpp; pytest builds it (if needed) and runs it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINARY = os.path.join(ROOT, "tests", "cpp", "bin", "integer_aggregate_operator_test")


def _ensure_built():
    if not os.path.exists(BINARY):
        subprocess.run(["make", "-C", os.path.join(ROOT, "quickstep_amd", "host")], check=True)


def test_integer_aggregate_operators_refuse_to_run_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    _ensure_built()
    r = subprocess.run([BINARY], capture_output=True, text=True)
    assert r.returncode == 2 and "no CPU fallback" in r.stderr


@pytest.mark.gpu
def test_integer_aggregate_arguments_through_the_operators():
    """SUM(x + x), SUM(x * 5000000000), MIN(x - 7), AVG(x * x), SUM(w + x) grouped by z under Foreman + Workers and the
    synchronous driver, work orders per block and per run of blocks, all three grouped strategies: LONG / INT result attributes
    equal to integer arithmetic with the flag, DOUBLE ones without it."""
    _ensure_built()
    r = subprocess.run([BINARY], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "[  PASSED  ]" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
