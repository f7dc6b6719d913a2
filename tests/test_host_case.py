"""Scalar::kCaseExpression of the C++ host layer (quickstep_amd/host): a Select projecting a DOUBLE CASE and a nullable INT
CASE; SUM(CASE WHEN p_type LIKE 'PROMO%' THEN x * (1 - y) ELSE 0 END) per block and over a run (which must stay on the run path);
two WHENs with CHAR(15) equality summed as LONG under integer_argument_arithmetic with a CHAR(10) group-by key; the reference's
SUM(CASE WHEN i < 4 THEN i ELSE i * i END) = 47; COUNT / AVG / SUM over a CASE with NULLs, an all-NULL group finalizing as NULL;
nested CASE, CHAR results and DISTINCT refused with QSX_ERR_UNSUPPORTED.  The C++ test is tests/cpp/case_operator_test.cpp;
pytest builds it (if needed) and runs it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINARY = os.path.join(ROOT, "tests", "cpp", "bin", "case_operator_test")


def _ensure_built():
    if not os.path.exists(BINARY):
        subprocess.run(["make", "-C", os.path.join(ROOT, "quickstep_amd", "host")], check=True)


def test_case_operators_refuse_to_run_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    _ensure_built()
    r = subprocess.run([BINARY], capture_output=True, text=True)
    assert r.returncode == 2 and "no CPU fallback" in r.stderr


@pytest.mark.gpu
def test_case_expressions_through_the_operators():
    _ensure_built()
    r = subprocess.run([BINARY], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "[  PASSED  ]" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
