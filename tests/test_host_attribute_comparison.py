"""Comparisons of two attributes of one relation through the C++ host layer (quickstep_amd/host): Q12's conjunction through a
SelectOperator per block and over a run (which must stay ONE run), INT against LONG and LONG against DOUBLE, a nullable
attribute on either side, COUNT(*) / SUM and a CASE WHEN under such a predicate, plain and compressed blocks (dictionary-coded
dates, an INT attribute truncated in some blocks only), and the refusals.  The C++ test is
tests/cpp/attribute_comparison_operator_test.cpp; pytest builds it (if needed) and runs it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINARY = os.path.join(ROOT, "tests", "cpp", "bin", "attribute_comparison_operator_test")


def _ensure_built():
    if not os.path.exists(BINARY):
        subprocess.run(["make", "-C", os.path.join(ROOT, "quickstep_amd", "host")], check=True)


def test_attribute_comparison_operators_refuse_to_run_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    _ensure_built()
    r = subprocess.run([BINARY], capture_output=True, text=True)
    assert r.returncode == 2 and "no CPU fallback" in r.stderr


@pytest.mark.gpu
def test_attribute_comparisons_through_the_operators():
    _ensure_built()
    r = subprocess.run([BINARY], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "[  PASSED  ]" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
