"""ComparisonID::kLike / kNotLike of the C++ host layer (quickstep_amd/host): SelectOperator over plain, dictionary-coded,
nullable and sorted CHAR(25) attributes, per block and over runs; an aggregation whose predicate holds a LIKE term; a join
with a LIKE residual on a build-side attribute; LIKE on an INT attribute and a 65-byte pattern refused with
QSX_ERR_UNSUPPORTED.  The C++ test is tests/cpp/like_operator_test.cpp; pytest builds it (if needed) and runs it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINARY = os.path.join(ROOT, "tests", "cpp", "bin", "like_operator_test")


def _ensure_built():
    if not os.path.exists(BINARY):
        subprocess.run(["make", "-C", os.path.join(ROOT, "quickstep_amd", "host")], check=True)


def test_like_operators_refuse_to_run_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    _ensure_built()
    r = subprocess.run([BINARY], capture_output=True, text=True)
    assert r.returncode == 2 and "no CPU fallback" in r.stderr


@pytest.mark.gpu
def test_like_and_not_like_through_the_operators():
    _ensure_built()
    r = subprocess.run([BINARY], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "[  PASSED  ]" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
