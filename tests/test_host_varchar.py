"""VARCHAR attributes through the C++ host layer (quickstep_amd/host): CompressedColumnStore images with VARCHAR(25) and a
nullable VARCHAR(55) behind variable-length dictionaries, written as the reference's builder leaves them and adopted in place;
SelectOperator with LIKE, NOT LIKE and the six comparisons against a string literal, per block and over runs; a predicate tree
with a VARCHAR LIKE leaf; projection of VARCHAR attributes; GROUP BY a VARCHAR(25); the refused uses (IN lists, join and ORDER BY
keys, aggregate arguments, attribute-vs-attribute comparisons, SUBSTRING, loadBlock with compress, basic column store images)
with QSX_ERR_UNSUPPORTED and malformed dictionaries with QSX_ERR_INVALID_ARGUMENT.  The C++ test is
tests/cpp/varchar_operator_test.cpp; pytest builds it (if needed) and runs it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINARY = os.path.join(ROOT, "tests", "cpp", "bin", "varchar_operator_test")


def _ensure_built():
    if not os.path.exists(BINARY):
        subprocess.run(["make", "-C", os.path.join(ROOT, "quickstep_amd", "host")], check=True)


def test_varchar_operators_refuse_to_run_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    _ensure_built()
    r = subprocess.run([BINARY], capture_output=True, text=True)
    assert r.returncode == 2 and "no CPU fallback" in r.stderr


@pytest.mark.gpu
def test_varchar_attributes_through_the_operators():
    _ensure_built()
    r = subprocess.run([BINARY], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "[  PASSED  ]" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
