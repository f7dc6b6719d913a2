"""Predicates over a unary operation in the C++ host layer (quickstep_amd/host): Q22's SUBSTRING(c_phone FROM 1 FOR 2) IN (7
codes) AND c_acctbal > x with the balance as a conjunct and as a leaf, NOT IN over a nullable phone (the NULL rows are selected),
a unary leaf next to a leaf over the attribute itself, EXTRACT(YEAR) = y, a range of two conjuncts, EXTRACT(MONTH) IN (..) - on
plain and dictionary-compressed blocks, per block and over a run (which must stay on the run path); an aggregation whose
predicate holds such terms against exact integer sums; SUM(CASE WHEN EXTRACT(YEAR ..) = y THEN v ELSE 0 END); every refusal with
its status and message.  The C++ test is tests/cpp/unary_predicate_operator_test.cpp; pytest builds it (if needed) and runs it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINARY = os.path.join(ROOT, "tests", "cpp", "bin", "unary_predicate_operator_test")


def _ensure_built():
    if not os.path.exists(BINARY):
        subprocess.run(["make", "-C", os.path.join(ROOT, "quickstep_amd", "host")], check=True)


def test_unary_predicate_operators_refuse_to_run_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    _ensure_built()
    r = subprocess.run([BINARY], capture_output=True, text=True)
    assert r.returncode == 2 and "no CPU fallback" in r.stderr


@pytest.mark.gpu
def test_unary_predicates_through_the_operators():
    _ensure_built()
    r = subprocess.run([BINARY], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "[  PASSED  ]" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
