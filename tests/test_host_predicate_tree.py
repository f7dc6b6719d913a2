"""Predicate trees of the C++ host layer (quickstep_amd/host): a Select with a Q19-shaped OR of three conjunctions, Q12's IN
behind a range on the sort column, Q16's NOT IN with NOT LIKE and <>, NOT over a nullable attribute (the NULL rows are selected)
and an IN list of 40 literals - on plain, compressed, sorted and sorted compressed blocks, per block and over a run (which must
stay on the run path); an aggregation with a tree predicate against exact integer sums; SUM(CASE WHEN a = x OR a = y THEN 1 ELSE
0 END) with one WHEN; the refusals (a join's residual predicate, qsx_agg_config_t.pred); a conjuncts-only predicate against the
same terms as a tree.  The C++ test is tests/cpp/predicate_tree_operator_test.cpp; pytest builds it (if needed) and runs it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINARY = os.path.join(ROOT, "tests", "cpp", "bin", "predicate_tree_operator_test")


def _ensure_built():
    if not os.path.exists(BINARY):
        subprocess.run(["make", "-C", os.path.join(ROOT, "quickstep_amd", "host")], check=True)


def test_predicate_tree_operators_refuse_to_run_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    _ensure_built()
    r = subprocess.run([BINARY], capture_output=True, text=True)
    assert r.returncode == 2 and "no CPU fallback" in r.stderr


@pytest.mark.gpu
def test_predicate_trees_through_the_operators():
    _ensure_built()
    r = subprocess.run([BINARY], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "[  PASSED  ]" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
