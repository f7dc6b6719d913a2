"""GROUP BY CHAR(n) through the C++ host layer (quickstep_amd/host): CHAR(10) / CHAR(15) / CHAR(25) and nullable CHAR(12)
group-by attributes interned into ids on the device, plain and dictionary-coded, per block and over runs, under Foreman + 4
Workers, GENERIC and COMPACT_KEY, a dictionary that has to grow, a partitioned finalize, the sort operators behind the
aggregation; a DISTINCT aggregate beside such a key and an exchange of such a state refused with QSX_ERR_UNSUPPORTED.  The C++
test is tests/cpp/char_group_by_operator_test.cpp; pytest builds it (if needed) and runs it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINARY = os.path.join(ROOT, "tests", "cpp", "bin", "char_group_by_operator_test")


def _ensure_built():
    if not os.path.exists(BINARY):
        subprocess.run(["make", "-C", os.path.join(ROOT, "quickstep_amd", "host")], check=True)


def test_char_group_by_operators_refuse_to_run_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    _ensure_built()
    r = subprocess.run([BINARY], capture_output=True, text=True)
    assert r.returncode == 2 and "no CPU fallback" in r.stderr


@pytest.mark.gpu
def test_group_by_char_keys_through_the_operators():
    _ensure_built()
    r = subprocess.run([BINARY], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "[  PASSED  ]" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
