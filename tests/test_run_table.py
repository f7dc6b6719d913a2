"""The host side of a run table (csrc/run_table.hpp): tile index, array positions, appended words."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "bin", "run_table_test")


def test_run_table_builder_without_a_device():
    """first_tile[], the tile total and the `uniform` shortcut against a plain loop, every tile located by the division and by
    the binary search, for single / equal / shorter-last / longer-last / unequal / zero-row / empty / too-long runs at 64- and
    2048-row tiles; the named array positions, the coding arrays, appended words, the CASE run's index-only form."""
    if not os.path.exists(BIN):
        subprocess.run(["make", "-C", os.path.join(ROOT, "quickstep_amd", "host")], check=True)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "[  PASSED  ]" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
