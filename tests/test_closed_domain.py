"""The guarantee behind closed aggregation states (csrc/aggregate.hip closed_key_bits / hash_table_cap), on the CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "bin", "closed_domain_test")


def test_whole_key_domain_never_exhausts_a_probe_sequence():
    """For every b in 1..16 all 2^b key codes are inserted, by the library's own code_slot, into a table of the capacity a
    closed state over b bits gets: the longest circular run of occupied slots stays below kGlobalMaxProbes, so no subset of
    the domain can make global_find_or_insert give up.  Which plans are closed (one or two CHAR(1) keys, one CHAR(2); not
    three CHAR(1), not an INT) and the capacity their states get come from the library as well."""
    if not os.path.exists(BIN):
        subprocess.run(["make", "-C", os.path.join(ROOT, "quickstep_amd", "host")], check=True)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "[  PASSED  ]" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
