"""CPU checks of tests/exact_reference.py: the generators keep their invariants at the largest sizes the GPU tests use, the
references equal math.fsum and Fraction, the family-B bound stays below the smallest term at every group size the GPU tests use,
and the integer families reach the ranges they claim."""
import math
from fractions import Fraction

import numpy as np
import pytest

import exact_reference as R
from exact_reference import LAYOUTS        # (rows, groups, order, heavy) of every layout tests/test_gpu_agg_exact.py draws


def test_gamma_and_unit_roundoff():
    assert R.U == 2.0 ** -53 and 1.0 + R.U == 1.0 and 1.0 + 2 * R.U > 1.0
    assert R.gamma(1) == pytest.approx(R.U, rel=1e-15)
    assert R.gamma(10**6) == pytest.approx(10**6 * R.U / (1 - 10**6 * R.U), rel=1e-15)


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_group_layouts_and_family_invariants_at_every_gpu_size(layout):
    """Every family's generator on every layout the GPU file uses: their own asserts must hold (they raise otherwise)."""
    n, groups, order, heavy = LAYOUTS[layout]
    rng = np.random.default_rng(1)
    gid = R.make_gids(rng, n, groups, order, heavy)
    cnt = np.bincount(gid, minlength=groups)
    assert cnt.min() >= 2 and cnt.sum() == n
    if order == "clustered":
        assert np.all(np.diff(gid) >= 0)
    R.family_a(rng, gid, groups)
    sub = R.family_a_subnormal(rng, gid, groups)
    if cnt.max() >= 8192:
        assert R.subnormal_groups_with_normal_sums(sub, gid, groups).size > 0
    R.family_c(rng, gid, groups)
    R.family_d(rng, gid, groups)


def test_family_a_at_the_largest_group_the_suite_forms():
    """One group of 17 M rows (the largest call of the suite): the Q1 nodes stay exact, sum |t3| 2^13 < 2^53."""
    rng = np.random.default_rng(2)
    n = 17_000_017
    gid = np.zeros(n, dtype=np.int64)
    cols = R.family_a(rng, gid, 1)
    m = R.assert_exact_sums(cols["t3"], 13, gid, 1)
    assert int(np.abs(m).sum()) < 2**53


def test_exact_sums_equal_fsum_and_fraction_on_small_draws():
    rng = np.random.default_rng(3)
    gid = R.make_gids(rng, 5_001, 7)
    a = R.family_a(rng, gid, 7)
    sub = R.family_a_subnormal(rng, gid, 7)
    for x in (a["price"], a["t1"], a["t3"], a["fl"], sub["sd"], sub["sf"]):
        got = R.exact_group_sums(x, gid, 7)
        for g in range(7):
            vals = np.asarray(x, dtype=np.float64)[gid == g]
            assert got[g] == math.fsum(vals) == float(sum(Fraction(float(v)) for v in vals))
        # any order: reversed and sorted partial sums give the same doubles
        for perm in (np.arange(gid.size)[::-1], np.argsort(np.asarray(x, dtype=np.float64))):
            again = np.zeros(7)
            for r in perm:
                again[gid[r]] += float(x[r])
            assert np.array_equal(again, got)
    s = R.exact_group_sums(a["fl"], gid, 7)
    assert np.all(s.astype(np.float32).astype(np.float64) != s)
    b = R.family_b(rng, gid, 7)
    ref = R.family_b_reference(b["t3"], gid, 7)
    for g in range(7):
        assert ref[g] == float(sum(Fraction(float(v)) for v in b["t3"][gid == g]))


def test_family_b_reference_error_is_within_the_bound():
    """The bincount reference (more than 64 groups) against Fraction: within gamma(n_g) S_g, which half of tol_g covers."""
    rng = np.random.default_rng(4)
    gid = R.make_gids(rng, 20_000, 100)
    b = R.family_b(rng, gid, 100)
    tol = R.family_b_tolerance(b["t3"], gid, 100, R.FAMILY_B_ROUNDINGS["t3"])
    ref = R.family_b_reference(b["t3"], gid, 100)
    for g in range(0, 100, 9):
        exact = sum(Fraction(float(v)) for v in b["t3"][gid == g])
        assert abs(Fraction(float(ref[g])) - exact) <= Fraction(float(tol[g])) / 2


@pytest.mark.parametrize("rows", [1_000_000, 3_000_000])
def test_family_b_bound_is_below_the_smallest_term_for_groups_up_to_3m_rows(rows):
    rng = np.random.default_rng(rows)
    gid = np.zeros(rows, dtype=np.int64)
    b = R.family_b(rng, gid, 1)
    for name, k in R.FAMILY_B_ROUNDINGS.items():
        tol = R.family_b_tolerance(b[name], gid, 1, k)            # asserts tol < min |term|
        assert tol[0] > 0


def test_family_b_bound_at_every_gpu_layout():
    for layout, (n, groups, order, heavy) in LAYOUTS.items():
        rng = np.random.default_rng(5)
        gid = R.make_gids(rng, n, groups, order, heavy)
        b = R.family_b(rng, gid, groups)
        for name, k in R.FAMILY_B_ROUNDINGS.items():
            R.family_b_tolerance(b[name], gid, groups, k)


def test_family_b_bound_fails_where_the_issue_says_it_must():
    """10 M rows in one group: the bound exceeds the smallest t3 term (so family-B groups stay at 3 M rows or fewer)."""
    rng = np.random.default_rng(6)
    gid = np.zeros(10_000_000, dtype=np.int64)
    b = R.family_b(rng, gid, 1)
    with pytest.raises(AssertionError):
        R.family_b_tolerance(b["t3"], gid, 1, 4)


def test_integer_families_reach_their_ranges():
    for layout, (n, groups, order, heavy) in LAYOUTS.items():
        rng = np.random.default_rng(7)
        gid = R.make_gids(rng, n, groups, order, heavy)
        c = R.family_c(rng, gid, groups)
        if groups == 1:
            si, sl = R.family_c_sums(c, gid, groups)
            assert abs(sl[0]) > 2**53 and int(float(sl[0])) != sl[0]
            continue
        R.assert_family_c_ranges(c, gid, groups)


def test_int_avg_rule():
    R.assert_int_avg(float(Fraction(7, 3)), 7, 3)
    s = 2**60 + 1
    R.assert_int_avg(float(s) / 3.0, s, 3)
    with pytest.raises(AssertionError):
        R.assert_int_avg(float(Fraction(7, 3)) + 1e-15, 7, 3)


def test_family_d_extremes_and_identity_groups():
    rng = np.random.default_rng(8)
    gid = R.make_gids(rng, 10_000, 40)
    d = R.family_d(rng, gid, 40)
    lo, hi, _ = R.group_min_max(d["l"], gid, 40)
    assert lo[0] == hi[0] == R.INT64_MAX and lo[1] == hi[1] == R.INT64_MIN
    lo, hi, _ = R.group_min_max(d["d"], gid, 40)
    assert lo[0] == np.inf and hi[1] == -np.inf
    assert np.any(d["d"] == 2.0**-1074) and np.any(d["f"] == np.float32(2.0**-149))


def test_generators_refuse_data_that_breaks_their_invariants():
    gid = np.zeros(4, dtype=np.int64)
    with pytest.raises(AssertionError):
        R.assert_exact_sums(np.array([0.5, 0.25, 1.0, 2.0]), 1, gid, 1)              # 0.25 is no multiple of 2^-1
    with pytest.raises(AssertionError):
        R.assert_exact_sums(np.full(4, 2.0**51), 0, gid, 1)                          # sum |x| reaches 2^53
    with pytest.raises(AssertionError):
        R.make_gids(np.random.default_rng(0), 3, 2)                                  # fewer than two rows per group
