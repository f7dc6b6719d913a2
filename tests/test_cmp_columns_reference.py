"""CPU: the two restatements of qsx_select_cmp_columns_blocks in tests/cmp_columns_reference.py agree with each other, with
the oracle's qso_select_cmp_columns where both operands share a type, and with a table of pairs that pins the usual
arithmetic conversions (what numpy's own mixed comparison would get wrong)."""
import numpy as np
import pytest

import cmp_columns_reference as R
from quickstep_amd import types as T

# values every numeric type can hold exactly, around which every op has both outcomes; each type adds its own edges
INT_EDGES = [0, 1, -1, 2, 16777216, 16777217, -16777217, 2**31 - 1, -2**31]
LONG_EDGES = INT_EDGES + [4294967295, 2**53, 2**53 + 1, -(2**53) - 1, 2**60 + 2**36 + 1, 2**60 + 2**36, 2**63 - 1, -2**63]
FLOAT_EDGES = [0.0, -0.0, 1.0, -1.0, 2.0, 16777216.0, -16777216.0, 2.0**31, -2.0**31, 2.0**53, 2.0**60, 2.0**60 + 2.0**37, 2.0**63,
               float("nan"), float("inf"), float("-inf"), 0.5]
DOUBLE_EDGES = FLOAT_EDGES + [16777217.0, 2.0**53 + 2.0, 4294967295.0, 0.1]
EDGES = {T.INT: INT_EDGES, T.LONG: LONG_EDGES, T.FLOAT: FLOAT_EDGES, T.DOUBLE: DOUBLE_EDGES}


def cross(lhs_type, rhs_type):
    """Every edge value of the one type against every edge value of the other, as two plain operands."""
    a = np.array(EDGES[lhs_type], dtype=R.NP_DTYPE[lhs_type])
    b = np.array(EDGES[rhs_type], dtype=R.NP_DTYPE[rhs_type])
    return R.Operand(lhs_type, np.repeat(a, b.size)), R.Operand(rhs_type, np.tile(b, a.size))


@pytest.mark.parametrize("lhs_type", R.NUMERIC)
@pytest.mark.parametrize("rhs_type", R.NUMERIC)
def test_numpy_and_row_forms_agree_on_every_pair_of_types(lhs_type, rhs_type):
    lhs, rhs = cross(lhs_type, rhs_type)
    for op in R.OPS:
        got, want = R.compare_numpy(lhs, rhs, op), R.compare_rows(lhs, rhs, op)
        assert np.array_equal(got, want), (lhs_type, rhs_type, op, np.flatnonzero(got != want)[:5])
        assert got.any() and not got.all(), "every op must have both outcomes on the edge values"


def some_dates(rng, n):
    years = rng.integers(1992, 1995, size=n)
    return np.array([T.date_raw(y, m, d, p) for y, m, d, p in zip(years, rng.integers(1, 4, size=n), rng.integers(1, 4, size=n),
                                                                  rng.integers(0, 1 << 16, size=n))], dtype=np.int64)


def test_dates_compare_by_year_month_day_in_both_forms():
    rng = np.random.default_rng(5)
    lhs, rhs = R.Operand(T.DATE, some_dates(rng, 400)), R.Operand(T.DATE, some_dates(rng, 400))
    for op in R.OPS:
        got = R.compare_numpy(lhs, rhs, op)
        assert np.array_equal(got, R.compare_rows(lhs, rhs, op))
        assert got.any() and not got.all()


@pytest.mark.parametrize("qtype", R.NUMERIC + (T.DATE,))
def test_equal_types_match_the_oracle(oracle, qtype):
    rng = np.random.default_rng(11)
    if qtype == T.DATE:
        a, b = some_dates(rng, 333), some_dates(rng, 333)
    else:
        edges = np.array(EDGES[qtype], dtype=R.NP_DTYPE[qtype])
        a, b = rng.choice(edges, size=333), rng.choice(edges, size=333)
    for op in R.OPS:
        want = oracle.select_cmp_columns(np.ascontiguousarray(a), np.ascontiguousarray(b), op, qt=qtype)
        got = R.bitmap_from_bools(R.compare_numpy(R.Operand(qtype, a), R.Operand(qtype, b), op))
        assert np.array_equal(got, want[: got.size]), (qtype, op)


def one(lhs_type, lhs_value, rhs_type, rhs_value, op):
    lhs = R.Operand(lhs_type, np.array([lhs_value], dtype=R.NP_DTYPE[lhs_type]))
    rhs = R.Operand(rhs_type, np.array([rhs_value], dtype=R.NP_DTYPE[rhs_type]))
    got = bool(R.compare_numpy(lhs, rhs, op)[0])
    assert got == bool(R.compare_rows(lhs, rhs, op)[0])
    return got


def test_the_table_of_pairs():
    assert one(T.INT, 16777217, T.FLOAT, 16777216.0, T.EQ)              # compared in float: 2^24 + 1 rounds to 2^24
    assert one(T.LONG, 2**53 + 1, T.DOUBLE, 2.0**53, T.EQ)              # compared in double
    assert one(T.LONG, 2**53 + 1, T.FLOAT, 2.0**53, T.EQ)               # compared in float, not in double as numpy would
    assert not one(T.INT, -1, T.LONG, 4294967295, T.EQ)                 # compared in int64: no wrap to unsigned
    assert one(T.INT, -1, T.LONG, 4294967295, T.LT)
    assert one(T.LONG, 2**60 + 2**36 + 1, T.FLOAT, 2.0**60 + 2.0**37, T.EQ)   # one rounding (through a double it would be 2^60)
    nan = float("nan")
    for other_type, other in ((T.INT, 3), (T.LONG, -7), (T.FLOAT, 1.5), (T.DOUBLE, nan), (T.FLOAT, nan)):
        for nan_type in (T.FLOAT, T.DOUBLE):
            for op in R.OPS:
                assert one(nan_type, nan, other_type, other, op) == (op == T.NE)
                assert one(other_type, other, nan_type, nan, op) == (op == T.NE)
    for qtype in (T.FLOAT, T.DOUBLE):
        assert one(qtype, -0.0, qtype, 0.0, T.EQ) and not one(qtype, -0.0, qtype, 0.0, T.LT)
    assert one(T.DATE, T.date_raw(1994, 2, 28, 0), T.DATE, T.date_raw(1994, 2, 28, 0xBEEF), T.EQ)   # padding bytes do not count
    assert one(T.DATE, T.date_raw(1994, 2, 28, 0xFFFF), T.DATE, T.date_raw(1994, 3, 1, 0), T.LT)
    assert one(T.DATE, T.date_raw(-5, 1, 1), T.DATE, T.date_raw(4, 1, 1), T.LT)                      # the year is signed


def test_codes_stand_for_their_values_and_the_null_code_is_false_under_every_op():
    dictionary = np.array([-9, 0, 5, 16777217], dtype=np.int64)
    codes = np.array([0, 1, 2, 3, 4, 255, 2], dtype=np.uint8)          # 4 and 255 are past the dictionary: NULL
    lhs = R.Operand(T.LONG, codes, width=1, dictionary=dictionary)
    rhs = R.Operand(T.INT, np.array([5, 5, 5, 5, 5, 5, 70000], dtype=np.uint32), width=4)   # truncated values
    plain_lhs = R.Operand(T.LONG, np.array([-9, 0, 5, 16777217, 0, 0, 5], dtype=np.int64))
    plain_rhs = R.Operand(T.INT, np.array([5, 5, 5, 5, 5, 5, 70000], dtype=np.int32))
    null = np.array([0, 0, 0, 0, 1, 1, 0], dtype=bool)
    for op in R.OPS:
        got = R.compare_numpy(lhs, rhs, op)
        assert np.array_equal(got, R.compare_rows(lhs, rhs, op))
        assert np.array_equal(got, R.compare_numpy(plain_lhs, plain_rhs, op) & ~null)
        assert not got[null].any()
        assert not R.compare_numpy(rhs, lhs, op)[null].any() and not R.compare_rows(rhs, lhs, op)[null].any()   # NULL on the right
    # a truncated value is widened without sign
    assert R.Operand(T.LONG, np.array([0xFFFF], dtype=np.uint16), width=2).values()[0][0] == 65535
    # a date dictionary holds 8-byte DateLit words
    dates = np.array([T.date_raw(1993, 1, 1), T.date_raw(1994, 6, 30, 7)], dtype=np.int64)
    a = R.Operand(T.DATE, np.array([1, 0, 2], dtype=np.uint16), width=2, dictionary=dates)
    b = R.Operand(T.DATE, np.array([T.date_raw(1994, 6, 30), T.date_raw(1994, 6, 30), T.date_raw(1994, 6, 30)], dtype=np.int64))
    assert R.compare_numpy(a, b, T.EQ).tolist() == [True, False, False] and R.compare_rows(a, b, T.NE).tolist() == [False, True, False]


def test_bitmaps_are_msb_first_and_zero_behind_the_rows():
    bools = np.zeros(70, dtype=bool)
    bools[[0, 63, 64, 69]] = True
    words = R.bitmap_from_bools(bools)
    assert words.tolist() == [(1 << 63) | 1, (1 << 63) | (1 << 58)]
    assert R.bitmap_from_bools(bools, np.array([1, 1 << 63], dtype=np.uint64)).tolist() == [1, 1 << 63]
    assert R.compare_class(T.CHAR, T.CHAR) is None and R.compare_class(T.DATE, T.LONG) is None
