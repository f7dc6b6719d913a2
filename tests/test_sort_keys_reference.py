"""CPU: tests/sort_keys_reference.py, the checker of qsx_sort_permutation_keys, pinned three ways: its two forms agree, on
NULL-free plain keys both equal the oracle's comparator sort, and the data of the reference's own unit test
(relational_operators/tests/SortRunGenerationOperator_unittest.cpp) reproduces the expectations of all of that file's NULL cases."""
import itertools

import numpy as np
import pytest

import sort_keys_reference as R
from quickstep_amd import types as T

INT_MIN, INT_MAX = -2**31, 2**31 - 1


def _column(rng, kind, n):
    if kind == "int":
        return rng.integers(-6, 6, size=n).astype(np.int32), T.INT
    if kind == "int extremes":
        return rng.choice(np.array([INT_MIN, -1, 0, 1, INT_MAX], dtype=np.int32), size=n), T.INT
    if kind == "long":
        return rng.choice(np.array([-2**63, -2**40, -1, 0, 3, 2**40, 2**63 - 1], dtype=np.int64), size=n), T.LONG
    if kind == "float":
        return rng.choice(np.array([-1.5, -0.0, 0.0, 1e-30, 2.5, np.inf, -np.inf], dtype=np.float32), size=n), T.FLOAT
    if kind == "double":
        return np.round(rng.normal(size=n), 1) + 0.0 * rng.choice([-1.0, 1.0], size=n), T.DOUBLE
    if kind == "date":
        raw = [T.date_raw(int(y), int(m), int(d), int(p)) for y, m, d, p in
               zip(rng.integers(-3, 4, size=n), rng.integers(1, 4, size=n), rng.integers(1, 4, size=n), rng.integers(0, 65536, size=n))]
        return np.array(raw, dtype=np.int64), T.DATE
    width = int(kind.split()[1])
    return R.random_chars(rng, n, width, alphabet=np.array([1, 65, 66, 127, 128, 255], dtype=np.uint8)), T.CHAR


KINDS = ["int", "int extremes", "long", "float", "double", "date", "char 1", "char 2", "char 7", "char 8", "char 9", "char 25"]


@pytest.mark.parametrize("kind", KINDS)
def test_the_two_forms_agree_on_single_keys(kind):
    rng = np.random.default_rng(len(kind) * 7 + 1)
    for n, fraction, desc, first in itertools.product((0, 1, 2, 65, 300), (0.0, 0.3, 1.0), (False, True), (False, True)):
        values, qt = _column(rng, kind, n)
        nulls = None if fraction == 0.0 else rng.random(n) < fraction
        key = R.Key(values, qt, desc, first, nulls)
        a, b = R.permutation_plain([key]), R.permutation_numpy([key])
        assert np.array_equal(a, b), (kind, n, fraction, desc, first)
        assert sorted(a.tolist()) == list(range(n))


def test_the_two_forms_agree_on_composite_keys():
    rng = np.random.default_rng(11)
    for trial in range(40):
        n = int(rng.integers(1, 400))
        keys = []
        for _ in range(int(rng.integers(2, 5))):
            values, qt = _column(rng, KINDS[int(rng.integers(0, len(KINDS)))], n)
            nulls = rng.random(n) < rng.choice([0.0, 0.2, 0.6]) if rng.random() < 0.7 else None
            keys.append(R.Key(values, qt, bool(rng.integers(0, 2)), bool(rng.integers(0, 2)), nulls))
        assert np.array_equal(R.permutation_plain(keys), R.permutation_numpy(keys)), trial


def test_null_rows_keep_the_order_of_the_less_significant_keys_and_their_bytes_do_not_matter():
    rng = np.random.default_rng(5)
    n = 200
    a, b = rng.integers(0, 3, size=n).astype(np.int32), rng.integers(0, 4, size=n).astype(np.int32)
    nulls = rng.random(n) < 0.5
    garbage = np.where(nulls, rng.integers(-99, 99, size=n), a).astype(np.int32)
    for form in (R.permutation_plain, R.permutation_numpy):
        got = form([R.Key(a, nulls=nulls, nulls_first=True), R.Key(b, descending=True)])
        assert np.array_equal(got, form([R.Key(garbage, nulls=nulls, nulls_first=True), R.Key(b, descending=True)]))
        head = got[:int(nulls.sum())]
        assert nulls[head].all()
        # the NULL rows among themselves: by b DESC, then input order
        assert head.tolist() == sorted(np.flatnonzero(nulls).tolist(), key=lambda r: (-int(b[r]), r))


def test_both_forms_equal_the_oracle_on_null_free_plain_keys(oracle):
    rng = np.random.default_rng(3)
    n = 5000
    cols = [rng.integers(-50, 50, size=n).astype(np.int32), rng.integers(-2**62, 2**62, size=n).astype(np.int64),
            (rng.normal(size=n) * 10).round().astype(np.float32), np.round(rng.normal(size=n), 1),
            rng.choice(np.array([0.0, -0.0, 1.5], dtype=np.float64), size=n), rng.choice(np.frombuffer(b"ANRF\0", dtype=np.uint8), size=n)]
    for desc in (False, True):
        for c in cols:
            want = oracle.sort_permutation([c], [desc])
            assert np.array_equal(R.permutation_numpy([R.Key(c, descending=desc)]), want)
            assert np.array_equal(R.permutation_plain([R.Key(c, descending=desc)]), want)
    for picks, desc in (((0, 3), (False, True)), ((5, 4, 0), (True, False, True)), ((2, 5, 1, 3), (False, False, True, True))):
        want = oracle.sort_permutation([cols[i] for i in picks], list(desc))
        keys = [R.Key(cols[i], descending=d) for i, d in zip(picks, desc)]
        assert np.array_equal(R.permutation_numpy(keys), want) and np.array_equal(R.permutation_plain(keys), want)
    dates = np.array([T.date_raw(int(y), int(m), int(d)) for y, m, d in zip(rng.integers(1990, 1999, size=n), rng.integers(1, 13, size=n),
                                                                             rng.integers(1, 29, size=n))], dtype=np.int64)
    for desc in (False, True):
        want = oracle.sort_permutation([dates, cols[0]], [desc, False], types=[T.DATE, T.INT])
        keys = [R.Key(dates, T.DATE, desc), R.Key(cols[0])]
        assert np.array_equal(R.permutation_numpy(keys), want) and np.array_equal(R.permutation_plain(keys), want)


# ---- the reference's unit test ------------------------------------------------------------------------------------------
def reference_unit_test_columns(seeds):
    """TestTuple of the reference's unit test: three columns cut out of the bits of a seed (offset, length) = (3, 5), (6, 2),
    (1, 3); columns 4-6 repeat columns 1-3 and are NULL where those are zero."""
    seeds = np.asarray(seeds, dtype=np.int64)
    cols = [((seeds >> off) & (0xFFFF >> (16 - length))).astype(np.int32) for off, length in ((3, 5), (6, 2), (1, 3))]
    return cols, [c == 0 for c in cols]


# (name, columns in ORDER BY order, ascending per column, NULLs first per column) — every NULL case of the file (four single-column, four three-column, one mixed)
REFERENCE_NULL_CASES = [
    ("1Column_NullLast_Asc", [0], [True], [False]),
    ("1Column_NullFirst_Asc", [0], [True], [True]),
    ("1Column_NullLast_Desc", [0], [False], [False]),
    ("1Column_NullFirst_Desc", [0], [False], [True]),
    ("3Column_NullLast_Asc", [0, 1, 2], [True] * 3, [False] * 3),
    ("3Column_NullLast_Desc", [0, 1, 2], [False] * 3, [False] * 3),
    ("3Column_NullFirst_Asc", [0, 1, 2], [True] * 3, [True] * 3),
    ("3Column_NullFirst_Desc", [0, 1, 2], [False] * 3, [True] * 3),
    ("3Column_MixedNullOrdering_MixedOrdering", [0, 1, 2], [True, False, True], [True, False, False]),
]


def reference_expectation(cols, nulls, columns, ascending, nulls_first):
    """The order that file's comparators state: a NULL stands for the integer that sorts where the NULLs belong — INT_MAX for
    ASC NULLS LAST and DESC NULLS FIRST, INT_MIN for the other two — and the rows are ordered by the substituted tuples
    (a stable sort, so that the expectation is one permutation)."""
    n = cols[0].size
    substituted = []
    for c, asc, first in zip(columns, ascending, nulls_first):
        stand_in = INT_MAX if asc != first else INT_MIN
        v = np.where(nulls[c], stand_in, cols[c]).astype(np.int64)
        substituted.append(v if asc else -v)
    return np.asarray(sorted(range(n), key=lambda r: tuple(int(s[r]) for s in substituted)), dtype=np.int32)


@pytest.mark.parametrize("case", REFERENCE_NULL_CASES, ids=[c[0] for c in REFERENCE_NULL_CASES])
def test_the_reference_unit_tests_null_expectations(case):
    _, columns, ascending, nulls_first = case
    rng = np.random.default_rng(17)
    seeds = rng.integers(0, 256, size=10 * 100)          # createBlocks: seeds uniform in [0, 255]
    cols, nulls = reference_unit_test_columns(seeds)
    assert all(m.any() and not m.all() for m in nulls)
    keys = [R.Key(cols[c], T.INT, not asc, first, nulls[c]) for c, asc, first in zip(columns, ascending, nulls_first)]
    want = reference_expectation(cols, nulls, columns, ascending, nulls_first)
    assert np.array_equal(R.permutation_plain(keys), want)
    assert np.array_equal(R.permutation_numpy(keys), want)
