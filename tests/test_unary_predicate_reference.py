"""CPU: the checker of predicates over a unary operation (tests/unary_predicate_reference.py) against its own row-at-a-time
form and against cases written out by hand."""
import numpy as np

import unary_predicate_reference as R
import unary_reference as U

EQ, NE, LT, LE, GT, GE = range(6)


def chars(width, *texts):
    col = np.zeros((len(texts), width), dtype=np.uint8)
    for i, text in enumerate(texts):
        col[i, :len(text)] = np.frombuffer(text, dtype=np.uint8)
    return col


def dates(*ymd):
    return np.frombuffer(b"".join(U.date_bytes(y, m, d, b"\xAB\xCD") for y, m, d in ymd), dtype=np.int64)


def test_the_two_forms_agree_on_random_fields(oracle):
    rng = np.random.default_rng(20241020)
    alphabet = np.frombuffer(b"ab\0\x80", dtype=np.uint8)
    for width in (1, 2, 3, 15, 17, 25):
        col = rng.choice(alphabet, size=(300, width), p=[0.4, 0.35, 0.15, 0.1])
        for start in sorted({0, width // 2, width - 1}):
            for length in (1, 2, 300):
                operand = ("substring", start, length)
                m = U.substring_width(width, start, length)
                literals = [b"", b"a", b"ab", b"b\x80", b"a" * (m + 1), bytes(col[7, start:start + m]), b"ab\0zz"]
                for op in range(6):
                    for lit in literals[:5]:
                        got = R.cmp_rows(oracle, operand, col, op, lit)
                        want = [R.cmp_row(operand, col, op, lit, i) for i in range(col.shape[0])]
                        assert got.tolist() == want, (width, start, length, op, lit)
                for negate in (False, True):
                    got = R.in_rows(operand, col, literals, negate)
                    want = [R.in_row(operand, col, literals, negate, i) for i in range(col.shape[0])]
                    assert got.tolist() == want, (width, start, length, negate)


def test_the_two_forms_agree_on_random_dates(oracle):
    rng = np.random.default_rng(7)
    n = 500
    year = rng.integers(-(1 << 31), 1 << 31, size=n, dtype=np.int64)
    year[::2] = rng.integers(1992, 1999, size=year[::2].size)
    month = rng.integers(1, 13, size=n)
    raw = ((year & 0xFFFFFFFF) | (month << 32) | (rng.integers(1, 32, size=n) << 40) | (rng.integers(0, 1 << 16, size=n) << 48))
    raw = raw.astype(np.uint64).view(np.int64)
    for operand, literals in ((("year",), [1995, 1992, -3, int(year[1]), 1 << 30]), (("month",), [1, 12, 7, 0, 13, -1])):
        for op in range(6):
            for lit in literals:
                got = R.cmp_rows(oracle, operand, raw, op, lit)
                assert got.tolist() == [R.cmp_row(operand, raw, op, lit, i) for i in range(n)], (operand, op, lit)
        for negate in (False, True):
            got = R.in_rows(operand, raw, literals, negate)
            assert got.tolist() == [R.in_row(operand, raw, literals, negate, i) for i in range(n)], (operand, negate)


def test_substring_cases_by_hand(oracle):
    #                 0           1           2            3           4             5
    col = chars(6, b"13-555", b"1\0-555", b"\0" b"3-555", b"31", b"\x80\xff-555", b"1")
    q22 = ("substring", 0, 2)
    assert R.cmp_rows(oracle, q22, col, EQ, b"13").tolist() == [True, False, False, False, False, False]
    # a NUL inside the window ends the text there; a NUL in front of the window makes it the empty string
    assert R.cmp_rows(oracle, q22, col, EQ, b"1").tolist() == [False, True, False, False, False, True]
    assert R.cmp_rows(oracle, q22, col, EQ, b"").tolist() == [False, False, True, False, False, False]
    assert R.cmp_rows(oracle, ("substring", 1, 2), col, EQ, b"").tolist() == [False, True, True, False, False, True]
    assert R.cmp_rows(oracle, ("substring", 2, 4), col, EQ, b"-555").tolist() == [True, False, False, False, True, False]
    # start >= len against '': row 3 has two bytes, row 5 one
    assert R.cmp_rows(oracle, ("substring", 2, 1), col, EQ, b"").tolist() == [False, True, True, True, False, True]
    assert R.in_rows(("substring", 5, 300), col, [b""]).tolist() == [False, True, True, True, False, True]
    # a literal longer than m = 2 equals no window, and is greater than its own prefix
    assert not R.cmp_rows(oracle, q22, col, EQ, b"13-").any()
    assert R.cmp_rows(oracle, q22, col, LT, b"13-").tolist() == [True, True, True, False, False, True]
    assert R.in_rows(q22, col, [b"13-", b"31-"]).tolist() == [False] * 6
    assert R.in_rows(q22, col, [b"13-", b"31-"], negate=True).tolist() == [True] * 6
    # bytes >= 0x80 are unsigned: greater than every ASCII text
    assert R.cmp_rows(oracle, q22, col, GT, b"~~").tolist() == [False, False, False, False, True, False]
    assert R.cmp_rows(oracle, q22, col, EQ, b"\x80\xff").tolist() == [False, False, False, False, True, False]
    assert R.in_rows(q22, col, [b"13", b"31", b"\x80\xff"]).tolist() == [True, False, False, True, True, False]
    # a literal ends at its first NUL
    assert R.cmp_rows(oracle, q22, col, EQ, b"31\0x").tolist() == [False, False, False, True, False, False]
    for i, want in enumerate([b"13", b"1", b"", b"31", b"\x80\xff", b"1"]):
        assert R.operand_value_row(q22, col, i) == want
    words, count = R.result(R.in_rows(q22, col, [b"13", b"31"]), 6)
    assert words.tolist() == [0x9000000000000000] and count == 2
    words, count = R.result(R.in_rows(q22, col, [b"13", b"31"], negate=True), 6, filter_words=np.array([0x7C00000000000000], dtype=np.uint64))
    assert words.tolist() == [0x6C00000000000000] and count == 4          # bits >= n stay zero under negate


def test_date_cases_by_hand(oracle):
    raw = dates((1995, 1, 31), (-44, 3, 15), (1995, 12, 1), (40000, 12, 31), (1996, 1, 1))
    assert R.cmp_rows(oracle, ("year",), raw, EQ, 1995).tolist() == [True, False, True, False, False]
    assert R.cmp_rows(oracle, ("year",), raw, LT, 0).tolist() == [False, True, False, False, False]           # a negative year
    assert R.cmp_rows(oracle, ("year",), raw, EQ, -44).tolist() == [False, True, False, False, False]
    assert R.cmp_rows(oracle, ("year",), raw, GE, 1996).tolist() == [False, False, False, True, True]
    assert R.cmp_rows(oracle, ("month",), raw, EQ, 1).tolist() == [True, False, False, False, True]            # month 1
    assert R.cmp_rows(oracle, ("month",), raw, EQ, 12).tolist() == [False, False, True, True, False]           # month 12
    assert R.cmp_rows(oracle, ("month",), raw, LE, 0).tolist() == [False] * 5
    assert R.in_rows(("month",), raw, [1, 12]).tolist() == [True, False, True, True, True]
    assert R.in_rows(("year",), raw, [-44, 40000], negate=True).tolist() == [True, False, True, False, True]
    assert [R.operand_value_row(("year",), raw, i) for i in range(5)] == [1995, -44, 1995, 40000, 1996]
    assert [R.operand_value_row(("month",), raw, i) for i in range(5)] == [1, 3, 12, 12, 1]
    assert R.cmp_rows(oracle, ("year",), raw[:0], EQ, 1).shape == (0,)
