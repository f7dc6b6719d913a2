"""CPU: the unary-operation checker (tests/unary_reference.py) against recorded answers — the reference's SUBSTRING query
(Select.test:812-835) and DateLit byte patterns with their year and month — and against its own second implementation."""
import numpy as np
import pytest

import unary_reference as R


def test_substring_gives_the_answers_of_the_references_query(golden):
    case = golden["unary_unittest"]["substring"]
    width, start, length = case["width"], case["start"], case["length"]
    assert (start, length) == (0, 2) and len(case["rows"]) == 12             # SQL's FROM 1 FOR 2
    col = np.zeros((len(case["rows"]), width), dtype=np.uint8)
    for i, row in enumerate(case["rows"]):
        text = row["char_col"].encode("latin-1")
        col[i, :len(text)] = np.frombuffer(text, dtype=np.uint8)
    got = R.substring(col, start, length)
    assert got.shape == (12, 2)
    assert [bytes(r).rstrip(b"\0").decode() for r in got] == [row["substring"] for row in case["rows"]]
    assert bytes(got[5]) == b"-1" and case["rows"][5]["char_col"] == "-11 3.316625"
    assert np.array_equal(R.substring_fast(col, start, length), got)


def test_year_and_month_of_the_recorded_date_bytes(golden):
    dates = golden["unary_unittest"]["dates"]
    raw = np.frombuffer(b"".join(bytes.fromhex(d["bytes"]) for d in dates), dtype=np.uint8).reshape(-1, 8)
    assert R.date_extract(R.DATE_YEAR, raw).tolist() == [d["year"] for d in dates]
    assert R.date_extract(R.DATE_MONTH, raw).tolist() == [d["month"] for d in dates]
    assert R.date_extract(R.DATE_YEAR, raw.view(np.int64).reshape(-1)).tolist() == [d["year"] for d in dates]
    assert min(d["year"] for d in dates) < 0 and max(d["year"] for d in dates) > 32767
    assert {1, 12} <= {d["month"] for d in dates}
    for d in dates:
        assert R.date_bytes(d["year"], d["month"], d["day"])[:6] == bytes.fromhex(d["bytes"])[:6]
    assert R.date_extract(R.DATE_YEAR, raw).dtype == np.int32 and R.date_extract(R.DATE_MONTH, raw).dtype == np.int32
    with pytest.raises(ValueError):
        R.date_extract(2, raw)                                                 # DAY belongs to Datetime


def test_substring_rules():
    col = np.frombuffer(b"ab\0zz" b"abcde" b"\0abcd" b"a\x80\xffd\0", dtype=np.uint8).reshape(4, 5)
    assert [bytes(r) for r in R.substring(col, 0, 2)] == [b"ab", b"ab", b"\0\0", b"a\x80"]
    assert [bytes(r) for r in R.substring(col, 1, 3)] == [b"b\0\0", b"bcd", b"\0\0\0", b"\x80\xffd"]     # zero-filled, not NUL + leftovers
    assert [bytes(r) for r in R.substring(col, 2, 300)] == [b"\0\0\0", b"cde", b"\0\0\0", b"\xffd\0"]  # m = width - start
    assert [bytes(r) for r in R.substring(col, 4, 1)] == [b"\0", b"e", b"\0", b"\0"]                   # start >= len: empty
    assert R.substring_width(15, 0, 2) == 2 and R.substring_width(15, 14, 2) == 1 and R.substring_width(255, 0, 300) == 255
    for bad in ((5, -1, 1), (5, 5, 1), (5, 0, 0), (0, 0, 1), (256, 0, 1)):
        with pytest.raises(ValueError):
            R.substring_width(*bad)
    assert R.substring(np.zeros((0, 5), dtype=np.uint8), 1, 2).shape == (0, 2)


def test_the_two_substring_implementations_agree_on_random_fields():
    rng = np.random.default_rng(20240812)
    for width in (1, 2, 7, 15, 25):
        col = rng.choice(np.frombuffer(b"ab\0\x80", dtype=np.uint8), size=(400, width), p=[0.4, 0.35, 0.15, 0.1])
        for start in {0, width // 2, width - 1}:
            for length in (1, 2, 3, width, 300):
                assert np.array_equal(R.substring(col, start, length), R.substring_fast(col, start, length)), (width, start, length)
