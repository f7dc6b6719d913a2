"""CPU: the LIKE checker (tests/like_reference.py) against the reference's own unit test and against itself — two
implementations of PatternMatchingComparators.hpp:60-232, the translation to a regular expression and a recursive matcher."""
import numpy as np

import like_reference as R


def test_both_implementations_give_the_answers_of_the_references_unit_test(golden):
    case = golden["like_unittest"]
    text = case["text"].encode("latin-1")
    assert len(text) == 31 and text.count(b"\\") == 1 and text.count(b"\n") == 1
    assert len(case["matched_like_patterns"]) == 6 and len(case["not_matched_like_patterns"]) == 4
    for pattern in case["matched_like_patterns"]:
        assert R.match_regex(text, pattern.encode("latin-1")), pattern
        assert R.match_recursive(text, pattern.encode("latin-1")), pattern
        assert R.match_bits(text, pattern.encode("latin-1")), pattern
    for pattern in case["not_matched_like_patterns"]:
        assert not R.match_regex(text, pattern.encode("latin-1")), pattern
        assert not R.match_recursive(text, pattern.encode("latin-1")), pattern
        assert not R.match_bits(text, pattern.encode("latin-1")), pattern


def test_a_backslash_is_a_literal_backslash():
    assert R.match_regex(b"a\\b", b"a\\b") and R.match_recursive(b"a\\b", b"a\\b")
    assert not R.match_regex(b"a%b", b"a\\%b") and not R.match_recursive(b"a%b", b"a\\%b")   # no escape: '\' then any run
    assert R.match_regex(b"a\\xxb", b"a\\%b") and R.match_recursive(b"a\\xxb", b"a\\%b")


def test_the_two_implementations_agree_on_random_pairs():
    matched = total = 0
    for text, pattern in R.random_pairs(120_000, seed=20240611):
        a, b = R.match_regex(text, pattern), R.match_recursive(text, pattern)
        assert a == b == R.match_bits(text, pattern), (text, pattern)
        matched += a
        total += 1
    assert total >= 100_000
    assert 0.05 * total < matched < 0.5 * total     # the small alphabets keep both outcomes common


def test_percent_and_underscore_take_newlines_and_high_bytes():
    for match in (R.match_regex, R.match_recursive, R.match_bits):
        assert match(b"a\nb", b"a_b") and match(b"a\n\nb", b"a%b") and match(b"\n", b"_") and match(b"", b"%")
        assert match(b"a\xc3\xa9b", b"a__b") and not match(b"a\xc3\xa9b", b"a_b")   # '_' is one byte, not one code point
        assert not match(b"", b"_") and not match(b"a", b"a%a") and not match(b"aba", b"ab%ba") and match(b"abba", b"ab%ba")


def test_nul_and_width_rules():
    # garbage behind the terminator is not part of the value
    assert R.field_text(b"ab\0zz%") == b"ab"
    assert R.field_text(b"abcde") == b"abcde"                      # a full-width value has no terminator
    assert R.field_text(b"\0abcd") == b""
    col = np.frombuffer(b"ab\0zz" b"abzzz" b"\0abzz" b"zzab\0", dtype=np.uint8).reshape(4, 5)
    assert R.like_rows(col, b"ab").tolist() == [True, False, False, False]
    assert R.like_rows(col, b"ab%").tolist() == [True, True, False, False]
    assert R.like_rows(col, b"%zz%").tolist() == [False, True, False, True]      # the zz behind row 0's NUL does not count
    assert R.like_rows(col, b"%ab").tolist() == [True, False, False, True]
    assert R.like_rows(col, b"").tolist() == [False, False, True, False]
    assert R.like_rows(col, b"_____").tolist() == [False, True, False, False]
    assert R.like_rows(col, b"ab\0%zz").tolist() == [True, False, False, False]  # the pattern ends at its NUL too
    # NOT LIKE is the negation; a NULL is in neither
    nulls = np.array([False, True, False, False])
    assert R.like_rows(col, b"ab%", negate=True).tolist() == [False, False, True, True]
    assert R.like_rows(col, b"ab%", nulls=nulls).tolist() == [True, False, False, False]
    assert R.like_rows(col, b"ab%", negate=True, nulls=nulls).tolist() == [False, False, True, True]


def test_bitmap_packing():
    bits = np.zeros(65, dtype=bool)
    bits[[0, 1, 63, 64]] = True
    words = R.pack_bitmap(bits)
    assert words.tolist() == [(1 << 63) | (1 << 62) | 1, 1 << 63]
    assert R.unpack_bitmap(words, 65).tolist() == bits.tolist()
    assert R.pack_bitmap(np.zeros(0, dtype=bool)).size == 0
