"""CPU: tests/varchar_reference.py pinned on hand-written cases — the layout of a variable-length dictionary image, the
length of the last entry, the empty string, a text of exactly n bytes, sorted order, and match / decode over it."""
import numpy as np

import like_reference as L
import varchar_reference as V


def test_the_image_is_the_documented_layout_byte_for_byte():
    texts = V.sorted_texts([b"b", b"", b"ab"])
    assert texts == [b"", b"ab", b"b"]
    buffer, start = V.build_dictionary(texts, with_null=True, misalign=5)
    assert start == 5
    want = (b"\x03\0\0\0" + b"\x03\0\0\0"                     # num_codes, null_code = num_codes
            + b"\0\0\0\0" + b"\x01\0\0\0" + b"\x04\0\0\0"      # offsets from the first value byte, ascending
            + b"\0" + b"ab\0" + b"b\0")                        # every value with its terminator, back to back
    assert bytes(buffer[start:start + len(want)]) == want
    assert set(buffer[:start]) <= {0xEE} and set(buffer[start + len(want):]) == {0xEE}
    num_codes, null_code, offsets, values = V.parse_dictionary(buffer, start, len(want))
    assert (num_codes, null_code) == (3, 3) and offsets.tolist() == [0, 1, 4] and bytes(values) == b"\0ab\0b\0"


def test_without_nulls_the_null_code_is_all_ones():
    buffer, start = V.build_dictionary([b"x"], with_null=False)
    assert V.parse_dictionary(buffer, start, 8 + 4 + 2)[1] == 0xFFFFFFFF == V.NO_NULL_CODE


def test_the_last_entry_ends_where_the_dictionary_does():
    texts = [b"a", b"bcd"]
    buffer, start = V.build_dictionary(texts)
    size = 8 + 8 + 2 + 4
    _, _, offsets, values = V.parse_dictionary(buffer, start, size)
    assert V.entry_bytes(offsets, values, 0) == b"a\0" and V.entry_bytes(offsets, values, 1) == b"bcd\0"
    # one byte less of dictionary: the last entry is one byte shorter — its length comes from the size, not from a NUL
    _, _, offsets, values = V.parse_dictionary(buffer, start, size - 1)
    assert V.entry_bytes(offsets, values, 1) == b"bcd" and not V.check_dictionary(offsets, values)


def test_the_empty_string_is_an_entry_of_one_byte():
    buffer, start = V.build_dictionary([b""])
    _, _, offsets, values = V.parse_dictionary(buffer, start, 8 + 4 + 1)
    assert V.entry_bytes(offsets, values, 0) == b"\0" and V.entry_text(offsets, values, 0) == b""
    assert V.like_entries(offsets, values, b"").tolist() == [True]
    assert V.like_entries(offsets, values, b"%").tolist() == [True]
    assert V.like_entries(offsets, values, b"_").tolist() == [False]
    assert V.decode_rows([0, 1], offsets, values, 3).tolist() == [[0, 0, 0], [0, 0, 0]]


def test_a_text_of_exactly_n_bytes_has_n_plus_one_bytes_here_and_no_terminator_decoded():
    n = 4
    texts = V.sorted_texts([b"abcd", b"ab"])
    buffer, start = V.build_dictionary(texts)
    _, _, offsets, values = V.parse_dictionary(buffer, start, 8 + 8 + 3 + 5)
    assert len(V.entry_bytes(offsets, values, 1)) == n + 1
    out = V.decode_rows([1, 0, 2], offsets, values, n)
    assert out.tolist() == [list(b"abcd"), list(b"ab\0\0"), [0, 0, 0, 0]]
    # cut without a terminator when the field is narrower than the text
    assert V.decode_rows([1], offsets, values, 3).tolist() == [list(b"abc")]


def test_sorted_order_is_byte_order_and_prefixes_come_first():
    texts = V.sorted_texts([b"b", b"a\x80", b"ab", b"a", b"B", b"", b"ab"])
    assert texts == [b"", b"B", b"a", b"ab", b"a\x80", b"b"]          # unsigned bytes: 0x80 behind 'b' of "ab"
    # the same order as comparing the NUL-terminated values with strcmp
    keys = [t + b"\0" for t in texts]
    assert keys == sorted(keys)


def test_match_and_decode_over_a_small_dictionary():
    texts = V.sorted_texts([b"PROMO BRUSHED", b"PROMO", b"STANDARD BRASS", b"", b"SMALL BRASS"])
    buffer, start = V.build_dictionary(texts, with_null=True, misalign=3)
    size = 8 + 4 * len(texts) + sum(len(t) + 1 for t in texts)
    num_codes, null_code, offsets, values = V.parse_dictionary(buffer, start, size)
    assert V.check_dictionary(offsets, values) and num_codes == null_code == 5
    assert [V.entry_text(offsets, values, c) for c in range(5)] == texts
    assert V.like_entries(offsets, values, b"PROMO%").tolist() == [False, True, True, False, False]
    assert V.like_entries(offsets, values, b"%BRASS", negate=True).tolist() == [True, True, True, False, False]
    codes = np.array([4, 5, 0, 1, 1], dtype=np.uint8)
    assert V.like_rows_coded(codes, offsets, values, b"%S%").tolist() == [True, False, False, False, False]
    assert V.like_rows_coded(codes, offsets, values, b"%S%", negate=True).tolist() == [False, False, True, True, True]
    rows = V.decode_rows(codes, offsets, values, 14)
    assert [L.field_text(r.tobytes()) for r in rows] == [b"STANDARD BRASS", b"", b"", b"PROMO", b"PROMO"]
    assert not rows[1].any()


def test_check_dictionary_turns_down_what_the_host_layer_refuses():
    values = np.frombuffer(b"a\0bc\0", dtype=np.uint8)
    assert V.check_dictionary([0, 2], values)
    assert not V.check_dictionary([2, 0], values)                      # descending
    assert not V.check_dictionary([0, 5], values)                      # an entry behind the end
    assert not V.check_dictionary([0, 2], values[:-1])                 # no final NUL
    assert V.check_dictionary([], values[:0])
