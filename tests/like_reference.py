"""The checker of LIKE / NOT LIKE on CHAR(n) values (qsx_select_like, include/qsx.h), pure Python on `bytes`.

Three independent implementations of one definition (types/operations/comparisons/PatternMatchingComparators.hpp:60-232 of the
reference):

  * `match_regex`: the reference's own translation (transformLikeToRegex, :207-232) — '_' becomes `(.|\\n)`, '%' becomes
    `(.|\\n)*`, every other byte is escaped — through `re.fullmatch` (the reference calls RE2::FullMatch).  On a bytes
    pattern `.` is one BYTE: the library's documented deviation from re2's UTF-8 mode, where '_' takes a code point.
  * `match_recursive`: a recursive matcher that knows nothing about regular expressions.
  * `match_bits`: the pattern's positions as a bit set, one step per byte: what `like_rows` uses over whole stripes (the
    other two take too long on a 255-byte text against a pattern with six '%').

tests/test_like_reference.py pins one against the other and both against the expectations of the reference's unit test
(tests/golden/like_unittest.json).

The text of a CHAR(width) field is its bytes up to the first NUL, or all `width` bytes when it has none (`field_text`); a
pattern likewise ends at its first NUL.  There is no escape character: a backslash is a literal backslash.
"""
import functools
import re

import numpy as np


def field_text(field):
    """The value of a CHAR(n) field (bytes of length n): up to its first NUL (strnlen)."""
    field = bytes(field)
    end = field.find(b"\0")
    return field if end < 0 else field[:end]


def clean_pattern(pattern):
    """A pattern ends at its first NUL."""
    return field_text(pattern)


@functools.lru_cache(maxsize=None)
def _compiled(pattern):
    out = []
    for byte in pattern:
        c = bytes([byte])
        out.append(b"(.|\n)" if c == b"_" else b"(.|\n)*" if c == b"%" else re.escape(c))
    return re.compile(b"".join(out))


def match_regex(text, pattern):
    return _compiled(clean_pattern(pattern)).fullmatch(bytes(text)) is not None


def match_recursive(text, pattern):
    text, pattern = bytes(text), clean_pattern(pattern)

    @functools.lru_cache(maxsize=None)
    def at(t, p):
        if p == len(pattern):
            return t == len(text)
        if pattern[p] == 0x25:                                  # '%': the empty run, or one more byte under it
            return at(t, p + 1) or (t < len(text) and at(t + 1, p))
        if t == len(text):
            return False
        return (pattern[p] == 0x5F or pattern[p] == text[t]) and at(t + 1, p + 1)   # '_' or the byte itself

    return at(0, 0)


def match_bits(text, pattern):
    """A third form for long texts and many '%' (where the regular expression backtracks without end and the recursion is
    slow): the pattern's positions as the bits of an integer, one step per byte of the text.  Bit i = the first i bytes of
    the pattern (runs of '%' collapsed, which changes no answer) have been matched."""
    text, pattern = bytes(text), re.sub(b"%+", b"%", clean_pattern(pattern))
    percent = sum(1 << i for i, q in enumerate(pattern) if q == 0x25)
    any_byte = sum(1 << i for i, q in enumerate(pattern) if q == 0x5F)
    by_byte = {}
    for i, q in enumerate(pattern):
        if q not in (0x25, 0x5F):
            by_byte[q] = by_byte.get(q, 0) | (1 << i)
    state = 1
    state |= (state & percent) << 1
    for c in text:
        state = ((state & (by_byte.get(c, 0) | any_byte)) << 1) | (state & percent)
        state |= (state & percent) << 1
        if state == 0:
            return False
    return (state >> len(pattern)) & 1 == 1


def like_rows(col, pattern, negate=False, nulls=None):
    """LIKE (negate: NOT LIKE) over a stripe: col is a uint8 array of shape (n, width); a boolean array of n.  A row that is
    NULL (nulls[i]) matches neither."""
    col = np.ascontiguousarray(col, dtype=np.uint8)
    cache = {}
    out = np.zeros(col.shape[0], dtype=bool)
    for i in range(col.shape[0]):
        text = field_text(col[i].tobytes())
        hit = cache.get(text)
        if hit is None:
            hit = cache[text] = match_bits(text, pattern)
        out[i] = hit != bool(negate)
    if nulls is not None:
        out &= ~np.asarray(nulls, dtype=bool)
    return out


def pack_bitmap(bits):
    """A boolean array as a TupleIdSequence: uint64 words, bit i = bit 63 - i % 64 of word i // 64, trailing bits zero."""
    bits = np.asarray(bits, dtype=bool)
    words = (bits.size + 63) // 64
    padded = np.zeros(words * 64, dtype=np.uint8)
    padded[:bits.size] = bits
    return np.packbits(padded).reshape(words, 8)[:, ::-1].copy().view(np.uint64).reshape(words) if words else np.zeros(0, dtype=np.uint64)


def unpack_bitmap(words, n):
    words = np.ascontiguousarray(words, dtype=np.uint64)
    return np.unpackbits(words.view(np.uint8).reshape(-1, 8)[:, ::-1].reshape(-1))[:n].astype(bool)


def random_pairs(count, seed):
    """The generator of the cross-check: text of 0..8 bytes from `ab%_\\n`, pattern of 0..6 bytes from `ab%%__\\n`."""
    rng = np.random.default_rng(seed)
    text_alphabet, pattern_alphabet = b"ab%_\n", b"ab%%__\n"
    text_bytes = np.frombuffer(text_alphabet, dtype=np.uint8)[rng.integers(0, len(text_alphabet), size=(count, 8))]
    pattern_bytes = np.frombuffer(pattern_alphabet, dtype=np.uint8)[rng.integers(0, len(pattern_alphabet), size=(count, 6))]
    text_len, pattern_len = rng.integers(0, 9, size=count), rng.integers(0, 7, size=count)
    for i in range(count):
        yield text_bytes[i, :text_len[i]].tobytes(), pattern_bytes[i, :pattern_len[i]].tobytes()
