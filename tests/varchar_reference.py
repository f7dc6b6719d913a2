"""The checker of VARCHAR attributes behind variable-length compression dictionaries (qsx_select_like_var,
qsx_decode_codes_var, include/qsx.h), pure numpy / Python.

The dictionary is the reference's (compression/CompressionDictionary.hpp:46-58, CompressionDictionaryLite.hpp:248-290,
CompressionDictionaryBuilder.cpp:53-66):

    uint32 num_codes | uint32 null_code | uint32 offset[num_codes] | value bytes

little-endian; the offsets count from the first value byte and ascend; the values lie back to back in code order, which is
the order of the type's LessComparison — for VARCHAR byte-wise strcmp order (AsciiStringComparators.hpp), i.e. Python's order
of `bytes` that hold no NUL.  Entry c is [offset[c], offset[c + 1]), the last one ends where the dictionary does.  A VARCHAR
value carries its terminating NUL (types/VarCharType.hpp:42,112).  null_code is num_codes when the block holds NULLs, else
2^32 - 1.

`build_dictionary` writes such an image from a list of texts at a chosen byte misalignment inside a larger buffer;
`parse_dictionary` reads one back knowing only its start and size; `like_entries` and `decode_rows` restate what the device
entry points compute.  The matcher is tests/like_reference.py's.
"""
import numpy as np

import like_reference as L

NO_NULL_CODE = 0xFFFFFFFF


def sorted_texts(texts):
    """The distinct texts in dictionary (strcmp) order.  A text holds no NUL: it would end there."""
    texts = sorted(set(bytes(t) for t in texts))
    assert all(b"\0" not in t for t in texts)
    return texts


def build_dictionary(texts, with_null=False, misalign=0):
    """texts: byte strings, already distinct and in code order (sorted_texts).  Returns (buffer, start): `buffer` is a uint8
    array that is 16-byte aligned as numpy allocates it plus whatever the caller does with it, and the dictionary image begins
    at buffer[start] with start % 16 == misalign; bytes outside the image are 0xEE."""
    texts = [bytes(t) for t in texts]
    offsets, at = [], 0
    for t in texts:
        offsets.append(at)
        at += len(t) + 1
    image = (np.array([len(texts), len(texts) if with_null else NO_NULL_CODE], dtype="<u4").tobytes()
             + np.array(offsets, dtype="<u4").tobytes() + b"".join(t + b"\0" for t in texts))
    buffer = np.full(16 + len(image) + 16, 0xEE, dtype=np.uint8)
    start = misalign % 16
    buffer[start:start + len(image)] = np.frombuffer(image, dtype=np.uint8)
    return buffer, start


def parse_dictionary(buffer, start, size):
    """The image of `size` bytes at buffer[start]: (num_codes, null_code, offsets uint32[num_codes], value bytes uint8[...])."""
    image = bytes(np.asarray(buffer, dtype=np.uint8)[start:start + size])
    num_codes, null_code = (int(v) for v in np.frombuffer(image[:8], dtype="<u4"))
    offsets = np.frombuffer(image[8:8 + 4 * num_codes], dtype="<u4").copy()
    values = np.frombuffer(image[8 + 4 * num_codes:], dtype=np.uint8).copy()
    return num_codes, null_code, offsets, values


def entry_bytes(offsets, values, code):
    """Entry `code` as it lies, terminator included: the last one's end is the dictionary's."""
    end = int(offsets[code + 1]) if code + 1 < len(offsets) else len(values)
    return bytes(values[int(offsets[code]):end])


def entry_text(offsets, values, code):
    return L.field_text(entry_bytes(offsets, values, code))


def check_dictionary(offsets, values):
    """What the host layer requires of an adopted dictionary: ascending offsets inside the dictionary, a final NUL."""
    offsets = np.asarray(offsets, dtype=np.int64)
    if offsets.size == 0:
        return True
    if offsets[0] < 0 or np.any(np.diff(offsets) < 0) or offsets[-1] >= len(values):
        return False
    return int(values[-1]) == 0


def like_entries(offsets, values, pattern, negate=False):
    """LIKE (negate: NOT LIKE) over every entry: a boolean array of num_codes — the code set."""
    return np.array([L.match_bits(entry_text(offsets, values, c), pattern) != bool(negate) for c in range(len(offsets))], dtype=bool)


def decode_rows(codes, offsets, values, out_width):
    """codes -> uint8 array (n, out_width): the entry's text, NUL-padded, cut at out_width without a terminator; all NUL for
    a code >= num_codes (the NULL code)."""
    codes = np.asarray(codes).astype(np.int64)
    table = np.zeros((len(offsets) + 1, out_width), dtype=np.uint8)          # the last row: NULL
    for c in range(len(offsets)):
        text = entry_text(offsets, values, c)[:out_width]
        table[c, :len(text)] = np.frombuffer(text, dtype=np.uint8)
    return table[np.minimum(codes, len(offsets))]


def like_rows_coded(codes, offsets, values, pattern, negate=False):
    """Row by row: the decoded text of every row against the pattern; a NULL row matches neither."""
    codes = np.asarray(codes).astype(np.int64)
    out = np.zeros(codes.size, dtype=bool)
    for i, c in enumerate(codes):
        if c < len(offsets):
            out[i] = L.match_bits(entry_text(offsets, values, int(c)), pattern) != bool(negate)
    return out
