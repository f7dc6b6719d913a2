"""CPU checker of the unary operations (include/qsx.h: qsx_eval_date_extract, qsx_eval_substring) in numpy.

EXTRACT restates DateExtractUncheckedOperator (types/operations/unary_operations/DateExtractOperation.cpp:117-142, 277-286)
over the 8-byte DateLit {int32 year; uint8 month; uint8 day; 2 bytes of padding} (types/DatetimeLit.hpp:38-43): on a Date
only YEAR and MONTH exist.  SUBSTRING restates SubstringUncheckedOperator::computeSubstring
(SubstringOperation.cpp:74-91) with a 0-based start, the result zero-filled to its width
m = min(width - start, length) (SubstringOperation.hpp:174-182)."""
import numpy as np

DATE_YEAR, DATE_MONTH = 0, 1


def date_bytes(year, month, day, padding=b"\0\0"):
    """The 8 bytes of a DateLit as they lie in a stripe (little endian)."""
    return int(year).to_bytes(4, "little", signed=True) + bytes([month, day]) + bytes(padding)


def date_extract(unit, dates):
    """dates: n DateLits as an int64 / uint64 array or as raw bytes of shape (n, 8).  Returns int32[n]."""
    raw = np.ascontiguousarray(dates).view(np.uint8).reshape(-1, 8)
    if unit == DATE_YEAR:
        return np.ascontiguousarray(raw[:, 0:4]).view("<i4").reshape(-1).astype(np.int32)
    if unit == DATE_MONTH:
        return raw[:, 4].astype(np.int32)
    raise ValueError("a Date has a year and a month only")


def substring_width(width, start, length):
    if not (1 <= width <= 255 and 0 <= start < width and length >= 1):
        raise ValueError("start in [0, width), length >= 1, width in 1..255")
    return min(width - start, length)


def substring_text(field, start, length):
    """One field (bytes of its full width) -> the bytes of the result's text, without padding."""
    end = field.find(b"\0")
    text = field if end < 0 else field[:end]
    return text[start:start + length] if start < len(text) else b""


def substring(col, start, length):
    """col: uint8 array of shape (n, width).  Returns uint8 (n, m), every text zero-filled to m.  Row by row, on purpose:
    this is the restatement the vectorised form below is checked against."""
    n, width = col.shape
    m = substring_width(width, start, length)
    out = np.zeros((n, m), dtype=np.uint8)
    for i in range(n):
        text = substring_text(col[i].tobytes(), start, length)
        out[i, :len(text)] = np.frombuffer(text, dtype=np.uint8)
    return out


def substring_fast(col, start, length):
    """The same without a Python loop over rows: a byte survives when no NUL lies at or in front of it."""
    n, width = col.shape
    m = substring_width(width, start, length)
    alive = np.logical_and.accumulate(col != 0, axis=1)
    return np.where(alive[:, start:start + m], col[:, start:start + m], 0).astype(np.uint8)
