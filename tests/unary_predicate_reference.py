"""The checker of predicates over a unary operation (include/qsx.h: qsx_select_cmp_unary, qsx_select_in_unary), in numpy.
TEST INFRASTRUCTURE: nothing here is product code.

The contract is a composition, and so is this file: the operand is what tests/unary_reference.py computes (date_extract,
substring), the comparison over it is the oracle's (select_cmp on the INTs, select_cmp_char on the CHAR(m) fields: strcmpHelper,
AsciiStringComparators.hpp:218-251) and the IN list is tests/predicate_reference.py's (in_rows, in_char_rows).  The `_row` forms
say the same one row at a time on Python values; tests/test_unary_predicate_reference.py pins one against the other.

An operand is ("year",) / ("month",) or ("substring", start, length) with a 0-based start."""
import operator

import numpy as np

import predicate_reference as P
import unary_reference as U
from like_reference import field_text, pack_bitmap, unpack_bitmap  # noqa: F401  (re-exported: one bitmap layout for all checkers)

OPS = {0: operator.eq, 1: operator.ne, 2: operator.lt, 3: operator.le, 4: operator.gt, 5: operator.ge}     # QSX_EQ .. QSX_GE
_UNITS = {"year": U.DATE_YEAR, "month": U.DATE_MONTH}


def is_date(operand):
    return operand[0] in _UNITS


def operand_values(operand, col):
    """The operand's column vector: int32[n] for a date field, uint8 (n, m) for a substring."""
    if is_date(operand):
        return U.date_extract(_UNITS[operand[0]], col)
    return U.substring_fast(np.ascontiguousarray(col, dtype=np.uint8), operand[1], operand[2])


def cmp_rows(oracle, operand, col, op, literal):
    """`operand(col) op literal` as booleans, before any filter: the oracle's comparison over the operand's values."""
    values = operand_values(operand, col)
    n = values.shape[0]
    if n == 0:
        return np.zeros(0, dtype=bool)
    if is_date(operand):
        words = oracle.select_cmp(np.ascontiguousarray(values), op, int(literal))
    else:
        words = oracle.select_cmp_char(np.ascontiguousarray(values), op, bytes(literal))
    return oracle.bools_from_bitmap(words, n)


def in_rows(operand, col, literals, negate=False):
    values = operand_values(operand, col)
    if is_date(operand):
        return P.in_rows(values, literals, negate)
    return P.in_char_rows(values, literals, negate)


def result(bits, n, filter_words=None):
    """Booleans -> (words, count) as the entry points leave them: MSB-first, ANDed with the filter, bits >= n zero."""
    words = pack_bitmap(np.asarray(bits, dtype=bool)[:n])
    if filter_words is not None:
        words = words & np.ascontiguousarray(filter_words, dtype=np.uint64)[:words.size]
    return words, int(unpack_bitmap(words, n).sum())


# ------------------------------------------------------------------------------------------------------ one row at a time
def operand_value_row(operand, col, i):
    """Row i's operand as a Python value: an int, or the window's text as bytes."""
    if is_date(operand):
        raw = np.ascontiguousarray(col).view(np.uint8).reshape(-1, 8)[i].tobytes()
        return int.from_bytes(raw[0:4], "little", signed=True) if operand[0] == "year" else raw[4]
    start, length = operand[1], operand[2]
    width = col.shape[1]
    m = U.substring_width(width, start, length)
    return U.substring_text(col[i].tobytes(), start, m)


def _literal_value(operand, literal):
    return int(np.int32(literal)) if is_date(operand) else field_text(literal)


def cmp_row(operand, col, op, literal, i):
    """Python's comparison of bytes objects is strcmpHelper's on NUL-free texts: unsigned bytes, a proper prefix is smaller."""
    return bool(OPS[op](operand_value_row(operand, col, i), _literal_value(operand, literal)))


def in_row(operand, col, literals, negate, i):
    value = operand_value_row(operand, col, i)
    return any(value == _literal_value(operand, lit) for lit in literals) != bool(negate)
