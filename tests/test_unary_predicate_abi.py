"""CPU: the entry points of predicates over a unary operation (qsx_select_cmp_unary, qsx_select_in_unary and their run forms,
include/qsx.h): declared, exported, mirrored by the binding, and refusing to compute without a GPU.  QSX_ABI_VERSION did not
change: a caller detects the capability by the presence of the symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from quickstep_amd import types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("qsx_select_cmp_unary", "qsx_select_in_unary", "qsx_select_cmp_unary_blocks", "qsx_select_in_unary_blocks")


def _header():
    return open(os.path.join(ROOT, "include", "qsx.h")).read()


def test_the_header_declares_the_functions_the_operand_and_the_macros():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(\s*const\s+qsx_unary_operand_t\s*\*" % name, text), name
    assert re.search(r"^#define QSX_UNARY_DATE_FIELD 0\s*$", text, flags=re.M)
    assert re.search(r"^#define QSX_UNARY_SUBSTRING 1\s*$", text, flags=re.M)
    struct = re.search(r"typedef struct qsx_unary_operand \{(.*?)\} qsx_unary_operand_t;", text, flags=re.S)
    assert struct and re.findall(r"int32_t\s+(\w+);", struct.group(1)) == [name for name, _ in T.UnaryOperand._fields_]
    assert C.sizeof(T.UnaryOperand) == 16
    assert "#define QSX_ABI_VERSION 19" in _header()
    # the contract is stated where the caller reads it, next to the reference lines it replaces
    assert "ComparisonPredicate.cpp:209-240" in _header() and "ScalarUnaryExpression.cpp:92-115" in _header()
    assert (T.UNARY_DATE_FIELD, T.UNARY_SUBSTRING) == (0, 1)
    year, sub = T.date_field(T.DATE_YEAR), T.substring_of(0, 2)
    assert (year.kind, year.unit) == (T.UNARY_DATE_FIELD, T.DATE_YEAR) and (sub.kind, sub.start, sub.length) == (T.UNARY_SUBSTRING, 0, 2)


def test_the_library_exports_them_and_the_binding_lists_them(capi):
    lib = C.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in capi.EXPORTED
    for wrapper in ("select_cmp_unary", "select_in_unary", "select_cmp_unary_blocks", "select_in_unary_blocks"):
        assert callable(getattr(capi, wrapper)), wrapper
    assert capi.lib.qsx_abi_version() == T.ABI_VERSION == 19
    # the tile sizes the GPU tests place their row counts around
    assert capi.UNARY_DATE_TILE_ROWS == 512
    assert [capi.unary_substring_tile_rows(w) for w in (1, 15, 48, 49, 255)] == [1024, 1024, 1024, 960, 192]


def test_every_call_refuses_to_compute_without_a_gpu(capi):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    dates = np.zeros(8, dtype=np.int64)
    col = np.zeros((8, 15), dtype=np.uint8)
    out = np.zeros(1, dtype=np.uint64)
    one = lambda a: (C.c_void_p * 1)(a.ctypes.data)      # noqa: E731
    rows = (C.c_int64 * 1)(8)
    year, sub = T.date_field(T.DATE_YEAR), T.substring_of(0, 2)
    lit = (C.c_int32 * 2)(1995, 1996)
    slots = C.create_string_buffer(2 * T.MAX_CHAR_LITERAL)
    lengths = (C.c_int32 * 2)(2, 2)
    lib = capi.lib
    assert lib.qsx_select_cmp_unary(C.byref(year), dates.ctypes.data, 8, 8, T.EQ, lit, 0, None, out.ctypes.data, None, None) == T.ERR_NO_DEVICE
    assert lib.qsx_select_cmp_unary(C.byref(sub), col.ctypes.data, 15, 8, T.EQ, b"13", 2, None, out.ctypes.data, None, None) == T.ERR_NO_DEVICE
    assert lib.qsx_select_in_unary(C.byref(year), dates.ctypes.data, 8, 8, lit, None, 2, 0, None, out.ctypes.data, None, None) == T.ERR_NO_DEVICE
    assert lib.qsx_select_in_unary(C.byref(sub), col.ctypes.data, 15, 8, slots, lengths, 2, 1, None, out.ctypes.data, None, None) == T.ERR_NO_DEVICE
    assert lib.qsx_select_cmp_unary_blocks(C.byref(year), 8, 1, rows, one(dates), T.GE, lit, 0, None, one(out), None, None) == T.ERR_NO_DEVICE
    assert lib.qsx_select_in_unary_blocks(C.byref(sub), 15, 1, rows, one(col), slots, lengths, 2, 0, None, one(out), None, None) == T.ERR_NO_DEVICE
    # QSX_ERR_NO_DEVICE comes first: also in front of the argument checks
    assert lib.qsx_select_cmp_unary(None, None, 0, -1, 17, None, -1, None, None, None, None) == T.ERR_NO_DEVICE
    assert lib.qsx_select_in_unary(None, None, 300, -1, None, None, 0, 7, None, None, None, None) == T.ERR_NO_DEVICE
    assert lib.qsx_select_cmp_unary_blocks(None, 0, -1, None, None, 17, None, -1, None, None, None, None) == T.ERR_NO_DEVICE
    assert lib.qsx_select_in_unary_blocks(None, 0, -1, None, None, None, None, 99, 7, None, None, None, None) == T.ERR_NO_DEVICE
    bad = T.UnaryOperand(9, 9, -1, 0)
    assert lib.qsx_select_cmp_unary(C.byref(bad), dates.ctypes.data, 8, 8, T.EQ, lit, 0, None, out.ctypes.data, None, None) == T.ERR_NO_DEVICE
