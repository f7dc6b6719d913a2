"""CPU: the C ABI of predicate trees - qsx_select_in(_blocks), qsx_select_in_char(_blocks), qsx_bitmap_eval(_blocks) - is
declared, exported and bound; its macros have their mirrors in quickstep_amd/types.py; the header cites the reference lines the
semantics come from; QSX_ABI_VERSION did not move; and without a GPU every call refuses with QSX_ERR_NO_DEVICE."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("qsx_select_in", "qsx_select_in_blocks", "qsx_select_in_char", "qsx_select_in_char_blocks", "qsx_bitmap_eval",
               "qsx_bitmap_eval_blocks")


def _header():
    return open(os.path.join(ROOT, "include", "qsx.h")).read()


def test_symbols_are_declared_exported_and_bound(capi):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = C.CDLL(capi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, code), f"{name} is not declared in include/qsx.h"
        assert hasattr(lib, name), f"{name} is not exported by libqsx.so"
        assert name in capi.EXPORTED


def test_macros_and_their_mirrors(capi):
    from quickstep_amd import types as T
    header = _header()
    for macro, value in (("QSX_MAX_IN_LIST", T.MAX_IN_LIST), ("QSX_MAX_BOOL_LEAVES", T.MAX_BOOL_LEAVES),
                         ("QSX_MAX_BOOL_INSTRS", T.MAX_BOOL_INSTRS), ("QSX_MAX_BOOL_DEPTH", T.MAX_BOOL_DEPTH),
                         ("QSX_MAX_CHAR_LITERAL", T.MAX_CHAR_LITERAL)):
        assert re.search(r"#define %s %d\b" % (macro, value), header), macro
    for macro, value in (("QSX_BOOL_AND", T.BOOL_AND), ("QSX_BOOL_OR", T.BOOL_OR), ("QSX_BOOL_NOT", T.BOOL_NOT)):
        assert re.search(r"#define %s \(%d\)" % (macro, value), header), macro
    assert (T.MAX_IN_LIST, T.MAX_BOOL_LEAVES, T.MAX_BOOL_INSTRS, T.MAX_BOOL_DEPTH) == (32, 32, 64, 8)
    assert (T.BOOL_AND, T.BOOL_OR, T.BOOL_NOT) == (-1, -2, -3)
    assert capi.lib.qsx_abi_version() == T.ABI_VERSION == 19
    assert "#define QSX_ABI_VERSION 19" in header


def test_header_cites_the_reference_and_states_the_null_behaviour():
    header = _header()
    for cite in ("DisjunctionPredicate.cpp:109-157", "NegationPredicate.cpp:70-90", "InValueList.cpp:40-65",
                 "LiteralComparators-inl.hpp:330-370", "AsciiStringComparators.hpp:218-251"):
        assert cite in header, cite
    at = header.index("#define QSX_MAX_BOOL_LEAVES")
    contract = header[header.rindex("/*", 0, at):at]
    assert "SELECTS a row whose x is NULL" in contract and "three-valued" in contract


def test_every_new_call_refuses_without_a_gpu(capi):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from quickstep_amd import types as T
    lib = capi.lib
    col = np.zeros(8, dtype=np.int32)
    out = np.zeros(1, dtype=np.uint64)
    lits = (C.c_int32 * 2)(1, 2)
    rows = (C.c_int64 * 1)(8)
    cols = (C.c_void_p * 1)(col.ctypes.data)
    outs = (C.c_void_p * 1)(out.ctypes.data)
    slots = C.create_string_buffer(2 * T.MAX_CHAR_LITERAL)
    lengths = (C.c_int32 * 2)(1, 1)
    program = (C.c_int32 * 1)(0)
    bad_program = (C.c_int32 * 1)(T.BOOL_AND)
    assert lib.qsx_select_in(T.INT, col.ctypes.data, 8, lits, 2, 0, None, out.ctypes.data, None, None) == T.ERR_NO_DEVICE
    assert lib.qsx_select_in_blocks(T.INT, 1, rows, cols, lits, 2, 0, None, outs, None, None) == T.ERR_NO_DEVICE
    assert lib.qsx_select_in_char(col.ctypes.data, 4, 8, slots, lengths, 2, 1, None, out.ctypes.data, None, None) == T.ERR_NO_DEVICE
    assert lib.qsx_select_in_char_blocks(4, 1, rows, cols, slots, lengths, 2, 1, None, outs, None, None) == T.ERR_NO_DEVICE
    assert lib.qsx_bitmap_eval(1, cols, 1, program, 8, None, out.ctypes.data, None, None) == T.ERR_NO_DEVICE
    assert lib.qsx_bitmap_eval_blocks(1, 1, program, 1, rows, cols, None, outs, None, None) == T.ERR_NO_DEVICE
    # in front of every argument check, as for qsx_eval_case
    assert lib.qsx_select_in(T.INT, None, 8, lits, 0, 7, None, None, None, None) == T.ERR_NO_DEVICE
    assert lib.qsx_select_in_char(None, 0, 8, slots, lengths, 99, 0, None, None, None, None) == T.ERR_NO_DEVICE
    assert lib.qsx_bitmap_eval(1, cols, 1, bad_program, 8, None, out.ctypes.data, None, None) == T.ERR_NO_DEVICE
