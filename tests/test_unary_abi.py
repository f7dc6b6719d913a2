"""CPU: the unary-operation entry points (qsx_eval_date_extract, qsx_eval_substring and their run forms, include/qsx.h):
declared, exported, mirrored by the binding, and refusing to compute without a GPU.  QSX_ABI_VERSION did not change: a caller
detects the capability by the presence of the symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from quickstep_amd import types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("qsx_eval_date_extract", "qsx_eval_date_extract_blocks", "qsx_eval_substring", "qsx_eval_substring_blocks")


def _header():
    return open(os.path.join(ROOT, "include", "qsx.h")).read()


def test_the_header_declares_the_functions_and_the_macros():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    assert re.search(r"^#define QSX_DATE_YEAR 0\s*$", text, flags=re.M)
    assert re.search(r"^#define QSX_DATE_MONTH 1\s*$", text, flags=re.M)
    assert "#define QSX_ABI_VERSION 19" in _header()
    # the contract is stated where the caller reads it, next to the reference lines it replaces
    assert "DateExtractOperation.cpp" in _header() and "SubstringOperation.cpp:74-91" in _header()
    assert (T.DATE_YEAR, T.DATE_MONTH) == (0, 1)


def test_the_library_exports_them_and_the_binding_lists_them(capi):
    lib = C.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in capi.EXPORTED
    for wrapper in ("eval_date_extract", "eval_date_extract_blocks", "eval_substring", "eval_substring_blocks"):
        assert callable(getattr(capi, wrapper)), wrapper
    assert capi.lib.qsx_abi_version() == T.ABI_VERSION == 19


def test_every_call_refuses_to_compute_without_a_gpu(capi):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    dates = np.zeros(8, dtype=np.int64)
    years = np.zeros(8, dtype=np.int32)
    col = np.zeros((8, 15), dtype=np.uint8)
    out = np.zeros((8, 2), dtype=np.uint8)
    one = lambda a: (C.c_void_p * 1)(a.ctypes.data)      # noqa: E731
    rows = (C.c_int64 * 1)(8)
    lib = capi.lib
    assert lib.qsx_eval_date_extract(T.DATE_YEAR, dates.ctypes.data, 8, years.ctypes.data, None) == T.ERR_NO_DEVICE
    assert lib.qsx_eval_date_extract_blocks(T.DATE_MONTH, 1, rows, one(dates), one(years), None) == T.ERR_NO_DEVICE
    assert lib.qsx_eval_substring(col.ctypes.data, 15, 8, 0, 2, out.ctypes.data, None) == T.ERR_NO_DEVICE
    assert lib.qsx_eval_substring_blocks(15, 1, rows, one(col), 0, 2, one(out), None) == T.ERR_NO_DEVICE
    # QSX_ERR_NO_DEVICE comes first: also in front of the argument checks
    assert lib.qsx_eval_date_extract(7, None, -1, None, None) == T.ERR_NO_DEVICE
    assert lib.qsx_eval_date_extract(T.DATE_YEAR, None, 0, None, None) == T.ERR_NO_DEVICE
    assert lib.qsx_eval_date_extract_blocks(7, -1, None, None, None, None) == T.ERR_NO_DEVICE
    assert lib.qsx_eval_substring(None, 0, -1, -1, 0, None, None) == T.ERR_NO_DEVICE
    assert lib.qsx_eval_substring(None, 300, 0, 300, 1, None, None) == T.ERR_NO_DEVICE
    assert lib.qsx_eval_substring_blocks(0, -1, None, None, -1, 0, None, None) == T.ERR_NO_DEVICE
