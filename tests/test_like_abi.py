"""CPU: the LIKE and code-membership entry points (qsx_select_like, qsx_select_like_blocks, qsx_select_codes_in_set,
qsx_select_codes_in_set_blocks, include/qsx.h): declared, exported, mirrored by the binding, and refusing to compute without
a GPU.  QSX_ABI_VERSION did not change: a caller detects the capability by the presence of the symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from quickstep_amd import types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("qsx_select_like", "qsx_select_like_blocks", "qsx_select_codes_in_set", "qsx_select_codes_in_set_blocks")


def _header():
    return open(os.path.join(ROOT, "include", "qsx.h")).read()


def test_the_header_declares_the_four_functions_and_the_macro():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    assert re.search(r"^#define QSX_MAX_LIKE_PATTERN 64$", text, flags=re.M)
    assert "#define QSX_ABI_VERSION 19" in _header()
    # the one documented deviation from the reference is stated where the caller reads it
    assert "UTF-8" in _header() and "escape" in _header()


def test_the_library_exports_them_and_the_binding_lists_them(capi):
    lib = C.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in capi.EXPORTED
    for wrapper in ("select_like", "select_like_blocks", "select_codes_in_set", "select_codes_in_set_blocks"):
        assert callable(getattr(capi, wrapper)), wrapper
    assert capi.lib.qsx_abi_version() == T.ABI_VERSION == 19


def test_every_call_refuses_to_compute_without_a_gpu(capi):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    col = np.zeros((8, 4), dtype=np.uint8)
    codes = np.zeros(8, dtype=np.uint8)
    words = np.zeros(1, dtype=np.uint64)
    out = np.zeros(1, dtype=np.uint64)
    rows = (C.c_int64 * 1)(8)
    one = lambda a: (C.c_void_p * 1)(a.ctypes.data)
    lib = capi.lib
    assert lib.qsx_select_like(col.ctypes.data, 4, 8, b"a%", 2, 0, None, out.ctypes.data, None, None) == T.ERR_NO_DEVICE
    assert lib.qsx_select_like_blocks(4, 1, rows, one(col), b"a%", 2, 1, None, one(out), None, None) == T.ERR_NO_DEVICE
    assert lib.qsx_select_codes_in_set(1, codes.ctypes.data, 8, words.ctypes.data, 5, None, out.ctypes.data, None, None) == T.ERR_NO_DEVICE
    assert lib.qsx_select_codes_in_set_blocks(1, 1, rows, one(codes), one(words), (C.c_int64 * 1)(5), None, one(out), None,
                                              None) == T.ERR_NO_DEVICE
    # QSX_ERR_NO_DEVICE comes first: also in front of the argument checks
    assert lib.qsx_select_like(None, 0, -1, None, 65, 2, None, None, None, None) == T.ERR_NO_DEVICE
