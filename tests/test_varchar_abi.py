"""CPU: the VARCHAR entry points (qsx_select_like_var, qsx_select_like_var_blocks, qsx_decode_codes_var, include/qsx.h):
declared, exported, mirrored by the binding, and refusing to compute without a GPU.  QSX_ABI_VERSION did not change: a caller
detects the capability by the presence of the symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from quickstep_amd import types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("qsx_select_like_var", "qsx_select_like_var_blocks", "qsx_decode_codes_var")


def _header():
    return open(os.path.join(ROOT, "include", "qsx.h")).read()


def test_the_header_declares_the_three_functions_and_the_macro():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    assert re.search(r"^#define QSX_MAX_VARCHAR_LENGTH 255$", text, flags=re.M)
    assert "#define QSX_ABI_VERSION 19" in _header()
    # every entry point cites the reference loop it replaces
    for cited in ("PatternMatchingComparators-inl.hpp:190-268", "CompressedTupleStorageSubBlock.hpp:225-300",
                  "CompressionDictionaryLite.hpp:248-290"):
        assert cited in _header(), cited


def test_the_library_exports_them_and_the_binding_lists_them(capi):
    lib = C.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in capi.EXPORTED
    for wrapper in ("select_like_var", "select_like_var_blocks", "decode_codes_var"):
        assert callable(getattr(capi, wrapper)), wrapper
    assert capi.lib.qsx_abi_version() == T.ABI_VERSION == 19


def test_every_call_refuses_to_compute_without_a_gpu(capi):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    offsets = np.array([0, 2], dtype=np.uint32)
    values = np.frombuffer(b"a\0bc\0", dtype=np.uint8).copy()
    codes = np.zeros(8, dtype=np.uint8)
    out = np.zeros(1, dtype=np.uint64)
    field = np.zeros((8, 4), dtype=np.uint8)
    one = lambda a: (C.c_void_p * 1)(a.ctypes.data)
    lib = capi.lib
    assert lib.qsx_select_like_var(offsets.ctypes.data, values.ctypes.data, 2, 5, 4, b"a%", 2, 0, None, out.ctypes.data, None,
                                   None) == T.ERR_NO_DEVICE
    assert lib.qsx_select_like_var_blocks(4, 1, (C.c_int64 * 1)(2), one(offsets), one(values), (C.c_int64 * 1)(5), b"a%", 2, 1, None,
                                          one(out), None, None) == T.ERR_NO_DEVICE
    assert lib.qsx_decode_codes_var(1, codes.ctypes.data, 8, offsets.ctypes.data, values.ctypes.data, 2, 5, 4, field.ctypes.data,
                                    None) == T.ERR_NO_DEVICE
    # QSX_ERR_NO_DEVICE comes first: also in front of the argument checks
    assert lib.qsx_select_like_var(None, None, -1, -1, 0, None, 65, 2, None, None, None, None) == T.ERR_NO_DEVICE
    assert lib.qsx_select_like_var_blocks(0, -1, None, None, None, None, None, 65, 2, None, None, None, None) == T.ERR_NO_DEVICE
    assert lib.qsx_decode_codes_var(3, None, -1, None, None, -1, -1, 0, None, None) == T.ERR_NO_DEVICE
