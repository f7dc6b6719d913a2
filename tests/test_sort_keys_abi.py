"""CPU: the ORDER BY entry points with NULL ordering and CHAR(n) keys (qsx_sort_permutation_keys / qsx_sort_top_k_keys,
include/qsx.h): declared, exported, mirrored by the binding, and refusing to compute without a GPU.  QSX_ABI_VERSION did not
change: a caller detects the capability by the presence of the symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from quickstep_amd import types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("qsx_abi_sizeof_sort_key", "qsx_sort_permutation_keys", "qsx_sort_top_k_keys")


def _header():
    return open(os.path.join(ROOT, "include", "qsx.h")).read()


def test_the_header_declares_the_struct_and_the_three_functions():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
    struct = re.search(r"typedef struct qsx_sort_key \{(.*?)\} qsx_sort_key_t;", text, flags=re.S)
    assert struct is not None
    fields = re.findall(r"(\w+)\s*;", struct.group(1))
    assert fields == ["col_dev", "null_bitmap_dev", "type", "width", "descending", "nulls_first"]
    assert fields == [f[0] for f in T.SortKey._fields_]
    assert "#define QSX_ABI_VERSION 19" in _header()


def test_the_library_exports_them_and_the_binding_lists_them(capi):
    lib = C.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in capi.EXPORTED
    assert callable(capi.sort_permutation_keys) and callable(capi.sort_top_k_keys)


def test_the_struct_mirror_has_the_librarys_size(capi):
    assert capi.lib.qsx_abi_sizeof_sort_key() == C.sizeof(T.SortKey) == 32
    assert capi.lib.qsx_abi_version() == T.ABI_VERSION == 19


def test_both_calls_refuse_to_compute_without_a_gpu(capi):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    col = np.arange(8, dtype=np.int32)
    out = np.zeros(8, dtype=np.int32)
    key = T.SortKey(col.ctypes.data, None, T.INT, 0, 0, 0)
    assert capi.lib.qsx_sort_permutation_keys(1, C.byref(key), 8, out.ctypes.data, None, 0, None) == T.ERR_NO_DEVICE
    assert capi.lib.qsx_sort_top_k_keys(1, C.byref(key), 8, 3, out.ctypes.data, None, 0, None) == T.ERR_NO_DEVICE
