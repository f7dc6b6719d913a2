"""CPU: qsx_select_cmp_columns_blocks is exported, bound, and — like every compute entry point — answers QSX_ERR_NO_DEVICE in
front of every other check on a machine without a gfx950 device."""
import ctypes as C

import pytest

from quickstep_amd import types as T


def test_the_symbol_is_exported_and_bound(capi):
    assert hasattr(capi.lib, "qsx_select_cmp_columns_blocks")
    assert "qsx_select_cmp_columns_blocks" in capi.EXPORTED
    assert callable(capi.select_cmp_columns_blocks)
    assert C.sizeof(capi.OperandCoding) == 3 * C.sizeof(C.c_void_p)      # qsx_operand_coding_t: three pointers


def test_no_device_comes_in_front_of_the_argument_checks(capi):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    fn = capi.lib.qsx_select_cmp_columns_blocks
    # arguments that are wrong in every other respect: CHAR operands, a negative number of blocks, no arrays, op 99
    assert fn(T.CHAR, T.CHAR, -1, None, None, None, None, None, 99, None, None, None, None) == T.ERR_NO_DEVICE
    rows = (C.c_int64 * 1)(-5)
    assert fn(T.DATE, T.INT, 1, rows, None, None, None, None, T.LT, None, None, None, None) == T.ERR_NO_DEVICE
    assert fn(T.INT, T.LONG, 0, None, None, None, None, None, T.LT, None, None, None, None) == T.ERR_NO_DEVICE
