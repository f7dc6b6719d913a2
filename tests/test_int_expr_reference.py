"""The reference of tests/test_gpu_agg_int_expr.py tested on its own (no GPU, no library): i_op against Python-int arithmetic on
the edge values, and the data invariants of int_expr_data on every layout the GPU cases use."""
import itertools
import zlib

import numpy as np
import pytest

import exact_reference as R
import int_expr_reference as X
from exact_reference import LAYOUTS

INT_EDGES = [R.INT32_MIN, R.INT32_MIN + 1, -7, -1, 0, 1, 3, 46341, R.INT32_MAX - 1, R.INT32_MAX]
LONG_EDGES = [R.INT64_MIN, R.INT64_MIN + 1, -2**53 - 1, -2**32, -1, 0, 1, 2**31, 3037000500, 2**53 + 1, R.INT64_MAX - 1, R.INT64_MAX]


def _c_arith(op, x, y, bits):
    """x OP y on `bits`-bit two's-complement integers with Python ints: the rules of include/qsx.h."""
    if op == "/":
        if y == 0:
            v = 0
        elif y == -1:
            v = -x
        else:
            v = abs(x) // abs(y) * (1 if (x < 0) == (y < 0) else -1)
    else:
        v = x + y if op == "+" else x - y if op == "-" else x * y
    return (v + 2**(bits - 1)) % 2**bits - 2**(bits - 1)


@pytest.mark.parametrize("op", "+-*/")
@pytest.mark.parametrize("types", [(X.INT, X.INT), (X.INT, X.LONG), (X.LONG, X.INT), (X.LONG, X.LONG)])
def test_i_op_against_python_ints(op, types):
    ta, tb = types
    pairs = list(itertools.product(INT_EDGES if ta == X.INT else LONG_EDGES, INT_EDGES if tb == X.INT else LONG_EDGES))
    a = np.array([p[0] for p in pairs], dtype=np.int64)
    b = np.array([p[1] for p in pairs], dtype=np.int64)
    got, ty = X.i_op(op, a, ta, b, tb)
    bits = 32 if ta == X.INT and tb == X.INT else 64
    assert ty == (X.INT if bits == 32 else X.LONG) and got.dtype == np.int64
    for (x, y), g in zip(pairs, got.tolist()):
        assert g == _c_arith(op, x, y, bits), (op, x, y, bits, g)


def test_division_rules():
    got, _ = X.i_op("/", np.array([R.INT64_MIN, R.INT64_MIN, 7, -7, 7, -7, 5]), X.LONG, np.array([-1, 0, 2, 2, -2, -2, 0]), X.LONG)
    assert got.tolist() == [R.INT64_MIN, 0, 3, -3, -3, 3, 0]
    got, ty = X.i_op("/", np.array([R.INT32_MIN, R.INT32_MIN, R.INT32_MAX]), X.INT, np.array([-1, 0, -1]), X.INT)
    assert ty == X.INT and got.tolist() == [R.INT32_MIN, 0, -R.INT32_MAX]


def test_constant_types():
    assert X.const_type(3) == X.INT and X.const_type(-2**31) == X.INT and X.const_type(2**31) == X.LONG
    assert X.const_type(5_000_000_000) == X.LONG


GPU_LAYOUTS = ["single", "five", "few", "dense", "midsize", "directory", "growth", "two_level", "lds_flush"]


@pytest.mark.parametrize("layout", GPU_LAYOUTS)
def test_data_invariants_on_every_layout(layout):
    n, groups, order, heavy = LAYOUTS[layout]
    for seed in ("a", "b"):
        rng = np.random.default_rng(zlib.crc32(f"{layout}/{seed}".encode()))
        gid = R.make_gids(rng, n, groups, order, heavy)
        cols, t = X.int_expr_data(rng, gid, groups)                  # (asserts the invariants itself)
        assert cols["j"].dtype == np.int32 and cols["k"].dtype == np.int32 and set(np.unique(cols["k"])) == set(X.K_VALUES.tolist())
        assert t["t0"][0].min() >= R.INT32_MIN and t["t0"][0].max() <= R.INT32_MAX
        # the same nodes with Python ints on a sample of the rows
        for r in rng.integers(0, n, size=200):
            i, j, k, l = (int(cols[c][r]) for c in "ijkl")
            assert int(t["t0"][0][r]) == _c_arith("+", i, j, 32) and int(t["t1"][0][r]) == _c_arith("*", i, j, 32)
            assert int(t["t3"][0][r]) == _c_arith("+", _c_arith("*", l, 3, 64), i, 64)
            assert int(t["t4"][0][r]) == _c_arith("*", l, l, 64) and int(t["t5"][0][r]) == _c_arith("/", l, k, 64)
            assert t["t6"][0][r] == _c_arith("+", i, j, 32) / 2
