"""The reference of integer aggregate arguments (QSX_EX_IADD .. IDIV of include/qsx.h): plain numpy and Python ints.

i_op() is one node of an integer expression as the reference's ArithmeticBinaryOperators compute it on C++ int / long:
INT op INT is an INT (32-bit two's-complement wrap-around), anything with a LONG a LONG (64-bit wrap-around), division truncates
toward zero, x / 0 = 0 and x / -1 = 0 - x wrapped.  The data is exact_reference.family_c (`i` INT, `l` LONG) plus `j` (INT,
uniform over the full range) and `k` (INT, from K_VALUES); nodes() evaluates the temps the tests aggregate:

    t0 = i + j (INT)     t1 = i * j (INT)     t2 = l * 3 (LONG)     t3 = t2 + i (LONG)     t4 = l * l (LONG)
    t5 = l / k (LONG)    t6 = t0 * 0.5 (a double node over an integer temp)

and asserts what makes a wrong evaluation fail (see int_expr_data)."""
import numpy as np

import exact_reference as R

INT, LONG = "int", "long"
K_VALUES = np.array([-7, -1, 0, 1, 3, 50], dtype=np.int32)


def _wrap64(values):
    """Python ints -> int64 array, two's complement."""
    return np.array([(int(v) + 2**63) % 2**64 - 2**63 for v in values], dtype=np.int64)


def i_op(op, a, type_a, b, type_b):
    """(int64 values, type) of a OP b; a, b: int64 arrays (or scalars) holding INT / LONG values; op: one of + - * /."""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64))
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if op in "+-*":
        ua, ub = a.view(np.uint64), b.view(np.uint64)
        with np.errstate(over="ignore"):
            r = (ua + ub if op == "+" else ua - ub if op == "-" else ua * ub).view(np.int64)
    else:
        assert op == "/"
        out = []
        for x, y in zip(a.tolist(), b.tolist()):
            if y == 0:
                out.append(0)
            elif y == -1:
                out.append(-x)
            else:
                q = abs(x) // abs(y)
                out.append(q if (x < 0) == (y < 0) else -q)
        r = _wrap64(out)
    if type_a == INT and type_b == INT:
        return r.astype(np.int32).astype(np.int64), INT
    return r, LONG


def const_type(c):
    return INT if -2**31 <= c < 2**31 else LONG


def nodes(cols):
    """{temp name: (values, type)}: int64 arrays for the integer temps, float64 for t6."""
    i, j, k, l = (cols[c].astype(np.int64) for c in "ijkl")
    t = {}
    t["t0"] = i_op("+", i, INT, j, INT)
    t["t1"] = i_op("*", i, INT, j, INT)
    t["t2"] = i_op("*", l, LONG, 3, const_type(3))
    t["t3"] = i_op("+", t["t2"][0], t["t2"][1], i, INT)
    t["t4"] = i_op("*", l, LONG, l, LONG)
    t["t5"] = i_op("/", l, LONG, k, INT)
    t["t6"] = (t["t0"][0].astype(np.float64) * 0.5, "double")      # (|t0| < 2^31: the conversion and the halving are exact)
    assert [t[x][1] for x in ("t0", "t1", "t2", "t3", "t4", "t5")] == [INT, INT, LONG, LONG, LONG, LONG]
    return t


def _is_double(s):
    return int(float(s)) == s


def int_expr_data(rng, gid, groups):
    """family_c's `i` and `l` plus `j` and `k`, and the temps.  Asserts:

    - i + j wraps in more than 0.3 of the rows: evaluated in double, or in 64 bits without narrowing, it is wrong there;
    - every l * l differs from the Python-int product (all of them wrap);
    - with two groups and more, one group's SUM(t3) lies in (2^53, 2^63) and one in (-2^63, -2^53), neither of them a double (one
      group: the positive one only), and sum |t3| < 2^63 in every group, so that no partial sum of any order wraps;
    - k contains 0 and -1, and 2 sum |t6| < 2^53 in every group: multiples of 1/2 below 2^31 whose every partial sum is exact, so
      every summation order gives the same double and SUM(t6) is compared with ==.

    A heavy group whose SUM(t3) happens to be a double gets one row's `i` moved by one (an odd sum beyond 2^53 is none)."""
    cols = R.family_c(rng, gid, groups)
    n = gid.size
    cols["j"] = rng.integers(R.INT32_MIN, R.INT32_MAX, size=n, endpoint=True).astype(np.int32)
    cols["k"] = rng.choice(K_VALUES, size=n).astype(np.int32)
    for g in range(min(groups, 2)):
        rows = np.nonzero((gid == g) & (np.abs(cols["i"].astype(np.int64)) > 1) & (np.abs(cols["i"].astype(np.int64)) < 2**30))[0]
        s = R.int_group_sums(gid, nodes(cols)["t3"][0], groups)[g]
        if abs(s) > 2**53 and _is_double(s) and rows.size:
            cols["i"][rows[0]] += 1
    t = nodes(cols)
    i64, j64, l64 = (cols[c].astype(np.int64) for c in "ijl")
    assert np.mean(i64 + j64 != t["t0"][0]) > 0.3, "i + j hardly ever wraps"
    assert all(int(a) * int(a) != int(b) for a, b in zip(l64[:4096], t["t4"][0][:4096])) and np.all(np.abs(l64) >= 2**32), "an l * l that fits"
    s3 = R.int_group_sums(gid, t["t3"][0], groups)
    assert max(R.int_group_sums(gid, np.abs(t["t3"][0]), groups)) < 2**63, "a partial sum of t3 could wrap"
    assert any(2**53 < s < 2**63 and not _is_double(s) for s in s3), "no SUM(t3) beyond 2^53 that is not a double"
    if groups >= 2:
        assert any(-2**63 < s < -2**53 and not _is_double(s) for s in s3), "no negative SUM(t3) beyond 2^53 that is not a double"
    assert np.any(cols["k"] == 0) and np.any(cols["k"] == -1)
    assert max(R.int_group_sums(gid, np.abs(t["t0"][0]), groups)) < 2**53, "SUM(t6) depends on the order of summation"
    return cols, t


# ---- the plans (value columns i, j, k, l behind the key columns, in that order) ---------------------------------------------------
NAMES = ["i", "j", "k", "l"]
OPERANDS = {"t0": ("i", "j"), "t1": ("i", "j"), "t3": ("l", "i"), "t4": ("l",), "t5": ("l", "k"), "t6": ("i", "j"), "d0": ("i", "j"),
            "i": ("i",)}
PLANS = {
    # purely integer
    "E1": [("sum", "t0"), ("avg", "t0"), ("min", "t0"), ("max", "t0"), ("sum", "t3"), ("avg", "t3"), ("count", None)],
    "E2": [("sum", "t1"), ("min", "t4"), ("max", "t4"), ("sum", "t5"), ("sum", "t6"), ("sum", "i"), ("count", None)],
    # no integer instruction: d0 = i + j in double, the behaviour before the integer instructions existed
    "PLAIN": [("sum", "d0"), ("avg", "d0"), ("min", "d0"), ("max", "d0"), ("count", None)],
}


def plan_program(plan, first):
    """(instrs, consts, {argument name: operand}) of a plan whose value columns start at column `first`."""
    from quickstep_amd import types as T
    i, j, k, l = (T.col(first + n) for n in range(4))
    if plan == "E1":
        instrs = [(T.EX_IADD, 0, i, j), (T.EX_IMUL, 2, l, T.const(0)), (T.EX_IADD, 3, T.temp(2), i)]
    elif plan == "E2":
        instrs = [(T.EX_IMUL, 1, i, j), (T.EX_IMUL, 4, l, l), (T.EX_IDIV, 5, l, k), (T.EX_IADD, 0, i, j), (T.EX_MUL, 6, T.temp(0), T.const(1))]
    else:
        assert plan == "PLAIN"
        instrs = [(T.EX_ADD, 0, i, j)]
    args = {f"t{n}": T.temp(n) for n in range(7)}
    args.update(d0=T.temp(0), i=i)
    return instrs, [3.0, 0.5], args


def make_config(plan, key_layout, strategy, est=0, num_entries=0, nullable=(), code_widths=None):
    """The qsx_agg_config_t of a plan behind `key_layout` key columns; nullable / code_widths: by value column name."""
    from quickstep_amd import types as T
    fn = {"sum": T.AGG_SUM, "avg": T.AGG_AVG, "min": T.AGG_MIN, "max": T.AGG_MAX, "count": T.AGG_COUNT_STAR}
    first = len(key_layout)
    instrs, consts, args = plan_program(plan, first)
    layout = list(key_layout) + [(T.INT, None), (T.INT, None), (T.INT, None), (T.LONG, None)]
    widths = None if code_widths is None else [0] * first + [code_widths.get(c, 0) for c in NAMES]
    return T.make_agg_config(strategy, layout, keys=list(range(first)), instrs=instrs, consts=consts,
                             aggs=[(fn[f], None if a is None else args[a]) for f, a in PLANS[plan]], est_groups=est,
                             num_entries=num_entries, code_widths=widths, nullable=[first + NAMES.index(c) for c in nullable])


# dtype of every aggregate's output column: what the reference's catalog says
EXPECTED_DTYPES = {
    "E1": ["int64", "float64", "int32", "int32", "int64", "float64", "int64"],
    "E2": ["int64", "int64", "int64", "int64", "float64", "int64", "int64"],
    "PLAIN": ["float64", "float64", "float64", "float64", "int64"],
}
