"""The reference of searched CASE expressions (qsx_eval_case of include/qsx.h): plain numpy.

A restatement of ScalarCaseExpression::getAllValues (expressions/scalar/ScalarCaseExpression.cpp:273-350):

  - the rows a WHEN takes are the rows its predicate holds on among those no earlier WHEN took (first match wins), the rest
    go to ELSE;
  - every result expression is evaluated over ITS OWN rows only (here: the shared program runs on the sub-arrays of those
    rows), so a NULL in a column that only other branches read is never looked at;
  - every node is materialised on its own: double nodes are numpy float64 operations (no contraction), integer nodes are
    int_expr_reference.i_op (INT wraps to 32 bits, x / 0 = 0, x / -1 = 0 - x); a node is NULL when any operand is;
  - the pieces are cast to the unified type (Resolver.cpp:2819-2829: INT -> LONG sign-extends, INT / LONG / FLOAT -> DOUBLE
    converts) and multiplexed into one column; a NULL row holds 0.

Operands are tuples: ("col", c), ("const", k), ("temp", t), ("null",).  Instructions are (op, dst, a, b) with op one of
"+ - * /" (double) or "i+ i- i* i/" (integer)."""
import numpy as np

import int_expr_reference as IR

INT, LONG, FLOAT, DOUBLE = "int", "long", "float", "double"
NP_TYPE = {np.dtype(np.int32): INT, np.dtype(np.int64): LONG, np.dtype(np.float32): FLOAT, np.dtype(np.float64): DOUBLE}
OUT_DTYPE = {INT: np.int32, LONG: np.int64, DOUBLE: np.float64}


def const_type(c):
    """The type of a constant as an operand: INT / LONG when integral (|c| <= 2^53), else DOUBLE."""
    c = float(c)
    if np.isfinite(c) and c == int(c) and abs(c) <= 2.0 ** 53:
        return INT if -2 ** 31 <= int(c) < 2 ** 31 else LONG
    return DOUBLE


def _as_double(values, kind):
    return values.astype(np.float64)            # INT / LONG (held as int64), FLOAT and DOUBLE alike: one rounding at most


def _operand(o, cols, nulls, consts, temps, rows):
    """(values, type, is-null) of an operand over `rows` rows; integers are held as int64."""
    if o[0] == "col":
        v = cols[o[1]]
        kind = NP_TYPE[v.dtype]
        return (v.astype(np.int64) if kind in (INT, LONG) else v), kind, nulls[o[1]]
    if o[0] == "const":
        c = consts[o[1]]
        kind = const_type(c)
        v = np.full(rows, int(c), dtype=np.int64) if kind != DOUBLE else np.full(rows, float(c), dtype=np.float64)
        return v, kind, np.zeros(rows, dtype=bool)
    assert o[0] == "temp", o
    return temps[o[1]]


def run_program(cols, nulls, instrs, consts):
    """{temp: (values, type, is-null)} after the program, every node on its own."""
    rows = cols[0].size if cols else 0
    temps = {}
    for op, dst, a, b in instrs:
        va, ta, na = _operand(a, cols, nulls, consts, temps, rows)
        vb, tb, nb = _operand(b, cols, nulls, consts, temps, rows)
        if op.startswith("i"):
            assert ta in (INT, LONG) and tb in (INT, LONG), "no implicit double -> integer conversion"
            v, kind = IR.i_op(op[1], va, IR.INT if ta == INT else IR.LONG, vb, IR.INT if tb == INT else IR.LONG)
            kind = INT if kind == IR.INT else LONG
        else:
            x, y = _as_double(va, ta), _as_double(vb, tb)
            with np.errstate(all="ignore"):
                v = x + y if op == "+" else x - y if op == "-" else x * y if op == "*" else x / y
            kind = DOUBLE
        temps[dst] = (v, kind, na | nb)
    return temps


def cast(values, kind, out_type):
    """The resolver's Cast of a branch to the unified type."""
    if out_type == DOUBLE:
        return _as_double(values, kind)
    assert kind in (INT, LONG) and not (out_type == INT and kind == LONG), "the Cast never narrows"
    return values.astype(OUT_DTYPE[out_type])


def eval_case(cols, col_nulls, instrs, consts, values, whens, out_type):
    """(out, is-null): out an array of OUT_DTYPE[out_type], NULL rows 0.  cols: numpy arrays; col_nulls: None or one bool array
    (or None) per column; values: the THEN operand of every WHEN, then the ELSE operand; whens: one bool array per WHEN."""
    n = whens[0].size
    nulls = [np.zeros(n, dtype=bool) if col_nulls is None or col_nulls[c] is None else np.asarray(col_nulls[c], dtype=bool)
             for c in range(len(cols))]
    assert len(values) == len(whens) + 1
    out = np.zeros(n, dtype=OUT_DTYPE[out_type])
    out_null = np.zeros(n, dtype=bool)
    remaining = np.ones(n, dtype=bool)          # else_matches
    pieces = []
    for w in whens:
        pieces.append(np.asarray(w, dtype=bool) & remaining)
        remaining = remaining & ~pieces[-1]
    pieces.append(remaining)
    for match, value in zip(pieces, values):
        idx = np.nonzero(match)[0]
        if idx.size == 0:
            continue
        if value[0] == "null":
            out_null[idx] = True
            continue
        sub_cols = [c[idx] for c in cols]
        sub_nulls = [m[idx] for m in nulls]
        temps = run_program(sub_cols, sub_nulls, instrs, consts)
        v, kind, isnull = _operand(value, sub_cols, sub_nulls, consts, temps, idx.size)
        out[idx] = np.where(isnull, 0, cast(v, kind, out_type))
        out_null[idx] = isnull
    return out, out_null


def pack_bits(bits):
    """A bool array as TupleIdSequence words: uint64, bit i of the sequence is bit 63 - (i & 63) of word i >> 6, trailing bits 0."""
    bits = np.asarray(bits, dtype=bool)
    words = (bits.size + 63) // 64
    padded = np.zeros(max(words, 1) * 64, dtype=np.uint8)
    padded[:bits.size] = bits
    packed = np.packbits(padded.reshape(-1, 64), axis=1, bitorder="big")      # 8 bytes per word, most significant first
    return packed.view(">u8").astype(np.uint64).reshape(-1)[:max(words, 1)]


def load_golden_case(case):
    """A case of tests/golden/case_unittest.json as eval_case arguments plus (expected values, expected is-null)."""
    dtypes = {INT: np.int32, LONG: np.int64, FLOAT: np.float32, DOUBLE: np.float64}
    cols = [np.array(c["values"], dtype=dtypes[c["type"]]) for c in case["cols"]]
    col_nulls = [None if "nulls" not in c else np.array(c["nulls"], dtype=bool) for c in case["cols"]]
    if all(m is None for m in col_nulls):
        col_nulls = None
    tup = lambda o: tuple(o)      # noqa: E731
    instrs = [(op, dst, tup(a), tup(b)) for op, dst, a, b in case["instrs"]]
    values = [tup(v) for v in case["values"]]
    whens = [np.array(w, dtype=bool) for w in case["whens"]]
    expect = np.array(case["expect"], dtype=OUT_DTYPE[case["out_type"]])
    expect_null = np.array(case["expect_null"], dtype=bool)
    return (cols, col_nulls, instrs, case["consts"], values, whens, case["out_type"]), expect, expect_null


# ---- the same program for the C ABI ---------------------------------------------------------------------------------------
def abi_program(instrs, values, out_type):
    """(instrs, values, out_type) as quickstep_amd.types operands / op codes."""
    from quickstep_amd import types as T
    ops = {"+": T.EX_ADD, "-": T.EX_SUB, "*": T.EX_MUL, "/": T.EX_DIV, "i+": T.EX_IADD, "i-": T.EX_ISUB, "i*": T.EX_IMUL, "i/": T.EX_IDIV}

    def opd(o):
        return T.null() if o[0] == "null" else {"col": T.col, "const": T.const, "temp": T.temp}[o[0]](o[1])
    return ([(ops[op], dst, opd(a), opd(b)) for op, dst, a, b in instrs], [opd(v) for v in values],
            {INT: T.INT, LONG: T.LONG, DOUBLE: T.DOUBLE}[out_type])
