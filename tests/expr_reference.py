"""The battery of scalar expression programs (qsx_expr_instr_t[], include/qsx.h) and its reference: plain numpy and Python ints.

The contract is the reference's (ScalarBinaryExpression::getAllValues materialises every node): every node is rounded on its own.
evaluate() restates it with the per-node arithmetic the suite already has: a double node is case_reference.run_program over the
two operand arrays (numpy float64 operations, INT / LONG / FLOAT operands converted with .astype(np.float64)), an integer node is
int_expr_reference.i_op (INT op INT wraps to 32 bits, anything with a LONG to 64, / truncates, x / 0 = 0, x / -1 = 0 - x).

A program runs in one of three modes, the three ways the library reads the same instruction array:

    DOUBLE   qsx_eval_expression: ops + - * / on doubles, consts[] doubles.
    LONG     qsx_eval_expression_long: every op an integer op (+ and i+ are synonyms), consts[] exact int64, INT when they fit
             32 bits, else LONG.  case_reference.const_type refuses |c| > 2^53, so such constants are typed here.
    AGG      qsx_agg_config_t::instrs: + - * / double nodes, i+ i- i* i/ integer nodes, consts[] doubles typed by
             case_reference.const_type.

Operands are ("col", index into the program's column names) / ("const", k) / ("temp", t); instructions are (op, dst, a, b).

battery() is the data: named columns whose first rows hold Cartesian products of edge values (every ordered pair of the edges of
d0 x d1, i x j and l x m meets in one row, and so does every edge of l with every edge of i and of f), and whose tail follows the
distributions the conditions of tests/test_expr_reference.py are stated for."""
import collections

import numpy as np

import case_reference as CR
import int_expr_reference as IR

DOUBLE_MODE, LONG_MODE, AGG_MODE = "double", "long", "agg"
SEED = 20260
CHECKED_ROWS = 4096                      # the CPU tests look at these first rows: all edge rows and a tail behind them

col, const, temp = (lambda i: ("col", i)), (lambda i: ("const", i)), (lambda i: ("temp", i))

# ---- the data -----------------------------------------------------------------------------------------------------------------
INF, NAN = float("inf"), float("nan")
D_EDGES = np.array([0.0, -0.0, 1.0, -1.0, INF, -INF, NAN, 5e-324, -5e-324, 2.2250738585072014e-308, 1.7976931348623157e308, 1e200,
                    1e-200, 1e-160, 2.0 ** 53, 2.0 ** 53 + 2, 1 / 3, 0.1], dtype=np.float64)
F_EDGES = np.array([0.0, -0.0, 1e-45, 1.1754942e-38, 3.4028235e38, INF, NAN], dtype=np.float32)
I_EDGES = np.array([0, 1, -1, 2 ** 31 - 1, -2 ** 31, 46341, 65536, -7, 3], dtype=np.int32)
L_EDGES = np.array([0, 1, -1, 2 ** 63 - 1, -2 ** 63, 2 ** 53, 2 ** 53 + 1, -(2 ** 53 + 1), 2 ** 54 + 2, 2 ** 54 + 6, 2 ** 63 - 512,
                    2 ** 63 - 513, 2 ** 32, 3037000500, -3], dtype=np.int64)
ND, NF, NI, NL = D_EDGES.size, F_EDGES.size, I_EDGES.size, L_EDGES.size
# Row r of the edge region holds d0 = D[r % 18], d1 = D[r // 18 % 18]; l = L[r % 15], m = L[r // 15 % 15]; i = I[r // 15 % 9],
# j = I[r // 135 % 9]; f = F[r // 15 % 7].  The longest period is that of (i, j): 15 * 9 * 9 rows.
EDGE_ROWS = NL * NI * NI
assert EDGE_ROWS == 1215 and EDGE_ROWS < CHECKED_ROWS


def battery(rng, n):
    """{name: column} of n rows: d0 d1 d2 DOUBLE, f FLOAT, i j k INT, l m LONG."""
    cols = {
        "d0": np.round(rng.uniform(900, 105000, size=n), 2),
        "d1": rng.integers(0, 11, size=n) / 100.0,
        "d2": rng.normal(size=n) * 1e4,
        "f": rng.normal(size=n).astype(np.float32),
        "i": rng.integers(-2 ** 31, 2 ** 31, size=n).astype(np.int32),
        "j": rng.integers(-2 ** 31, 2 ** 31, size=n).astype(np.int32),
        "l": rng.integers(-2 ** 62, 2 ** 62, size=n),
        "m": rng.integers(-2 ** 62, 2 ** 62, size=n),
        "k": rng.choice(IR.K_VALUES, size=n).astype(np.int32),
    }
    r = np.arange(min(n, EDGE_ROWS))
    cols["d0"][:min(n, ND * ND)] = D_EDGES[r[:ND * ND] % ND]
    cols["d1"][:min(n, ND * ND)] = D_EDGES[r[:ND * ND] // ND % ND]
    cols["l"][:min(n, NL * NL)] = L_EDGES[r[:NL * NL] % NL]
    cols["m"][:min(n, NL * NL)] = L_EDGES[r[:NL * NL] // NL % NL]
    cols["f"][:min(n, NL * NF)] = F_EDGES[r[:NL * NF] // NL % NF]
    cols["i"][:r.size] = I_EDGES[r // NL % NI]
    cols["j"][:r.size] = I_EDGES[r // (NL * NI) % NI]
    return cols


# ---- the programs -------------------------------------------------------------------------------------------------------------
# results: operands read back besides the temps (a bare column: its conversion; a constant)
Program = collections.namedtuple("Program", "name mode cols instrs consts results")

D1 = Program("D1", DOUBLE_MODE, ("d0", "d1", "d2"),                 # Q1's charge: price = d0, disc = d1, and d2 where the tax stands
             [("-", 0, const(0), col(1)),                           # t0 = 1 - disc
              ("*", 1, col(0), temp(0)),                            # t1 = price * t0
              ("+", 2, const(0), col(2)),                           # t2 = 1 + tax
              ("*", 3, temp(1), temp(2))],                          # t3 = t1 * t2
             [1.0], [])
D2 = Program("D2", DOUBLE_MODE, ("d0", "d1", "d2"),                 # a multiply feeding an add and a subtract: what contraction fuses
             [("*", 0, col(0), col(1)),                             # t0 = d0 * d1
              ("+", 1, temp(0), col(2)),                            # t1 = t0 + d2
              ("-", 2, col(2), temp(0)),                            # t2 = d2 - t0
              ("*", 3, temp(1), temp(2))],                          # t3 = t1 * t2
             [], [])
D3 = Program("D3", DOUBLE_MODE, ("d0", "d1", "l", "i", "f"),        # division and operand order
             [("/", 0, col(0), col(1)),                             # t0 = d0 / d1
              ("/", 1, col(1), col(0)),                             # t1 = d1 / d0
              ("/", 2, col(2), col(3)),                             # t2 = l / i        (both converted first)
              ("/", 3, col(4), const(0)),                           # t3 = f / 3.0
              ("-", 4, col(0), col(1)),                             # t4 = d0 - d1
              ("-", 5, col(1), col(0))],                            # t5 = d1 - d0
             [3.0], [])
D4 = Program("D4", DOUBLE_MODE, ("l", "i", "f", "d0", "m"),         # conversions
             [("*", 0, col(0), col(4)),                             # t0 = l * m
              ("*", 1, col(2), col(0)),                             # t1 = f * l
              ("+", 2, col(1), col(3))],                            # t2 = i + d0
             [7.0], [col(0), col(1), col(2), col(3), const(0)])
D5 = Program("D5", DOUBLE_MODE, ("d0", "d1", "d2", "f", "i", "l"),  # the limits: 16 instructions, 8 temps, 8 constants
             [("-", 0, const(0), col(1)),                           # t0 = 1 - d1
              ("*", 1, col(0), temp(0)),                            # t1 = d0 * t0      (defined early, never redefined: read last)
              ("+", 2, temp(1), col(2)),                            # t2 = t1 + d2
              ("*", 3, temp(2), const(1)),                          # t3 = t2 * 0.5
              ("/", 4, temp(3), const(2)),                          # t4 = t3 / 3
              ("*", 5, col(3), const(3)),                           # t5 = f * -2.25
              ("+", 6, col(4), const(4)),                           # t6 = i + 0.001
              ("*", 7, col(5), const(5)),                           # t7 = l * 7
              ("*", 0, temp(0), temp(0)),                           # t0 = t0 * t0      (one temp twice, its own dst, redefined after use)
              ("-", 2, temp(2), temp(4)),                           # t2 = t2 - t4      (reads its own dst, redefined after use)
              ("+", 3, temp(5), temp(6)),                           # t3 = t5 + t6      (redefined after use)
              ("/", 4, temp(7), temp(3)),                           # t4 = t7 / t3
              ("*", 5, temp(0), const(6)),                          # t5 = t0 * 0.1
              ("+", 6, temp(2), const(7)),                          # t6 = t2 + -0.75
              ("-", 7, temp(4), temp(5)),                           # t7 = t4 - t5
              ("*", 0, temp(6), temp(7))],                          # t0 = t6 * t7
             [1.0, 0.5, 3.0, -2.25, 1e-3, 7.0, 0.1, -0.75], [])
DOUBLE_PROGRAMS = {p.name: p for p in (D1, D2, D3, D4, D5)}

I1 = Program("I1", LONG_MODE, ("i", "j"),
             [("+", 0, col(0), col(1)), ("*", 1, col(0), col(1)), ("-", 2, col(0), col(1))], [], [])       # INT, wrap
I2 = Program("I2", LONG_MODE, ("l", "i", "m"),
             [("*", 0, col(0), const(0)),                           # t0 = l * 3
              ("+", 1, temp(0), col(1)),                            # t1 = t0 + i
              ("*", 2, col(0), col(2)),                             # t2 = l * m
              ("-", 3, col(0), col(2))],                            # t3 = l - m
             [3], [])
I3 = Program("I3", LONG_MODE, ("l", "k", "i", "m", "j"),
             [("/", 0, col(0), col(1)),                             # t0 = l / k        (k holds 0 and -1)
              ("/", 1, col(2), col(1)),                             # t1 = i / k
              ("/", 2, col(0), col(3)),                             # t2 = l / m        (INT64_MIN / -1 among the edges)
              ("/", 3, col(2), col(4)),                             # t3 = i / j        (INT32_MIN / -1 among the edges)
              ("/", 4, col(1), col(0))],                            # t4 = k / l        (a small dividend over a large divisor)
             [], [])
I4 = Program("I4", LONG_MODE, ("i", "l"),                           # a constant is an INT operand when it fits 32 bits, else a LONG
             [("+", 0, col(0), const(0)),                           # t0 = i + (2^31 - 1)    INT
              ("+", 1, col(0), const(1)),                           # t1 = i + 2^31          LONG
              ("+", 2, col(0), const(2)),                           # t2 = i + -2^31         INT: i - 2^31 with an operand that is still an INT
              ("+", 3, col(0), const(3)),                           # t3 = i + (-2^31 - 1)   LONG
              ("+", 4, col(1), const(4)),                           # t4 = l + (2^60 + 1)    LONG, the constant is no double
              ("-", 5, col(0), const(2))],                          # t5 = i - -2^31         INT
             [2 ** 31 - 1, 2 ** 31, -2 ** 31, -2 ** 31 - 1, 2 ** 60 + 1], [])
I5A = Program("I5a", LONG_MODE, ("i", "j", "l"),                    # a temp has the type of its latest definition: INT, then LONG
              [("+", 0, col(0), col(1)),                            # t0 = i + j        INT
               ("+", 0, temp(0), col(2)),                           # t0 = t0 + l       LONG
               ("*", 1, temp(0), col(0))],                          # t1 = t0 * i       LONG
              [], [])
I5B = Program("I5b", LONG_MODE, ("i", "j", "l", "m"),               # ... and LONG, then INT
              [("*", 0, col(2), col(3)),                            # t0 = l * m        LONG
               ("*", 0, col(0), col(1)),                            # t0 = i * j        INT
               ("+", 1, temp(0), col(1))],                          # t1 = t0 + j       INT: must narrow
              [], [])
I6 = Program("I6", LONG_MODE, ("i", "l"), [], [7, 2 ** 60 + 1], [col(0), col(1), const(0), const(1)])
LONG_PROGRAMS = {p.name: p for p in (I1, I2, I3, I4, I5A, I5B, I6)}


def fused(program):
    """The program as an aggregation reads it (qsx_agg_config_t::instrs): the integer programs with i+ i- i* i/."""
    if program.mode == DOUBLE_MODE:
        return program._replace(mode=AGG_MODE)
    assert all(abs(c) <= 2 ** 53 for c in program.consts), "the aggregation's consts[] are doubles"
    return program._replace(mode=AGG_MODE, instrs=[("i" + op, dst, a, b) for op, dst, a, b in program.instrs],
                            consts=[float(c) for c in program.consts])


# ---- the evaluator ------------------------------------------------------------------------------------------------------------
def _typed(values, kind):
    """The array run_program takes as a column of that type (it tells INT from LONG by the dtype)."""
    return values.astype(np.int32) if kind == CR.INT else values


def operand(program, cols, o, temps):
    """(values, type) of an operand; integers are held as int64, whatever their type."""
    rows = cols[program.cols[0]].size
    if o[0] == "col":
        v = cols[program.cols[o[1]]]
        kind = CR.NP_TYPE[v.dtype]
        return (v.astype(np.int64) if kind in (CR.INT, CR.LONG) else v), kind
    if o[0] == "const":
        c = program.consts[o[1]]
        if program.mode == LONG_MODE:
            assert isinstance(c, int) and -2 ** 63 <= c < 2 ** 63
            return np.full(rows, c, dtype=np.int64), (CR.INT if IR.const_type(c) == IR.INT else CR.LONG)
        kind = CR.const_type(c) if program.mode == AGG_MODE else CR.DOUBLE
        return (np.full(rows, int(c), dtype=np.int64) if kind != CR.DOUBLE else np.full(rows, float(c), dtype=np.float64)), kind
    assert o[0] == "temp", o
    return temps[o[1]]


def evaluate(program, cols):
    """One {temp: (values, type)} per instruction: the temps as they stand after it.  cols: {name: column}."""
    temps, steps = {}, []
    for op, dst, a, b in program.instrs:
        (va, ta), (vb, tb) = operand(program, cols, a, temps), operand(program, cols, b, temps)
        integer = program.mode == LONG_MODE or op.startswith("i")
        assert not (program.mode == DOUBLE_MODE and op.startswith("i")), "qsx_eval_expression refuses integer instructions"
        if integer:
            assert ta in (CR.INT, CR.LONG) and tb in (CR.INT, CR.LONG), "no implicit double -> integer conversion"
            v, kind = IR.i_op(op[-1], va, IR.INT if ta == CR.INT else IR.LONG, vb, IR.INT if tb == CR.INT else IR.LONG)
            kind = CR.INT if kind == IR.INT else CR.LONG
        else:
            pair = [_typed(va, ta), _typed(vb, tb)]
            v, kind, _ = CR.run_program(pair, [np.zeros(va.size, dtype=bool)] * 2, [(op, 0, col(0), col(1))], [])[0]
            assert kind == CR.DOUBLE and v.dtype == np.float64
        temps = dict(temps)
        temps[dst] = (v, kind)
        steps.append(temps)
    return steps


def result_of(program, cols, o, temps):
    """(values, type) an entry point writes for the result operand `o`: DOUBLE mode converts, LONG mode keeps the type."""
    v, kind = operand(program, cols, o, temps)
    if program.mode == DOUBLE_MODE:
        return _typed(v, kind).astype(np.float64), CR.DOUBLE
    return v, kind


def readbacks(program, cols):
    """[(label, number of instructions to run, result operand, expected values, type)]: every definition step read back through
    the program cut off behind it, every temp after the whole program, and the program's own `results`."""
    steps = evaluate(program, cols)
    out = []
    for k, (op, dst, a, b) in enumerate(program.instrs):
        out.append((f"{program.name} step {k}: t{dst}", k + 1, temp(dst)) + result_of(program, cols, temp(dst), steps[k]))
    last = steps[-1] if steps else {}
    for t in sorted(last):
        out.append((f"{program.name} whole: t{t}", len(program.instrs), temp(t)) + result_of(program, cols, temp(t), last))
    for o in program.results:
        out.append((f"{program.name} whole: {o[0]} {o[1]}", len(program.instrs), o) + result_of(program, cols, o, last))
    return out


# ---- the same program for the C ABI -------------------------------------------------------------------------------------------
def abi_operand(o, first=0):
    """first: the index of the program's first column among the caller's columns (an aggregation's keys come before it)."""
    from quickstep_amd import types as T
    return T.col(first + o[1]) if o[0] == "col" else {"const": T.const, "temp": T.temp}[o[0]](o[1])


def abi_instrs(program, count=None, integer_codes=False, first=0):
    """The first `count` instructions as (op code, dst, Operand, Operand); integer_codes: + - * / as EX_IADD .. EX_IDIV."""
    from quickstep_amd import types as T
    ops = {"+": T.EX_ADD, "-": T.EX_SUB, "*": T.EX_MUL, "/": T.EX_DIV, "i+": T.EX_IADD, "i-": T.EX_ISUB, "i*": T.EX_IMUL, "i/": T.EX_IDIV}
    instrs = program.instrs if count is None else program.instrs[:count]
    return [(ops["i" + op if integer_codes else op], dst, abi_operand(a, first), abi_operand(b, first)) for op, dst, a, b in instrs]


def abi_consts(program):
    from quickstep_amd import types as T
    zero = 0 if program.mode == LONG_MODE else 0.0
    return list(program.consts) + [zero] * (T.MAX_CONSTS - len(program.consts))


def same_bits(got, want):
    """The comparison rule: bit-equal; where the reference is NaN the value must be NaN and its bits are not compared (the sign
    and payload of a generated NaN differ between processors).  Returns the rows that differ."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    if want.dtype != np.float64:
        return np.nonzero(got != want)[0]
    nan = np.isnan(want)
    return np.nonzero(np.where(nan, ~np.isnan(got), got.view(np.uint64) != want.view(np.uint64)))[0]
