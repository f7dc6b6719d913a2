"""CPU: tests/expr_reference.py — the battery of expression programs the GPU tests of tests/test_gpu_expression.py run and the
numpy / Python-int reference they compare with — pinned from three sides: every double node equals the correctly rounded exact
result (fractions.Fraction; IEEE's rules written out by hand where an operand is not finite), the programs through the oracle's
qso_eval_expression give the same bits, and the integer rules give the answers worked out by hand.  The rest are conditions on
the data: the battery must be able to tell a contracted, reordered, narrowed or widened node from a right one."""
import math
from fractions import Fraction

import numpy as np
import pytest

import case_reference as CR
import expr_reference as E
from expr_reference import col, const, temp

N = E.CHECKED_ROWS
_cols = {}


def cols():
    if not _cols:
        _cols.update(E.battery(np.random.default_rng(E.SEED), N))
        for c in _cols.values():
            c.setflags(write=False)
    return _cols


def tail(name):
    return cols()[name][E.EDGE_ROWS:]


# ---- correct rounding -----------------------------------------------------------------------------------------------------------
def rounded(q):
    """The double nearest to the Fraction q (float(Fraction) is correctly rounded, subnormals included); beyond the finite range
    the infinity of q's sign."""
    try:
        return float(q)
    except OverflowError:
        return math.inf if q > 0 else -math.inf


def exact_node(op, x, y):
    """x OP y as IEEE 754 binary64 with round-to-nearest-even wants it, for Python floats x and y."""
    if math.isnan(x) or math.isnan(y):
        return math.nan
    if op == "-":
        op, y = "+", -y
    if op == "+":
        if math.isinf(x) or math.isinf(y):
            if math.isinf(x) and math.isinf(y) and x != y:
                return math.nan                                     # inf - inf
            return x if math.isinf(x) else y
        s = Fraction(x) + Fraction(y)
        if s == 0:                                                   # an exact zero sum is +0 unless both terms are -0
            return -0.0 if math.copysign(1.0, x) < 0 and math.copysign(1.0, y) < 0 else 0.0
        return rounded(s)
    sign = math.copysign(1.0, x) * math.copysign(1.0, y)
    if op == "*":
        if math.isinf(x) or math.isinf(y):
            return math.nan if x == 0 or y == 0 else sign * math.inf   # inf * 0
        q = Fraction(x) * Fraction(y)
    else:
        assert op == "/"
        if math.isinf(x):
            return math.nan if math.isinf(y) else sign * math.inf    # inf / inf
        if math.isinf(y):
            return sign * 0.0
        if y == 0:
            return math.nan if x == 0 else sign * math.inf           # 0 / 0, x / 0
        q = Fraction(x) / Fraction(y)
    r = rounded(q)
    return sign * 0.0 if r == 0 else r                              # a zero, exact or by underflow, has the sign of the operands


def exact_double(values, kind):
    """An operand's conversion to double, correctly rounded, by Python's own int -> float (FLOAT -> DOUBLE is exact)."""
    if kind in (CR.INT, CR.LONG):
        return [float(int(v)) for v in values.tolist()]
    return [float(v) for v in values.tolist()]


def test_exact_node_knows_ieee():
    inf, nan = math.inf, math.nan
    bits = lambda v: np.float64(v).view(np.uint64)      # noqa: E731
    for op, x, y, want in [("+", inf, -inf, nan), ("-", inf, inf, nan), ("+", inf, 1.0, inf), ("-", 1.0, inf, -inf), ("*", inf, 0.0, nan),
                           ("*", -inf, 2.0, -inf), ("/", inf, inf, nan), ("/", 0.0, 0.0, nan), ("/", 1.0, -0.0, -inf), ("/", -1.0, inf, -0.0),
                           ("/", inf, -0.0, -inf), ("+", 0.0, -0.0, 0.0), ("+", -0.0, -0.0, -0.0), ("-", -0.0, 0.0, -0.0), ("-", 1.0, 1.0, 0.0),
                           ("*", -0.0, 1.0, -0.0), ("*", 5e-324, -0.1, -0.0), ("*", 5e-324, 0.5, 0.0), ("*", 5e-324, 0.75, 5e-324),
                           ("/", 5e-324, 2.0, 0.0), ("/", -5e-324, 1.5, -5e-324), ("*", 1e200, 1e200, inf), ("*", -1e200, 1e200, -inf),
                           ("+", 1.7976931348623157e308, 1.7976931348623157e308, inf), ("+", 1.7976931348623157e308, 1e291, 1.7976931348623157e308),
                           ("+", 2.0 ** 53, 1.0, 2.0 ** 53), ("+", 2.0 ** 53 + 2, 1.0, 2.0 ** 53 + 4), ("*", 1e-200, 1e-160, 0.0),
                           ("/", 1.0, 3.0, 1 / 3), ("*", 1e-160, 1e-160, 1e-320), ("+", nan, 1.0, nan), ("/", 1.0, nan, nan)]:
        got = exact_node(op, x, y)
        assert (math.isnan(got) and math.isnan(want)) or bits(got) == bits(want), (op, x, y, got, want)


@pytest.mark.parametrize("name", list(E.DOUBLE_PROGRAMS))
def test_every_double_node_is_the_correctly_rounded_exact_result(name):
    program = E.DOUBLE_PROGRAMS[name]
    steps = E.evaluate(program, cols())
    for k, (op, dst, a, b) in enumerate(program.instrs):
        before = steps[k - 1] if k else {}
        x = exact_double(*E.operand(program, cols(), a, before))
        y = exact_double(*E.operand(program, cols(), b, before))
        want = np.array([exact_node(op, p, q) for p, q in zip(x, y)], dtype=np.float64)
        values, kind = steps[k][dst]
        assert kind == CR.DOUBLE
        bad = E.same_bits(values, want)
        assert bad.size == 0, f"{name} step {k}: row {bad[0]}: {x[bad[0]]!r} {op} {y[bad[0]]!r} = {values[bad[0]]!r}, exactly rounded {want[bad[0]]!r}"
    for label, _, o, values, kind in E.readbacks(program, cols()):
        if o[0] == "col":                                            # a bare column: its conversion
            want = np.array(exact_double(*E.operand(program, cols(), o, {})), dtype=np.float64)
            assert E.same_bits(values, want).size == 0, label


@pytest.mark.parametrize("name", list(E.DOUBLE_PROGRAMS))
def test_the_oracle_computes_the_same_bits(oracle, name):
    program = E.DOUBLE_PROGRAMS[name]
    data = [cols()[c] for c in program.cols]
    for label, count, o, want, kind in E.readbacks(program, cols()):
        got = oracle.eval_expression(data, E.abi_instrs(program, count), E.abi_consts(program), E.abi_operand(o))
        bad = E.same_bits(got, want)
        assert bad.size == 0, f"{label}: row {bad[0]}: oracle {got[bad[0]]!r}, reference {want[bad[0]]!r}"


def test_the_comparison_rule_compares_bits_except_where_the_reference_is_nan():
    want = np.array([0.0, -0.0, np.nan, np.inf, 5e-324, 1.0, np.nan])
    assert E.same_bits(want.copy(), want).size == 0
    other_nan = np.array([np.nan]).view(np.uint64) | np.uint64(1 << 63 | 5)                    # another sign and payload: still a NaN
    got = want.copy()
    got[2] = other_nan.view(np.float64)[0]
    assert E.same_bits(got, want).size == 0
    got = np.array([-0.0, 0.0, 1.0, -np.inf, 1e-323, 1.0 + 2.0 ** -52, np.inf])
    assert E.same_bits(got, want).tolist() == [0, 1, 2, 3, 4, 5, 6]                             # a signed zero and an infinity count, a number is no NaN
    assert E.same_bits(np.array([np.nan]), np.array([1.0])).tolist() == [0]
    assert E.same_bits(np.array([1, 2], dtype=np.int32), np.array([1, 3], dtype=np.int32)).tolist() == [1]
    with pytest.raises(AssertionError):
        E.same_bits(np.array([1], dtype=np.int64), np.array([1], dtype=np.int32))


# ---- conditions on the battery ----------------------------------------------------------------------------------------------------
def test_every_ordered_pair_of_edges_meets_in_one_row():
    c = cols()
    pairs = lambda a, b: {(x.tobytes(), y.tobytes()) for x, y in zip(c[a][:E.EDGE_ROWS], c[b][:E.EDGE_ROWS])}       # noqa: E731
    want = lambda p, q: {(x.tobytes(), y.tobytes()) for x in p for y in q}                                          # noqa: E731
    assert want(E.D_EDGES, E.D_EDGES) <= pairs("d0", "d1")
    assert want(E.I_EDGES, E.I_EDGES) <= pairs("i", "j")
    assert want(E.L_EDGES, E.L_EDGES) <= pairs("l", "m")
    assert want(E.L_EDGES, E.I_EDGES) <= pairs("l", "i")             # D3's l / i
    assert want(E.F_EDGES, E.L_EDGES) <= pairs("f", "l")             # D4's f * l
    assert len(want(E.D_EDGES, E.D_EDGES)) == 18 * 18 and len(want(E.L_EDGES, E.L_EDGES)) == 15 * 15 and len(want(E.F_EDGES, E.L_EDGES)) == 7 * 15
    # the smallest sizes the GPU tests run still begin with edges: row 0 pairs the first edges, row 1 the second of d0 and l
    assert c["d0"][1].tobytes() == np.float64(-0.0).tobytes() and c["l"][1] == 1


def test_a_contracted_multiply_add_differs_from_the_reference():
    """t1 = d0 * d1 + d2 and t2 = d2 - d0 * d1 of D2: rounded once (a fused multiply-add) they differ from the reference's two
    roundings in more than a tenth of the tail rows (0.18 with these distributions), so a build that contracts fails D2."""
    steps = E.evaluate(E.D2, cols())
    d0, d1, d2 = (tail(c).tolist() for c in ("d0", "d1", "d2"))
    fused_add = np.array([rounded(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(d0, d1, d2)])
    fused_sub = np.array([rounded(Fraction(z) - Fraction(x) * Fraction(y)) for x, y, z in zip(d0, d1, d2)])
    share_add = np.mean(fused_add != steps[1][1][0][E.EDGE_ROWS:])
    share_sub = np.mean(fused_sub != steps[2][2][0][E.EDGE_ROWS:])
    print(f"singly rounded d0 * d1 + d2 differs in {share_add:.3f}, d2 - d0 * d1 in {share_sub:.3f} of the tail rows")
    assert share_add > 0.10 and share_sub > 0.10


def test_a_division_turned_into_a_reciprocal_multiply_differs():
    d0, d2 = tail("d0"), tail("d2")
    share = np.mean(d0 * (1.0 / d2) != d0 / d2)
    print(f"d0 * (1 / d2) != d0 / d2 in {share:.3f} of the tail rows")
    assert share > 0.10


def test_the_long_column_asks_the_conversion_to_round():
    l = tail("l")
    not_a_double = np.mean([float(v) != v for v in l.tolist()])
    through_float = np.mean(l.astype(np.float64) != l.astype(np.float32).astype(np.float64))
    print(f"l is no double in {not_a_double:.3f}, double(l) != double(float(l)) in {through_float:.3f} of the tail rows")
    assert not_a_double > 0.9 and through_float > 0.9
    # both round-to-even ties are among the edges: 2^53 + 1 rounds down, 2^54 + 6 up
    edges = E.L_EDGES.tolist()
    assert 2 ** 53 + 1 in edges and 2 ** 54 + 6 in edges and -(2 ** 53 + 1) in edges
    conv = dict(zip(edges, E.L_EDGES.astype(np.float64).tolist()))
    assert conv[2 ** 53 + 1] == 2.0 ** 53 and conv[-(2 ** 53 + 1)] == -2.0 ** 53 and conv[2 ** 54 + 6] == 2.0 ** 54 + 8
    assert conv[2 ** 54 + 2] == 2.0 ** 54 and conv[2 ** 63 - 512] == 2.0 ** 63 and conv[2 ** 63 - 513] == 2.0 ** 63 - 1024


def test_the_integer_columns_wrap_and_divide_by_zero_and_minus_one():
    i, j = tail("i").astype(np.int64), tail("j").astype(np.int64)
    wraps = np.mean((i + j) != (i + j).astype(np.int32))
    print(f"i + j wraps in {wraps:.3f} of the tail rows")
    assert wraps > 0.2
    t2 = E.evaluate(E.I2, cols())[2][2][0][E.EDGE_ROWS:]
    assert all(int(a) * int(b) != int(p) for a, b, p in zip(tail("l").tolist(), tail("m").tolist(), t2.tolist())), "an l * m that fits"
    assert np.any(cols()["k"] == 0) and np.any(cols()["k"] == -1)


def test_d5_reaches_the_limits():
    from quickstep_amd import types as T
    instrs = E.D5.instrs
    assert len(instrs) == T.MAX_INSTRS and {dst for _, dst, _, _ in instrs} == set(range(T.MAX_TEMPS))
    used = {o[1] for _, _, a, b in instrs for o in (a, b) if o[0] == "const"}
    assert used == set(range(T.MAX_CONSTS)) and len(E.D5.consts) == T.MAX_CONSTS
    redefined_after_use = set()
    for k, (_, dst, _, _) in enumerate(instrs):
        first = next(n for n, ins in enumerate(instrs) if ins[1] == dst)
        if first < k and any(temp(dst) in (a, b) for _, _, a, b in instrs[first + 1:k + 1]):
            redefined_after_use.add(dst)
    assert len(redefined_after_use) >= 2
    assert any(a == b == temp(a[1]) for _, _, a, b in instrs if a[0] == "temp")
    assert any(temp(dst) in (a, b) for _, dst, a, b in instrs)
    assert [dst for _, dst, _, _ in instrs].count(1) == 1 and instrs[1][1] == 1          # t1: defined by the second instruction only


# ---- the integer rules, by hand ---------------------------------------------------------------------------------------------------
def one(op, a, b, consts=()):
    """a OP b over two one-row columns (numpy scalars of the column type) or constants (Python ints, given as consts)."""
    data, names, operands = {}, [], []
    for name, v in (("a", a), ("b", b)):
        if isinstance(v, tuple):
            operands.append(v)
        else:
            data[name] = np.array([v])
            operands.append(col(len(names)))
            names.append(name)
    if not names:
        data, names = {"z": np.zeros(1, dtype=np.int32)}, ["z"]
    program = E.Program("hand", E.LONG_MODE, tuple(names), [(op, 0, operands[0], operands[1])], list(consts), [])
    values, kind = E.evaluate(program, data)[0][0]
    return int(values[0]), kind


def test_hand_written_integer_expectations():
    i32, i64 = np.int32, np.int64
    assert one("/", i32(-2 ** 31), i32(-1)) == (-2 ** 31, CR.INT)
    assert one("/", i64(-2 ** 63), i64(-1)) == (-2 ** 63, CR.LONG)
    assert one("/", i64(-2 ** 63), i32(-1)) == (-2 ** 63, CR.LONG)
    assert one("/", i32(-2 ** 31), i64(-1)) == (2 ** 31, CR.LONG)                      # as a LONG it fits
    assert one("/", i32(-7), i32(2)) == (-3, CR.INT) and one("/", i32(7), i32(-2)) == (-3, CR.INT)
    assert one("/", i64(-7), i32(2)) == (-3, CR.LONG) and one("/", i32(7), i64(2)) == (3, CR.LONG)
    assert one("/", i32(5), i32(0)) == (0, CR.INT) and one("/", i64(-2 ** 63), i32(0)) == (0, CR.LONG) and one("/", i32(0), i32(0)) == (0, CR.INT)
    assert one("/", i32(3), i64(2 ** 62)) == (0, CR.LONG) and one("/", i32(-1), i64(-2 ** 63)) == (0, CR.LONG)
    assert one("*", i32(46341), i32(46341)) == (-2147479015, CR.INT)
    assert one("*", i64(46341), i32(46341)) == (46341 * 46341, CR.LONG)
    assert one("*", i64(3037000500), i64(3037000500)) == (3037000500 ** 2 - 2 ** 64, CR.LONG) and 3037000500 ** 2 - 2 ** 64 < 0
    assert one("+", i32(2 ** 31 - 1), i32(1)) == (-2 ** 31, CR.INT) and one("-", i32(-2 ** 31), i32(1)) == (2 ** 31 - 1, CR.INT)
    assert one("+", i64(2 ** 63 - 1), i32(1)) == (-2 ** 63, CR.LONG)
    # a constant is an INT operand when it fits 32 bits, else a LONG; beyond 2^53 it is still exact
    assert one("+", i32(1), const(0), [2 ** 31 - 1]) == (-2 ** 31, CR.INT)
    assert one("+", i32(1), const(0), [2 ** 31]) == (2 ** 31 + 1, CR.LONG)
    assert one("+", i32(-1), const(0), [-2 ** 31]) == (2 ** 31 - 1, CR.INT)
    assert one("+", i32(-1), const(0), [-2 ** 31 - 1]) == (-2 ** 31 - 2, CR.LONG)
    assert one("+", i64(2), const(0), [2 ** 60 + 1]) == (2 ** 60 + 3, CR.LONG)
    assert one("*", const(0), const(1), [65536, 65536]) == (0, CR.INT)


def test_the_battery_holds_the_hand_written_cases():
    """The rows of the battery where the edges above meet, read out of the programs' reference."""
    c = cols()
    row = lambda a, x, b, y: int(np.nonzero((c[a] == x) & (c[b] == y))[0][0])       # noqa: E731
    t1 = E.evaluate(E.I1, c)[-1][1]
    assert t1[1] == CR.INT and t1[0][row("i", 46341, "j", 46341)] == -2147479015
    last = E.evaluate(E.I3, c)[-1]
    assert last[3][1] == CR.INT and last[3][0][row("i", -2 ** 31, "j", -1)] == -2 ** 31
    assert last[2][1] == CR.LONG and last[2][0][row("l", -2 ** 63, "m", -1)] == -2 ** 63
    assert last[2][0][row("l", 2 ** 63 - 1, "m", 0)] == 0 and last[3][0][row("i", -7, "j", 0)] == 0
    assert last[3][0][row("i", -7, "j", 3)] == -2
    t2 = E.evaluate(E.I2, c)[-1][2]
    assert t2[0][row("l", 3037000500, "m", 3037000500)] == 3037000500 ** 2 - 2 ** 64


def test_a_temp_has_the_type_of_its_latest_definition():
    c = cols()
    assert [s[t][1] for t, s in zip((0, 1, 2, 3, 4, 5), E.evaluate(E.I4, c))] == [CR.INT, CR.LONG, CR.INT, CR.LONG, CR.LONG, CR.INT]
    a, b = E.evaluate(E.I5A, c), E.evaluate(E.I5B, c)
    assert [a[0][0][1], a[1][0][1], a[2][1][1]] == [CR.INT, CR.LONG, CR.LONG]
    assert [b[0][0][1], b[1][0][1], b[2][1][1]] == [CR.LONG, CR.INT, CR.INT]
    i, j = c["i"].astype(np.int64), c["j"].astype(np.int64)
    assert np.array_equal(b[2][1][0], ((i * j).astype(np.int32).astype(np.int64) + j).astype(np.int32).astype(np.int64))
    assert np.mean(b[2][1][0] != (i * j).astype(np.int32).astype(np.int64) + j) > 0.2        # unnarrowed, t1 would differ
    # the earlier snapshots are not rewritten by the redefinition
    assert a[0][0][0] is not a[1][0][0] and np.array_equal(a[0][0][0], (i + j).astype(np.int32))


def test_case_reference_still_refuses_a_constant_beyond_2_53():
    """Why the int64 constants are typed in expr_reference: case_reference takes them for doubles."""
    with pytest.raises(AssertionError):
        CR.run_program([np.zeros(1, dtype=np.int64)], [np.zeros(1, dtype=bool)], [("i+", 0, col(0), const(0))], [2 ** 60 + 1])
    assert CR.const_type(2 ** 60 + 1) == CR.DOUBLE


def test_the_fused_forms_keep_their_constants_exact():
    for name in ("I1", "I2", "I3"):
        f = E.fused(E.LONG_PROGRAMS[name])
        assert f.mode == E.AGG_MODE and all(op.startswith("i") for op, _, _, _ in f.instrs)
        want, got = E.evaluate(E.LONG_PROGRAMS[name], cols()), E.evaluate(f, cols())
        for w, g in zip(want, got):
            assert all(w[t][1] == g[t][1] and np.array_equal(w[t][0], g[t][0]) for t in w)
    with pytest.raises(AssertionError):
        E.fused(E.I4)
