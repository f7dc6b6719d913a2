"""CPU: the checker of predicate trees (tests/predicate_reference.py) against the reference's own result tables
(tests/golden/predicate_unittest.json: Select.test:838-862 and NULL cases derived from the cited source lines), its two
evaluations against each other on random trees, and the compiled postfix program against both."""
import numpy as np
import pytest

import predicate_reference as P


def _tree(obj):
    """JSON lists -> the tuples of predicate_reference."""
    kind = obj[0]
    if kind == "cmp":
        return ("cmp", obj[1], obj[2], obj[3])
    if kind == "in":
        return ("in", obj[1], list(obj[2]))
    if kind == "not":
        return ("not", _tree(obj[1]))
    return (kind, [_tree(child) for child in obj[1]])


def test_in_and_not_in_reproduce_the_reference_tables(golden):
    g = golden["predicate_unittest"]
    series = np.array(g["series"], dtype=np.int32)
    assert series[P.in_rows(series, g["in_list"])].tolist() == g["in_result"]
    assert series[P.in_rows(series, g["in_list"], negate=True)].tolist() == g["not_in_result"]
    columns = {"i": series}
    assert series[P.eval_tree(("in", "i", g["in_list"]), columns)].tolist() == g["in_result"]
    assert series[P.eval_tree(("not", ("in", "i", g["in_list"])), columns)].tolist() == g["not_in_result"]
    # the same as the disjunction of equalities InValueList::concretize builds
    as_or = ("or", [("cmp", "i", "=", v) for v in g["in_list"]])
    assert series[P.eval_tree(as_or, columns)].tolist() == g["in_result"]


def test_not_over_null_selects_the_row(golden):
    g = golden["predicate_unittest"]["derived_null_cases"]
    nulls = {"x": np.array([v is None for v in g["values"]])}
    columns = {"x": np.array([0 if v is None else v for v in g["values"]], dtype=np.int32)}
    for case in g["cases"]:
        tree = _tree(case["tree"])
        assert np.nonzero(P.eval_tree(tree, columns, nulls))[0].tolist() == case["selected_rows"], case
        assert [i for i in range(len(g["values"])) if P.eval_tree_row(tree, columns, nulls, i)] == case["selected_rows"], case


def test_float_equality_and_char_equality():
    col = np.array([0.0, -0.0, np.nan, 1.5], dtype=np.float64)
    assert P.in_rows(col, [0.0]).tolist() == [True, True, False, False]
    assert P.in_rows(col, [np.nan, 1.5]).tolist() == [False, False, False, True]
    assert P.in_rows(col, [np.nan], negate=True).tolist() == [True, True, True, True]
    chars = np.frombuffer(b"MAIL\0xSHIP\0\0AIR\0\0\0MAILS\0", dtype=np.uint8).reshape(4, 6)
    assert P.in_char_rows(chars, [b"MAIL", b"SHIP\0junk"]).tolist() == [True, True, False, False]
    assert P.in_char_rows(chars, [b"MAIL"], negate=True).tolist() == [False, True, True, True]


@pytest.mark.parametrize("seed", range(20))
def test_vector_and_row_evaluations_agree_on_random_trees(seed):
    rng = np.random.default_rng(seed)
    n = 97
    columns = {a: rng.integers(0, 8, size=n).astype(np.int32) for a in "abc"}
    nulls = {"a": rng.random(n) < 0.2, "c": rng.random(n) < 0.5}
    while True:          # (a tree whose program is longer than one call holds is split by the caller: not this test's subject)
        tree = P.random_tree(rng, ["a", "b", "c"], depth=3)
        leaves, program = P.compile_tree(tree, nullable=("a", "c"))
        if P.program_ok(len(leaves), program):
            break
    whole = P.eval_tree(tree, columns, nulls)
    assert whole.tolist() == [P.eval_tree_row(tree, columns, nulls, i) for i in range(n)]
    # and the compiled program over leaf bitmaps gives the same rows
    words = [P.pack_bitmap(P.leaf_rows(entry[1], columns) if entry[0] == "leaf" else nulls[entry[1]]) for entry in leaves]
    keep = rng.random(n) < 0.7
    out, count = P.eval_program(words, program, n, P.pack_bitmap(keep))
    assert P.unpack_bitmap(out, n).tolist() == (whole & keep).tolist() and count == int((whole & keep).sum())


def test_program_validation_and_tail_bits():
    A, O, N = P.BOOL_AND, P.BOOL_OR, P.BOOL_NOT
    assert P.program_ok(2, [0, 1, A]) and P.program_ok(1, [0, N]) and P.program_ok(1, [0])
    assert not P.program_ok(2, [0, A])                 # underflow
    assert not P.program_ok(1, [N])
    assert not P.program_ok(2, [0, 1])                 # two values left
    assert not P.program_ok(2, [0, 2, O])              # a leaf that is not there
    assert not P.program_ok(2, [0, 1, -4])             # an unknown code
    assert not P.program_ok(1, [])
    assert P.program_ok(1, [0] * 8 + [A] * 7) and not P.program_ok(1, [0] * 9 + [A] * 8)     # depth 8 / 9
    assert not P.program_ok(1, [0] + [N] * 64) and P.program_ok(1, [0] + [N] * 63)           # 65 / 64 instructions
    out, count = P.eval_program([None], [0, N], 70)
    assert out.tolist() == [0xFFFFFFFFFFFFFFFF, 0xFC00000000000000] and count == 70
    rng = np.random.default_rng(3)
    for want in (1, 2, 8):
        assert P.program_depth(P.random_program(rng, 5, want_depth=want)) == want
    assert len(P.random_program(rng, 32, length=64)) == 64
