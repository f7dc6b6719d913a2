"""CPU: tests/case_reference.py — the numpy restatement of ScalarCaseExpression::getAllValues the GPU tests compare against —
checked against the reference's own known answer (query_optimizer/tests/execution_generator/Select.test:742-752) and against
cases worked out by hand (tests/golden/case_unittest.json)."""
import numpy as np
import pytest

import case_reference as CR


def _cases(golden):
    return {c["name"]: c for c in golden["case_unittest"]["cases"]}


def test_the_references_own_known_answer(golden):
    """SELECT SUM(CASE WHEN i < 4 THEN i ELSE i * i END) FROM generate_series(1, 5) = 47, every node an INT."""
    i = np.arange(1, 6, dtype=np.int32)
    out, isnull = CR.eval_case([i], None, [("i*", 0, ("col", 0), ("col", 0))], [0.0] * 8, [("col", 0), ("temp", 0)], [i < 4], CR.INT)
    assert out.dtype == np.int32 and out.tolist() == [1, 2, 3, 16, 25] and not isnull.any()
    assert int(out.astype(np.int64).sum()) == 47
    case = _cases(golden)["reference_sum_47"]
    assert case["expect_sum"] == 47 and case["expect"] == out.tolist()


@pytest.mark.parametrize("name", ["reference_sum_47", "overlapping_whens_first_wins", "else_null",
                                  "null_operand_counts_only_in_the_chosen_branch", "null_operand_through_a_temp",
                                  "int_branch_cast_to_double", "int_wraps_inside_a_branch_then_widens"])
def test_hand_written_cases(golden, name):
    args, expect, expect_null = CR.load_golden_case(_cases(golden)[name])
    out, isnull = CR.eval_case(*args)
    assert out.dtype == expect.dtype
    assert out.tobytes() == expect.tobytes(), (out, expect)
    assert np.array_equal(isnull, expect_null)


def test_every_golden_case_is_run(golden):
    assert len(_cases(golden)) == 7


def test_an_unchosen_branch_is_never_evaluated_on_a_row():
    """Per-branch evaluation: 1 / d is taken only where d != 0, so no division by zero is ever computed for a stored value,
    and the rows of the other branch do not see d's NULLs."""
    d = np.array([0.0, 2.0, 0.0, 4.0])
    d_null = np.array([True, False, False, False])
    out, isnull = CR.eval_case([d], [d_null], [("/", 0, ("const", 0), ("col", 0))], [1.0] + [0.0] * 7,
                               [("temp", 0), ("const", 1)], [d != 0.0], CR.DOUBLE)
    assert out.tolist() == [0.0, 0.5, 0.0, 0.25] and not isnull.any()


def test_mixed_branch_types_unify_to_double_and_long():
    i = np.array([2 ** 31 - 1, -5], dtype=np.int32)
    l = np.array([2 ** 62, -(2 ** 53) - 1], dtype=np.int64)
    f = np.array([0.1, 0.2], dtype=np.float32)
    w = np.array([True, False])
    out, _ = CR.eval_case([i, l, f], None, [], [0.0] * 8, [("col", 1), ("col", 2)], [w], CR.DOUBLE)
    assert out.tolist() == [float(2 ** 62), float(np.float32(0.2))]           # LONG -> DOUBLE rounds once, FLOAT -> DOUBLE is exact
    out, _ = CR.eval_case([i, l, f], None, [], [0.0] * 8, [("col", 0), ("col", 1)], [w], CR.LONG)
    assert out.dtype == np.int64 and out.tolist() == [2 ** 31 - 1, -(2 ** 53) - 1]
    with pytest.raises(AssertionError):
        CR.eval_case([i, l, f], None, [], [0.0] * 8, [("col", 0), ("col", 1)], [~w], CR.INT)   # a LONG branch never narrows


def test_bitmap_words_are_msb_first():
    bits = np.zeros(70, dtype=bool)
    bits[[0, 63, 64, 69]] = True
    words = CR.pack_bits(bits)
    assert words.dtype == np.uint64 and words.tolist() == [(1 << 63) | 1, (1 << 63) | (1 << 58)]
    assert CR.pack_bits(np.zeros(0, dtype=bool)).tolist() == [0]
