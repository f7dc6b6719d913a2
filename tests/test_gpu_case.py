"""GPU: qsx_eval_case / qsx_eval_case_blocks against tests/case_reference.py, bit for bit: values compare as raw bytes, null
bitmaps word by word.  No tolerance: every node is rounded on its own on both sides.

Sizes cover the seams of csrc/case_expr.hip: a lane owns 4 rows and a wave 256 (four bitmap words), so 1 / 63 / 64 / 65 / 127
are partial tiles with one or two words, 1000 is three whole tiles and a partial one, 4099 more than one workgroup's worth
of waves (1024 rows) with a three-row tail."""
import ctypes as C

import numpy as np
import pytest
import torch

import case_reference as CR
from helpers import bitmap_dev, bitmap_np, to_dev
from quickstep_amd import types as T

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 127, 1000, 4099)
col, const, temp, NULL = (lambda i: ("col", i)), (lambda i: ("const", i)), (lambda i: ("temp", i)), ("null",)

# columns of every shape: 0 x DOUBLE, 1 y DOUBLE, 2 i INT, 3 j INT, 4 l LONG, 5 f FLOAT
X, Y, I, J, L, F = range(6)
CONSTS = [1.0, 3.0, 2.5, -5.0, 7.0, 0.0, 2.0 ** 40, 0.0]
DOUBLE_PROGRAM = [("-", 0, const(0), col(Y)),          # t0 = 1 - y
                  ("*", 1, col(X), temp(0)),           # t1 = x * (1 - y)            (shared by several branches)
                  ("i*", 2, col(I), col(I)),           # t2 = i * i                  (INT, wraps)
                  ("+", 3, temp(1), temp(2)),          # t3 = t1 + t2                (a double node over an integer temp)
                  ("/", 4, col(X), temp(0)),           # t4 = x / (1 - y)
                  ("*", 5, col(F), col(L))]            # t5 = f * l                  (FLOAT and LONG operands)
INTEGER_PROGRAM = [("i+", 0, col(I), col(J)),          # t0 = i + j                  (INT, wraps)
                   ("i*", 1, col(L), const(1)),        # t1 = l * 3                  (LONG)
                   ("i+", 2, temp(1), temp(0)),        # t2 = t1 + t0                (LONG; t0 shared)
                   ("i/", 3, col(L), col(J)),          # t3 = l / j                  (j holds 0 and -1)
                   ("i-", 4, col(J), const(4))]        # t4 = j - 7                  (INT)
SHAPES = {
    # name: (program, branch values: THENs then ELSE, output type)
    "double_1when_else_0": (DOUBLE_PROGRAM[:2], [temp(1), const(5)], CR.DOUBLE),                       # the TPC-H Q14 shape
    "double_3whens_mixed": (DOUBLE_PROGRAM, [temp(1), col(I), col(F), temp(3)], CR.DOUBLE),
    "double_8whens_null_else": (DOUBLE_PROGRAM, [temp(1), col(I), col(L), NULL, const(2), temp(3), temp(2), temp(4), NULL], CR.DOUBLE),
    "double_integer_branches_only": (INTEGER_PROGRAM, [temp(0), temp(2), col(L), const(6)], CR.DOUBLE),
    "long_1when": (INTEGER_PROGRAM, [temp(2), col(I)], CR.LONG),
    "long_3whens": (INTEGER_PROGRAM, [temp(0), temp(2), col(L), const(6)], CR.LONG),
    "long_8whens_null_then": (INTEGER_PROGRAM, [temp(0), NULL, temp(1), temp(2), temp(3), col(J), const(3), col(L), temp(4)], CR.LONG),
    "int_1when_null_else": (INTEGER_PROGRAM, [temp(0), NULL], CR.INT),
    "int_3whens": (INTEGER_PROGRAM, [temp(0), NULL, const(3), col(J)], CR.INT),
    "int_8whens": (INTEGER_PROGRAM, [temp(0), col(I), temp(4), const(4), col(J), temp(0), const(1), NULL, temp(4)], CR.INT),
}
PATTERNS = ("random", "zeros", "ones", "sparse")
NULLABLE = (None, (Y, I, L))          # no null bitmaps at all / three nullable columns


def make_columns(n, seed):
    rng = np.random.default_rng(seed)
    x = np.round(rng.uniform(900.0, 105000.0, size=n), 2)
    y = rng.integers(0, 11, size=n) / 100.0
    i = rng.integers(-2 ** 31, 2 ** 31, size=n).astype(np.int32)
    j = rng.choice(np.array([-7, -1, 0, 1, 3, 2 ** 31 - 1, -2 ** 31], dtype=np.int64), size=n).astype(np.int32)
    l = rng.integers(-2 ** 62, 2 ** 62, size=n)
    f = rng.normal(size=n).astype(np.float32)
    return [x, y, i, j, l, f]


def make_whens(n, count, pattern, seed):
    rng = np.random.default_rng(seed + 1)
    if pattern == "zeros":
        return [np.zeros(n, dtype=bool) for _ in range(count)]
    if pattern == "ones":
        return [np.ones(n, dtype=bool) for _ in range(count)]
    density = 0.3 if pattern == "random" else 0.02
    return [rng.random(n) < density for _ in range(count)]        # independent: they overlap


def make_nulls(n, nullable, seed):
    if nullable is None:
        return None
    rng = np.random.default_rng(seed + 2)
    return [rng.random(n) < 0.25 if c in nullable else None for c in range(6)]


_reference = {}


def reference(shape, n, pattern, nullable):
    """(inputs, expected values, expected null words), computed once per case and never modified."""
    key = (shape, n, pattern, nullable)
    if key not in _reference:
        program, values, out_type = SHAPES[shape]
        seed = 1000 * list(SHAPES).index(shape) + n
        cols, whens, nulls = make_columns(n, seed), make_whens(n, len(values) - 1, pattern, seed), make_nulls(n, nullable, seed)
        out, isnull = CR.eval_case(cols, nulls, program, CONSTS, values, whens, out_type)
        for a in (out, isnull):
            a.setflags(write=False)
        _reference[key] = ((cols, whens, nulls), out, CR.pack_bits(isnull))
    return _reference[key]


def run_gpu(capi, dev, shape, cols, whens, nulls, want_nulls=True, dev_cols=None, out=None, out_nulls=None):
    program, values, out_type = SHAPES[shape]
    instrs, vals, qtype = CR.abi_program(program, values, out_type)
    dcols = dev_cols if dev_cols is not None else [to_dev(c, dev) for c in cols]
    dwhens = [bitmap_dev(CR.pack_bits(w), dev) for w in whens]
    dnulls = None if nulls is None else [None if m is None else bitmap_dev(CR.pack_bits(m), dev) for m in nulls]
    return capi.eval_case(dcols, instrs, CONSTS, vals, dwhens, qtype, col_nulls=dnulls, want_nulls=want_nulls, n=cols[0].size, out=out, out_nulls=out_nulls)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_case_matches_the_reference_bit_for_bit(capi, dev, shape, n):
    has_null_branch = NULL in SHAPES[shape][1]
    for pattern in PATTERNS:
        for nullable in NULLABLE:
            (cols, whens, nulls), want, want_nulls = reference(shape, n, pattern, nullable)
            got, got_nulls = run_gpu(capi, dev, shape, cols, whens, nulls)
            assert got.cpu().numpy().tobytes() == want.tobytes(), (shape, n, pattern, nullable)
            assert np.array_equal(bitmap_np(got_nulls)[:want_nulls.size], want_nulls), (shape, n, pattern, nullable)
            if not has_null_branch and nullable is None:
                # nothing can be NULL: the call is legal without a null bitmap and gives the same values
                alone, none = run_gpu(capi, dev, shape, cols, whens, nulls, want_nulls=False)
                assert none is None and alone.cpu().numpy().tobytes() == want.tobytes()


def test_the_reference_cases_cover_what_they_are_meant_to():
    """The data makes a wrong evaluation visible: INT sums wrap, the first-match rule matters, NULLs fall on chosen and on
    unchosen branches, and every branch of the widest shapes is taken."""
    (cols, whens, nulls), want, _ = reference("long_8whens_null_then", 4099, "random", NULLABLE[1])
    i64, j64 = cols[I].astype(np.int64), cols[J].astype(np.int64)
    assert np.mean(i64 + j64 != (i64 + j64).astype(np.int32)) > 0.1                      # i + j wraps (j is +-2^31 in 2 rows of 7, half of those wrap)
    assert np.any(cols[J] == 0) and np.any(cols[J] == -1)                                # both division special cases
    overlap = whens[0] & whens[1]
    assert overlap.sum() > 100                                                            # first match wins somewhere
    taken = np.full(4099, len(whens))
    for k in reversed(range(len(whens))):
        taken[whens[k]] = k
    assert set(taken.tolist()) == set(range(len(whens) + 1))                              # every branch, ELSE included
    # branch 0 reads i and j only, l is nullable: rows of branch 0 whose l is NULL are not NULL; rows of branch 2 (l * 3) are
    assert np.any((taken == 0) & nulls[L] & ~nulls[I]) and np.any((taken == 2) & nulls[L])


@pytest.mark.parametrize("name", ["reference_sum_47", "overlapping_whens_first_wins", "else_null",
                                  "null_operand_counts_only_in_the_chosen_branch", "null_operand_through_a_temp",
                                  "int_branch_cast_to_double", "int_wraps_inside_a_branch_then_widens"])
def test_hand_written_cases_on_the_device(capi, dev, golden, name):
    case = {c["name"]: c for c in golden["case_unittest"]["cases"]}[name]
    (cols, col_nulls, program, consts, values, whens, out_type), expect, expect_null = CR.load_golden_case(case)
    instrs, vals, qtype = CR.abi_program(program, values, out_type)
    dnulls = None if col_nulls is None else [None if m is None else bitmap_dev(CR.pack_bits(m), dev) for m in col_nulls]
    got, got_nulls = capi.eval_case([to_dev(c, dev) for c in cols], instrs, consts, vals, [bitmap_dev(CR.pack_bits(w), dev) for w in whens],
                                    qtype, col_nulls=dnulls)
    assert got.cpu().numpy().tobytes() == expect.tobytes()
    assert bitmap_np(got_nulls).tolist() == CR.pack_bits(expect_null).tolist()
    if "expect_sum" in case:
        assert int(got.sum().item()) == case["expect_sum"]


@pytest.mark.parametrize("shape", ["double_3whens_mixed", "long_3whens", "int_3whens"])
@pytest.mark.parametrize("offset_bytes", [4, 8])
def test_stripes_off_16_byte_alignment(capi, dev, shape, offset_bytes):
    """A column base (and the output) 4 / 8 bytes past a 16-byte boundary: the 16-byte loads and stores must not be used."""
    n = 1000
    (cols, whens, nulls), want, want_nulls = reference(shape, n, "random", NULLABLE[1])
    dev_cols = []
    for c in cols:
        shift = max(offset_bytes // c.itemsize, 1)          # (an 8-byte stripe cannot sit 4 bytes off: it gets 8)
        buf = torch.zeros(n + 4, dtype=torch.from_numpy(c[:1]).dtype, device=dev)
        view = buf[shift:shift + n]
        view.copy_(to_dev(c, dev))
        assert view.data_ptr() % 16 == shift * c.itemsize % 16 != 0
        dev_cols.append(view)
    shift = max(offset_bytes // want.itemsize, 1)
    out = torch.zeros(n + 4, dtype=torch.from_numpy(want[:1]).dtype, device=dev)
    got, got_nulls = run_gpu(capi, dev, shape, cols, whens, nulls, dev_cols=dev_cols, out=out[shift:shift + n])
    assert got.data_ptr() % 16 != 0
    assert got.cpu().numpy().tobytes() == want.tobytes()
    assert np.array_equal(bitmap_np(got_nulls)[:want_nulls.size], want_nulls)
    guard = out.cpu().numpy()
    assert not guard[:shift].any() and not guard[shift + n:].any()          # nothing written outside the n values


@pytest.mark.parametrize("n", [1, 65, 1000])
def test_every_null_word_is_written_whole(capi, dev, n):
    """Every word of the null bitmap that covers a row is written in full, bits >= n are 0, and nothing behind the last word is
    touched: the bitmap starts as all ones."""
    for shape in ("double_8whens_null_else", "int_3whens"):
        (cols, whens, nulls), want, want_nulls = reference(shape, n, "random", NULLABLE[1])
        words = (n + 63) // 64
        bits = torch.full((words + 2,), -1, dtype=torch.int64, device=dev)
        got, got_nulls = run_gpu(capi, dev, shape, cols, whens, nulls, out_nulls=bits)
        assert got.cpu().numpy().tobytes() == want.tobytes()
        host = bitmap_np(got_nulls)
        assert host[:words].tolist() == want_nulls.tolist()
        assert host[words:].tolist() == [2 ** 64 - 1] * 2
        if n % 64:
            assert int(host[words - 1]) & ((1 << (64 - n % 64)) - 1) == 0


def test_a_case_over_no_columns(capi, dev):
    """Constant and NULL branches only: legal in the C ABI, the row counts are given explicitly."""
    n = 130
    whens = [np.arange(n) % 3 == 0, np.arange(n) % 2 == 0]
    instrs, vals, qtype = CR.abi_program([], [const(1), NULL, const(3)], CR.INT)
    want, isnull = CR.eval_case([], None, [], CONSTS, [const(1), NULL, const(3)], whens, CR.INT)
    dwhens = [bitmap_dev(CR.pack_bits(w), dev) for w in whens]
    got, got_nulls = capi.eval_case([], instrs, CONSTS, vals, dwhens, qtype, n=n)
    assert got.cpu().numpy().tobytes() == want.tobytes()
    assert bitmap_np(got_nulls)[:3].tolist() == CR.pack_bits(isnull).tolist()
    outs, out_nulls = capi.eval_case_blocks([[], []], instrs, CONSTS, vals, [dwhens, dwhens], qtype, rows=[n, n])
    for b in range(2):
        assert outs[b].cpu().numpy().tobytes() == want.tobytes()
        assert bitmap_np(out_nulls[b])[:3].tolist() == CR.pack_bits(isnull).tolist()


@pytest.mark.parametrize("rows", [(130, 61, 64), (256, 256, 100), (300, 0, 5), (64,)])
@pytest.mark.parametrize("shape", ["double_8whens_null_else", "long_3whens", "int_8whens", "double_1when_else_0"])
def test_a_run_of_blocks_equals_the_per_block_calls_byte_for_byte(capi, dev, shape, rows):
    """Every block of a run has its own stripes and bitmaps; one launch over the run gives what a call per block gives."""
    program, values, out_type = SHAPES[shape]
    instrs, vals, qtype = CR.abi_program(program, values, out_type)
    nullable = NULLABLE[1] if NULL in values else None
    blocks, block_whens, block_nulls, singles, wanted = [], [], [], [], []
    for b, n in enumerate(rows):
        if n == 0:
            cols = [c[:0] for c in make_columns(1, 5)]
            whens = [np.zeros(0, dtype=bool)] * (len(values) - 1)
            nulls = None if nullable is None else [np.zeros(0, dtype=bool) if c in nullable else None for c in range(6)]
            want, want_null_words = np.zeros(0, dtype=CR.OUT_DTYPE[out_type]), None
        else:
            seed = 77 * (b + 1) + n
            cols, whens, nulls = make_columns(n, seed), make_whens(n, len(values) - 1, "random", seed), make_nulls(n, nullable, seed)
            want, isnull = CR.eval_case(cols, nulls, program, CONSTS, values, whens, out_type)
            want_null_words = CR.pack_bits(isnull)
        blocks.append([to_dev(c, dev) for c in cols])
        block_whens.append([bitmap_dev(CR.pack_bits(w), dev) for w in whens])
        block_nulls.append(None if nulls is None else [None if m is None else bitmap_dev(CR.pack_bits(m), dev) for m in nulls])
        wanted.append((want, want_null_words))
        if n > 0:
            singles.append(capi.eval_case(blocks[-1], instrs, CONSTS, vals, block_whens[-1], qtype, col_nulls=block_nulls[-1]))
        else:
            singles.append(None)
    outs, out_nulls = capi.eval_case_blocks(blocks, instrs, CONSTS, vals, block_whens, qtype,
                                            block_col_nulls=None if nullable is None else block_nulls)
    for b, n in enumerate(rows):
        if n == 0:
            continue
        words = (n + 63) // 64
        assert outs[b].cpu().numpy().tobytes() == singles[b][0].cpu().numpy().tobytes() == wanted[b][0].tobytes(), (shape, rows, b)
        assert (bitmap_np(out_nulls[b])[:words].tolist() == bitmap_np(singles[b][1])[:words].tolist() == wanted[b][1].tolist()), (shape, rows, b)


def test_argument_refusals(capi, dev):
    n = 8
    cols = [to_dev(c, dev) for c in make_columns(n, 3)]
    when = [bitmap_dev(CR.pack_bits(np.ones(n, dtype=bool)), dev)]
    ops = {"+": T.EX_ADD, "i+": T.EX_IADD}

    def status(instrs, values, out_type, whens=when, col_nulls=None, want_nulls=True, consts=CONSTS):
        try:
            capi.eval_case(cols, instrs, consts, values, whens, out_type, col_nulls=col_nulls, want_nulls=want_nulls)
        except capi.QsxError as e:
            return e.status
        return T.OK
    add = [(ops["+"], 0, T.col(X), T.col(Y))]
    iadd = [(ops["i+"], 0, T.col(I), T.col(J))]
    ladd = [(ops["i+"], 0, T.col(I), T.col(L))]
    bad = T.ERR_INVALID_ARGUMENT
    assert status(add, [T.temp(0), T.const(5)], T.DOUBLE) == T.OK
    # an integer output never takes a double: a double temp, a FLOAT / DOUBLE column, a non-integral constant
    assert status(add, [T.temp(0), T.const(5)], T.LONG) == bad
    assert status(iadd, [T.temp(0), T.col(F)], T.LONG) == bad
    assert status(iadd, [T.temp(0), T.col(X)], T.INT) == bad
    assert status(iadd, [T.temp(0), T.const(2)], T.LONG) == bad               # 2.5
    assert status(iadd, [T.temp(0), T.const(1)], T.LONG) == T.OK              # 3.0 is integral
    # INT output with a LONG branch: a LONG column, a LONG temp, a constant beyond 32 bits
    assert status(iadd, [T.temp(0), T.col(L)], T.INT) == bad
    assert status(ladd, [T.temp(0), T.col(I)], T.INT) == bad
    assert status(iadd, [T.temp(0), T.const(6)], T.INT) == bad                # 2^40
    assert status(iadd, [T.temp(0), T.const(6)], T.LONG) == T.OK
    # the NULL literal is a branch value only
    assert status([(ops["+"], 0, T.col(X), T.null())], [T.temp(0), T.const(5)], T.DOUBLE) == bad
    assert status([(ops["i+"], 0, T.null(), T.col(I))], [T.temp(0), T.const(5)], T.LONG) == bad
    assert status(add, [T.temp(0), T.null()], T.DOUBLE) == T.OK
    # operand indices
    assert status(add, [T.temp(1), T.const(5)], T.DOUBLE) == bad              # a temp no instruction wrote
    assert status(add, [T.temp(T.MAX_TEMPS), T.const(5)], T.DOUBLE) == bad
    assert status(add, [T.col(6), T.const(5)], T.DOUBLE) == bad
    assert status(add, [T.col(-1), T.const(5)], T.DOUBLE) == bad
    assert status(add, [T.temp(0), T.const(T.MAX_CONSTS)], T.DOUBLE) == bad
    assert status([(ops["+"], 0, T.col(X), T.col(9))], [T.temp(0), T.const(5)], T.DOUBLE) == bad
    assert status([(ops["+"], T.MAX_TEMPS, T.col(X), T.col(Y))], [T.const(5), T.const(5)], T.DOUBLE) == bad
    assert status([(ops["i+"], 0, T.col(I), T.col(X))], [T.const(5), T.const(5)], T.DOUBLE) == bad   # no double -> integer conversion
    # the number of WHENs and the output type
    desc = T.make_case_desc([T.const(5)], T.DOUBLE)
    for whens in (0, 9, -1):
        desc.num_whens = whens
        types = (C.c_int32 * 6)(*[capi.qsx_type_of(c) for c in cols])
        out = torch.zeros(n, dtype=torch.float64, device=dev)
        nulls = capi.new_bitmap(n, dev)
        ptrs = (C.c_void_p * 9)(*[when[0].data_ptr()] * 9)
        rc = capi.lib.qsx_eval_case(6, (C.c_void_p * 6)(*[c.data_ptr() for c in cols]), types, None, 0, None, (C.c_double * 8)(), C.byref(desc),
                                    ptrs, n, out.data_ptr(), nulls.data_ptr(), None)
        assert rc == bad, whens
    assert status(add, [T.temp(0), T.const(5)], T.FLOAT) == bad
    assert status(add, [T.temp(0), T.const(5)], T.CHAR) == bad
    # the null bitmap may be left out only when nothing can be NULL
    assert status(add, [T.temp(0), T.const(5)], T.DOUBLE, want_nulls=False) == T.OK
    assert status(add, [T.temp(0), T.null()], T.DOUBLE, want_nulls=False) == bad
    assert status(add, [T.temp(0), T.const(5)], T.DOUBLE, col_nulls=[None] * 6, want_nulls=False) == bad
    assert status(add, [T.temp(0), T.const(5)], T.DOUBLE, col_nulls=[None] * 6) == T.OK
    # a missing WHEN bitmap
    assert status(add, [T.temp(0), T.const(5)], T.DOUBLE, whens=[None]) == bad
    # the same checks guard the run form
    instrs, vals, qtype = CR.abi_program([("+", 0, col(X), col(Y))], [temp(0), NULL], CR.DOUBLE)
    with pytest.raises(capi.QsxError) as err:
        capi.eval_case_blocks([cols], instrs, CONSTS, vals, [when], qtype, want_nulls=False)
    assert err.value.status == bad
    with pytest.raises(capi.QsxError) as err:
        capi.eval_case_blocks([cols], instrs, CONSTS, vals, [when], T.LONG)
    assert err.value.status == bad
    torch.cuda.synchronize()
