"""GPU: qsx_select_cmp_columns_blocks against tests/cmp_columns_reference.py — every output word and every count exactly.
Outputs are pre-filled with all-ones plus two spare words and counts with -1, so a word that is not written, or written
behind the bitmap, shows.

Sizes: bitmap-word edges (0, 1, 63, 64, 65, 127), the kernel's tile (4096, 4097: a full tile, and one row of a second), several
tiles (3 * 4096 + 17); a batch of a wave is 512 rows, so 4097 and 3 * 4096 + 17 end in partial batches and 4096 does not.
Stripes also start 4 bytes behind an aligned allocation.  The kernel stages no dictionary, so there is no staging bound to step
over; dictionaries have 1, 2, 255, 256, 257 and 2526 entries (the edges of 1- and 2-byte codes, and a block's dates)."""
import ctypes as C

import numpy as np
import pytest
import torch

import cmp_columns_reference as R
from helpers import bitmap_np
from quickstep_amd import types as T

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 127, 4096, 4097, 3 * 4096 + 17)
RUN_ROWS = [0, 1, 64, 65, 4097, 0, 130]
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
NAN, INF = float("nan"), float("inf")
# small domains that hold the edge values of the reference's table; their first four values are the same in every type and
# open every plain stripe in this order (random_plain), so that every op has both outcomes for every pair of types
DOMAIN = {
    T.INT: [0, 1, -1, 16777216, 16777217, -16777217, 2**31 - 1, -2**31],
    T.LONG: [0, 1, -1, 16777216, 16777217, 4294967295, 2**53, 2**53 + 1, 2**60 + 2**36 + 1, -2**63],
    T.FLOAT: [0.0, 1.0, -1.0, 16777216.0, -0.0, 2.0**31, 2.0**53, 2.0**60 + 2.0**37, NAN, -INF],
    T.DOUBLE: [0.0, 1.0, -1.0, 16777216.0, -0.0, 16777217.0, 2.0**53, 4294967295.0, NAN, INF, 0.5],
}
DATES = [T.date_raw(y, m, d, p) for y in (1993, 1994) for m in (1, 2) for d in (1, 28) for p in (0, 0xBEEF)]
PAIRS_EVERYWHERE = ((T.INT, T.LONG), (T.LONG, T.FLOAT), (T.DATE, T.DATE))


def domain(qtype):
    return np.array(DATES if qtype == T.DATE else DOMAIN[qtype], dtype=R.NP_DTYPE[qtype])


def words_of(n):
    return (n + 63) // 64


class Side:
    """One operand of one block: the reference's Operand and the same bytes on the device."""

    def __init__(self, operand, dev, offset=False):
        self.operand = operand
        raw = operand.stripe.view(np.uint8)
        # offset: the stripe starts 4 bytes behind an aligned allocation
        room = torch.zeros(raw.size + 16, dtype=torch.uint8, device=dev)
        self.byte_offset = 4 if offset else 0
        room[self.byte_offset:self.byte_offset + raw.size] = torch.from_numpy(raw.copy()).to(dev)
        self.room = room
        self.dictionary = None
        if operand.dictionary is not None:
            table = np.ascontiguousarray(operand.dictionary, dtype=R.NP_DTYPE[operand.qtype])
            self.dictionary = torch.from_numpy(table.copy()).to(dev)       # exactly len(dictionary) entries, nothing behind them

    def ptr(self):
        return self.room.data_ptr() + self.byte_offset if self.operand.stripe.size else None


def plain(qtype, values):
    return R.Operand(qtype, np.asarray(values, dtype=R.NP_DTYPE[qtype]))


def truncated(qtype, values, width):
    """Non-negative values below 2^(8 width) as `width`-byte codes without a dictionary."""
    return R.Operand(qtype, np.asarray(values).astype(R.CODE_DTYPE[width]), width=width)


def coded(qtype, rng, n, width, entries, null_codes=False):
    """n rows of `width`-byte codes into a dictionary of `entries` values of the type's domain (repeated as often as it takes:
    what matters is where a code lands).  null_codes: some rows hold codes past the dictionary, the largest code among them."""
    dom = domain(qtype)
    table = dom[rng.integers(0, dom.size, size=entries)]
    table[: min(entries, dom.size)] = dom[: min(entries, dom.size)]
    top = 1 << (8 * width)
    assert entries <= top
    codes = rng.integers(0, entries, size=n, dtype=np.int64)
    if entries > 1 and n > 1:
        codes[-1] = entries - 1                       # the last entry is read
    if null_codes and n:
        assert entries < top
        where = rng.random(n) < 0.2
        where[0] = True
        codes[where] = rng.integers(entries, min(top, entries + 1000), size=int(where.sum()))
        codes[0] = top - 1                            # the largest code there is
        if n > 2:
            codes[n // 2] = entries                   # the first code past the dictionary
    return R.Operand(qtype, codes.astype(R.CODE_DTYPE[width]), width=width, dictionary=table, num_codes=entries)


def random_plain(qtype, rng, n):
    dom = domain(qtype)
    values = dom[rng.integers(0, dom.size, size=n)]
    values[: min(n, 4)] = dom[: min(n, 4)]
    return R.Operand(qtype, values)


def random_filter(rng, n):
    return rng.integers(0, 1 << 64, size=max(words_of(n), 1), dtype=np.uint64)


def coding_of(sides):
    return [(s.operand.width, s.dictionary, s.operand.num_codes) for s in sides]


def run_and_check(capi, dev, lhs, rhs, op, rng, with_filter=False, with_counts=True, offset=False):
    """lhs, rhs: lists of Operand, one per block.  Launches once and checks every word, the spare words and the counts."""
    nb = len(lhs)
    rows = [o.stripe.size for o in lhs]
    ls = [Side(o, dev, offset) for o in lhs]
    rs = [Side(o, dev, offset) for o in rhs]
    filters_np = [random_filter(rng, n) if (with_filter and b % 3 != 2) else None for b, n in enumerate(rows)]   # some entries NULL
    filters = None if not with_filter else [None if f is None else torch.from_numpy(f.view(np.int64).copy()).to(dev) for f in filters_np]
    outs = [torch.full((words_of(n) + 2,), -1, dtype=torch.int64, device=dev) for n in rows]
    counts = torch.full((nb,), -1, dtype=torch.int64, device=dev) if with_counts else False
    fn = capi.lib.qsx_select_cmp_columns_blocks
    c_rows = (C.c_int64 * nb)(*rows)
    lptr = (C.c_void_p * nb)(*[s.ptr() for s in ls])
    rptr = (C.c_void_p * nb)(*[s.ptr() for s in rs])
    optr = (C.c_void_p * nb)(*[o.data_ptr() for o in outs])
    fptr = None if filters is None else (C.c_void_p * nb)(*[None if f is None else f.data_ptr() for f in filters])
    lcod, lkeep = capi._operand_coding(coding_of(ls), nb)
    rcod, rkeep = capi._operand_coding(coding_of(rs), nb)
    if all(o.width == 0 for o in lhs):
        lcod = None                                   # plain operands may come without a coding at all
    rc = fn(lhs[0].qtype, rhs[0].qtype, nb, c_rows, lptr, lcod, rptr, rcod, op, fptr, optr,
            None if counts is False else C.c_void_p(counts.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == T.OK, rc
    torch.cuda.synchronize()
    want = R.select_blocks(lhs, rhs, op, filters_np if with_filter else None)
    for b, n in enumerate(rows):
        got = bitmap_np(outs[b])
        assert np.array_equal(got[:words_of(n)], want[b][0]), f"block {b} ({n} rows): bitmap words differ"
        assert (got[words_of(n):] == ONES).all(), f"block {b}: a word behind the bitmap was written"
        if with_counts:
            assert int(counts[b].item()) == want[b][1], f"block {b}: count"
    return want


def variants(n):
    """(offset stripe?, filter?, counts?) per size: two complementary combinations everywhere, all eight at 65 and 4097."""
    if n in (65, 4097):
        return [(o, f, c) for o in (False, True) for f in (False, True) for c in (False, True)]
    return [(False, False, True), (True, True, False)]


@pytest.mark.parametrize("lhs_type", R.NUMERIC)
def test_every_pair_of_numeric_types_and_every_op(capi, dev, lhs_type):
    rng = np.random.default_rng(100 + lhs_type)
    for rhs_type in R.NUMERIC:
        for n in (65, 4097):
            lhs, rhs = random_plain(lhs_type, rng, n), random_plain(rhs_type, rng, n)
            for op in R.OPS:
                want = run_and_check(capi, dev, [lhs], [rhs], op, rng)
                assert 0 < want[0][1] < n, "the domain must give every op both outcomes"


@pytest.mark.parametrize("n", SIZES)
def test_sizes_with_and_without_filter_counts_and_offset(capi, dev, n):
    rng = np.random.default_rng(n)
    for lhs_type, rhs_type in PAIRS_EVERYWHERE:
        lhs, rhs = random_plain(lhs_type, rng, n), random_plain(rhs_type, rng, n)
        for offset, with_filter, with_counts in variants(n):
            for op in (T.LT, T.EQ, T.NE, T.GE) if n in (65, 4097) else (T.LT, T.NE):
                run_and_check(capi, dev, [lhs], [rhs], op, rng, with_filter, with_counts, offset)


def test_a_run_of_blocks(capi, dev):
    rng = np.random.default_rng(7)
    for lhs_type, rhs_type in PAIRS_EVERYWHERE:
        lhs = [random_plain(lhs_type, rng, n) for n in RUN_ROWS]
        rhs = [random_plain(rhs_type, rng, n) for n in RUN_ROWS]
        for op in R.OPS:
            run_and_check(capi, dev, lhs, rhs, op, rng, with_filter=op in (T.LT, T.NE), with_counts=op != T.GT, offset=op == T.LE)


def small_values(rng, n, width):
    v = rng.integers(0, 6, size=n)
    if n:
        v[0] = (1 << (8 * width)) - 1 if width < 4 else (1 << 31) - 1     # the largest code is widened without sign
    return v


@pytest.mark.parametrize("n", (65, 4097, 3 * 4096 + 17))
def test_truncated_operands(capi, dev, n):
    rng = np.random.default_rng(n + 1)
    for width in (1, 2, 4):
        for qtype, other in ((T.INT, T.LONG), (T.LONG, T.DOUBLE), (T.LONG, T.INT)):
            coded_side = truncated(qtype, small_values(rng, n, width), width)
            other_side = plain(other, rng.integers(0, 6, size=n) if other != T.DOUBLE else rng.integers(0, 6, size=n) + 0.5 * rng.integers(0, 2, size=n))
            for op in (T.LT, T.EQ, T.NE):
                run_and_check(capi, dev, [coded_side], [other_side], op, rng, with_filter=op == T.EQ, offset=op == T.NE)
                run_and_check(capi, dev, [other_side], [coded_side], op, rng)
        # both sides truncated, at different widths
        a, b = truncated(T.LONG, small_values(rng, n, width), width), truncated(T.INT, small_values(rng, n, 2), 2)
        run_and_check(capi, dev, [a], [b], T.LE, rng)


@pytest.mark.parametrize("entries", (1, 2, 255, 256, 257, 2526))
def test_dictionary_operands(capi, dev, entries):
    rng = np.random.default_rng(entries)
    for n in (65, 4097):
        for width in (1, 2, 4):
            if entries > 1 << (8 * width):
                continue
            for qtype, other in ((T.DATE, T.DATE), (T.INT, T.LONG), (T.DOUBLE, T.FLOAT), (T.LONG, T.FLOAT)):
                a = coded(qtype, rng, n, width, entries)
                b_plain = random_plain(other, rng, n)
                b_coded = coded(other, rng, n, 2 if entries <= 65536 else 4, min(entries, 300))
                for op in (T.LT, T.EQ, T.NE):
                    run_and_check(capi, dev, [a], [b_plain], op, rng, with_filter=op == T.EQ, offset=op == T.LT)
                    run_and_check(capi, dev, [b_plain], [a], op, rng)
                    run_and_check(capi, dev, [a], [b_coded], op, rng, offset=op == T.NE)


@pytest.mark.parametrize("n", (1, 65, 4097, 3 * 4096 + 17))
def test_the_null_code_is_false_under_every_op_and_is_not_looked_up(capi, dev, n):
    """The dictionaries here are allocated with exactly num_codes entries (Side), so an unguarded lookup of a NULL code — up to
    the largest code of its width — has nothing valid behind it; what is asserted is the result bits."""
    rng = np.random.default_rng(n + 2)
    for width, entries in ((1, 200), (2, 2526), (4, 2526), (1, 1)):
        for qtype, other in ((T.DATE, T.DATE), (T.INT, T.DOUBLE)):
            a = coded(qtype, rng, n, width, entries, null_codes=True)
            b = random_plain(other, rng, n)
            c = coded(other, rng, n, 2, 300, null_codes=True)
            for op in R.OPS:
                for lhs, rhs in ((a, b), (b, a), (a, c)):
                    want = run_and_check(capi, dev, [lhs], [rhs], op, rng, with_filter=op == T.GE)
                    null = np.zeros(n, dtype=bool)
                    for side in (lhs, rhs):
                        null |= ~side.values()[1]
                    assert null.any() and not (R.compare_numpy(lhs, rhs, op) & null).any()
                    bits = np.unpackbits(want[0][0].astype(">u8").view(np.uint8), bitorder="big")[:n].astype(bool)
                    assert not (bits & null).any()
    # a block whose dictionary has no entries (num_codes 0): every row is NULL, and entry 0 is not read either
    no_codes = R.Operand(T.LONG, rng.integers(0, 5, size=n).astype(np.uint8), width=1, dictionary=np.array([3], dtype=np.int64), num_codes=0)
    for op in R.OPS:
        want = run_and_check(capi, dev, [no_codes], [plain(T.LONG, rng.integers(0, 5, size=n))], op, rng)
        assert want[0][1] == 0


def test_a_run_whose_blocks_differ_in_coding_on_both_sides(capi, dev):
    rng = np.random.default_rng(9)
    rows = [2500, 1001, 0, 777, 3000, 4097, 64]
    lhs = [coded(T.DATE, rng, rows[0], 2, 2526), random_plain(T.DATE, rng, rows[1]), random_plain(T.DATE, rng, rows[2]),
           coded(T.DATE, rng, rows[3], 1, 200, null_codes=True), coded(T.DATE, rng, rows[4], 4, 257), random_plain(T.DATE, rng, rows[5]),
           coded(T.DATE, rng, rows[6], 1, 1)]
    rhs = [coded(T.DATE, rng, rows[0], 2, 2400, null_codes=True), coded(T.DATE, rng, rows[1], 1, 255), coded(T.DATE, rng, rows[2], 2, 5),
           random_plain(T.DATE, rng, rows[3]), coded(T.DATE, rng, rows[4], 2, 2526), random_plain(T.DATE, rng, rows[5]),
           coded(T.DATE, rng, rows[6], 4, 2)]
    for op in R.OPS:
        run_and_check(capi, dev, lhs, rhs, op, rng, with_filter=op in (T.LT, T.GE), with_counts=op != T.EQ, offset=op in (T.NE, T.LT))
    # INT against LONG: plain, truncated at three widths, dictionary-coded — and a FLOAT side that is plain or coded
    ints = [plain(T.INT, rng.integers(-3, 6, size=rows[0])), truncated(T.INT, small_values(rng, rows[1], 1), 1), plain(T.INT, []),
            truncated(T.INT, small_values(rng, rows[3], 2), 2), coded(T.INT, rng, rows[4], 2, 257), truncated(T.INT, small_values(rng, rows[5], 4), 4),
            coded(T.INT, rng, rows[6], 1, 8, null_codes=True)]
    longs = [truncated(T.LONG, small_values(rng, rows[0], 2), 2), coded(T.LONG, rng, rows[1], 1, 10), truncated(T.LONG, [], 1),
             plain(T.LONG, rng.integers(-3, 6, size=rows[3])), truncated(T.LONG, small_values(rng, rows[4], 4), 4),
             coded(T.LONG, rng, rows[5], 2, 2526, null_codes=True), plain(T.LONG, rng.integers(0, 3, size=rows[6]))]
    floats = [coded(T.FLOAT, rng, n, 1 if b % 2 else 2, 10 + b) if b % 3 else random_plain(T.FLOAT, rng, n) for b, n in enumerate(rows)]
    for op in R.OPS:
        run_and_check(capi, dev, ints, longs, op, rng, with_filter=op == T.NE, offset=op == T.GT)
        run_and_check(capi, dev, longs, floats, op, rng, with_counts=op != T.LT)
        run_and_check(capi, dev, floats, ints, op, rng)


def test_the_binding_returns_bitmaps_and_counts_per_block(capi, dev):
    rng = np.random.default_rng(3)
    rows = [130, 0, 4097]
    lhs = [coded(T.DATE, rng, n, 2, 2526) for n in rows]
    rhs = [random_plain(T.DATE, rng, n) for n in rows]
    ls, rs = [Side(o, dev) for o in lhs], [Side(o, dev) for o in rhs]
    stripes = lambda sides: [torch.from_numpy(s.operand.stripe.view(np.int64 if s.operand.width == 0 else np.int16).copy()).to(dev) for s in sides]  # noqa: E731
    outs, counts = capi.select_cmp_columns_blocks(stripes(ls), stripes(rs), T.LT, T.DATE, T.DATE, lhs_coding=coding_of(ls))
    want = R.select_blocks(lhs, rhs, T.LT)
    for b, n in enumerate(rows):
        assert np.array_equal(bitmap_np(outs[b])[:words_of(n)], want[b][0]) and int(counts[b].item()) == want[b][1]


def test_argument_errors_write_nothing_and_unsupported_pairs_are_refused(capi, dev):
    rng = np.random.default_rng(4)
    n = 130
    a, b = Side(random_plain(T.LONG, rng, n), dev), Side(random_plain(T.LONG, rng, n), dev)
    table = torch.zeros(8, dtype=torch.int64, device=dev)
    fn = capi.lib.qsx_select_cmp_columns_blocks
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(lhs_type=T.LONG, rhs_type=T.LONG, rows=n, lhs=a.ptr(), rhs=b.ptr(), op=T.LT, lhs_coding=None, rhs_coding=None, has_out=True):
        out = torch.full((words_of(n) + 2,), -1, dtype=torch.int64, device=dev)
        counts = torch.full((1,), -1, dtype=torch.int64, device=dev)
        lcod, lkeep = capi._operand_coding(lhs_coding, 1)
        rcod, rkeep = capi._operand_coding(rhs_coding, 1)
        rc = fn(lhs_type, rhs_type, 1, (C.c_int64 * 1)(rows), (C.c_void_p * 1)(lhs), lcod, (C.c_void_p * 1)(rhs), rcod, op, None,
                (C.c_void_p * 1)(out.data_ptr() if has_out else None), C.c_void_p(counts.data_ptr()), stream)
        torch.cuda.synchronize()
        if rc != T.OK:
            assert (bitmap_np(out) == ONES).all() and int(counts.item()) == -1, "an argument error wrote something"
        return rc

    assert call() == T.OK
    assert call(rows=-1) == T.ERR_INVALID_ARGUMENT
    assert call(op=-1) == T.ERR_INVALID_ARGUMENT and call(op=6) == T.ERR_INVALID_ARGUMENT
    assert call(lhs=None) == T.ERR_INVALID_ARGUMENT and call(rhs=None) == T.ERR_INVALID_ARGUMENT and call(has_out=False) == T.ERR_INVALID_ARGUMENT
    for width in (3, 8, -1):
        assert call(lhs_coding=[(width, None)]) == T.ERR_INVALID_ARGUMENT
        assert call(rhs_coding=[(width, table, 8)]) == T.ERR_INVALID_ARGUMENT
    for qtype in (T.FLOAT, T.DOUBLE, T.DATE):          # truncation is for INT / LONG
        other = T.DATE if qtype == T.DATE else T.LONG
        assert call(lhs_type=qtype, rhs_type=other, lhs_coding=[(2, None)]) == T.ERR_INVALID_ARGUMENT
        assert call(lhs_type=other, rhs_type=qtype, rhs_coding=[(1, None)]) == T.ERR_INVALID_ARGUMENT
    assert call(lhs_coding=[(0, table, 8)]) == T.ERR_INVALID_ARGUMENT          # a dictionary without codes
    assert call(rhs_coding=[(2, table, -1)]) == T.ERR_INVALID_ARGUMENT         # a negative code count
    for lhs_type, rhs_type in ((T.CHAR, T.CHAR), (T.DATE, T.LONG), (T.INT, T.DATE), (T.CHAR, T.INT), (5, 5), (T.LONG, 7)):
        assert call(lhs_type=lhs_type, rhs_type=rhs_type) == T.ERR_UNSUPPORTED
    # no blocks at all is fine, with or without arrays
    assert fn(T.LONG, T.INT, 0, None, None, None, None, None, T.EQ, None, None, None, stream) == T.OK
    assert fn(T.LONG, T.INT, -1, None, None, None, None, None, T.EQ, None, None, None, stream) == T.ERR_INVALID_ARGUMENT
