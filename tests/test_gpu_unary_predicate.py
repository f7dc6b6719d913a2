"""GPU: qsx_select_cmp_unary / qsx_select_in_unary and their run forms against tests/unary_predicate_reference.py — every
output word and every count exact.  Outputs are pre-filled with 0xFF (and two guard words behind them) and counts with -1, so an
unwritten or overrun word shows.  Row counts sit around the kernels' tiles (csrc/unary_ops.hip): a wave of the date-field kernel
takes 512 rows, the substring kernels stage min(1024, 48 KiB / width rounded down to 64) rows in LDS; windows of up to 16
bytes are compared in registers, longer ones byte by byte."""
import ctypes as C

import numpy as np
import pytest
import torch

import unary_predicate_reference as R
import unary_reference as U
from quickstep_amd import types as T

pytestmark = pytest.mark.gpu

GUARD_WORDS = 2
WIDTHS = (1, 2, 3, 15, 16, 17, 25, 64, 255)
RUN_ROWS = [0, 1, 64, 65, 4097, 0, 130]
OPS = (T.EQ, T.NE, T.LT, T.LE, T.GT, T.GE)
FILL = -1     # every byte 0xFF


def rows_around(tile):
    return sorted({0, 1, 63, 64, 65, 127, tile, tile + 1, 3 * tile + 17})


def windows(width):
    """(start, length): at start 0, in the middle, at start = width - 1, and with a length beyond the field."""
    return sorted({(0, min(2, width)), (width // 2, 3), (width - 1, 1), (width // 3, 300)})


def _ptr(t):
    return None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def operand_of(spec):
    return T.date_field({"year": T.DATE_YEAR, "month": T.DATE_MONTH}[spec[0]]) if R.is_date(spec) else T.substring_of(spec[1], spec[2])


def literal_args(spec, literal):
    if R.is_date(spec):
        return (C.c_int32 * 1)(literal), 0
    return C.create_string_buffer(bytes(literal), max(len(literal), 1)), len(literal)


def list_args(capi, spec, literals):
    if R.is_date(spec):
        return (C.c_int32 * len(literals))(*literals), None
    return capi._in_char_literals(literals)


class Calls:
    """Issues calls and keeps (outputs, expectation) until check(): one synchronisation for all of them."""

    def __init__(self, capi, dev):
        self.capi, self.dev, self.pending = capi, dev, []

    def outputs(self, n, want_count):
        words = (n + 63) // 64
        out = torch.full((words + GUARD_WORDS,), FILL, dtype=torch.int64, device=self.dev)
        count = torch.full((1,), FILL, dtype=torch.int64, device=self.dev) if want_count else None
        return out, count

    def cmp(self, spec, stripe, width, n, op, literal, bits, filt, want_count, what):
        out, count = self.outputs(n, want_count)
        lit, length = literal_args(spec, literal)
        status = self.capi.lib.qsx_select_cmp_unary(C.byref(operand_of(spec)), _ptr(stripe), width, n, op, lit, length,
                                                    _ptr(filt[1]) if filt else None, C.c_void_p(out.data_ptr()), _ptr(count), _stream())
        assert status == T.OK, (what, status)
        self.pending.append((out, count, n, bits, filt[0] if filt else None, what))

    def in_list(self, spec, stripe, width, n, literals, negate, bits, filt, want_count, what):
        out, count = self.outputs(n, want_count)
        slots, lengths = list_args(self.capi, spec, literals)
        status = self.capi.lib.qsx_select_in_unary(C.byref(operand_of(spec)), _ptr(stripe), width, n, slots, lengths, len(literals), int(negate),
                                                   _ptr(filt[1]) if filt else None, C.c_void_p(out.data_ptr()), _ptr(count), _stream())
        assert status == T.OK, (what, status)
        self.pending.append((out, count, n, bits, filt[0] if filt else None, what))

    def check(self):
        assert self.pending
        for out, count, n, bits, filter_words, what in self.pending:
            words = (n + 63) // 64
            want, want_count = R.result(bits[:n], n, filter_words)
            got = out.cpu().numpy().view(np.uint64)
            assert np.array_equal(got[:words], want), what
            assert np.all(got[words:] == np.uint64(0xFFFFFFFFFFFFFFFF)), what + ": words behind the bitmap were written"
            if count is not None:
                assert int(count.item()) == want_count, what
        self.pending = []


def make_filter(rng, n, dev):
    """(host words, device tensor) of a random filter of n bits; the bits behind n are set on purpose."""
    words = rng.integers(0, 1 << 63, size=(n + 63) // 64 + 1, dtype=np.int64) | (rng.integers(0, 2, size=(n + 63) // 64 + 1, dtype=np.int64) << 63)
    return words.view(np.uint64), torch.from_numpy(words).to(dev)


def char_stripes(col, dev):
    """The CHAR stripe at a 16-byte boundary and 1 byte behind one."""
    flat = torch.from_numpy(col.reshape(-1))
    aligned = flat.to(dev)
    holder = torch.zeros(flat.numel() + 17, dtype=torch.uint8, device=dev)
    holder[1:1 + flat.numel()] = aligned
    assert aligned.data_ptr() % 16 == 0 and holder[1:].data_ptr() % 16 == 1
    return aligned, holder[1:1 + flat.numel()]


def random_chars(rng, rows, width):
    return rng.choice(np.frombuffer(b"ab\0\x80", dtype=np.uint8), size=(rows, width), p=[0.45, 0.4, 0.07, 0.08])


def window_texts(col, start, length, rows):
    m = U.substring_width(col.shape[1], start, length)
    return [U.substring_text(col[i].tobytes(), start, m)[:T.MAX_CHAR_LITERAL] for i in rows]


def char_lists(col, start, length):
    """IN lists of 1, 7 and 32 literals: window texts of the stripe's first rows, the empty string, one longer than m."""
    m = U.substring_width(col.shape[1], start, length)
    texts = window_texts(col, start, length, range(30))
    longer = (b"a" * (m + 1))[:T.MAX_CHAR_LITERAL]
    return [texts[3:4], texts[:7], texts + [b"", longer]]


# ------------------------------------------------------------------------------------------------------------------ SUBSTRING
@pytest.mark.parametrize("width", WIDTHS)
def test_substring_predicates_match_the_reference(capi, oracle, dev, width):
    tile = capi.unary_substring_tile_rows(width)
    sizes = rows_around(tile)
    rng = np.random.default_rng(1000 + width)
    col = random_chars(rng, max(sizes), width)
    stripes = char_stripes(col, dev)
    calls = Calls(capi, dev)
    turn = 0
    for start, length in windows(width):
        spec = ("substring", start, length)
        literal = window_texts(col, start, length, [5])[0]
        cmp_bits = [R.cmp_rows(oracle, spec, col, op, literal) for op in OPS]
        lists = char_lists(col, start, length)
        assert [len(lit) for lit in lists] == [1, 7, 32]
        in_bits = [R.in_rows(spec, col, lit) for lit in lists]
        for offset, stripe in enumerate(stripes):
            for n in sizes if offset == 0 else (1, 65, tile + 1, 3 * tile + 17):
                filt = make_filter(rng, n, dev)
                for k, op in enumerate(OPS):
                    turn += 1
                    calls.cmp(spec, stripe, width, n, op, literal, cmp_bits[k], filt if turn & 1 else None, bool(turn & 2),
                              "w=%d window=(%d,%d) n=%d offset=%d op=%d" % (width, start, length, n, offset, op))
                for k, literals in enumerate(lists):
                    for negate in (False, True):
                        turn += 1
                        calls.in_list(spec, stripe, width, n, literals, negate, in_bits[k] != negate, filt if turn & 2 else None, bool(turn & 1),
                                      "w=%d window=(%d,%d) n=%d offset=%d list=%d negate=%d" % (width, start, length, n, offset, len(literals), negate))
    calls.check()


def test_substring_edges_by_hand(capi, oracle, dev):
    """A NUL inside and in front of the window, start >= len against '', a literal longer than m (also longer than 16 bytes),
    bytes >= 0x80: the rows of tests/test_unary_predicate_reference.py, on the device."""
    texts = (b"13-555", b"1\0-555", b"\0" b"3-555", b"31", b"\x80\xff-555", b"1")
    col = np.zeros((len(texts), 6), dtype=np.uint8)
    for i, text in enumerate(texts):
        col[i, :len(text)] = np.frombuffer(text, dtype=np.uint8)
    stripe = torch.from_numpy(col.reshape(-1)).to(dev)
    calls = Calls(capi, dev)
    n = len(texts)
    for spec in (("substring", 0, 2), ("substring", 1, 2), ("substring", 2, 4), ("substring", 2, 1), ("substring", 5, 300)):
        for literal in (b"13", b"1", b"", b"-555", b"13-", b"~~", b"\x80\xff", b"31\0x", b"13-555-0123456789abc"):
            for op in OPS:
                calls.cmp(spec, stripe, 6, n, op, literal, R.cmp_rows(oracle, spec, col, op, literal), None, True, repr((spec, literal, op)))
        for literals in ([b""], [b"13", b"31", b"\x80\xff"], [b"13-", b"31-"], [b"1", b"", b"-555"]):
            for negate in (False, True):
                calls.in_list(spec, stripe, 6, n, literals, negate, R.in_rows(spec, col, literals, negate), None, True, repr((spec, literals, negate)))
    calls.check()
    bitmap, count = capi.select_in_unary(T.substring_of(0, 2), torch.from_numpy(col).to(dev), [b"13", b"31"])
    assert bitmap.cpu().numpy().view(np.uint64).tolist() == [0x9000000000000000] and int(count.item()) == 2


# ----------------------------------------------------------------------------------------------------------------- DATE FIELD
def random_dates(rng, n):
    year = rng.integers(-(1 << 31), 1 << 31, size=n, dtype=np.int64)
    year[::2] = rng.integers(1992, 1999, size=year[::2].size)                 # TPC-H's
    year[1::7] = rng.integers(-5000, 0, size=year[1::7].size)                 # negative
    month = rng.integers(1, 13, size=n)
    month[:24] = np.tile(np.arange(1, 13), 2)[:min(n, 24)]
    raw = (year & 0xFFFFFFFF) | (month << 32) | (rng.integers(1, 32, size=n) << 40) | (rng.integers(0, 1 << 16, size=n) << 48)
    return raw.astype(np.uint64).view(np.int64)


def date_stripes(raw, dev):
    """The date stripe at a 16-byte boundary and 8 bytes behind one."""
    aligned = torch.from_numpy(raw).to(dev)
    holder = torch.zeros(raw.size + 3, dtype=torch.int64, device=dev)
    holder[1:1 + raw.size] = aligned
    assert aligned.data_ptr() % 16 == 0 and holder[1:].data_ptr() % 16 == 8
    return aligned, holder[1:1 + raw.size]


def date_literals(spec, raw):
    values = R.operand_values(spec, raw)
    if spec[0] == "year":
        return 1995, [[1996], [1992, 1994, 1995, 1998, int(values[1]), -3, 1 << 30], [int(v) for v in values[:30]] + [0, -1]]
    return 7, [[12], [1, 3, 5, 7, 8, 10, 12], list(range(-19, 12)) + [13]]      # (the long list leaves December out)


@pytest.mark.parametrize("unit", ("year", "month"))
def test_date_field_predicates_match_the_reference(capi, oracle, dev, unit):
    tile = capi.UNARY_DATE_TILE_ROWS
    sizes = rows_around(tile)
    rng = np.random.default_rng(77)
    raw = random_dates(rng, max(sizes))
    stripes = date_stripes(raw, dev)
    spec = (unit,)
    literal, lists = date_literals(spec, raw)
    assert [len(lit) for lit in lists] == [1, 7, 32]
    cmp_bits = [R.cmp_rows(oracle, spec, raw, op, literal) for op in OPS]
    in_bits = [R.in_rows(spec, raw, lit) for lit in lists]
    assert all(bits.any() and not bits.all() for bits in cmp_bits + in_bits)
    calls = Calls(capi, dev)
    turn = 0
    for offset, stripe in enumerate(stripes):
        for n in sizes:
            filt = make_filter(rng, n, dev)
            for k, op in enumerate(OPS):
                turn += 1
                calls.cmp(spec, stripe, 8, n, op, literal, cmp_bits[k], filt if turn & 1 else None, bool(turn & 2),
                          "%s n=%d offset=%d op=%d" % (unit, n, 8 * offset, op))
            for k, literals in enumerate(lists):
                for negate in (False, True):
                    turn += 1
                    calls.in_list(spec, stripe, 8, n, literals, negate, in_bits[k] != negate, filt if turn & 2 else None, bool(turn & 1),
                                  "%s n=%d offset=%d list=%d negate=%d" % (unit, n, 8 * offset, len(literals), negate))
    # the extremes of an INT literal: nothing wraps
    for literal in (-(1 << 31), (1 << 31) - 1):
        for op in OPS:
            calls.cmp(spec, stripes[0], 8, 1553, op, literal, R.cmp_rows(oracle, spec, raw, op, literal), None, True, "%s literal=%d op=%d" % (unit, literal, op))
    calls.check()


# ------------------------------------------------------------------------------------------------------------------ RUN FORMS
def _check_run(outs, counts, singles, what):
    torch.cuda.synchronize()
    for b, (out, (bitmap, count)) in enumerate(zip(outs, singles)):
        words = (RUN_ROWS[b] + 63) // 64
        assert torch.equal(out[:words], bitmap[:words]), (what, b)
        assert int(counts[b].item()) == int(count.item()), (what, b)


@pytest.mark.parametrize("spec,width", [(("substring", 0, 2), 15), (("substring", 1, 300), 3), (("substring", 5, 18), 25),
                                        (("substring", 254, 1), 255), (("year",), 8), (("month",), 8)],
                         ids=("char15", "char3", "char25-walk", "char255", "year", "month"))
def test_run_forms_equal_the_single_calls_block_by_block(capi, oracle, dev, spec, width):
    rng = np.random.default_rng(5)
    operand = operand_of(spec)
    if R.is_date(spec):
        host = [random_dates(rng, n) for n in RUN_ROWS]
        blocks = [torch.from_numpy(h).to(dev) for h in host]
        literal, lists = date_literals(spec, host[4])
    else:
        host = [random_chars(rng, n, width) for n in RUN_ROWS]
        blocks = [torch.from_numpy(h).to(dev) for h in host]
        literal = window_texts(host[4], spec[1], spec[2], [5])[0]
        lists = char_lists(host[4], spec[1], spec[2])
    filters_host = [make_filter(rng, n, dev) for n in RUN_ROWS]
    filters = [f[1] if b % 2 == 0 else None for b, f in enumerate(filters_host)]
    for op in OPS:
        outs, counts = capi.select_cmp_unary_blocks(operand, blocks, op, literal, filters=filters)
        singles = [capi.select_cmp_unary(operand, blk, op, literal, filter_bitmap=f) for blk, f in zip(blocks, filters)]
        _check_run(outs, counts, singles, ("cmp", op))
        for b, n in enumerate(RUN_ROWS):   # and the reference
            want, want_count = R.result(R.cmp_rows(oracle, spec, host[b], op, literal), n, filters_host[b][0] if b % 2 == 0 else None)
            assert np.array_equal(outs[b].cpu().numpy().view(np.uint64)[:want.size], want) and int(counts[b].item()) == want_count, (op, b)
    for literals in lists:
        for negate in (False, True):
            outs, counts = capi.select_in_unary_blocks(operand, blocks, literals, negate=negate, filters=None if negate else filters)
            singles = [capi.select_in_unary(operand, blk, literals, negate=negate, filter_bitmap=None if negate else f) for blk, f in zip(blocks, filters)]
            _check_run(outs, counts, singles, ("in", len(literals), negate))
            for b, n in enumerate(RUN_ROWS):
                want, want_count = R.result(R.in_rows(spec, host[b], literals, negate), n, filters_host[b][0] if b % 2 == 0 and not negate else None)
                assert np.array_equal(outs[b].cpu().numpy().view(np.uint64)[:want.size], want) and int(counts[b].item()) == want_count, (len(literals), negate, b)


# ----------------------------------------------------------------------------------------------------------------- DICTIONARIES
def test_over_a_dictionary_the_result_is_the_code_set(capi, oracle, dev):
    rng = np.random.default_rng(11)
    n = 5000
    # CHAR(15) phone numbers behind a dictionary of 300 entries, 2-byte codes
    phones = np.zeros((300, 15), dtype=np.uint8)
    for i in range(300):
        text = b"%02d-%03d-%03d-%04d" % (10 + i % 25, i, (7 * i) % 1000, (13 * i) % 10000)
        phones[i, :len(text)] = np.frombuffer(text, dtype=np.uint8)
    codes = rng.integers(0, 300, size=n).astype(np.uint16)
    spec, literals = ("substring", 0, 2), [b"13", b"31", b"23", b"29", b"30", b"18", b"17"]
    for negate in (False, True):
        code_set, _ = capi.select_in_unary(operand_of(spec), torch.from_numpy(phones).to(dev), literals, negate=negate)
        assert np.array_equal(code_set.cpu().numpy().view(np.uint64), R.result(R.in_rows(spec, phones, literals, negate), 300)[0])
        bitmap, count = capi.select_codes_in_set(torch.from_numpy(codes.view(np.int16)).to(dev), code_set, 300)
        want, want_count = R.result(R.in_rows(spec, phones[codes], literals, negate), n)
        assert np.array_equal(bitmap.cpu().numpy().view(np.uint64), want) and int(count.item()) == want_count
    code_set, _ = capi.select_cmp_unary(operand_of(("substring", 3, 3)), torch.from_numpy(phones).to(dev), T.GE, b"150")
    bitmap, count = capi.select_codes_in_set(torch.from_numpy(codes.view(np.int16)).to(dev), code_set, 300)
    want, want_count = R.result(R.cmp_rows(oracle, ("substring", 3, 3), phones[codes], T.GE, b"150"), n)
    assert np.array_equal(bitmap.cpu().numpy().view(np.uint64), want) and int(count.item()) == want_count and 0 < want_count < n
    # dates behind a dictionary of 200 entries, 1-byte codes
    dictionary = np.sort(random_dates(rng, 200))
    dcodes = rng.integers(0, 200, size=n).astype(np.uint8)
    for spec, op, literal in ((("year",), T.EQ, 1995), (("year",), T.LT, 1994), (("month",), T.GE, 11)):
        code_set, _ = capi.select_cmp_unary(operand_of(spec), torch.from_numpy(dictionary).to(dev), op, literal)
        bitmap, count = capi.select_codes_in_set(torch.from_numpy(dcodes).to(dev), code_set, 200)
        want, want_count = R.result(R.cmp_rows(oracle, spec, dictionary[dcodes], op, literal), n)
        assert np.array_equal(bitmap.cpu().numpy().view(np.uint64), want) and int(count.item()) == want_count and 0 < want_count < n
    code_set, _ = capi.select_in_unary(operand_of(("month",)), torch.from_numpy(dictionary).to(dev), [1, 6, 12], negate=True)
    bitmap, count = capi.select_codes_in_set(torch.from_numpy(dcodes).to(dev), code_set, 200)
    want, want_count = R.result(R.in_rows(("month",), dictionary[dcodes], [1, 6, 12], True), n)
    assert np.array_equal(bitmap.cpu().numpy().view(np.uint64), want) and int(count.item()) == want_count


# ----------------------------------------------------------------------------------------------------------------- DIFFERENTIAL
def test_the_fused_calls_equal_the_two_existing_calls_on_the_device(capi, dev):
    rng = np.random.default_rng(3)
    n = 3 * 1024 + 17
    filt = make_filter(rng, n, dev)[1]
    for width, start, length in ((15, 0, 2), (15, 14, 2), (25, 3, 20), (2, 1, 1), (64, 10, 300)):
        col = random_chars(rng, n, width)
        stripe = torch.from_numpy(col).to(dev)
        values = capi.eval_substring(stripe, start, length)
        literal = window_texts(col, start, length, [5])[0]
        lists = char_lists(col, start, length)
        for op in OPS:
            a = capi.select_cmp_unary(T.substring_of(start, length), stripe, op, literal, filter_bitmap=filt)
            b = capi.select_cmp_char(values, op, literal, filter_bitmap=filt)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (width, start, length, op)
        for literals in lists:
            for negate in (False, True):
                a = capi.select_in_unary(T.substring_of(start, length), stripe, literals, negate=negate, filter_bitmap=filt)
                b = capi.select_in_char(values, literals, negate=negate, filter_bitmap=filt)
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (width, start, length, len(literals), negate)
    raw = random_dates(rng, n)
    stripe = torch.from_numpy(raw).to(dev)
    for unit, spec in ((T.DATE_YEAR, ("year",)), (T.DATE_MONTH, ("month",))):
        values = capi.eval_date_extract(unit, stripe)
        literal, lists = date_literals(spec, raw)
        for op in OPS:
            a = capi.select_cmp_unary(T.date_field(unit), stripe, op, literal, filter_bitmap=filt)
            b = capi.select_cmp(values, op, literal, filter_bitmap=filt)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (unit, op)
        for literals in lists:
            for negate in (False, True):
                a = capi.select_in_unary(T.date_field(unit), stripe, literals, negate=negate, filter_bitmap=filt)
                b = capi.select_in(values, literals, negate=negate, filter_bitmap=filt)
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (unit, len(literals), negate)


# -------------------------------------------------------------------------------------------------------------------- ARGUMENTS
def test_argument_errors_are_those_of_the_composed_calls(capi, dev):
    lib = capi.lib
    dates = torch.zeros(9, dtype=torch.int64, device=dev)
    col = torch.zeros((8, 15), dtype=torch.uint8, device=dev)
    out = torch.full((3,), FILL, dtype=torch.int64, device=dev)
    count = torch.full((1,), FILL, dtype=torch.int64, device=dev)
    year, sub = T.date_field(T.DATE_YEAR), T.substring_of(0, 2)
    lit = (C.c_int32 * 2)(1995, 1996)
    slots, lengths = capi._in_char_literals([b"13", b"31"])
    d, c, o = C.c_void_p(dates.data_ptr()), C.c_void_p(col.data_ptr()), C.c_void_p(out.data_ptr())
    s = _stream()
    INV, UNS = T.ERR_INVALID_ARGUMENT, T.ERR_UNSUPPORTED

    def cmp(operand, stripe, width, n, op, literal, length, out_ptr=o):
        return lib.qsx_select_cmp_unary(C.byref(operand) if operand is not None else None, stripe, width, n, op, literal, length, None, out_ptr, None, s)

    def in_list(operand, stripe, width, n, literals, lens, num, negate, out_ptr=o):
        return lib.qsx_select_in_unary(C.byref(operand) if operand is not None else None, stripe, width, n, literals, lens, num, negate, None, out_ptr, None, s)

    assert cmp(None, d, 8, 8, T.EQ, lit, 0) == INV
    assert cmp(year, d, 8, -1, T.EQ, lit, 0) == INV
    assert cmp(year, d, 8, 8, 6, lit, 0) == INV and cmp(year, d, 8, 8, -1, lit, 0) == INV
    assert cmp(year, None, 8, 8, T.EQ, lit, 0) == INV and cmp(year, d, 8, 8, T.EQ, lit, 0, None) == INV
    assert cmp(year, d, 8, 8, T.EQ, None, 0) == INV
    assert cmp(year, d, 4, 8, T.EQ, lit, 0) == INV                                       # a date is 8 bytes wide
    assert cmp(year, C.c_void_p(dates.data_ptr() + 4), 8, 8, T.EQ, lit, 0) == INV         # and 8-byte aligned
    assert cmp(T.date_field(2), d, 8, 8, T.EQ, lit, 0) == UNS                             # DAY belongs to Datetime
    assert cmp(T.UnaryOperand(2, 0, 0, 1), d, 8, 8, T.EQ, lit, 0) == UNS                  # no such operation
    assert cmp(sub, c, 0, 8, T.EQ, b"13", 2) == INV and cmp(sub, c, 256, 8, T.EQ, b"13", 2) == INV
    assert cmp(T.substring_of(-1, 2), c, 15, 8, T.EQ, b"13", 2) == INV and cmp(T.substring_of(15, 2), c, 15, 8, T.EQ, b"13", 2) == INV
    assert cmp(T.substring_of(0, 0), c, 15, 8, T.EQ, b"13", 2) == INV
    assert cmp(sub, c, 15, 8, T.EQ, b"13", -1) == INV and cmp(sub, c, 15, 8, T.EQ, None, 2) == INV
    assert cmp(sub, c, 15, 8, T.EQ, b"x" * 65, 65) == UNS
    spare = torch.zeros(1, dtype=torch.int64, device=dev)
    assert cmp(sub, c, 15, 8, T.EQ, None, 0, C.c_void_p(spare.data_ptr())) == T.OK       # the empty literal needs no pointer
    assert spare.cpu().numpy().view(np.uint64).tolist() == [0xFF00000000000000]          # (and equals the eight empty texts)
    assert in_list(None, d, 8, 8, lit, None, 2, 0) == INV
    assert in_list(year, d, 8, 8, None, None, 2, 0) == INV
    assert in_list(year, d, 8, 8, lit, None, 0, 0) == INV and in_list(year, d, 8, 8, lit, None, T.MAX_IN_LIST + 1, 0) == INV
    assert in_list(year, d, 8, 8, lit, None, 2, 2) == INV
    assert in_list(year, C.c_void_p(dates.data_ptr() + 4), 8, 8, lit, None, 2, 0) == INV
    assert in_list(T.date_field(5), d, 8, 8, lit, None, 2, 0) == UNS
    assert in_list(sub, c, 15, 8, slots, None, 2, 0) == INV
    assert in_list(sub, c, 15, 8, slots, (C.c_int32 * 2)(2, -1), 2, 0) == INV
    assert in_list(sub, c, 15, 8, slots, (C.c_int32 * 2)(2, 65), 2, 0) == UNS
    assert in_list(T.substring_of(15, 1), c, 15, 8, slots, lengths, 2, 0) == INV
    rows = (C.c_int64 * 2)(8, -1)
    cols = (C.c_void_p * 2)(col.data_ptr(), col.data_ptr())
    outs = (C.c_void_p * 2)(out.data_ptr(), out.data_ptr())
    assert lib.qsx_select_cmp_unary_blocks(C.byref(sub), 15, 2, rows, cols, T.EQ, b"13", 2, None, outs, None, s) == INV        # negative rows
    assert lib.qsx_select_in_unary_blocks(C.byref(sub), 15, 2, rows, cols, slots, lengths, 2, 0, None, outs, None, s) == INV
    assert lib.qsx_select_cmp_unary_blocks(C.byref(sub), 15, -1, None, None, T.EQ, b"13", 2, None, None, None, s) == INV
    assert lib.qsx_select_cmp_unary_blocks(C.byref(sub), 15, 1, None, cols, T.EQ, b"13", 2, None, outs, None, s) == INV
    rows = (C.c_int64 * 2)(8, 1)
    assert lib.qsx_select_cmp_unary_blocks(C.byref(year), 8, 2, rows, (C.c_void_p * 2)(dates.data_ptr(), dates.data_ptr() + 4), T.EQ, lit, 0, None,
                                           outs, None, s) == INV
    assert lib.qsx_select_in_unary_blocks(C.byref(T.date_field(9)), 8, 2, rows, (C.c_void_p * 2)(dates.data_ptr(), dates.data_ptr() + 8), lit, None, 2, 0,
                                          None, outs, None, s) == UNS
    assert lib.qsx_select_cmp_unary_blocks(C.byref(year), 8, 0, None, None, T.EQ, lit, 0, None, None, None, s) == T.OK
    torch.cuda.synchronize()
    # n == 0: the count is overwritten, nothing else is touched
    assert lib.qsx_select_cmp_unary(C.byref(year), None, 8, 0, T.EQ, lit, 0, None, None, C.c_void_p(count.data_ptr()), s) == T.OK
    assert int(count.item()) == 0
    count.fill_(FILL)
    assert lib.qsx_select_in_unary(C.byref(sub), None, 15, 0, slots, lengths, 2, 1, None, None, C.c_void_p(count.data_ptr()), s) == T.OK
    assert int(count.item()) == 0
    assert torch.all(out == FILL)
