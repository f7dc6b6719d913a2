"""GPU: qsx_select_in, qsx_select_in_char, qsx_bitmap_eval and their run forms against tests/predicate_reference.py - every
output word and every count exactly.  Outputs are pre-filled with 0xFF (and counts with -1), so a word that is not written, or
written beyond the bitmap, shows.

Sizes: bitmap-word edges (0, 1, 63, 64, 65, 127), the tile of the CHAR register path and of a packed workgroup (4096, 4097),
several workgroups (3 * 4096 + 17); the evaluator's tile is 128 words, so it also gets 16384 + 1 rows (a third tile) and
32768 + 65 (a fifth).  Stripes also start 4 bytes (numeric) / 1 byte (CHAR) behind an aligned allocation."""
import ctypes as C

import numpy as np
import pytest
import torch

import predicate_reference as P
from helpers import bitmap_dev, bitmap_np, to_dev
from quickstep_amd import types as T

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 127, 4096, 4097, 3 * 4096 + 17)
N_MAX = SIZES[-1]
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
RUN_ROWS = [0, 1, 64, 65, 4097, 0, 130]


def words_of(n):
    return (n + 63) // 64


def fresh_out(n, dev, spare=2):
    """A bitmap of words_of(n) + spare words, every bit set."""
    return torch.full((words_of(n) + spare,), -1, dtype=torch.int64, device=dev)


def fresh_count(dev):
    return torch.full((1,), -1, dtype=torch.int64, device=dev)


def check_out(out, count, want_bits, n):
    got = bitmap_np(out)
    want = P.pack_bitmap(want_bits)
    assert np.array_equal(got[:words_of(n)], want), "bitmap words differ"
    assert (got[words_of(n):] == ONES).all(), "a word behind the bitmap was written"
    if count is not None:
        assert int(count.item()) == int(np.count_nonzero(want_bits))


def ptr(t, byte_offset=0):
    return None if t is None else C.c_void_p(t.data_ptr() + byte_offset)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def variants(n):
    """(offset stripe?, filter?, count?) per size: two complementary combinations everywhere, all eight at 65 and 4097."""
    if n in (65, 4097):
        return [(o, f, c) for o in (False, True) for f in (False, True) for c in (False, True)]
    return [(False, False, True), (True, True, False)]


# ------------------------------------------------------------------------------------------------------------ numeric IN
NP_TYPE = {T.INT: np.int32, T.LONG: np.int64, T.FLOAT: np.float32, T.DOUBLE: np.float64, T.DATE: np.int64}
C_TYPE = {T.INT: C.c_int32, T.LONG: C.c_int64, T.FLOAT: C.c_float, T.DOUBLE: C.c_double, T.DATE: C.c_int64}


def domain(qt):
    """Few distinct values, so that lists of every length hit: the extremes, and for floats NaN, both zeros and infinity."""
    if qt == T.INT:
        return np.array([-2**31, 2**31 - 1, -1, 0, 1, 2, 3, 5, 8, 13, 21, 34], dtype=np.int32)
    if qt == T.LONG:
        return np.array([-2**63, 2**63 - 1, -1, 0, 1, 2**32, 2**32 + 1, 5, 8, 13, 21, 34], dtype=np.int64)
    if qt in (T.FLOAT, T.DOUBLE):
        return np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, 1.5, -1.5, 2.0, 3.0, 1e30, 7.0, 0.1], dtype=NP_TYPE[qt])
    return np.array([T.date_raw(1995 + i // 4, 1 + i % 12, 1 + (7 * i) % 28) for i in range(12)], dtype=np.int64)


def literal_list(qt, k):
    d = domain(qt)
    if qt in (T.FLOAT, T.DOUBLE):
        base = [d[1], d[0], d[5], 99.0, d[3], 2.0, 2.0]          # 0.0 (equals -0.0 too), NaN (equals nothing), a miss, a duplicate
    elif qt == T.DATE:
        base = [int(d[0]) | (0x7B << 48), int(d[5]), T.date_raw(1900, 1, 1), int(d[7]), int(d[7]), int(d[2]), int(d[9])]  # padding differs
    else:
        base = [int(d[0]), int(d[2]), 77, int(d[1]), int(d[6]), int(d[6]), int(d[9])]    # the minimum, a miss, the maximum, a duplicate
    out = (base * 5)[:k] if k <= 7 else base + [base[i % 7] if i % 3 else 1000 + i for i in range(k - 7)]
    return out[:k]


_numeric = {}


def numeric_stripe(qt, dev):
    if qt not in _numeric:
        rng = np.random.default_rng(100 + qt)
        d = domain(qt)
        col = d[rng.integers(0, d.size, size=N_MAX)]
        if qt == T.DATE:                                        # random bytes in the two padding bytes: they never take part
            col = col | (rng.integers(0, 1 << 15, size=N_MAX).astype(np.int64) << 48)
        raw = torch.from_numpy(col.view(np.uint8).copy())
        aligned = raw.to(dev)
        shifted = torch.zeros(raw.numel() + 32, dtype=torch.uint8, device=dev)
        shifted[4:4 + raw.numel()] = aligned
        assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 0
        keep = rng.random(N_MAX) < 0.6
        _numeric[qt] = (col, aligned, shifted, keep)
    return _numeric[qt]


def call_select_in(capi, qt, col_ptr, n, lits, negate, filt, out, count):
    arr = (C_TYPE[qt] * len(lits))(*[float(v) if qt in (T.FLOAT, T.DOUBLE) else int(v) for v in lits])
    return capi.lib.qsx_select_in(qt, col_ptr, n, arr, len(lits), negate, ptr(filt), ptr(out), ptr(count), stream())


@pytest.mark.parametrize("k", (1, 2, 7, 32))
@pytest.mark.parametrize("qt", (T.INT, T.LONG, T.FLOAT, T.DOUBLE, T.DATE), ids=("int", "long", "float", "double", "date"))
def test_select_in_matches_the_reference(capi, dev, qt, k):
    col, aligned, shifted, keep = numeric_stripe(qt, dev)
    lits = literal_list(qt, k)
    assert len(lits) == k
    for negate in (0, 1):
        want_all = P.in_rows(col, lits, negate=negate, date=qt == T.DATE)
        for n in SIZES:
            filt = bitmap_dev(P.pack_bitmap(keep[:n]), dev) if n else None
            for offset, filtered, counted in variants(n):
                out, count = fresh_out(n, dev), fresh_count(dev) if counted else None
                rc = call_select_in(capi, qt, ptr(shifted, 4) if offset else ptr(aligned), n, lits, negate, filt if filtered else None, out, count)
                assert rc == T.OK
                want = want_all[:n] & keep[:n] if filtered and n else want_all[:n]
                check_out(out, count, want, n)


def test_select_in_special_values(capi, dev):
    """NaN is in no list (so NOT IN selects it), -0.0 equals 0.0, the integer minima are ordinary values."""
    for qt, values in ((T.DOUBLE, [np.nan, 0.0, -0.0, 1.0]), (T.FLOAT, [np.nan, 0.0, -0.0, 1.0])):
        col = np.array(values, dtype=NP_TYPE[qt])
        bm, cnt = capi.select_in(to_dev(col, dev), [float("nan"), -0.0])
        assert P.unpack_bitmap(bitmap_np(bm), 4).tolist() == [False, True, True, False] and int(cnt.item()) == 2
        bm, cnt = capi.select_in(to_dev(col, dev), [float("nan"), -0.0], negate=True)
        assert P.unpack_bitmap(bitmap_np(bm), 4).tolist() == [True, False, False, True] and int(cnt.item()) == 2
    for np_type, low in ((np.int32, -2**31), (np.int64, -2**63)):
        col = np.array([low, low + 1, 0, -low - 1], dtype=np_type)
        bm, _ = capi.select_in(to_dev(col, dev), [low, -low - 1])
        assert P.unpack_bitmap(bitmap_np(bm), 4).tolist() == [True, False, False, True]


def test_select_in_argument_errors(capi, dev):
    col = to_dev(np.arange(8, dtype=np.int32), dev)
    out, count = fresh_out(8, dev), fresh_count(dev)
    bad = [call_select_in(capi, T.INT, ptr(col), 8, [1] * k, 0, None, out, count) for k in (33,)]
    bad.append(capi.lib.qsx_select_in(T.INT, ptr(col), 8, (C.c_int32 * 1)(1), 0, 0, None, ptr(out), ptr(count), stream()))
    bad.append(call_select_in(capi, T.INT, ptr(col), 8, [1], 2, None, out, count))
    bad.append(call_select_in(capi, T.INT, None, 8, [1], 0, None, out, count))
    bad.append(call_select_in(capi, T.INT, ptr(col), 8, [1], 0, None, None, count))
    assert bad == [T.ERR_INVALID_ARGUMENT] * 5
    torch.cuda.synchronize()
    assert (bitmap_np(out) == ONES).all() and int(count.item()) == -1


# --------------------------------------------------------------------------------------------------------------- CHAR IN
WIDTHS = (1, 2, 10, 16, 17, 25, 64, 255)


def char_vocabulary(width):
    """Texts of a CHAR(width) attribute: the empty text, short ones, one of the full width (no NUL in the field), one a byte
    shorter, and pairs that are equal up to some byte."""
    texts = [b"", b"A", b"B", b"MAIL"[:width], b"SHIP"[:width], b"MAILS"[:width], b"X" * width, b"X" * (width - 1), b"Y" * width,
             (b"X" * (width - 1) + b"Z")[:width], b"REG AIR"[:width], b"\x80\xff"[:width]]
    return list(dict.fromkeys(texts))


_chars = {}


def char_stripe(width, dev):
    if width not in _chars:
        rng = np.random.default_rng(500 + width)
        vocabulary = char_vocabulary(width)
        pick = rng.integers(0, len(vocabulary), size=N_MAX)
        col = rng.integers(1, 256, size=(N_MAX, width)).astype(np.uint8)        # what lies behind a NUL is random: it never takes part
        for i, v in enumerate(vocabulary):
            rows = np.nonzero(pick == i)[0]
            col[rows, :len(v)] = np.frombuffer(v, dtype=np.uint8)
            if len(v) < width:
                col[rows, len(v)] = 0
        flat = torch.from_numpy(col.reshape(-1))
        aligned = flat.to(dev)
        shifted = torch.zeros(flat.numel() + 32, dtype=torch.uint8, device=dev)
        shifted[1:1 + flat.numel()] = aligned
        keep = rng.random(N_MAX) < 0.6
        _chars[width] = (col, aligned, shifted, keep)
    return _chars[width]


def char_lists(width):
    full = b"X" * width
    lists = [[b"MAIL"[:width]],                                            # K = 1
             [b"", b"SHIP"[:width]],                                       # the empty literal
             [b"MA\0IL", b"B"] if width >= 2 else [b"A\0B", b"B"],         # a NUL inside ends the literal: "MA" / "A"
             [b"MAIL"[:width], b"Q", b"MAIL"[:width], b"REG AIR"[:width], b"Y" * min(width, 64), b"nothing"[:width], b"A"]]   # 7, a duplicate
    if width <= 64:
        lists.append([full, b"B"])                                         # a full-width field without NUL against an equal literal
    if width < 64:
        lists.append([full + b"X", b"A"])                                  # longer than the field: equals none
    lists.append([(b"%04d" % i)[:width] if i % 4 else char_vocabulary(width)[i % len(char_vocabulary(width))][:64] for i in range(32)])   # 32
    return lists


def call_select_in_char(capi, col_ptr, width, n, lits, negate, filt, out, count, lengths=None):
    slots, lens = capi._in_char_literals(lits)
    if lengths is not None:
        lens = (C.c_int32 * len(lengths))(*lengths)
    return capi.lib.qsx_select_in_char(col_ptr, width, n, slots, lens, len(lits), negate, ptr(filt), ptr(out), ptr(count), stream())


@pytest.mark.parametrize("width", WIDTHS)
def test_select_in_char_matches_the_reference(capi, dev, width):
    col, aligned, shifted, keep = char_stripe(width, dev)
    for lits in char_lists(width):
        for negate in (0, 1):
            want_all = P.in_char_rows(col, lits, negate=negate)
            for n in SIZES:
                filt = bitmap_dev(P.pack_bitmap(keep[:n]), dev) if n else None
                for offset, filtered, counted in variants(n):
                    out, count = fresh_out(n, dev), fresh_count(dev) if counted else None
                    rc = call_select_in_char(capi, ptr(shifted, 1) if offset else ptr(aligned), width, n, lits, negate,
                                             filt if filtered else None, out, count)
                    assert rc == T.OK
                    check_out(out, count, want_all[:n] & keep[:n] if filtered and n else want_all[:n], n)


def test_select_in_char_text_ends_at_the_nul(capi, dev):
    """Fields that differ only behind their NUL are the same text; a full-width field has no NUL and still equals its literal."""
    col = np.frombuffer(b"AB\0x" b"AB\0y" b"ABCD" b"ABC\0" b"\0zzz", dtype=np.uint8).reshape(5, 4)
    for lits, want in (([b"AB"], [1, 1, 0, 0, 0]), ([b"ABCD"], [0, 0, 1, 0, 0]), ([b""], [0, 0, 0, 0, 1]), ([b"ABCDE"], [0] * 5),
                       ([b"ABC", b"AB\0CD"], [1, 1, 0, 1, 0])):
        bm, cnt = capi.select_in_char(to_dev(col, dev), lits)
        assert P.unpack_bitmap(bitmap_np(bm), 5).tolist() == [bool(w) for w in want], lits
        assert int(cnt.item()) == sum(want)
        bm, cnt = capi.select_in_char(to_dev(col, dev), lits, negate=True)
        assert P.unpack_bitmap(bitmap_np(bm), 5).tolist() == [not w for w in want] and bitmap_np(bm)[0] & np.uint64((1 << 59) - 1) == 0


@pytest.mark.parametrize("width", (2, 10, 25))
def test_select_in_char_over_a_dictionary_gives_the_code_set(capi, dev, width):
    rng = np.random.default_rng(900 + width)
    vocabulary = sorted(set(char_vocabulary(width)) | {(b"v%03d" % i)[:width] for i in range(150)})
    dictionary = np.zeros((len(vocabulary), width), dtype=np.uint8)
    for i, v in enumerate(vocabulary):
        dictionary[i, :len(v)] = np.frombuffer(v, dtype=np.uint8)
    codes = rng.integers(0, len(vocabulary) + 1, size=4097).astype(np.uint8)      # the NULL code (= num_codes) among them
    lits = [b"MAIL"[:width], b"v007"[:width], b"", b"v149"[:width], b"nope"[:width]]
    for negate in (False, True):
        code_set, _ = capi.select_in_char(to_dev(dictionary, dev), lits, negate=negate, want_count=False)
        bm, cnt = capi.select_codes_in_set(to_dev(codes, dev), code_set, len(vocabulary))
        in_dictionary = codes < len(vocabulary)
        want = np.zeros(codes.size, dtype=bool)
        want[in_dictionary] = P.in_char_rows(dictionary[codes[in_dictionary]], lits, negate=negate)
        assert np.array_equal(bitmap_np(bm)[:words_of(codes.size)], P.pack_bitmap(want)) and int(cnt.item()) == int(want.sum())


def test_select_in_char_argument_errors(capi, dev):
    col = to_dev(np.zeros((8, 4), dtype=np.uint8), dev)
    out, count = fresh_out(8, dev), fresh_count(dev)
    invalid = [call_select_in_char(capi, ptr(col), 4, 8, [b"a"] * 33, 0, None, out, count),
               capi.lib.qsx_select_in_char(ptr(col), 4, 8, C.create_string_buffer(64), (C.c_int32 * 1)(1), 0, 0, None, ptr(out), ptr(count), stream()),
               call_select_in_char(capi, ptr(col), 4, 8, [b"a"], 2, None, out, count),
               call_select_in_char(capi, ptr(col), 0, 8, [b"a"], 0, None, out, count),
               call_select_in_char(capi, ptr(col), 256, 8, [b"a"], 0, None, out, count),
               call_select_in_char(capi, None, 4, 8, [b"a"], 0, None, out, count),
               call_select_in_char(capi, ptr(col), 4, 8, [b"a"], 0, None, None, count)]
    assert invalid == [T.ERR_INVALID_ARGUMENT] * 7
    assert call_select_in_char(capi, ptr(col), 4, 8, [b"a", b"b"], 0, None, out, count, lengths=[1, 65]) == T.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (bitmap_np(out) == ONES).all() and int(count.item()) == -1


# ------------------------------------------------------------------------------------------------------------- evaluator
EVAL_SIZES = SIZES + (16384 + 1, 32768 + 65)
A, O, N = T.BOOL_AND, T.BOOL_OR, T.BOOL_NOT

_leaves = {}


def leaf_bitmaps(dev):
    """32 random leaf bitmaps of the largest size (host words, device tensors) and a filter."""
    if not _leaves:
        rng = np.random.default_rng(4242)
        n = max(EVAL_SIZES)
        host = [P.pack_bitmap(rng.random(n) < p) for p in np.linspace(0.05, 0.95, 32)]
        _leaves["host"] = host
        _leaves["dev"] = [bitmap_dev(w, dev) for w in host]
        # the same bitmaps one word (8 bytes) behind an aligned allocation: where the host layer's leaf bitmaps lie
        _leaves["dev_odd"] = [bitmap_dev(np.concatenate([np.zeros(1, dtype=np.uint64), w]), dev)[1:] for w in host]
        assert all(t.data_ptr() % 16 == 8 for t in _leaves["dev_odd"])
        _leaves["filter"] = P.pack_bitmap(rng.random(n) < 0.7)
        _leaves["filter_dev"] = bitmap_dev(_leaves["filter"], dev)
    return _leaves["host"], _leaves["dev"], _leaves["filter"], _leaves["filter_dev"]


def head(words, n):
    """The first n bits of a bitmap as a bitmap of n bits (the tail of its last word cleared)."""
    return P.pack_bitmap(P.unpack_bitmap(words, n))


def call_eval(capi, leaves, program, n, filt, out, count, num_leaves=None):
    arr = (C.c_void_p * max(len(leaves), 1))(*[None if t is None else t.data_ptr() for t in leaves])
    prog = (C.c_int32 * max(len(program), 1))(*program)
    return capi.lib.qsx_bitmap_eval(len(leaves) if num_leaves is None else num_leaves, arr, len(program), prog, n, ptr(filt), ptr(out),
                                    ptr(count), stream())


def check_eval(capi, dev, leaves_host, leaves_dev, program, n, filt_host=None, filt_dev=None, counted=True):
    out, count = fresh_out(n, dev), fresh_count(dev) if counted else None
    assert call_eval(capi, leaves_dev, program, n, filt_dev, out, count) == T.OK
    want, want_count = P.eval_program([None if w is None else head(w, n) for w in leaves_host], program, n,
                                      None if filt_host is None else head(filt_host, n))
    got = bitmap_np(out)
    assert np.array_equal(got[:words_of(n)], want), program
    assert (got[words_of(n):] == ONES).all()
    if counted:
        assert int(count.item()) == want_count


def test_bitmap_eval_truth_tables(capi, dev):
    """Every function of one leaf and of two: the leaves, negated or not, under AND / OR, negated or not."""
    n = 127
    a = P.pack_bitmap(np.arange(n) % 4 >= 2)
    b = P.pack_bitmap(np.arange(n) % 2 == 1)
    host, device = [a, b], [bitmap_dev(a, dev), bitmap_dev(b, dev)]
    for program in ([0], [0, N], [1], [1, N], [0, N, N]):
        check_eval(capi, dev, host, device, program, n)
    tables = set()
    for na in (0, 1):
        for nb in (0, 1):
            for op in (A, O):
                for nout in (0, 1):
                    program = [0] + [N] * na + [1] + [N] * nb + [op] + [N] * nout
                    check_eval(capi, dev, host, device, program, n)
                    out, _ = P.eval_program(host, program, n)
                    tables.add(tuple(P.unpack_bitmap(out, 4).tolist()))
    assert len(tables) == 8                       # the eight AND / OR functions of two literals; XOR needs each leaf twice:
    check_eval(capi, dev, host, device, [0, 1, N, A, 0, N, 1, A, O], n)


@pytest.mark.parametrize("seed", range(12))
def test_bitmap_eval_random_programs(capi, dev, seed):
    host, device, filt, filt_dev = leaf_bitmaps(dev)
    rng = np.random.default_rng(seed)
    num_leaves = (1, 2, 5, 32)[seed % 4] if seed < 8 else int(rng.integers(1, 33))
    program = P.random_program(rng, num_leaves, length=64 if seed % 3 == 0 else None, want_depth=8 if seed % 4 == 1 else None)
    drop = rng.random(num_leaves) < (0.25 if seed % 2 else 0.0)          # NULL leaf pointers: the all-zero bitmap
    leaves_host = [None if drop[k] else host[k] for k in range(num_leaves)]
    if seed % 2:
        device = _leaves["dev_odd"]
    leaves_dev = [None if drop[k] else device[k] for k in range(num_leaves)]
    for i, n in enumerate(EVAL_SIZES):
        filtered = (i + seed) % 2 == 0
        check_eval(capi, dev, leaves_host, leaves_dev, program, n, filt if filtered else None, filt_dev if filtered else None,
                   counted=(i + seed) % 3 != 0)


def test_bitmap_eval_deepest_and_longest_program(capi, dev):
    host, device, filt, filt_dev = leaf_bitmaps(dev)
    deepest = list(range(8)) + [A, O, A, O, A, O, A]                      # depth exactly 8
    assert P.program_depth(deepest) == 8
    longest = [0] + [N] * 63                                               # 64 instructions
    q19 = []                                                               # three OR-ed conjunctions of six leaves and a seventh under NOT
    for g in range(3):
        for k in range(7):
            q19 += [7 * g + k] + ([N] if k == 6 else []) + ([A] if k else [])
        q19 += [O] if g else []
    for program in (deepest, longest, q19):
        for n in (65, 4097, 32768 + 65):
            check_eval(capi, dev, host, device, program, n, filt, filt_dev)


def test_bitmap_eval_refuses_invalid_programs_and_writes_nothing(capi, dev):
    host, device, _, _ = leaf_bitmaps(dev)
    n = 130
    out, count = fresh_out(n, dev), fresh_count(dev)
    invalid = {"underflow of a binary operator": [0, A], "underflow of NOT": [N], "two values left": [0, 1], "no instruction": [],
               "a leaf that is not there": [0, 2, O], "an unknown code": [0, 1, -4], "65 instructions": [0] + [N] * 64,
               "depth 9": list(range(2)) * 4 + [0] + [A] * 8}
    for what, program in invalid.items():
        assert not P.program_ok(2, program), what
        assert call_eval(capi, device[:2], program, n, None, out, count) == T.ERR_INVALID_ARGUMENT, what
    assert call_eval(capi, device[:2], [0], n, None, out, count, num_leaves=0) == T.ERR_INVALID_ARGUMENT
    assert call_eval(capi, device + device[:1], [0], n, None, out, count) == T.ERR_INVALID_ARGUMENT   # 33 leaves
    assert call_eval(capi, device[:2], [0], n, None, None, count) == T.ERR_INVALID_ARGUMENT         # no output
    assert call_eval(capi, [device[0], out], [0, 1, A], n, None, out, count) == T.ERR_INVALID_ARGUMENT   # the output is an input
    torch.cuda.synchronize()
    assert (bitmap_np(out) == ONES).all() and int(count.item()) == -1


# ------------------------------------------------------------------------------------------------------------- run forms
def run_cuts():
    ends = np.cumsum(RUN_ROWS)
    return list(zip(ends - RUN_ROWS, ends))


def run_filters(dev, keep):
    """A filter per block, every third entry NULL."""
    host = [None if b % 3 == 1 or e == s else keep[s:e] for b, (s, e) in enumerate(run_cuts())]
    return host, [None if h is None else bitmap_dev(P.pack_bitmap(h), dev) for h in host]


@pytest.mark.parametrize("qt", (T.INT, T.DOUBLE, T.DATE), ids=("int", "double", "date"))
def test_select_in_blocks_is_the_per_block_call(capi, dev, qt):
    col, _, _, keep = numeric_stripe(qt, dev)
    torch_type = {T.INT: torch.int32, T.DOUBLE: torch.float64, T.DATE: torch.int64}[qt]
    blocks = [torch.from_numpy(col[s:e].copy()).view(torch_type).to(dev) for s, e in run_cuts()]
    filters_host, filters_dev = run_filters(dev, keep)
    for k, negate in ((2, False), (7, True), (32, False)):
        lits = literal_list(qt, k)
        for filters in (None, filters_dev):
            outs, counts = capi.select_in_blocks(blocks, lits, negate=negate, filters=filters, qtype=qt)
            for b, (s, e) in enumerate(run_cuts()):
                f = None if filters is None else filters[b]
                one, one_count = capi.select_in(blocks[b], lits, negate=negate, filter_bitmap=f, qtype=qt)
                want = P.in_rows(col[s:e], lits, negate=negate, date=qt == T.DATE)
                if f is not None:
                    want = want & filters_host[b]
                assert np.array_equal(bitmap_np(outs[b])[:words_of(e - s)], bitmap_np(one)[:words_of(e - s)])
                assert np.array_equal(bitmap_np(outs[b])[:words_of(e - s)], P.pack_bitmap(want))
                assert int(counts[b].item()) == int(one_count.item()) == int(want.sum())


@pytest.mark.parametrize("width", (10, 25))
def test_select_in_char_blocks_is_the_per_block_call(capi, dev, width):
    col, _, _, keep = char_stripe(width, dev)
    blocks = [to_dev(col[s:e], dev) for s, e in run_cuts()]
    filters_host, filters_dev = run_filters(dev, keep)
    for lits, negate in ((char_lists(width)[1], False), (char_lists(width)[3], True), (char_lists(width)[-1], False)):
        for filters in (None, filters_dev):
            outs, counts = capi.select_in_char_blocks(blocks, lits, negate=negate, filters=filters)
            for b, (s, e) in enumerate(run_cuts()):
                f = None if filters is None else filters[b]
                one, one_count = capi.select_in_char(blocks[b], lits, negate=negate, filter_bitmap=f)
                want = P.in_char_rows(col[s:e], lits, negate=negate)
                if f is not None:
                    want = want & filters_host[b]
                assert np.array_equal(bitmap_np(outs[b])[:words_of(e - s)], bitmap_np(one)[:words_of(e - s)])
                assert np.array_equal(bitmap_np(outs[b])[:words_of(e - s)], P.pack_bitmap(want))
                assert int(counts[b].item()) == int(one_count.item()) == int(want.sum())


@pytest.mark.parametrize("width", (10, 16))
def test_char_runs_whose_blocks_differ_in_alignment(capi, dev, width):
    """A run of short CHAR fields in which one stripe lies 1 byte off and the others on a 16-byte boundary: the host sizes tiles
    and LDS once for the run, so every block has to take the path the host chose.  More than 1024 rows per block, so that all
    four waves of a workgroup work on a tile.  Both the IN list and the CHAR comparison's run form."""
    col, aligned, shifted, keep = char_stripe(width, dev)
    cuts = [(0, 4097), (4097, 4097 + 1500), (5597, 5597 + 3000), (8597, 8597 + 1024)]
    blocks = []
    for b, (s_, e_) in enumerate(cuts):
        rows = e_ - s_
        if b == 1:    # 1 byte behind a 16-byte boundary
            buf = torch.zeros(rows * width + 32, dtype=torch.uint8, device=dev)
            buf[1:1 + rows * width] = aligned[s_ * width:e_ * width]
            view = buf[1:1 + rows * width].view(rows, width)
            assert view.data_ptr() % 16 == 1
        else:
            view = aligned[s_ * width:e_ * width].clone().view(rows, width)
            assert view.data_ptr() % 16 == 0
        blocks.append(view)
    filters_host = [keep[s_:e_] if b % 2 == 0 else None for b, (s_, e_) in enumerate(cuts)]
    filters_dev = [None if h is None else bitmap_dev(P.pack_bitmap(h), dev) for h in filters_host]
    for lits in (char_lists(width)[1], char_lists(width)[3], char_lists(width)[-1]):
        for negate in (False, True):
            for filters in (None, filters_dev):
                outs, counts = capi.select_in_char_blocks(blocks, lits, negate=negate, filters=filters)
                for b, (s_, e_) in enumerate(cuts):
                    want = P.in_char_rows(col[s_:e_], lits, negate=negate)
                    if filters is not None and filters[b] is not None:
                        want = want & filters_host[b]
                    assert np.array_equal(bitmap_np(outs[b])[:words_of(e_ - s_)], P.pack_bitmap(want)), (b, lits, negate)
                    assert int(counts[b].item()) == int(want.sum())
    for op, name in ((T.EQ, "="), (T.LT, "<"), (T.GE, ">=")):
        literal = b"MAIL"[:width]
        outs, counts = capi.select_cmp_char_blocks(blocks, op, literal)
        for b, (s_, e_) in enumerate(cuts):
            want = P.leaf_rows(("cmp", "c", name, literal), {"c": col[s_:e_]})
            assert np.array_equal(bitmap_np(outs[b])[:words_of(e_ - s_)], P.pack_bitmap(want)), (b, name)
            assert int(counts[b].item()) == int(want.sum())


def test_bitmap_eval_refuses_an_output_inside_an_input(capi, dev):
    """The output may not share a byte with a leaf or the filter: not only the same address, any overlap of the two ranges."""
    n = 64 * 10
    big = torch.full((32,), -1, dtype=torch.int64, device=dev)
    other = torch.zeros(10, dtype=torch.int64, device=dev)
    count = fresh_count(dev)
    leaf, inside, behind = big[0:10], big[4:14], big[10:20]
    assert call_eval(capi, [leaf, other], [0, 1, O], n, None, inside, count) == T.ERR_INVALID_ARGUMENT
    assert call_eval(capi, [other], [0], n, leaf, inside, count) == T.ERR_INVALID_ARGUMENT            # inside the filter
    rows = (C.c_int64 * 1)(n)
    leaves = (C.c_void_p * 2)(leaf.data_ptr(), other.data_ptr())
    outs = (C.c_void_p * 1)(inside.data_ptr())
    program = (C.c_int32 * 3)(0, 1, O)
    assert capi.lib.qsx_bitmap_eval_blocks(2, 3, program, 1, rows, leaves, None, outs, ptr(count), stream()) == T.ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert (bitmap_np(big) == ONES).all() and int(count.item()) == -1
    assert call_eval(capi, [leaf, other], [0, 1, O], n, None, behind, count) == T.OK                  # directly behind the leaf: no overlap
    torch.cuda.synchronize()
    assert (bitmap_np(big)[:20] == ONES).all() and int(count.item()) == n


@pytest.mark.parametrize("seed", range(4))
def test_bitmap_eval_blocks_is_the_per_block_call(capi, dev, seed):
    rng = np.random.default_rng(70 + seed)
    num_leaves = (1, 3, 8, 32)[seed]
    program = P.random_program(rng, num_leaves, want_depth=8 if seed == 2 else None)
    rows = RUN_ROWS + ([40000] if seed == 3 else [])                      # (a block of more than one tile)
    bits = [[rng.random(r) < 0.5 for _ in range(num_leaves)] for r in rows]
    absent = [[r > 0 and rng.random() < 0.2 for _ in range(num_leaves)] for r in rows]        # NULL leaf entries
    leaves_host = [[None if absent[b][k] or rows[b] == 0 else P.pack_bitmap(bits[b][k]) for k in range(num_leaves)] for b in range(len(rows))]
    leaves_dev = [[None if w is None else bitmap_dev(w, dev) for w in block] for block in leaves_host]
    keep = [rng.random(r) < 0.7 for r in rows]
    filters_dev = [None if b % 3 == 1 or rows[b] == 0 else bitmap_dev(P.pack_bitmap(keep[b]), dev) for b in range(len(rows))]
    for filters in (None, filters_dev):
        outs = [fresh_out(r, dev) for r in rows]
        outs, counts = capi.bitmap_eval_blocks(leaves_dev, program, rows, dev, filters=filters, out_bitmaps=outs)
        for b, r in enumerate(rows):
            f = None if filters is None else filters[b]
            want, want_count = P.eval_program(leaves_host[b], program, r, None if f is None else P.pack_bitmap(keep[b]))
            got = bitmap_np(outs[b])
            assert np.array_equal(got[:words_of(r)], want) and (got[words_of(r):] == ONES).all()
            assert int(counts[b].item()) == want_count
            if r:
                one, one_count = capi.bitmap_eval(leaves_dev[b], program, r, filter_bitmap=f, out_bitmap=fresh_out(r, dev))
                assert np.array_equal(bitmap_np(one)[:words_of(r)], got[:words_of(r)]) and int(one_count.item()) == want_count


# ------------------------------------------------------------------------------------- the aligned-only knob of the K1 kernels
def _aligned_only_child():
    """Runs in a process of its own with QSX_SELECT_ALIGNED_ONLY=1 (the library reads it once): a stripe 4 bytes behind a 16-byte
    boundary then takes the row-per-lane IN kernel, and a run that holds one goes block by block."""
    import quickstep_amd.capi as capi
    dev = torch.device("cuda:0")
    for qt in (T.INT, T.LONG, T.DATE):
        col, aligned, shifted, keep = numeric_stripe(qt, dev)
        lits = literal_list(qt, 7)
        for negate in (0, 1):
            want_all = P.in_rows(col, lits, negate=negate, date=qt == T.DATE)
            for n in SIZES:
                filt = bitmap_dev(P.pack_bitmap(keep[:n]), dev) if n else None
                for filtered in (False, True):
                    out, count = fresh_out(n, dev), fresh_count(dev)
                    assert call_select_in(capi, qt, ptr(shifted, 4), n, lits, negate, filt if filtered else None, out, count) == T.OK
                    check_out(out, count, want_all[:n] & keep[:n] if filtered and n else want_all[:n], n)
    col, _, shifted, _ = numeric_stripe(T.INT, dev)
    width = 4
    cuts = [(0, 65), (65, 65), (65, 4200)]
    blocks = [shifted[4 + s * width:4 + e * width].view(torch.int32) for s, e in cuts]
    outs, counts = capi.select_in_blocks(blocks, literal_list(T.INT, 7), negate=True)
    for (s, e), o, c in zip(cuts, outs, counts):
        want = P.in_rows(col[s:e], literal_list(T.INT, 7), negate=True)
        assert np.array_equal(bitmap_np(o)[:words_of(e - s)], P.pack_bitmap(want)) and int(c.item()) == int(want.sum())
    print("aligned-only child ok")


def test_select_in_under_the_aligned_only_knob(dev):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, QSX_SELECT_ALIGNED_ONLY="1", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--aligned-only-child"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "aligned-only child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


if __name__ == "__main__":
    import sys
    if sys.argv[1:] == ["--aligned-only-child"]:
        _aligned_only_child()
