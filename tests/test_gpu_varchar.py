"""GPU: qsx_select_like_var, its run form and qsx_decode_codes_var against tests/varchar_reference.py — exact bitmaps, counts
and bytes.

Sizes cover the bitmap-word and tile edges of the kernels (csrc/varchar.hip: a LIKE tile holds min(1024, 48 KiB / (n + 1)
rounded down to 64) entries of a VARCHAR(n) dictionary, a decode tile min(1024, 32 KiB / out_width rounded down to 64) rows).
Every dictionary holds the empty string (an entry of 1 byte), a text of 1 byte (2) and texts of n bytes (n + 1).  A
VARCHAR(1) dictionary has at most 256 distinct values, fewer than a tile: its entry counts stop at 65, and the tile edge is
crossed for n = 23, 44 and 199.  The value bytes are read where the image leaves them, 0 / 1 / 7 / 15 bytes behind a 16-byte
boundary."""
import ctypes as C

import numpy as np
import pytest
import torch

import like_reference as L
import varchar_reference as V
from helpers import bitmap_dev, bitmap_np, to_dev
from quickstep_amd import types as T

pytestmark = pytest.mark.gpu

LENGTHS = (1, 23, 44, 199)
MISALIGN = (0, 1, 7, 15)
# as tests/test_gpu_like.py: a and b are common, the rest are the bytes a matcher could get wrong
ALPHABET = np.frombuffer(b"ab%_\\.*[(\n\x80", dtype=np.uint8)
WEIGHTS = np.array([0.34, 0.34] + [0.32 / 9] * 9)
PATTERNS = (b"ab", b"ab%", b"%ab", b"%ab%", b"a%b%a",          # lit, lit%, %lit, %lit%, a%b%c
            b"_b%", b"a_%", b"%_a", b"%a_", b"%a_b%",           # '_' at a segment's start and end
            b"%", b"")


def like_tile_entries(n):
    return max(64, min(1024, (48 * 1024 // (n + 1)) // 64 * 64))


def decode_tile_rows(width):
    return max(64, min(1024, (32 * 1024 // width) // 64 * 64))


def entry_counts(n):
    if n == 1:
        return (1, 63, 64, 65)
    tile = like_tile_entries(n)
    return tuple(sorted({1, 63, 64, 65, tile - 1, tile, tile + 1}))


def make_texts(n, count, seed):
    """`count` distinct texts of VARCHAR(n) in dictionary order: the empty string, a text of one byte and texts of exactly n
    bytes among them wherever `count` has room."""
    rng = np.random.default_rng(seed)
    texts = {b""} if count > 1 or n == 1 else set()
    if n == 1:
        pool = list(dict.fromkeys([bytes([c]) for c in ALPHABET] + [bytes([c]) for c in range(0x30, 0x7B)]))
        texts.update(pool[:count - 1])
        return V.sorted_texts(texts)
    if count > 2:
        texts.add(b"a")
    while len(texts) < count:
        kind = rng.random()
        length = n if kind < 0.25 or len(texts) + 1 == count else int(rng.integers(2, 13)) if kind < 0.7 else int(rng.integers(1, n + 1))
        texts.add(ALPHABET[rng.choice(ALPHABET.size, size=min(length, n), p=WEIGHTS)].tobytes())
    return V.sorted_texts(texts)


class Dictionary:
    """One dictionary image on the host and on the device, its value bytes at `at` bytes behind a 16-byte boundary."""

    def __init__(self, n, count, at, dev, with_null=True, seed=0):
        self.n, self.texts = n, make_texts(n, count, seed=seed + 31 * n + count)
        assert len(self.texts) == count
        header = 8 + 4 * count
        buffer, start = V.build_dictionary(self.texts, with_null=with_null, misalign=(at - header) % 16)
        self.size = header + sum(len(t) + 1 for t in self.texts)
        self.num_codes, self.null_code, self.offsets, self.values = V.parse_dictionary(buffer, start, self.size)
        assert V.check_dictionary(self.offsets, self.values) and self.num_codes == count
        self.image_dev = to_dev(buffer, dev)                                       # the whole image, as a block would hold it
        self.values_dev = self.image_dev[start + header:start + self.size]         # read in place
        assert self.values_dev.data_ptr() % 16 == at and self.values_dev.numel() == self.values.size
        self.offsets_dev = to_dev(self.offsets.view(np.int32), dev)                # the aligned copy the host layer makes


_dictionaries = {}


def dictionary(n, count, at, dev):
    key = (n, count, at)
    if key not in _dictionaries:
        _dictionaries[key] = Dictionary(n, count, at, dev)
    return _dictionaries[key]


def check_all(pending):
    """pending: (what, bitmap tensor, count tensor or None, expected bits).  One copy back for all of them."""
    words = torch.cat([bitmap.reshape(-1) for _, bitmap, _, _ in pending]).cpu().numpy().view(np.uint64)
    counted = [count for _, _, count, _ in pending if count is not None]
    counts = torch.cat(counted).cpu().numpy() if counted else np.zeros(0, dtype=np.int64)
    at = at_count = 0
    for what, bitmap, count, bits in pending:
        want = L.pack_bitmap(bits)
        assert np.array_equal(words[at:at + want.size], want), what
        at += bitmap.numel()
        if count is not None:
            assert counts[at_count] == int(bits.sum()), what
            at_count += 1


@pytest.mark.parametrize("n", LENGTHS)
def test_select_like_var_matches_the_reference(capi, dev, n):
    largest = max(entry_counts(n))
    keep = np.random.default_rng(7 + n).random(largest) < 0.7
    for count in entry_counts(n):
        words = L.pack_bitmap(keep[:count])
        words[-1] |= np.uint64((1 << ((-count) % 64)) - 1)       # set bits behind the last entry: they must not come through
        filter_dev = bitmap_dev(words, dev)
        pending = []
        for k, at in enumerate(MISALIGN):
            d = dictionary(n, count, at, dev)
            lengths = np.diff(np.append(d.offsets, d.values.size))
            if count > 2:
                assert lengths.min() == 1 and 2 in lengths and lengths.max() == n + 1      # "", one byte, n bytes
            for pattern in PATTERNS:
                for negate in (False, True):
                    bits = V.like_entries(d.offsets, d.values, pattern, negate)
                    if count >= 1023 and pattern not in (b"%", b""):
                        assert 0 < int(bits.sum()) < count, (n, count, pattern)            # a case that matches nothing shows nothing
                    # with and without a filter, with and without a count: every combination over the four alignments
                    with_filter, with_count = bool((k + negate) & 1), bool(k & 2) != negate
                    bitmap, got = capi.select_like_var(d.offsets_dev, d.values_dev, n, pattern, negate, filter_dev if with_filter else None,
                                                       want_count=with_count)
                    pending.append(((n, count, at, pattern, negate, with_filter), bitmap, got, bits & keep[:count] if with_filter else bits))
        check_all(pending)


def test_not_like_leaves_the_tail_bits_zero_and_the_count_is_overwritten(capi, dev):
    d = dictionary(23, 65, 1, dev)
    out = torch.full((2,), -1, dtype=torch.int64, device=dev)
    count = torch.full((1,), 12345, dtype=torch.int64, device=dev)
    for _ in range(2):       # the second call must not add to the first
        assert capi.lib.qsx_select_like_var(d.offsets_dev.data_ptr(), d.values_dev.data_ptr(), 65, d.values.size, 23, b"no such value", 13, 1,
                                            None, out.data_ptr(), count.data_ptr(), None) == 0
    words = bitmap_np(out)
    assert int(count.item()) == 65
    assert words[0] == np.uint64(0xFFFFFFFFFFFFFFFF) and words[1] == np.uint64(1 << 63)


def test_select_like_var_blocks_equals_the_per_dictionary_calls(capi, dev):
    n = 44
    tile = like_tile_entries(n)
    blocks = [dictionary(n, 65, 7, dev), None, dictionary(n, tile + 1, 15, dev), dictionary(n, 63, 0, dev)]      # None: no entries
    empty_offsets = torch.zeros(0, dtype=torch.int32, device=dev)
    empty_values = torch.zeros(0, dtype=torch.uint8, device=dev)
    offsets = [empty_offsets if d is None else d.offsets_dev for d in blocks]
    values = [empty_values if d is None else d.values_dev for d in blocks]
    keeps = [None if d is None else np.random.default_rng(90 + i).random(d.num_codes) < 0.6 for i, d in enumerate(blocks)]
    filters = [None if d is None or i == 3 else bitmap_dev(L.pack_bitmap(keeps[i]), dev) for i, d in enumerate(blocks)]
    for pattern in (b"%ab%", b"a%b%a", b"ab%"):
        for negate in (False, True):
            for use_filters in (None, filters):
                outs, counts = capi.select_like_var_blocks(offsets, values, n, pattern, negate, filters=use_filters)
                counts = counts.cpu().numpy()
                for i, d in enumerate(blocks):
                    if d is None:
                        assert counts[i] == 0
                        continue
                    f = use_filters[i] if use_filters else None
                    one, one_count = capi.select_like_var(d.offsets_dev, d.values_dev, n, pattern, negate, f)
                    bits = V.like_entries(d.offsets, d.values, pattern, negate)
                    if f is not None:
                        bits &= keeps[i]
                    want = L.pack_bitmap(bits)
                    assert np.array_equal(bitmap_np(outs[i])[:want.size], want), (pattern, negate, i)
                    assert np.array_equal(bitmap_np(one)[:want.size], want), (pattern, negate, i)
                    assert counts[i] == int(one_count.item()) == int(bits.sum()), (pattern, negate, i)


CODE_DTYPES = {1: np.uint8, 2: np.uint16, 4: np.uint32}
CODE_VIEWS = {1: np.uint8, 2: np.int16, 4: np.int32}


def make_codes(code_width, num_codes, rows, seed):
    """Random codes, the NULL code (= num_codes) among them."""
    codes = np.random.default_rng(seed).integers(0, num_codes + 1, size=rows).astype(CODE_DTYPES[code_width])
    if rows > 2:
        codes[1] = num_codes
    return codes


@pytest.mark.parametrize("code_width", (1, 2, 4))
def test_like_var_then_membership_equals_a_row_by_row_match(capi, dev, code_width):
    n = 23
    d = dictionary(n, 65 if code_width == 1 else like_tile_entries(n) + 1, 7, dev)
    rows = 10007
    codes = make_codes(code_width, d.num_codes, rows, seed=code_width)
    codes_dev = to_dev(codes.view(CODE_VIEWS[code_width]), dev)
    for pattern in (b"ab%", b"%ab", b"%a_b%", b"", b"%"):
        for negate in (False, True):
            code_set, _ = capi.select_like_var(d.offsets_dev, d.values_dev, n, pattern, negate)
            bitmap, count = capi.select_codes_in_set(codes_dev, code_set, d.num_codes)
            want = V.like_rows_coded(codes, d.offsets, d.values, pattern, negate)      # the NULL code is in no set, also for NOT LIKE
            assert np.array_equal(L.unpack_bitmap(bitmap_np(bitmap), rows), want), (pattern, negate)
            assert int(count.item()) == int(want.sum())
            if pattern not in (b"", b"%"):
                assert 0 < int(want.sum()) < rows - int((codes == d.num_codes).sum())


@pytest.mark.parametrize("n", LENGTHS)
def test_decode_codes_var_matches_the_reference(capi, dev, n):
    for code_width in (1, 2, 4):
        count = 65 if code_width == 1 or n == 1 else like_tile_entries(n) + 1
        d = dictionary(n, count, MISALIGN[code_width % 4], dev)
        tile = decode_tile_rows(n)
        sizes = sorted({1, 64, 65, 1000, tile + 1})
        codes = make_codes(code_width, d.num_codes, max(sizes), seed=10 * n + code_width)
        codes[0] = max(range(d.num_codes), key=lambda c: len(d.texts[c]))       # a text of exactly n = out_width bytes
        assert len(d.texts[int(codes[0])]) == n
        want = V.decode_rows(codes, d.offsets, d.values, n)
        assert want[0].all() and not want[1].any()                              # no terminator; the NULL code: all NUL
        codes_dev = to_dev(codes.view(CODE_VIEWS[code_width]), dev)
        for rows in sizes:
            out = torch.full((rows + 1, n), 0xAB, dtype=torch.uint8, device=dev)
            capi.decode_codes_var(codes_dev[:rows], d.offsets_dev, d.values_dev, n, out=out[:rows])
            got = out.cpu().numpy()
            assert np.array_equal(got[:rows], want[:rows]), (n, code_width, rows)     # the text, and zeros behind it
            assert (got[rows] == 0xAB).all(), (n, code_width, rows)                    # nothing behind the last row


def test_decode_codes_var_into_a_narrower_and_a_wider_field_at_an_odd_address(capi, dev):
    d = dictionary(44, 65, 15, dev)
    codes = make_codes(1, d.num_codes, 333, seed=3)
    codes_dev = to_dev(codes, dev)
    for out_width in (7, 44, 60, 255):
        buf = torch.full((333 * out_width + 32,), 0xAB, dtype=torch.uint8, device=dev)
        out = buf[3:3 + 333 * out_width].view(333, out_width)
        capi.decode_codes_var(codes_dev, d.offsets_dev, d.values_dev, out_width, out=out)
        got = buf.cpu().numpy()
        assert np.array_equal(got[3:3 + 333 * out_width].reshape(333, out_width), V.decode_rows(codes, d.offsets, d.values, out_width)), out_width
        assert (got[:3] == 0xAB).all() and (got[3 + 333 * out_width:] == 0xAB).all()


def test_argument_checks(capi, dev):
    lib = capi.lib
    d = dictionary(23, 65, 1, dev)
    out = torch.zeros(2, dtype=torch.int64, device=dev)
    codes = torch.zeros(8, dtype=torch.uint8, device=dev)
    field = torch.zeros(8 * 23, dtype=torch.uint8, device=dev)
    f, v, o, c, r, nb = d.offsets_dev.data_ptr(), d.values_dev.data_ptr(), out.data_ptr(), codes.data_ptr(), field.data_ptr(), d.values.size
    like = lib.qsx_select_like_var
    assert like(f, v, 65, nb, 23, b"a%", 2, 0, None, o, None, None) == 0
    assert like(f, v, 65, nb, 0, b"a%", 2, 0, None, o, None, None) == T.ERR_INVALID_ARGUMENT
    assert like(f, v, 65, nb, 256, b"a%", 2, 0, None, o, None, None) == T.ERR_UNSUPPORTED
    assert like(f, v, -1, nb, 23, b"a%", 2, 0, None, o, None, None) == T.ERR_INVALID_ARGUMENT
    assert like(f, v, 65, 64, 23, b"a%", 2, 0, None, o, None, None) == T.ERR_INVALID_ARGUMENT        # fewer bytes than entries
    assert like(f, v, 65, 1 << 32, 23, b"a%", 2, 0, None, o, None, None) == T.ERR_INVALID_ARGUMENT
    assert like(f + 1, v, 65, nb, 23, b"a%", 2, 0, None, o, None, None) == T.ERR_INVALID_ARGUMENT    # offsets are read as words
    assert like(f, v, 65, nb, 23, b"a%", -1, 0, None, o, None, None) == T.ERR_INVALID_ARGUMENT
    assert like(f, v, 65, nb, 23, b"a%", 2, 2, None, o, None, None) == T.ERR_INVALID_ARGUMENT
    assert like(None, v, 65, nb, 23, b"a%", 2, 0, None, o, None, None) == T.ERR_INVALID_ARGUMENT
    assert like(f, None, 65, nb, 23, b"a%", 2, 0, None, o, None, None) == T.ERR_INVALID_ARGUMENT
    assert like(f, v, 65, nb, 23, b"a%", 2, 0, None, None, None, None) == T.ERR_INVALID_ARGUMENT
    assert like(f, v, 65, nb, 23, None, 2, 0, None, o, None, None) == T.ERR_INVALID_ARGUMENT
    assert like(None, None, 0, 0, 23, b"", 0, 1, None, None, None, None) == 0                       # nothing to do is fine
    assert like(f, v, 65, nb, 23, b"a" * 65, 65, 0, None, o, None, None) == T.ERR_UNSUPPORTED
    assert like(f, v, 65, nb, 23, b"a" * 64, 64, 0, None, o, None, None) == 0
    one = lambda ptr: (C.c_void_p * 1)(ptr)
    i64 = lambda x: (C.c_int64 * 1)(x)
    blocks = lib.qsx_select_like_var_blocks
    assert blocks(23, 1, i64(65), one(f), one(v), i64(nb), b"a%", 2, 0, None, one(o), None, None) == 0
    assert blocks(23, 1, i64(65), one(f), one(v), i64(nb), b"a%", 2, 3, None, one(o), None, None) == T.ERR_INVALID_ARGUMENT
    assert blocks(23, 1, i64(65), one(None), one(v), i64(nb), b"a%", 2, 0, None, one(o), None, None) == T.ERR_INVALID_ARGUMENT
    assert blocks(23, 1, i64(65), one(f), one(None), i64(nb), b"a%", 2, 0, None, one(o), None, None) == T.ERR_INVALID_ARGUMENT
    assert blocks(23, 1, i64(65), one(f), one(v), i64(3), b"a%", 2, 0, None, one(o), None, None) == T.ERR_INVALID_ARGUMENT
    assert blocks(23, 1, i64(65), one(f), one(v), i64(nb), b"a" * 65, 65, 0, None, one(o), None, None) == T.ERR_UNSUPPORTED
    assert blocks(300, 1, i64(65), one(f), one(v), i64(nb), b"a%", 2, 0, None, one(o), None, None) == T.ERR_UNSUPPORTED
    assert blocks(23, 0, None, None, None, None, b"a%", 2, 0, None, None, None, None) == 0
    decode = lib.qsx_decode_codes_var
    assert decode(1, c, 8, f, v, 65, nb, 23, r, None) == 0
    assert decode(3, c, 8, f, v, 65, nb, 23, r, None) == T.ERR_UNSUPPORTED
    assert decode(1, c, 8, f, v, 65, nb, 0, r, None) == T.ERR_INVALID_ARGUMENT
    assert decode(1, c, 8, f, v, 65, nb, 256, r, None) == T.ERR_INVALID_ARGUMENT
    assert decode(1, None, 8, f, v, 65, nb, 23, r, None) == T.ERR_INVALID_ARGUMENT
    assert decode(1, c, 8, f, v, 65, nb, 23, None, None) == T.ERR_INVALID_ARGUMENT
    assert decode(1, c, 8, None, v, 65, nb, 23, r, None) == T.ERR_INVALID_ARGUMENT
    assert decode(1, c, -1, f, v, 65, nb, 23, r, None) == T.ERR_INVALID_ARGUMENT
    assert decode(1, None, 0, None, None, 0, 0, 23, None, None) == 0
    torch.cuda.synchronize()
