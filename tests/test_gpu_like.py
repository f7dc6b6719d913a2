"""GPU: qsx_select_like / qsx_select_codes_in_set and their run forms against tests/like_reference.py — exact bitmaps and
counts.  Sizes cover bitmap-word, tile and multi-workgroup edges of the kernels (csrc/like.hip: a LIKE tile holds
min(1024, 48 KiB / width rounded down to 64) rows, a membership tile 16384 / 8192 / 4096 rows of 1 / 2 / 4-byte codes)."""
import ctypes as C

import numpy as np
import pytest
import torch

import like_reference as R
from helpers import bitmap_dev, bitmap_np, to_dev
from quickstep_amd import types as T

pytestmark = pytest.mark.gpu

N_MAX = 20001
WIDTHS = (1, 3, 4, 8, 16, 25, 55, 64, 255)
# a and b are common (so that two-sided patterns match often enough), the rest are the bytes a matcher could get wrong:
# the two wildcards as text, regex metacharacters, a backslash, a newline, a byte >= 0x80
ALPHABET = np.frombuffer(b"ab%_\\.*[(\n\x80", dtype=np.uint8)
WEIGHTS = np.array([0.34, 0.34] + [0.32 / 9] * 9)


def like_tile_rows(width):
    return max(64, min(1024, (48 * 1024 // width) // 64 * 64))


def sizes_for(width):
    tile = like_tile_rows(width)
    return sorted({0, 1, 63, 64, 65, 1023, 1025, 4097, N_MAX, tile - 1, tile, tile + 1})


def make_stripe(width, n, seed):
    """n fields of CHAR(width): short terminated values with a random tail behind the NUL, and values of the full width."""
    rng = np.random.default_rng(seed)
    col = ALPHABET[rng.choice(ALPHABET.size, size=(n, width), p=WEIGHTS)]
    kind = rng.random(n)
    full = 0.85 if width <= 64 else 0.97     # (few of the 255-byte values: the checker walks them byte by byte)
    length = np.where(kind < 0.6, rng.integers(0, 7, size=n), np.where(kind < full, rng.integers(0, 13, size=n), width))
    length = np.minimum(length, width)
    rows = np.nonzero(length < width)[0]
    col[rows, length[rows]] = 0        # what lies behind stays random: it must never take part
    return np.ascontiguousarray(col)


def patterns_for(width):
    basic = [b"", b"%", b"%%", b"_", b"a", b"ab%", b"%ab", b"%ab%", b"a%b%a", b"%a_b%", b"_%_", b"a%a", b"ab%ba"]
    edge = [b"a" + b"%" * 62 + b"b",                 # 64 bytes, a run of '%' to collapse
            b"%a%b%a%b%a%b" + b"%" * 52,             # 64 bytes, six segments
            b"ab\0%zz"]                              # ends at its NUL: "ab"
    if width < 64:
        edge.append(b"_" * (width + 1))              # longer than the field: no value can match
    if width == 255:
        edge.append(b"%a%b" * 16)                    # 64 bytes, 32 segments
    return basic + edge


def trivial(pattern, width):
    """'all' / 'none' when the pattern's answer does not depend on the data, else None."""
    pattern = R.clean_pattern(pattern)
    if pattern and pattern.strip(b"%") == b"":
        return "all"
    if len(pattern.replace(b"%", b"")) > width:
        return "none"
    return None


_stripes = {}


def stripe(width, dev):
    """(host stripe, aligned device copy, copy at an odd address, filter bits, device filter), made once per width."""
    if width not in _stripes:
        col = make_stripe(width, N_MAX, seed=1000 + width)
        flat = torch.from_numpy(col.reshape(-1))
        aligned = flat.to(dev)
        buf = torch.zeros(flat.numel() + 17, dtype=torch.uint8, device=dev)
        buf[1:1 + flat.numel()] = aligned
        assert aligned.data_ptr() % 16 == 0 and buf[1:].data_ptr() % 16 == 1
        keep = np.random.default_rng(7 + width).random(N_MAX) < 0.7
        words = R.pack_bitmap(keep)
        words[-1] |= np.uint64(0xFFFF)       # set bits behind the last row: they must not come through
        _stripes[width] = (col, aligned, buf, keep, bitmap_dev(words, dev))
    return _stripes[width]


def check_all(pending):
    """pending: (what, bitmap tensor, count tensor or None, expected bits).  One copy back for all of them."""
    words = torch.cat([bitmap.reshape(-1) for _, bitmap, _, _ in pending]).cpu().numpy().view(np.uint64)
    counted = [count for _, _, count, _ in pending if count is not None]
    counts = torch.cat(counted).cpu().numpy() if counted else np.zeros(0, dtype=np.int64)
    at = at_count = 0
    for what, bitmap, count, bits in pending:
        want = R.pack_bitmap(bits)
        assert np.array_equal(words[at:at + want.size], want), what
        at += bitmap.numel()
        if count is not None:
            assert counts[at_count] == int(bits.sum()), what
            at_count += 1


@pytest.mark.parametrize("width", WIDTHS)
def test_select_like_matches_the_reference(capi, dev, width):
    col, aligned, buf, keep, filter_dev = stripe(width, dev)
    for pattern in patterns_for(width):
        ref = R.like_rows(col, pattern)
        kind = trivial(pattern, width)
        if kind is None:
            assert 0 < int(ref.sum()) < N_MAX, (width, pattern, int(ref.sum()))     # a test that matches nothing shows nothing
        else:
            assert int(ref.sum()) == (N_MAX if kind == "all" else 0), (width, pattern)
        pending = []
        for n in sizes_for(width):
            views = (aligned[:n * width].view(n, width), buf[1:1 + n * width].view(n, width))
            for negate in (False, True):
                bits = ref[:n] != negate
                # every case with and without a filter, with and without a count, at an aligned and at an odd address
                for view_at, with_filter, with_count in ((0, False, True), (0, True, False), (1, True, True), (1, False, False)):
                    bitmap, count = capi.select_like(views[view_at], pattern, negate, filter_dev if with_filter else None,
                                                     want_count=with_count)
                    pending.append(((width, pattern, n, negate, view_at, with_filter), bitmap, count,
                                    bits & keep[:n] if with_filter else bits))
        check_all(pending)


def test_not_like_leaves_the_tail_bits_zero(capi, dev):
    col = to_dev(make_stripe(25, 65, seed=5), dev)
    bitmap, count = capi.select_like(col, b"no such value", negate=True)
    words = bitmap_np(bitmap)
    assert int(count.item()) == 65
    assert words[0] == np.uint64(0xFFFFFFFFFFFFFFFF) and words[1] == np.uint64(1 << 63)


@pytest.mark.parametrize("width", (4, 25, 64))
def test_select_like_blocks_equals_the_per_block_calls(capi, dev, width):
    col, aligned, _, keep, _ = stripe(width, dev)
    rows = (0, 1, 64, 1000, 4097)
    cuts = np.concatenate([[0], np.cumsum(rows)])
    blocks = [to_dev(col[a:b].reshape(b - a, width), dev) for a, b in zip(cuts[:-1], cuts[1:])]
    filters = [None if i == 2 or b == a else bitmap_dev(R.pack_bitmap(keep[a:b]), dev) for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:]))]
    for pattern in (b"%ab%", b"a%b%a", b"ab%"):
        for negate in (False, True):
            for use_filters in (None, filters):
                outs, counts = capi.select_like_blocks(blocks, pattern, negate, filters=use_filters)
                counts = counts.cpu().numpy()
                for i, block in enumerate(blocks):
                    one, one_count = capi.select_like(block, pattern, negate, use_filters[i] if use_filters else None)
                    words = capi.bitmap_words(block.shape[0])
                    assert np.array_equal(bitmap_np(outs[i])[:words], bitmap_np(one)[:words]), (pattern, negate, i)
                    assert counts[i] == int(one_count.item()), (pattern, negate, i)
                    bits = R.like_rows(col[cuts[i]:cuts[i + 1]], pattern, negate)
                    if use_filters is not None and use_filters[i] is not None:
                        bits &= keep[cuts[i]:cuts[i + 1]]
                    assert counts[i] == int(bits.sum())


# ---- code membership ----------------------------------------------------------------------------------------------------------
CODE_DTYPES = {1: np.uint8, 2: np.uint16, 4: np.uint32}
TORCH_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32}


def codes_and_set(code_width, num_codes, n, seed):
    rng = np.random.default_rng(seed)
    top = min(num_codes + 3, 1 << (8 * code_width))            # codes >= num_codes appear where the width has room for them
    codes = rng.integers(0, top, size=n, dtype=np.uint64).astype(CODE_DTYPES[code_width])
    if n > 2 and num_codes < top:
        codes[1] = num_codes                                     # the reference's NULL code
    members = rng.random(num_codes) < 0.4
    return codes, members


def member_bits(codes, members):
    c = codes.astype(np.int64)
    return (c < members.size) & members[np.minimum(c, members.size - 1)]


def dev_codes(codes, dev, offset):
    """The stripe on the device, 16-byte aligned or one element further."""
    t = torch.from_numpy(codes.view({1: np.uint8, 2: np.int16, 4: np.int32}[codes.dtype.itemsize]))
    if not offset:
        return t.to(dev)
    buf = torch.zeros(t.numel() + 9, dtype=t.dtype, device=dev)
    buf[1:1 + t.numel()] = t.to(dev)
    assert buf[1:].data_ptr() % 16 != 0
    return buf[1:1 + t.numel()]


@pytest.mark.parametrize("code_width", (1, 2, 4))
def test_codes_in_set_matches_numpy(capi, dev, code_width):
    tile = 16384 // code_width
    sizes = sorted({0, 1, 63, 64, 65, 1023, 1025, tile - 1, tile, tile + 1, 2 * tile + 77})
    keep = np.random.default_rng(3).random(max(sizes)) < 0.7
    filter_dev = bitmap_dev(R.pack_bitmap(keep), dev)
    for num_codes in (1, 63, 64, 65, 256, 1000, 65536):
        codes, members = codes_and_set(code_width, num_codes, max(sizes), seed=num_codes)
        want_all = member_bits(codes, members)
        assert 0 < int(want_all.sum()) < codes.size or num_codes == 1
        set_dev = bitmap_dev(R.pack_bitmap(members), dev)
        stripes = (dev_codes(codes, dev, False), dev_codes(codes, dev, True))
        pending = []
        for n in sizes:
            for at, with_filter, with_count in ((0, False, True), (0, True, False), (1, True, True), (1, False, False)):
                bitmap, count = capi.select_codes_in_set(stripes[at][:n], set_dev, num_codes, filter_dev if with_filter else None,
                                                         want_count=with_count)
                pending.append(((code_width, num_codes, n, at, with_filter), bitmap, count,
                                want_all[:n] & keep[:n] if with_filter else want_all[:n]))
        check_all(pending)


def test_codes_in_set_with_a_set_larger_than_lds(capi, dev):
    num_codes, n = 2_000_000, 70001            # a 250 KB set: read through L2
    codes, members = codes_and_set(4, num_codes, n, seed=11)
    want = member_bits(codes, members)
    assert 0 < int(want.sum()) < n and int((codes >= num_codes).sum()) > 0
    bitmap, count = capi.select_codes_in_set(dev_codes(codes, dev, False), bitmap_dev(R.pack_bitmap(members), dev), num_codes)
    check_all([("large set", bitmap, count, want)])


@pytest.mark.parametrize("code_width", (1, 2, 4))
def test_codes_in_set_blocks_uses_each_blocks_own_set(capi, dev, code_width):
    tile = 16384 // code_width
    rows = (0, 1, 64, 1000, tile + 1, 2 * tile + 5)
    num_codes = (5, 1, 64, 200, 2_000_000 if code_width == 4 else 256, 77)
    blocks, sets, wants, filters = [], [], [], []
    for i, (n, k) in enumerate(zip(rows, num_codes)):
        codes, members = codes_and_set(code_width, k, n, seed=50 + i)
        keep = np.random.default_rng(90 + i).random(n) < 0.6
        blocks.append(dev_codes(codes, dev, False))
        sets.append(bitmap_dev(R.pack_bitmap(members), dev))
        filters.append(None if i == 3 or n == 0 else bitmap_dev(R.pack_bitmap(keep), dev))
        wants.append((member_bits(codes, members), keep))
    for use_filters in (None, filters):
        outs, counts = capi.select_codes_in_set_blocks(blocks, sets, num_codes, filters=use_filters)
        counts = counts.cpu().numpy()
        for i, (bits, keep) in enumerate(wants):
            if use_filters is not None and use_filters[i] is not None:
                bits = bits & keep
            want = R.pack_bitmap(bits)
            assert np.array_equal(bitmap_np(outs[i])[:want.size], want), (code_width, i)
            assert counts[i] == int(bits.sum()), (code_width, i)
            one, one_count = capi.select_codes_in_set(blocks[i], sets[i], num_codes[i], use_filters[i] if use_filters else None)
            assert np.array_equal(bitmap_np(one)[:want.size], want) and int(one_count.item()) == counts[i]


# ---- composition: LIKE over a dictionary-coded attribute -------------------------------------------------------------------------
def test_like_over_a_dictionary_then_membership_equals_like_over_the_values(capi, dev):
    rng = np.random.default_rng(21)
    words = [b"PROMO BRUSHED", b"PROMO PLATED", b"STANDARD BRASS", b"SMALL BRASS", b"ECONOMY ANODIZED", b"MEDIUM POLISHED TIN", b"", b"PROMO"]
    values = sorted(set(words))
    dictionary = np.zeros((len(values), 25), dtype=np.uint8)
    for i, v in enumerate(values):
        dictionary[i, :len(v)] = np.frombuffer(v, dtype=np.uint8)
        dictionary[i, len(v) + 1:] = rng.integers(1, 255, size=max(0, 25 - len(v) - 1))     # garbage behind the NUL
    n = 10007
    codes = rng.integers(0, len(values) + 1, size=n).astype(np.uint8)                        # len(values): the NULL code
    decoded = dictionary[np.minimum(codes, len(values) - 1)]
    is_null = codes == len(values)
    dict_dev, codes_dev, decoded_dev = to_dev(dictionary, dev), to_dev(codes, dev), to_dev(decoded, dev)
    for pattern in (b"PROMO%", b"%BRASS", b"%AN%", b"%O%I%", b"", b"%"):
        for negate in (False, True):
            code_set, _ = capi.select_like(dict_dev, pattern, negate)
            bitmap, count = capi.select_codes_in_set(codes_dev, code_set, len(values))
            direct, _ = capi.select_like(decoded_dev, pattern, negate)
            want = R.like_rows(decoded, pattern, negate, nulls=is_null)       # the NULL code is in no set, also for NOT LIKE
            got = R.unpack_bitmap(bitmap_np(bitmap), n)
            assert np.array_equal(got, want), (pattern, negate)
            assert int(count.item()) == int(want.sum())
            assert np.array_equal(R.unpack_bitmap(bitmap_np(direct), n) & ~is_null, want)
            if pattern not in (b"", b"%"):
                assert 0 < int(want.sum()) < n - int(is_null.sum())


# ---- argument checks ------------------------------------------------------------------------------------------------------------
def test_argument_checks(capi, dev):
    lib = capi.lib
    col = torch.zeros(8 * 4, dtype=torch.uint8, device=dev)
    out = torch.zeros(1, dtype=torch.int64, device=dev)
    codes = torch.zeros(8, dtype=torch.uint8, device=dev)
    p, o, c = col.data_ptr(), out.data_ptr(), codes.data_ptr()
    like = lib.qsx_select_like
    assert like(p, 4, 8, b"a%", 2, 0, None, o, None, None) == 0
    assert like(p, 0, 8, b"a%", 2, 0, None, o, None, None) == T.ERR_INVALID_ARGUMENT
    assert like(p, 256, 8, b"a%", 2, 0, None, o, None, None) == T.ERR_INVALID_ARGUMENT
    assert like(p, 4, -1, b"a%", 2, 0, None, o, None, None) == T.ERR_INVALID_ARGUMENT
    assert like(p, 4, 8, b"a%", -1, 0, None, o, None, None) == T.ERR_INVALID_ARGUMENT
    assert like(p, 4, 8, b"a%", 2, 2, None, o, None, None) == T.ERR_INVALID_ARGUMENT
    assert like(None, 4, 8, b"a%", 2, 0, None, o, None, None) == T.ERR_INVALID_ARGUMENT
    assert like(p, 4, 8, b"a%", 2, 0, None, None, None, None) == T.ERR_INVALID_ARGUMENT
    assert like(p, 4, 8, None, 2, 0, None, o, None, None) == T.ERR_INVALID_ARGUMENT
    assert like(None, 4, 0, b"", 0, 1, None, None, None, None) == 0                   # nothing to do is fine
    assert like(p, 4, 8, b"a" * 65, 65, 0, None, o, None, None) == T.ERR_UNSUPPORTED
    assert like(p, 4, 8, b"a" * 64, 64, 0, None, o, None, None) == 0
    rows = (C.c_int64 * 1)(8)
    one = lambda ptr: (C.c_void_p * 1)(ptr)
    blocks = lib.qsx_select_like_blocks
    assert blocks(4, 1, rows, one(p), b"a%", 2, 0, None, one(o), None, None) == 0
    assert blocks(4, 1, rows, one(p), b"a%", 2, 3, None, one(o), None, None) == T.ERR_INVALID_ARGUMENT
    assert blocks(4, 1, rows, one(None), b"a%", 2, 0, None, one(o), None, None) == T.ERR_INVALID_ARGUMENT
    assert blocks(4, 1, rows, one(p), b"a" * 65, 65, 0, None, one(o), None, None) == T.ERR_UNSUPPORTED
    assert blocks(300, 1, rows, one(p), b"a%", 2, 0, None, one(o), None, None) == T.ERR_INVALID_ARGUMENT
    in_set = lib.qsx_select_codes_in_set
    s = torch.zeros(1, dtype=torch.int64, device=dev).data_ptr()
    assert in_set(1, c, 8, s, 5, None, o, None, None) == 0
    assert in_set(3, c, 8, s, 5, None, o, None, None) == T.ERR_UNSUPPORTED
    assert in_set(1, None, 8, s, 5, None, o, None, None) == T.ERR_INVALID_ARGUMENT
    assert in_set(1, c, 8, None, 5, None, o, None, None) == T.ERR_INVALID_ARGUMENT
    assert in_set(1, c, 8, s, -1, None, o, None, None) == T.ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
