"""GPU: qsx_sort_permutation_keys / qsx_sort_top_k_keys (ORDER BY with NULLS FIRST / LAST and CHAR(n) keys) against the checker
of tests/sort_keys_reference.py — a restatement of StorageBlock::sort / sortColumn.  Every comparison is of the permutation
itself: the sort is stable, so there is exactly one right answer."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import sort_keys_reference as R
from helpers import to_dev
from quickstep_amd import types as T

pytestmark = pytest.mark.gpu


def spec_of(capi, dev, key, rng=None):
    """A checker key on the device.  With `rng`, the bytes under the NULLs are overwritten with garbage first: they must not matter."""
    values = key.values
    if rng is not None and key.nulls is not None and key.nulls.any():
        values = values.copy()
        flat = values.view(np.uint8).reshape(key.rows, -1)
        flat[key.nulls] = rng.integers(0, 256, size=(int(key.nulls.sum()), flat.shape[1]), dtype=np.uint8)
    bitmap = None if key.nulls is None else to_dev(R.pack_bitmap(key.nulls), dev)
    return capi.SortKeySpec(to_dev(values.reshape(-1), dev), key.type, key.width, key.descending, key.nulls_first, bitmap)


def gpu_permutation(capi, dev, keys, rng=None):
    return capi.sort_permutation_keys([spec_of(capi, dev, k, rng) for k in keys]).cpu().numpy()


def check(capi, dev, keys, what, rng=None):
    got = gpu_permutation(capi, dev, keys, rng)
    want = R.permutation_numpy(keys)
    assert np.array_equal(got, want), what
    if keys[0].rows <= 65:
        assert np.array_equal(got, R.permutation_plain(keys)), what


def dates(rng, n, years=(1992, 1999)):
    raw = (rng.integers(years[0], years[1], size=n).astype(np.int64) & 0xFFFFFFFF) | (rng.integers(1, 13, size=n).astype(np.int64) << 32) | \
        (rng.integers(1, 29, size=n).astype(np.int64) << 40) | (rng.integers(0, 65536, size=n).astype(np.int64) << 48)   # (padding bytes: ignored)
    return raw


def column(rng, kind, n):
    if kind == "int":
        return rng.integers(-50, 50, size=n).astype(np.int32), T.INT
    if kind == "long":
        return rng.integers(-2**62, 2**62, size=n).astype(np.int64), T.LONG
    if kind == "float":
        return np.where(rng.random(n) < 0.1, rng.choice(np.array([0.0, -0.0], dtype=np.float32), size=n), (rng.normal(size=n) * 1e3).astype(np.float32)), T.FLOAT
    if kind == "double":
        return np.round(rng.normal(size=n), 2) + 0.0, T.DOUBLE
    if kind == "date":
        return dates(rng, n), T.DATE
    return R.random_chars(rng, n, int(kind.split()[1]), distinct=max(2, n // 3)), T.CHAR


SINGLE_KINDS = ["int", "long", "float", "double", "date", "char 10"]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 2048, 2049, 100_003])
@pytest.mark.parametrize("kind", SINGLE_KINDS)
def test_single_keys_every_type_direction_and_null_ordering(capi, dev, kind, n):
    """n = 64 / 65 and 2048 / 2049 sit on the bitmap-word and LDS-sort boundaries."""
    rng = np.random.default_rng(n * 31 + len(kind))
    for fraction, desc, first in itertools.product((0.0, 0.3, 1.0), (False, True), (False, True)):
        values, qt = column(rng, kind, n)
        nulls = None if fraction == 0.0 else (np.ones(n, dtype=bool) if fraction == 1.0 else rng.random(n) < fraction)
        check(capi, dev, [R.Key(values, qt, desc, first, nulls)], (kind, n, fraction, desc, first), rng)


@pytest.mark.parametrize("width", [1, 2, 7, 8, 9, 10, 15, 16, 25, 64])
def test_char_keys_of_every_width(capi, dev, width):
    rng = np.random.default_rng(width)
    n = 20_011
    cases = {
        "every length, garbage behind the first NUL, bytes >= 0x80": R.random_chars(rng, n, width),
        "5 distinct values": R.random_chars(rng, n, width, distinct=5),
        "ascii": R.random_chars(rng, n, width, alphabet=np.arange(32, 127, dtype=np.uint8), distinct=n // 4),
    }
    last = np.tile(rng.integers(1, 256, size=width, dtype=np.uint8), (n, 1))     # values that differ only in their last byte
    last[:, width - 1] = rng.integers(0, 256, size=n)
    cases["differ in the last byte only"] = last
    high = np.tile(rng.integers(1, 256, size=width, dtype=np.uint8), (n, 1))     # 0x7F against 0x80 against 0xFF: unsigned chars
    high[:, 0] = rng.choice(np.array([0x01, 0x7F, 0x80, 0xFF], dtype=np.uint8), size=n)
    cases["first byte around 0x80"] = high
    for name, values in cases.items():
        for desc, first, with_nulls in itertools.product((False, True), (False, True), (False, True)):
            nulls = rng.random(n) < 0.2 if with_nulls else None
            check(capi, dev, [R.Key(values, T.CHAR, desc, first, nulls)], (width, name, desc, first, with_nulls), rng)
    small = R.random_chars(rng, 300, width, distinct=40)                           # the one-workgroup path
    check(capi, dev, [R.Key(small, T.CHAR, True, True, rng.random(300) < 0.3)], (width, "small"), rng)


def test_composite_keys_mixed_types_directions_and_null_orderings(capi, dev):
    rng = np.random.default_rng(21)
    for n in (1500, 250_000):
        a = rng.integers(0, 7, size=n).astype(np.int32)
        b = np.round(rng.normal(size=n), 1) + 0.0
        c = rng.integers(-3, 3, size=n).astype(np.int64)
        d = rng.choice(np.array([0.0, -0.0, 1.5, -1.5], dtype=np.float32), size=n)
        e = R.random_chars(rng, n, 10, alphabet=np.arange(65, 70, dtype=np.uint8), distinct=50)
        f = dates(rng, n, years=(1995, 1997))
        m = lambda p: rng.random(n) < p  # noqa: E731
        cases = [
            # the reference's 3Column_MixedNullOrdering_MixedOrdering shape: ASC NULLS FIRST, DESC NULLS LAST, ASC NULLS LAST
            [R.Key(a, T.INT, False, True, a == 0), R.Key(c, T.LONG, True, False, c == 0), R.Key(d, T.FLOAT, False, False, m(0.3))],
            [R.Key(e, T.CHAR, True, False, m(0.2)), R.Key(a, T.INT, False, True, m(0.5)), R.Key(b, T.DOUBLE, True, True, None)],
            [R.Key(d, T.FLOAT, False, True, m(0.1)), R.Key(f, T.DATE, True, True, m(0.4)), R.Key(e, T.CHAR, False, False, None),
             R.Key(b, T.DOUBLE, False, False, m(0.9))],
            [R.Key(c, T.LONG, False, False, m(1.1)), R.Key(a, T.INT, True, False, None), R.Key(e, T.CHAR, False, True, m(0.3)),
             R.Key(f, T.DATE, False, False, None)],
        ]
        for i, keys in enumerate(cases):
            check(capi, dev, keys, (n, i), rng)


def test_digits_and_words_that_do_not_vary(capi, dev):
    rng = np.random.default_rng(8)
    for n in (1000, 70_000):
        second = R.Key(rng.integers(0, 3, size=n).astype(np.int32), T.INT, True)
        padded = np.zeros((n, 25), dtype=np.uint8)                                   # CHAR(25) whose last two words are all padding
        padded[:, :9] = rng.integers(65, 91, size=(n, 9))
        cases = {
            "all equal": np.full(n, 1234567, dtype=np.int32),
            "varies in one bit": np.where(rng.random(n) < 0.5, 1 << 20, 0).astype(np.int64) + 5,
            "varies in the sign bit": rng.choice(np.array([-2.5, 2.5]), size=n),
            "ints below 64": rng.integers(0, 64, size=n).astype(np.int32),
            "char 25, padded": padded,
            "char 25, all equal": np.tile(np.frombuffer(b"Supplier#000000001\0\0\0\0\0\0\0", dtype=np.uint8), (n, 1)),
        }
        for name, values in cases.items():
            for desc, first, fraction in itertools.product((False, True), (False, True), (0.0, 0.3)):
                nulls = rng.random(n) < fraction if fraction else None
                check(capi, dev, [R.Key(values, None, desc, first, nulls), second], (n, name, desc, first, fraction), rng)
        for first in (False, True):
            check(capi, dev, [R.Key(cases["ints below 64"], None, False, first, np.ones(n, dtype=bool)), second], (n, "all NULL", first), rng)
            check(capi, dev, [R.Key(cases["ints below 64"], None, True, first, np.zeros(n, dtype=bool)), second], (n, "bitmap without NULLs", first))


def test_null_free_plain_keys_equal_the_old_entry_points(capi, dev):
    rng = np.random.default_rng(13)
    n = 250_000
    cols = [(rng.integers(-50, 50, size=n).astype(np.int32), T.INT), (rng.integers(-2**62, 2**62, size=n).astype(np.int64), T.LONG),
            ((rng.normal(size=n) * 1e3).astype(np.float32), T.FLOAT), (np.round(rng.normal(size=n), 2), T.DOUBLE),
            (dates(rng, n), T.DATE), (rng.choice(np.frombuffer(b"ANRF\0\xff", dtype=np.uint8), size=n), T.CHAR)]
    dev_cols = [to_dev(c, dev) for c, _ in cols]
    for picks, desc in (((0,), (False,)), ((1,), (True,)), ((2,), (True,)), ((3,), (False,)), ((4,), (True,)), ((5,), (False,)), ((5,), (True,)),
                        ((3, 4), (True, False)), ((5, 0, 2), (True, False, True)), ((0, 5, 4, 1), (False, True, False, True))):
        old = capi.sort_permutation([dev_cols[i] for i in picks], list(desc), types=[cols[i][1] for i in picks])
        new = capi.sort_permutation_keys([capi.SortKeySpec(dev_cols[i], cols[i][1], 1 if cols[i][1] == T.CHAR else 0, d) for i, d in zip(picks, desc)])
        assert torch.equal(old, new), (picks, desc)
        old_top = capi.sort_top_k([dev_cols[i] for i in picks], 100, list(desc), types=[cols[i][1] for i in picks])
        new_top = capi.sort_top_k_keys([(dev_cols[i], cols[i][1], 1 if cols[i][1] == T.CHAR else 0, d, False, None) for i, d in zip(picks, desc)], 100)
        assert torch.equal(old_top, new_top) and torch.equal(new_top, new[:100]), (picks, desc)


@pytest.mark.parametrize("n,k", [(10, 3), (10, 50), (70_000, 10), (1_500_000, 10), (1_500_000, 20_000), (300_000, 0)])
def test_top_k_is_the_head_of_the_full_sort(capi, dev, n, k):
    rng = np.random.default_rng(n + k)
    second = R.Key(R.random_chars(rng, n, 10, alphabet=np.arange(65, 91, dtype=np.uint8), distinct=1000), T.CHAR, False, True, rng.random(n) < 0.1)
    revenue = np.round(rng.uniform(1000, 500000, size=n), 4)
    many_nulls = rng.random(n) < 0.5 if n > 10 else np.arange(n) % 2 == 0         # more NULLs than k
    cases = {
        "plain key 0 (selection)": R.Key(revenue, T.DOUBLE, True),
        "plain int key 0 (selection, ties)": R.Key(rng.integers(0, 1000, size=n).astype(np.int32), T.INT, False),
        "nullable key 0, NULLS FIRST, more NULLs than k": R.Key(revenue, T.DOUBLE, True, True, many_nulls),
        "nullable key 0, NULLS LAST": R.Key(revenue, T.DOUBLE, False, False, rng.random(n) < 0.3),
        "char(10) key 0": R.Key(R.random_chars(rng, n, 10, distinct=max(2, n // 7)), T.CHAR, True),
    }
    for name, key0 in cases.items():
        keys = [key0, second]
        specs = [spec_of(capi, dev, key, rng) for key in keys]
        got = capi.sort_top_k_keys(specs, k).cpu().numpy()
        full = capi.sort_permutation_keys(specs).cpu().numpy()
        want = R.permutation_numpy(keys)
        assert got.size == min(k, n)
        assert np.array_equal(got, want[:k]), name
        assert np.array_equal(full, want), name


def test_q13_shaped_order_by(capi, dev):
    """ORDER BY custdist DESC, c_count DESC over groups whose aggregate is NULL when the group saw no non-NULL argument
    (the existence-map path): a nullable LONG DESC NULLS LAST, then an INT DESC, 1.2 M rows."""
    rng = np.random.default_rng(13)
    n = 1_200_000
    custdist = rng.integers(0, 5000, size=n).astype(np.int64)
    nulls = rng.random(n) < 0.33
    c_count = rng.integers(0, 42, size=n).astype(np.int32)
    check(capi, dev, [R.Key(custdist, T.LONG, True, False, nulls), R.Key(c_count, T.INT, True)], "q13", rng)


def test_refused_arguments(capi, dev):
    n = 100
    col = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
    out = torch.zeros(n, dtype=torch.int32, device=dev)
    ws_bytes = capi.lib.qsx_sort_workspace_bytes(n)
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def both(nkeys, keys, rows=n):
        arr = (T.SortKey * max(len(keys), 1))(*keys)
        a = capi.lib.qsx_sort_permutation_keys(nkeys, arr, rows, out.data_ptr(), ws.data_ptr(), ws_bytes, stream)
        b = capi.lib.qsx_sort_top_k_keys(nkeys, arr, rows, 5, out.data_ptr(), ws.data_ptr(), ws_bytes, stream)
        assert a == b
        return a
    key = lambda qt, width, ptr=col.data_ptr(): T.SortKey(ptr, None, qt, width, 0, 0)  # noqa: E731
    assert both(1, [key(T.INT, 0)]) == T.OK and both(1, [key(T.INT, 4)]) == T.OK and both(1, [key(T.CHAR, 64)]) == T.OK
    for width in (0, -1, 65, 1000):
        assert both(1, [key(T.CHAR, width)]) == T.ERR_UNSUPPORTED, width
    for qt in (-1, 5, 7, 99):                                                    # (5: no type of the list)
        assert both(1, [key(qt, 0)]) == T.ERR_UNSUPPORTED, qt
    assert both(1, [key(T.INT, 0, None)]) == T.ERR_INVALID_ARGUMENT              # a NULL column with n > 0 ...
    assert both(1, [key(T.INT, 0, None)], rows=0) == T.OK                        # ... is fine without rows
    assert both(0, [key(T.INT, 0)]) == T.ERR_INVALID_ARGUMENT
    assert both(T.MAX_KEYS + 1, [key(T.INT, 0)] * (T.MAX_KEYS + 1)) == T.ERR_INVALID_ARGUMENT
    assert both(T.MAX_KEYS, [key(T.INT, 0)] * T.MAX_KEYS) == T.OK
    assert both(1, [key(T.LONG, 4)]) == T.ERR_INVALID_ARGUMENT                   # neither 0 nor the natural width
    torch.cuda.synchronize()
