"""tests/partition_reference.py without a GPU: its numpy forms against Python-integer arithmetic and (mode 0) the oracle, and
every checker against mutants of a correct result — the ways a subtly wrong scatter kernel would be wrong: one count wrapped
modulo 256 (the histogram's packed bytes), two rows of a partition swapped, a row in the neighbouring partition, a column
gathered with the row ids of another tile, a piece start off by one, a write into a gap."""
import ctypes as C

import numpy as np
import pytest

import partition_reference as R

M64 = (1 << 64) - 1
CONST = 0x9E3779B97F4A7C15


def py_hash(k):
    k ^= k >> 32
    k = (k * CONST) & M64
    k ^= k >> 29
    return (k * CONST) & M64


def py_partition(mode, k, P, shift):
    if mode == 0:
        return k % P                                   # (a power of two: the same value as k & (P - 1))
    if mode == 1:
        return py_hash(k) >> (64 - (P.bit_length() - 1))
    if mode == 2:
        return (k >> shift) & 63
    return (py_hash(k) >> shift) & 63


def some_keys(dtype, rng):
    info = np.iinfo(dtype)
    edge = [0, 1, 2, 3, 7, 8, 31, 63, 64, -1, -2, -64, info.min, info.min + 1, info.max, info.max - 1]
    return np.concatenate([np.array(edge, dtype=dtype), rng.integers(-1000, 1000, size=150).astype(dtype),
                           rng.integers(info.min, info.max, size=150, dtype=dtype)])


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_numpy_forms_equal_python_integer_arithmetic(dtype):
    rng = np.random.default_rng(1)
    keys = some_keys(dtype, rng)
    bits = 8 * keys.itemsize
    image = R.key_image(keys)
    want_image = [int(k) & ((1 << bits) - 1) for k in keys]             # negative keys: the two's-complement pattern, zero-extended
    assert image.dtype == np.uint64 and image.tolist() == want_image
    assert R.hash64(image).tolist() == [py_hash(k) for k in want_image]
    for P in (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 32, 33, 63, 64):
        assert R.partition_ids(0, image, P).tolist() == [py_partition(0, k, P, 0) for k in want_image], P
    for P in (2, 4, 8, 16, 32, 64):
        assert R.partition_ids(1, image, P).tolist() == [py_partition(1, k, P, 0) for k in want_image], P
    for shift in (0, 6, 30, 52, 54, 58, 60):
        assert R.partition_ids(2, image, 64, shift).tolist() == [py_partition(2, k, 64, shift) for k in want_image], shift
        if shift <= 58:
            for mode in (3, 4):
                assert R.partition_ids(mode, image, 64, shift).tolist() == [py_partition(mode, k, 64, shift) for k in want_image]
    assert R.hash_bits12(image, 58).tolist() == [py_hash(k) >> 52 for k in want_image]
    assert R.hash_bits12(image, 58).tolist() == (R.partition_ids(3, image, 64, 58) * 64 + R.partition_ids(4, image, 64, 52)).tolist()


def test_packed_image_equals_python_integer_arithmetic():
    rng = np.random.default_rng(2)
    n = 300
    cols = [rng.integers(0, 256, size=n).astype(np.uint8), rng.integers(-2**15, 2**15, size=n).astype(np.int16),
            rng.integers(-2**31, 2**31, size=n).astype(np.int32)]
    shifts = [0, 8, 24]
    want = [(int(a) & 0xFF) | ((int(b) & 0xFFFF) << 8) | ((int(c) & 0xFFFFFFFF) << 24) for a, b, c in zip(*cols)]
    assert R.packed_image(cols, shifts).tolist() == want
    wide = rng.integers(-2**63, 2**63, size=n).astype(np.int64)
    assert R.packed_image([wide], [0]).tolist() == [int(v) & M64 for v in wide]


def test_offsets_and_pieces():
    pid = np.array([3, 0, 0, 3, 3, 1] + [4] * 17 + [5] * 16, dtype=np.int64)
    assert R.offsets_of(pid, 7).tolist() == [0, 2, 3, 3, 6, 23, 39, 39]
    assert R.pieces_of(pid, 7, 16).tolist() == [0, 16, 32, 32, 48, 80, 96] + [2, 1, 0, 3, 17, 16, 0]


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
@pytest.mark.parametrize("P", [1, 2, 3, 8, 17, 41, 64])
def test_mode_0_equals_the_oracle(oracle, dtype, P):
    rng = np.random.default_rng(P)
    keys = np.concatenate([some_keys(dtype, rng), rng.integers(-1000, 1_000_000, size=5000).astype(dtype)])
    pid = R.partition_ids(0, R.key_image(keys), P)
    assert np.array_equal(R.offsets_of(pid, P), oracle.partition_offsets(keys, P))
    rows = np.arange(keys.size, dtype=np.int64)
    assert np.array_equal(np.argsort(pid, kind="stable"), oracle.partition_scatter(keys, P, rows))


# ---- mutants ---------------------------------------------------------------------------------------------------------------
TILE = 2048


def correct_result(P, n=3 * TILE + 77, seed=5, stable=True):
    """A partitioning of n rows as the kernel leaves it: (pid, cols, outs, offsets); cols[0] the row ids."""
    rng = np.random.default_rng(seed)
    pid = rng.integers(0, P, size=n)
    pid[rng.integers(0, n, size=n // 3)] = P // 2                     # one partition of more than 256 rows
    cols = [np.arange(n, dtype=np.int32), rng.integers(-2**62, 2**62, size=n), rng.integers(0, 255, size=n).astype(np.uint8)]
    order = np.argsort(pid, kind="stable")
    offsets = R.offsets_of(pid, P)
    if not stable:                                                    # any order inside a partition is a correct result
        for p in range(P):
            order[offsets[p]:offsets[p + 1]] = rng.permutation(order[offsets[p]:offsets[p + 1]])
    return pid, cols, [c[order] for c in cols], offsets


def rejected(check, *args, **kwargs):
    try:
        check(*args, **kwargs)
    except AssertionError:
        return True
    return False


def swap_rows(outs, i, j):
    outs = [o.copy() for o in outs]
    for o in outs:
        o[[i, j]] = o[[j, i]]
    return outs


def count_wrapped(offsets, P):
    counts = np.diff(offsets)
    p = int(np.argmax(counts))
    assert counts[p] >= 256
    counts = counts.copy()
    counts[p] %= 256
    return np.concatenate([[0], np.cumsum(counts)])


def other_tile_column(cols, outs, c):
    """Column c of the second tile's output rows gathered with the row ids of the first tile's."""
    ids = outs[0].astype(np.int64)
    out = outs[c].copy()
    out[TILE:2 * TILE] = cols[c][ids[:TILE]]
    assert not np.array_equal(out, outs[c])
    return [out if k == c else o for k, o in enumerate(outs)]


@pytest.mark.parametrize("P", [2, 8, 17, 64])
def test_check_stable_rejects_every_mutant(P):
    pid, cols, outs, offsets = correct_result(P)
    R.check_stable(pid, P, cols, outs, offsets)
    assert rejected(R.check_stable, pid, P, cols, outs, count_wrapped(offsets, P))
    a = int(offsets[P // 2])                                          # two rows of one partition
    assert rejected(R.check_stable, pid, P, cols, swap_rows(outs, a, a + 1), offsets)
    assert rejected(R.check_stable, pid, P, cols, swap_rows(outs, a, int(offsets[P // 2 + 1]) - 1), offsets)
    b = int(offsets[1])                                               # the last row of partition 0 and the first of partition 1
    assert rejected(R.check_stable, pid, P, cols, swap_rows(outs, b - 1, b), offsets)
    for c in (1, 2):
        assert rejected(R.check_stable, pid, P, cols, other_tile_column(cols, outs, c), offsets)
    lost = [o.copy() for o in outs]                                   # a row written twice, another lost
    for o in lost:
        o[a] = o[a + 1]
    assert rejected(R.check_stable, pid, P, cols, lost, offsets)
    beyond = [o.copy() for o in outs]
    beyond[0][5] = pid.size
    assert rejected(R.check_stable, pid, P, cols, beyond, offsets)


@pytest.mark.parametrize("P", [16, 64])
def test_check_partitioned_rejects_every_mutant(P):
    pid, cols, outs, offsets = correct_result(P, stable=False)
    R.check_partitioned(pid, P, cols, outs, offsets)
    R.check_partitioned(pid, P, cols, correct_result(P)[2], offsets)  # (the stable order is one of the correct ones)
    assert rejected(R.check_stable, pid, P, cols, outs, offsets)      # (and this one is not the stable order)
    assert rejected(R.check_partitioned, pid, P, cols, outs, count_wrapped(offsets, P))
    a = int(offsets[P // 2])
    R.check_partitioned(pid, P, cols, swap_rows(outs, a, a + 1), offsets)   # whole rows swapped inside a partition: still correct
    half = [o.copy() for o in outs]                                   # ... the row ids alone: the columns no longer follow
    half[0][[a, a + 1]] = half[0][[a + 1, a]]
    assert rejected(R.check_partitioned, pid, P, cols, half, offsets)
    b = int(offsets[1])
    assert rejected(R.check_partitioned, pid, P, cols, swap_rows(outs, b - 1, b), offsets)
    for c in (1, 2):
        assert rejected(R.check_partitioned, pid, P, cols, other_tile_column(cols, outs, c), offsets)
    lost = [o.copy() for o in outs]
    for o in lost:
        o[a] = o[a + 1]
    assert rejected(R.check_partitioned, pid, P, cols, lost, offsets)


def second_digit_result(n=3 * TILE + 77, seed=9):
    """The input of the second pass (ordered by the hash digit at 52 only) and a correct output of the pass at 58."""
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, 3000, size=n).astype(np.int32)             # ~3000 groups: most 12-bit values hold several rows
    keys[rng.integers(0, n, size=n // 3)] = 7                         # one partition of more than 256 rows
    keys = keys[np.argsort(R.partition_ids(4, R.key_image(keys), 64, 52), kind="stable")]
    image = R.key_image(keys)
    cols = [np.arange(n, dtype=np.int64), keys, rng.integers(0, 65535, size=n).astype(np.uint16)]
    order = np.argsort(R.partition_ids(3, image, 64, 58), kind="stable")
    return image, cols, [c[order] for c in cols], R.offsets_of(R.partition_ids(3, image, 64, 58), 64)


def test_check_second_digit_rejects_every_mutant():
    image, cols, outs, offsets = second_digit_result()
    R.check_second_digit(image, 58, cols, outs, offsets)
    v12 = R.hash_bits12(image, 58)[outs[0]]
    assert rejected(R.check_second_digit, image, 58, cols, outs, count_wrapped(offsets, 64))
    same = int(np.flatnonzero((v12[1:] == v12[:-1]) & (outs[1][1:] != outs[1][:-1]))[0])     # two rows of one 12-bit value
    R.check_second_digit(image, 58, cols, swap_rows(outs, same, same + 1), offsets)           # no order is asked inside it
    inside = np.flatnonzero((v12[1:] != v12[:-1]) & (v12[1:] >> 6 == v12[:-1] >> 6))          # two rows of one partition, two values
    assert rejected(R.check_second_digit, image, 58, cols, swap_rows(outs, int(inside[0]), int(inside[0]) + 1), offsets)
    b = int(offsets[np.flatnonzero(np.diff(offsets) > 0)[1]])         # across the border of two partitions
    assert rejected(R.check_second_digit, image, 58, cols, swap_rows(outs, b - 1, b), offsets)
    for c in (1, 2):
        assert rejected(R.check_second_digit, image, 58, cols, other_tile_column(cols, outs, c), offsets)
    shuffled = np.random.default_rng(3).permutation(image.size)       # an input that the first pass did not order
    assert rejected(R.check_second_digit, image[shuffled], 58, cols, outs, offsets)


@pytest.mark.parametrize("P,stable", [(2, True), (16, False), (64, False)])
def test_check_pieces_rejects_every_mutant(P, stable):
    align = 16
    pid, cols, packed, offsets = correct_result(P, stable=stable)
    sentinels = [-1, -7, 0xA5]
    pieces = R.pieces_of(pid, P, align)

    def laid_out(starts):
        outs = [np.full(pid.size + align * P, s, dtype=c.dtype) for c, s in zip(cols, sentinels)]
        for p in range(P):
            for o, src in zip(outs, packed):
                o[starts[p]:starts[p] + pieces[P + p]] = src[offsets[p]:offsets[p + 1]]
        return outs
    outs = laid_out(pieces[:P])
    R.check_pieces(pid, P, align, cols, outs, pieces, sentinels, stable)
    off_by_one = pieces.copy()
    off_by_one[P - 1] += 1
    assert rejected(R.check_pieces, pid, P, align, cols, outs, off_by_one, sentinels, stable)          # reported one row late
    moved = pieces[:P].copy()
    moved[P - 1] += 1
    assert rejected(R.check_pieces, pid, P, align, cols, laid_out(moved), pieces, sentinels, stable)  # written one row late
    unaligned = np.concatenate([offsets[:P], pieces[P:]])
    assert rejected(R.check_pieces, pid, P, align, cols, outs, unaligned, sentinels, stable)
    wrapped = pieces.copy()
    wrapped[P + P // 2] %= 256
    assert rejected(R.check_pieces, pid, P, align, cols, outs, wrapped, sentinels, stable)
    gap = int(np.flatnonzero(outs[0] == -1)[0])
    for c in range(3):
        holed = [o.copy() for o in outs]
        holed[c][gap] = 1
        assert rejected(R.check_pieces, pid, P, align, cols, holed, pieces, sentinels, stable)
    a = int(pieces[P // 2])
    if stable:
        assert rejected(R.check_pieces, pid, P, align, cols, swap_rows(outs, a, a + 1), pieces, sentinels, stable)
    else:
        R.check_pieces(pid, P, align, cols, swap_rows(outs, a, a + 1), pieces, sentinels, stable)
    last_of_first = int(pieces[0] + pieces[P] - 1)
    assert rejected(R.check_pieces, pid, P, align, cols, swap_rows(outs, last_of_first, int(pieces[1])), pieces, sentinels, stable)
    assert rejected(R.check_pieces, pid, P, align, cols, other_tile_column(cols, outs, 1), pieces, sentinels, stable)


def test_the_hook_is_exported_and_asks_for_a_device(capi):
    """qsx_debug_partition_scatter: in the library, not in the ABI table, and without a device QSX_ERR_NO_DEVICE before anything else."""
    from quickstep_amd import types as T
    fn = capi.lib.qsx_debug_partition_scatter
    assert "qsx_debug_partition_scatter" not in capi.EXPORTED
    keys = (C.c_void_p * 1)()
    if capi.device_count() > 0:       # (with a device: a form that does not exist is turned down before anything is launched)
        assert fn(6, T.INT, 1, keys, None, None, None, 10, 8, 0, 0, 0, 0, None, None, None, None, None) == T.ERR_INVALID_ARGUMENT
        return
    for form in range(6):
        assert fn(form, T.INT, 1, keys, None, None, None, 10, 8, 0, 0, 0, 0, None, None, None, None, None) == T.ERR_NO_DEVICE
