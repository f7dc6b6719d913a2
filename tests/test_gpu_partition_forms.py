"""GPU: every form of the K9 partition scatter (quickstep_amd/csrc/partition.hip) against tests/partition_reference.py.

The forms no entry point of their own reaches — the packed-key partitioning of the mid-size aggregation (mode 1, aligned pieces),
the radix digit of the sorts (mode 2), the two hash digits of the two-level aggregation (modes 4 and 3) — and the public forms
(mode 0, a stripe or a run of blocks) go through qsx_debug_partition_scatter, once with the library's chunking (one 2048-row tile
per workgroup at these sizes) and once with the number of chunks capped, so that a workgroup walks several tiles: 10 241 rows
under a cap of 4 are chunks of 4096, 4096 and 2049 rows and a fourth that lies wholly behind the stripe; 300 000 rows under a
cap of 1 are one chunk of 147 tiles.  Every result goes through the reference's checkers (exact: offsets, row order or row
sets, every column), never through the oracle.  Outputs are prefilled and 64 rows longer than asked: a write behind the end shows.
"""
import numpy as np
import pytest
import torch

import partition_reference as R
from helpers import to_dev

pytestmark = pytest.mark.gpu

NS = (1, 63, 64, 65, 2047, 2048, 2049, 10_241, 300_000)
PAD = 64
SHAPES = ("all_first", "all_last", "one_each", "alternating", "sorted", "stranger_0", "stranger_63", "stranger_31")
SIGNED = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}


def caps_for(n):
    return (0, 1, 3, 4) if n == 10_241 else (0, 1, 3)


def sentinel_of(dtype):
    return 255 if np.dtype(dtype) == np.uint8 else -1


def random_column(width, n, rng):
    info = np.iinfo(SIGNED[width])
    return rng.integers(info.min, info.max, size=n, dtype=SIGNED[width], endpoint=True)


def payload(n, rng, widths=(8, 1)):
    """[row ids (int32), one random column per width]"""
    return [np.arange(n, dtype=np.int32)] + [random_column(w, n, rng) for w in widths]


def run(capi, dev, form, dkeys, dcols, num_partitions, cap, rows_out=None, **kw):
    """One call of the hook; returns (host outputs without their guard rows, host offsets)."""
    first = dcols[0] if form == 5 else dcols
    n = sum(k.numel() for k in dkeys) if form == 5 else dkeys[0].numel()
    rows_out = n if rows_out is None else rows_out
    outs = [torch.full((rows_out + PAD,), 255 if c.dtype == torch.uint8 else -1, dtype=c.dtype, device=dev) for c in first]
    outs, offs = capi.debug_partition_scatter(form, dkeys, dcols, num_partitions, max_chunks=cap, out_cols=outs, **kw)
    host = [o.cpu().numpy() for o in outs]
    for c, o in enumerate(host):
        assert np.all(o[rows_out:] == sentinel_of(o.dtype)), f"column {c}: a write behind the output's last row"
    return [o[:rows_out] for o in host], offs.cpu().numpy()


# ---- keys of a wanted shape ------------------------------------------------------------------------------------------------
def shaped(shape, P, n, rng):
    """The partition wanted for every row."""
    i = np.arange(n)
    if shape == "uniform":
        return rng.integers(0, P, size=n)
    if shape == "all_first":
        return np.zeros(n, dtype=np.int64)
    if shape == "all_last":
        return np.full(n, P - 1)
    if shape == "one_each":                     # one row in every other partition, the rest in one
        want = np.full(n, P // 2)
        others = np.array([p for p in range(P) if p != P // 2][:max(n - 1, 0)], dtype=np.int64)
        want[rng.choice(n, size=others.size, replace=False)] = others
        return want
    if shape == "alternating":
        return np.where(i % 2 == 0, 0, P - 1)
    if shape == "sorted":                       # whole waves in one partition, a partition's run as long as a tile for few partitions
        return np.sort(rng.integers(0, P, size=n))
    lane = int(shape.split("_")[1])             # waves of 63 equal partitions and one stranger
    wave = i // 64
    return np.where(i % 64 == lane, (wave + 1) % P, wave % P)


def pick(pool_pid, P, want, rng):
    """For every row a row of the pool whose partition is want[row]; the pool has to hold every partition asked for."""
    counts = np.bincount(pool_pid, minlength=P)
    missing = [int(p) for p in np.unique(want) if counts[p] == 0]
    assert not missing, f"the pool holds no key of partitions {missing}"
    order = np.argsort(pool_pid, kind="stable")
    starts = np.cumsum(counts) - counts
    return order[starts[want] + rng.integers(0, 1 << 62, size=want.size) % counts[want]]


LAYOUTS = [(1,), (2,), (4,), (8,), (1, 1), (2, 4), (4, 4), (1, 2, 4), (1, 1, 2, 4)]


def shifts_of(layout):
    """Bit offsets as the aggregation lays a key of up to 8 bytes out: the components side by side from bit 0."""
    return [8 * sum(layout[:k]) for k in range(len(layout))]


def packed_pool(layout, size, rng):
    cols = [random_column(w, size, rng) for w in layout]
    return cols, R.packed_image(cols, shifts_of(layout))


# ---- mode 0 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 32, 33, 63, 64])
def test_mode_0_every_partition_count_row_count_and_chunk_shape(capi, dev, dtype, P):
    """P = 4, 16, 32 (the other values of `bits` in step_ranks) and every other count, at every row count and chunk shape:
    uniform keys, negative ones and keys < P among them."""
    for n in NS:
        rng = np.random.default_rng(100 * n + P)
        keys = rng.integers(-1000, 1_000_000, size=n).astype(dtype)
        keys[::5] = rng.integers(0, P, size=keys[::5].size)
        cols = payload(n, rng) + [keys]
        pid = R.partition_ids(0, R.key_image(keys), P)
        dkeys, dcols = [to_dev(keys, dev)], [to_dev(c, dev) for c in cols]
        for cap in caps_for(n):
            outs, offs = run(capi, dev, 0, dkeys, dcols, P, cap)
            R.check_stable(pid, P, cols, outs, offs)


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
@pytest.mark.parametrize("P", [2, 5, 8, 16, 33, 64])
def test_mode_0_skewed_tiles(capi, dev, dtype, P):
    """All rows of a tile in one partition (empty partitions at either end, a run that fills the staging tile), one row in every
    other partition, two alternating partitions, sorted keys, waves with one stranger at lane 0 / 63 / 31."""
    rng = np.random.default_rng(P)
    pool = np.concatenate([np.arange(P), rng.integers(-1000, 1 << 30, size=20_000)]).astype(dtype)
    pool_pid = R.partition_ids(0, R.key_image(pool), P)
    for shape in SHAPES:
        for n in (65, 2048, 10_241):
            want = shaped(shape, P, n, rng)
            keys = pool[pick(pool_pid, P, want, rng)]
            pid = R.partition_ids(0, R.key_image(keys), P)
            assert np.array_equal(pid, want)
            cols = payload(n, rng)
            dkeys, dcols = [to_dev(keys, dev)], [to_dev(c, dev) for c in cols]
            for cap in (0, 3, 4) if n == 10_241 else (0,):
                outs, offs = run(capi, dev, 0, dkeys, dcols, P, cap)
                R.check_stable(pid, P, cols, outs, offs)


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
@pytest.mark.parametrize("P", [2, 8])
@pytest.mark.parametrize("offset", [0, 1])
def test_histogram_unpacks_its_packed_bytes(capi, dev, dtype, P, offset):
    """The <= 8-partition histogram counts in the bytes of one register and unpacks them every 60 reads of 16 bytes: 300 000 rows
    in ONE chunk are 75 000 / 256 = 293 reads per thread of INT keys (4 keys each) and 150 000 / 256 = 586 of LONG keys (2 each) —
    4 and 9 unpacks — and with all rows in one partition a byte that is unpacked late wraps.  The key stripe moved by one element
    is not 16-byte aligned: the ranking form counts instead.  Both give the reference's offsets (and the scatter behind them the
    stable order); with no column at all the offsets alone."""
    n = 300_000
    rng = np.random.default_rng(P + offset)
    for target in (0, P - 1):
        keys = (rng.integers(0, 1 << 20, size=n) * P + target).astype(dtype)
        pid = R.partition_ids(0, R.key_image(keys), P)
        assert np.all(pid == target)
        stripe = to_dev(np.concatenate([np.zeros(offset, dtype=dtype), keys]), dev)[offset:]
        assert (stripe.data_ptr() % 16 == 0) == (offset == 0) and stripe.numel() == n
        cols = payload(n, rng, widths=())
        for cap in (1, 0):
            _, offs = run(capi, dev, 0, [stripe], [], P, cap)
            assert np.array_equal(offs[:P + 1], R.offsets_of(pid, P)), (target, cap, offs[:P + 1])
            outs, offs = run(capi, dev, 0, [stripe], [to_dev(c, dev) for c in cols], P, cap)
            R.check_stable(pid, P, cols, outs, offs)


# ---- mode 1: packed keys -------------------------------------------------------------------------------------------------------
def check_mode_1(pid, P, cols, outs, offs):
    (R.check_stable if P <= 8 else R.check_partitioned)(pid, P, cols, outs, offs)


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: "x".join(map(str, l)))
@pytest.mark.parametrize("P", [2, 4, 8, 16, 32, 64])
def test_mode_1_packed_keys_of_every_layout(capi, dev, P, layout):
    """partition_scatter_packed_keys on keys of 1-4 components of 1 / 2 / 4 / 8 bytes: stable for P <= 8 (the ranked kernels), the
    rows' sets per partition beyond (LDS fetch-add ranks)."""
    for n in NS:
        rng = np.random.default_rng(100 * n + P + len(layout))
        key_cols = [random_column(w, n, rng) for w in layout]
        pid = R.partition_ids(1, R.packed_image(key_cols, shifts_of(layout)), P)
        cols = payload(n, rng) + key_cols[:1]
        dkeys, dcols = [to_dev(k, dev) for k in key_cols], [to_dev(c, dev) for c in cols]
        for cap in caps_for(n):
            outs, offs = run(capi, dev, 1, dkeys, dcols, P, cap, key_shifts=shifts_of(layout))
            check_mode_1(pid, P, cols, outs, offs)


@pytest.mark.parametrize("layout", [(4,), (1, 2, 4)], ids=lambda l: "x".join(map(str, l)))
@pytest.mark.parametrize("P", [2, 8, 16, 64])
def test_mode_1_skewed_tiles(capi, dev, P, layout):
    """The shapes of test_mode_0_skewed_tiles on the mixing hash: keys searched from a pool with the reference's hash.  Beyond 8
    partitions: the one-add-per-wave path of the unordered ranks (whole waves in one partition) next to the add per row."""
    rng = np.random.default_rng(P + len(layout))
    pool_cols, pool_image = packed_pool(layout, 1 << 16, rng)
    pool_pid = R.partition_ids(1, pool_image, P)
    for shape in SHAPES:
        for n in (65, 10_241):
            want = shaped(shape, P, n, rng)
            rows = pick(pool_pid, P, want, rng)
            key_cols = [c[rows] for c in pool_cols]
            pid = R.partition_ids(1, R.packed_image(key_cols, shifts_of(layout)), P)
            assert np.array_equal(pid, want)
            cols = payload(n, rng)
            dkeys, dcols = [to_dev(k, dev) for k in key_cols], [to_dev(c, dev) for c in cols]
            for cap in (0, 3, 4) if n == 10_241 else (0,):
                outs, offs = run(capi, dev, 1, dkeys, dcols, P, cap, key_shifts=shifts_of(layout))
                check_mode_1(pid, P, cols, outs, offs)


@pytest.mark.parametrize("P", [2, 16, 64])
def test_mode_1_aligned_pieces(capi, dev, P):
    """align_rows = 16 (align_starts_kernel): piece starts and counts, pieces of 0, 1, 15, 16 and 17 rows among them next to
    pieces of several tiles, outputs of n + 16 P rows whose rows outside the pieces keep what they were filled with."""
    align = 16
    layout = (4, 2)
    rng = np.random.default_rng(P)
    pool_cols, pool_image = packed_pool(layout, 1 << 16, rng)
    pool_pid = R.partition_ids(1, pool_image, P)
    sizes = {2: [[0, 17], [1, 15], [16, 16], [15, 5000], [17, 0]],
             16: [[0, 1, 15, 16, 17, 2049, 33, 0] * 2, [17, 16, 15, 1, 0, 0, 4100, 31] * 2],
             64: [[0, 1, 15, 16, 17, 300, 2, 0] * 8, [16] * 64, [0] * 63 + [17], [5000] + [0] * 62 + [1]]}[P]
    for counts in sizes:
        assert len(counts) == P
        want = rng.permutation(np.repeat(np.arange(P), counts))
        n = want.size
        rows = pick(pool_pid, P, want, rng)
        key_cols = [c[rows] for c in pool_cols]
        pid = R.partition_ids(1, R.packed_image(key_cols, shifts_of(layout)), P)
        assert np.array_equal(pid, want) and np.bincount(pid, minlength=P).tolist() == counts
        cols = payload(n, rng, widths=(8, 2, 1))
        dkeys, dcols = [to_dev(k, dev) for k in key_cols], [to_dev(c, dev) for c in cols]
        for cap in (0, 3):
            outs, pieces = run(capi, dev, 1, dkeys, dcols, P, cap, rows_out=n + align * P, key_shifts=shifts_of(layout), align_rows=align)
            R.check_pieces(pid, P, align, cols, outs, pieces, [sentinel_of(c.dtype) for c in cols], stable=P <= 8)


# ---- columns -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("P", [2, 8, 64])
def test_column_sets(capi, dev, form, P):
    """No column (offsets only), one column of each width, 16 columns; for P <= 8 three 8-byte columns — 3 * 2048 * 8 = 49 152
    bytes of staging, exactly the 48 KiB the side-by-side kernel takes — and the same plus a 1-byte column (51 200 bytes), which
    the general kernel takes."""
    n = 10_241
    rng = np.random.default_rng(P + form)
    keys = rng.integers(-1000, 1 << 30, size=n).astype(np.int32)
    pid = R.partition_ids(form, R.key_image(keys), P)
    dkeys = [to_dev(keys, dev)]
    ids8 = np.arange(n, dtype=np.int64)
    column_sets = [payload(n, rng, widths=(w,)) for w in (1, 2, 4, 8)]
    column_sets += [[np.arange(n, dtype=SIGNED[w])] for w in (2, 4, 8)]                       # (the row ids in every width that holds them)
    column_sets += [payload(n, rng, widths=(8, 2, 1, 8, 4, 2, 1, 8, 4, 2, 1, 8, 4, 2, 1))]   # 16 columns
    column_sets += [[ids8, random_column(8, n, rng), random_column(8, n, rng)],               # 49 152 bytes
                    [ids8, random_column(8, n, rng), random_column(8, n, rng), random_column(1, n, rng)]]
    assert len(column_sets[7]) == 16
    for cap in (0, 3):
        _, offs = run(capi, dev, form, dkeys, [], P, cap)
        assert np.array_equal(offs[:P + 1], R.offsets_of(pid, P))
        for cols in column_sets:
            outs, offs = run(capi, dev, form, dkeys, [to_dev(c, dev) for c in cols], P, cap)
            (R.check_stable if form == 0 else check_mode_1)(pid, P, cols, outs, offs)


# ---- mode 2: a radix digit -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 6, 30, 54, 60])
def test_mode_2_radix_digit(capi, dev, shift):
    """partition_scatter_digit: stable by (key >> shift) & 63 (at 60 four bits remain) — keys of all 64 bits, keys that vary
    only inside the digit, keys that do not vary in it at all."""
    for kind, sizes in (("random", NS), ("digit_only", (2049, 10_241)), ("constant_digit", (2049, 10_241))):
        for n in sizes:
            rng = np.random.default_rng(100 * n + shift)
            keys = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
            digit = np.uint64((63 << shift) & (2**64 - 1))             # (at 60 the digit's upper two bits lie beyond bit 63)
            if kind == "digit_only":
                keys &= digit
            elif kind == "constant_digit":
                keys = (keys & ~digit) | np.uint64((37 << shift) & int(digit))
            keys = keys.view(np.int64)
            pid = R.partition_ids(2, R.key_image(keys), 64, shift)
            if kind == "constant_digit":
                assert np.unique(pid).size == 1
            else:
                assert n < 2048 or np.unique(pid).size == (16 if shift == 60 else 64)
            cols = payload(n, rng, widths=()) + [keys]                 # (the sorts move the 8-byte key and a 4-byte row number)
            dkeys, dcols = [to_dev(keys, dev)], [to_dev(c, dev) for c in cols]
            for cap in caps_for(n):
                outs, offs = run(capi, dev, 2, dkeys, dcols, 64, cap, shift=shift)
                R.check_stable(pid, 64, cols, outs, offs)


# ---- modes 4 and 3: the two hash digits ------------------------------------------------------------------------------------------
TWO_LEVEL_CASES = [("uniform", (1, 64, 65, 2049, 4096, 10_241)), ("uniform", (300_000,)), ("three_low", (10_241,)),
                   ("three_low", (300_000,)), ("one_low", (5000,)), ("two_high", (10_241,))]


@pytest.mark.parametrize("layout", [(4,), (4, 4), (1, 2, 4)], ids=lambda l: "x".join(map(str, l)))
@pytest.mark.parametrize("name,sizes", TWO_LEVEL_CASES, ids=lambda v: v if isinstance(v, str) else "-".join(map(str, v)))
def test_two_hash_digits_as_the_two_level_aggregation_runs_them(capi, dev, layout, name, sizes):
    """Mode 4 at shift 52 (any order inside a bucket), then mode 3 at shift 58 over the first pass's output, which has to keep the
    first digit's order where a tile holds more than one of its runs.  Uniform hashes: 64 runs of n / 64 rows — at 300 000 rows a
    tile lies inside one run or straddles one border, at 4096 rows (64 per digit) a tile holds 32 borders; keys of three low
    digits only: runs of several tiles; of one low digit: no border at all; of two high digits: skewed second pass."""
    rng = np.random.default_rng(len(layout))
    pool_cols, pool_image = packed_pool(layout, 1 << 17, rng)
    low, high = R.partition_ids(4, pool_image, 64, 52), R.partition_ids(3, pool_image, 64, 58)
    some = lambda mask: np.flatnonzero(mask)                            # noqa: E731
    pools = {"uniform": np.arange(pool_image.size), "three_low": some(np.isin(low, (3, 17, 40))), "one_low": some(low == 63),
             "two_high": some(np.isin(high, (0, 63)))}
    shifts = shifts_of(layout)
    assert pools[name].size >= 200, "the pool holds too few keys of this shape"
    for n in sizes:
        rows = rng.choice(pools[name], size=n)
        key_cols = [c[rows] for c in pool_cols]
        image = R.packed_image(key_cols, shifts)
        pid = R.partition_ids(4, image, 64, 52)
        assert np.unique(pid).size == {"three_low": 3, "one_low": 1}.get(name, np.unique(pid).size)
        # (the key columns travel with the rows: the second pass reads them from the first pass's output)
        cols = [np.arange(n, dtype=np.int32), random_column(8, n, rng)] + key_cols
        dkeys, dcols = [to_dev(k, dev) for k in key_cols], [to_dev(c, dev) for c in cols]
        for cap in caps_for(n):
            outs, offs = run(capi, dev, 4, dkeys, dcols, 64, cap, key_shifts=shifts, shift=52)
            R.check_partitioned(pid, 64, cols, outs, offs)
            first_keys = outs[2:]
            first_image = R.packed_image(first_keys, shifts)
            second_cols = [np.arange(n, dtype=np.int32)] + outs          # fresh row ids of the second pass's input; the first's ride along
            dk2, dc2 = [to_dev(k, dev) for k in first_keys], [to_dev(c, dev) for c in second_cols]
            outs2, offs2 = run(capi, dev, 3, dk2, dc2, 64, cap, key_shifts=shifts, shift=58)
            R.check_second_digit(first_image, 58, second_cols, outs2, offs2)
            # both passes together: the rows in the order of the hash's top 12 bits, every row once
            assert np.all(np.diff(R.hash_bits12(image, 58)[outs2[1]]) >= 0) and np.array_equal(np.sort(outs2[1]), np.arange(n))


@pytest.mark.parametrize("shift", [0, 52, 58])
def test_mode_4_skewed_tiles(capi, dev, shift):
    """The unordered digit pass on the shapes of test_mode_0_skewed_tiles (64 buckets by (hash >> shift) & 63)."""
    layout = (4, 4)
    rng = np.random.default_rng(shift)
    pool_cols, pool_image = packed_pool(layout, 1 << 16, rng)
    pool_pid = R.partition_ids(4, pool_image, 64, shift)
    for shape in SHAPES:
        for n in (65, 10_241):
            want = shaped(shape, 64, n, rng)
            rows = pick(pool_pid, 64, want, rng)
            key_cols = [c[rows] for c in pool_cols]
            pid = R.partition_ids(4, R.packed_image(key_cols, shifts_of(layout)), 64, shift)
            assert np.array_equal(pid, want)
            cols = payload(n, rng)
            dkeys, dcols = [to_dev(k, dev) for k in key_cols], [to_dev(c, dev) for c in cols]
            for cap in (0, 3, 4) if n == 10_241 else (0,):
                outs, offs = run(capi, dev, 4, dkeys, dcols, 64, cap, key_shifts=shifts_of(layout), shift=shift)
                R.check_partitioned(pid, 64, cols, outs, offs)


# ---- the run form ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
@pytest.mark.parametrize("P,shape", [(8, "one_each"), (33, "sorted"), (2, "all_last"), (64, "stranger_63")])
def test_run_of_blocks_skewed_and_sorted(capi, dev, dtype, P, shape):
    """qsx_partition_scatter_blocks on skewed and sorted keys: blocks shorter than a tile, an empty one, and under a cap of 3 a
    block of 70 001 rows that is three chunks of 12 tiles (74 103 rows / 3 -> chunks of 24 576 rows, none straddles two blocks)."""
    block_rows = [5, 2047, 0, 2049, 70_001, 1]
    n = sum(block_rows)
    rng = np.random.default_rng(P)
    pool = np.concatenate([np.arange(P), rng.integers(-1000, 1 << 30, size=20_000)]).astype(dtype)
    pool_pid = R.partition_ids(0, R.key_image(pool), P)
    want = shaped(shape, P, n, rng)
    keys = pool[pick(pool_pid, P, want, rng)]
    pid = R.partition_ids(0, R.key_image(keys), P)
    assert np.array_equal(pid, want)
    cols = payload(n, rng, widths=(8, 2))
    cuts = np.concatenate([[0], np.cumsum(block_rows)])
    dkeys = [to_dev(keys[a:b], dev) for a, b in zip(cuts[:-1], cuts[1:])]
    dcols = [[to_dev(c[a:b], dev) for c in cols] for a, b in zip(cuts[:-1], cuts[1:])]
    for cap in (0, 1, 3):
        outs, offs = run(capi, dev, 5, dkeys, dcols, P, cap)
        R.check_stable(pid, P, cols, outs, offs)
