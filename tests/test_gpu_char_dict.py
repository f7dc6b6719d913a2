"""GPU: the device dictionary of CHAR(n) values (qsx_char_dict_*, csrc/char_dict.hip) against tests/char_dict_reference.py —
exact comparisons.  Sizes cover wave, tile and multi-workgroup edges (a tile holds min(1024, 48 KiB / width rounded down to
64) rows), the stripe lies at an aligned and at an odd address, with and without a filter."""
import threading

import numpy as np
import pytest
import torch

import char_dict_reference as R
from helpers import bitmap_dev
from like_reference import pack_bitmap
from quickstep_amd import types as T

pytestmark = pytest.mark.gpu

N_MAX = 20001
WIDTHS = (1, 3, 9, 10, 15, 16, 25, 64, 255)
MODES = (b"MAIL", b"SHIP", b"AIR", b"REG AIR", b"TRUCK", b"RAIL", b"FOB")


def tile_rows(width):
    return max(64, min(1024, (48 * 1024 // width) // 64 * 64))


def sizes_for(width):
    tile = tile_rows(width)
    return sorted({0, 1, 63, 64, 65, tile - 1, tile, tile + 1, 4097, N_MAX})


def device_views(col, dev):
    """(aligned device copy, copy at an odd address) of a host stripe, both of shape (n, width)."""
    n, width = col.shape
    flat = torch.from_numpy(col.reshape(-1)).to(dev)
    buf = torch.zeros(flat.numel() + 17, dtype=torch.uint8, device=dev)
    buf[1:1 + flat.numel()] = flat
    assert flat.data_ptr() % 16 == 0 and buf[1:].data_ptr() % 16 == 1
    return flat.view(n, width), buf[1:1 + flat.numel()].view(n, width)


def filter_for(n, seed, dev):
    keep = np.random.default_rng(seed).random(n) < 0.7
    words = pack_bitmap(keep)
    if words.size and n % 64:
        words[-1] |= np.uint64((1 << (64 - n % 64)) - 1)       # set bits behind the last row: they must not come through
    return keep, bitmap_dev(words, dev) if words.size else None


def check(d, col, view, keep=None, filter_dev=None, what=""):
    """One intern call into the EMPTY dictionary d, checked in full; returns the ids."""
    ids_dev = d.intern(view, filter_dev)
    values_dev = d.values(ids_dev)
    size, dropped = d.size()
    ids = ids_dev.cpu().numpy()
    values = values_dev.cpu().numpy()
    labels, distinct = R.intern(col, keep)
    assert dropped == 0, what
    assert size == distinct, what
    assert R.same_partition(ids, labels), what                              # ids[i] == ids[j] iff the texts are equal
    if keep is not None:
        assert np.all(ids[~keep] == -1), what
    assert np.array_equal(np.unique(ids[ids >= 0]), np.arange(size)), what   # dense
    want = R.canonical(col)
    if keep is not None:
        want[~keep] = 0
    assert np.array_equal(values, want), what
    return ids


@pytest.mark.parametrize("width", WIDTHS)
def test_intern_matches_the_reference_at_every_size(capi, dev, width):
    col = R.make_stripe(width, N_MAX, seed=300 + width)
    aligned, odd = device_views(col, dev)
    d = capi.CharDict(width, N_MAX)
    for n in sizes_for(width):
        keep, filter_dev = filter_for(n, 11 * width + n, dev)
        for view, filtered in ((aligned, False), (odd, True), (odd, False), (aligned, True)):
            d.clear()
            check(d, col[:n], view[:n], keep if filtered else None, filter_dev if filtered else None, (width, n, filtered))
    d.close()


def mixes(width, n):
    yield "one value", R.make_stripe(width, n, 1, values=[b"MAIL"[:width]])
    yield "seven values", R.make_stripe(width, n, 2, values=[m[:width] for m in MODES] if width >= 7 else [bytes([65 + i]) for i in range(7)])
    if width >= 6:
        yield "n/3 values", R.make_stripe(width, n, 3, values=[b"v%d" % i for i in range(n // 3)])
        distinct = np.stack([R.field(b"%d" % i, width) for i in range(n)])
        tails = R.make_stripe(width, n, 4)
        yield "all distinct", np.where(np.arange(width)[None, :] <= R.lengths(distinct)[:, None], distinct, tails).astype(np.uint8)
    if width >= 9:
        yield "equal in the first 8 bytes", R.make_stripe(width, n, 5, values=[b"ABCDEFGH" + bytes([97 + i]) for i in range(5)])
    if width >= 17:
        yield "equal in the first 16 bytes", R.make_stripe(width, n, 6, values=[b"ABCDEFGHIJKLMNOP" + b"x" * (width - 17) + bytes([97 + i])
                                                                               for i in range(5)])
    if width >= 3:
        yield "ab, abb, a and the empty text", R.make_stripe(width, n, 7, values=[b"ab", b"abb", b"a", b""])
    yield "full-width texts without a NUL", R.make_stripe(width, n, 8, values=[b"z" * (width - 1) + bytes([97 + i]) for i in range(4)])


@pytest.mark.parametrize("width", (1, 10, 25))
def test_value_mixes(capi, dev, width):
    n = 4097
    d = capi.CharDict(width, n)
    for name, col in mixes(width, n):
        assert R.intern(col)[1] >= 1
        aligned, odd = device_views(col, dev)
        keep, filter_dev = filter_for(n, 5, dev)
        d.clear()
        check(d, col, odd, None, None, (width, name))
        d.clear()
        check(d, col, aligned, keep, filter_dev, (width, name, "filtered"))
    d.close()


def test_equal_texts_with_different_garbage_behind_the_nul_share_an_id(capi, dev):
    col = R.make_stripe(10, 5000, 9, values=MODES)
    assert np.unique(col, axis=0).shape[0] > 1000 and R.intern(col)[1] == 7     # the raw fields differ, the texts do not
    d = capi.CharDict(10, 16)
    check(d, col, device_views(col, dev)[0])
    d.close()


def test_the_collision_pair_gets_two_ids_in_a_minimum_size_dictionary(capi, dev):
    a, b = R.COLLISION_PAIR
    width = R.COLLISION_WIDTH
    ha, hb = capi.char_dict_hash(a, width), capi.char_dict_hash(b, width)
    assert R.fingerprint(ha) == R.fingerprint(hb) and R.home_slot(ha) == R.home_slot(hb)
    col = R.make_stripe(width, 1000, 10, values=[a, b])
    d = capi.CharDict(width, 8)               # 16 slots: the smallest table
    ids = check(d, col, device_views(col, dev)[0])
    assert set(ids.tolist()) == {0, 1}
    ids2 = d.intern(device_views(col, dev)[1]).cpu().numpy()      # and again, now against the value store
    assert np.array_equal(ids, ids2) and d.size() == (2, 0)
    d.close()


def test_ids_are_stable_across_calls(capi, dev):
    col = R.make_stripe(15, N_MAX, 12, values=[b"value %d" % i for i in range(700)])
    view = device_views(col, dev)[0]
    d = capi.CharDict(15, 1024)
    first = d.intern(view[:12000]).cpu().numpy()
    size_first = d.size()[0]
    second = d.intern(view[8000:]).cpu().numpy()
    size, dropped = d.size()
    again = d.intern(view[:12000]).cpu().numpy()
    assert dropped == 0 and size == R.intern(col)[1] >= size_first
    assert np.array_equal(first[8000:], second[:4000]) and np.array_equal(first, again)
    ids = np.concatenate([first[:8000], second])
    assert R.same_partition(ids, R.intern(col)[0])
    assert np.array_equal(np.unique(ids), np.arange(size))
    assert d.size() == (size, 0)
    d.close()


def test_intern_blocks_equals_block_by_block_intern(capi, dev):
    width = 25
    rows = [3000, 0, 1025, 5000, 64]
    col = R.make_stripe(width, sum(rows), 13, values=[b"NATION %02d" % i for i in range(25)])
    view = device_views(col, dev)[1]
    starts = np.concatenate([[0], np.cumsum(rows)])
    blocks = [view[starts[b]:starts[b + 1]].contiguous() if b % 2 else view[starts[b]:starts[b + 1]] for b in range(len(rows))]
    keeps, filters = [], []
    for b, n in enumerate(rows):
        keep, f = filter_for(n, 20 + b, dev)
        use = b in (0, 3)
        keeps.append(keep if use else np.ones(n, dtype=bool))
        filters.append(f if use else None)                       # NULL filter entries next to real ones
    run = capi.CharDict(width, 64)
    one = capi.CharDict(width, 64)
    outs = run.intern_blocks(blocks, filters)
    singles = [one.intern(blocks[b], filters[b]) for b in range(len(rows))]
    ids_run = torch.cat(outs).cpu().numpy()
    ids_one = torch.cat(singles).cpu().numpy()
    keep = np.concatenate(keeps)
    labels, distinct = R.intern(col, keep)
    assert run.size() == one.size() == (distinct, 0)
    assert R.same_partition(ids_run, labels) and R.same_partition(ids_run, ids_one)         # equal up to a renaming of ids
    assert np.array_equal(np.unique(ids_run[ids_run >= 0]), np.arange(distinct))
    want = R.canonical(col)
    want[~keep] = 0
    assert np.array_equal(run.values(torch.cat(outs)).cpu().numpy(), want)
    all_filtered = run.intern_blocks(blocks, None)              # no filters at all, into the warm dictionary
    assert R.same_partition(torch.cat(all_filtered).cpu().numpy(), R.intern(col)[0])
    assert run.size() == (R.intern(col)[1], 0)
    run.close()
    one.close()


def test_clear_empties_the_dictionary(capi, dev):
    col = R.make_stripe(10, 3000, 14, values=MODES)
    view = device_views(col, dev)[0]
    d = capi.CharDict(10, 16)
    check(d, col, view)
    d.clear()
    assert d.size() == (0, 0)
    other = R.make_stripe(10, 3000, 15, values=MODES[:3])
    ids = check(d, other, device_views(other, dev)[0])
    assert set(ids.tolist()) == {0, 1, 2}
    zeros = d.values(torch.tensor([-1, 3, 99, -7, 2 ** 31 - 1], dtype=torch.int32, device=dev)).cpu().numpy()
    assert not zeros.any()                                       # ids outside [0, size): the zero value, never another's bytes
    d.close()


def test_capacity_drop_reserve_repeat(capi, dev):
    col = R.make_stripe(10, 5000, 16, values=[b"key%03d" % i for i in range(100)])
    labels, distinct = R.intern(col)
    assert distinct == 100
    view = device_views(col, dev)[0]
    d = capi.CharDict(10, 16)
    ids_dev = d.intern(view)                                     # returns OK: the call is stream-ordered
    size, dropped = d.size()
    ids = ids_dev.cpu().numpy()
    placed = ids >= 0
    assert size == 16
    assert dropped == int((~placed).sum()) > 0
    assert np.array_equal(np.unique(ids[placed]), np.arange(16))
    assert R.same_partition(ids[placed], labels[placed])
    assert not np.intersect1d(labels[placed], labels[~placed]).size           # a text is placed in all its rows or in none
    assert np.array_equal(d.values(ids_dev).cpu().numpy()[placed], R.canonical(col)[placed])
    again = d.intern(view).cpu().numpy()                         # without a reserve: the same rows are dropped again
    assert np.array_equal(again, ids) and d.size() == (16, 2 * dropped)
    d.reserve(256)
    assert d.size() == (16, 0)
    full_dev = d.intern(view)
    full = full_dev.cpu().numpy()
    assert d.size() == (100, 0)
    assert np.all(full >= 0) and np.array_equal(full[placed], ids[placed])    # the 16 early ids are unchanged
    assert R.same_partition(full, labels) and np.array_equal(np.unique(full), np.arange(100))
    assert np.array_equal(d.values(full_dev).cpu().numpy(), R.canonical(col))
    d.close()


def test_four_threads_on_four_streams_share_one_dictionary(capi, dev):
    col = R.make_stripe(25, N_MAX, 17, values=[b"customer#%05d" % i for i in range(3000)])
    view = device_views(col, dev)[0]
    d = capi.CharDict(25, 4096)
    bounds = [(0, 9000), (4000, 14000), (8000, N_MAX), (0, N_MAX)]
    streams = [torch.cuda.Stream(device=dev) for _ in bounds]
    torch.cuda.synchronize(dev)
    results, errors = [None] * 4, []

    def work(i):
        try:
            lo, hi = bounds[i]
            with torch.cuda.stream(streams[i]):
                outs = [d.intern(view[lo:hi], stream=streams[i]) for _ in range(3)]
            streams[i].synchronize()
            results[i] = [o.cpu().numpy() for o in outs]
        except Exception as e:      # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    size, dropped = d.size()
    labels, distinct = R.intern(col)
    assert (size, dropped) == (distinct, 0)
    ids = np.full(N_MAX, -1, dtype=np.int64)
    for (lo, hi), outs in zip(bounds, results):
        for o in outs:
            fresh = ids[lo:hi] < 0
            ids[lo:hi][fresh] = o[fresh]
            assert np.array_equal(ids[lo:hi], o)                 # the same id for a row in every output
    assert R.same_partition(ids, labels) and np.array_equal(np.unique(ids), np.arange(size))
    d.close()


def test_interned_ids_group_through_the_aggregation(capi, dev):
    n = N_MAX
    rng = np.random.default_rng(18)
    col = R.make_stripe(10, n, 19, values=MODES)
    x = rng.integers(-1000, 1000, size=n).astype(np.float64)      # integer-valued: every sum is exact
    d = capi.CharDict(10, 16)
    ids = d.intern(device_views(col, dev)[1])
    cfg = T.make_agg_config(T.AGG_COMPACT_KEY, [(T.INT, None), (T.DOUBLE, None)], keys=[0],
                            aggs=[(T.AGG_SUM, T.col(1)), (T.AGG_COUNT_STAR, None)], est_groups=16)
    state = capi.AggState(cfg)
    state.update([ids, torch.from_numpy(x).to(dev)])
    keys, vals, nulls, groups = state.finalize(dev)
    g = int(groups.cpu()[0])
    texts = d.values(keys[0][:g].contiguous()).cpu().numpy()
    sums, counts = vals[0][:g].cpu().numpy(), vals[1][:g].cpu().numpy()
    got = {(bytes(texts[i]), float(sums[i]), int(counts[i])) for i in range(g)}
    canon = R.canonical(col)
    want = set()
    for m in MODES:
        rows = np.all(canon == R.field(m, 10)[None, :], axis=1)
        want.add((bytes(R.field(m, 10)), float(x[rows].sum()), int(rows.sum())))
    assert g == 7 and got == want
    state.close()
    d.close()
