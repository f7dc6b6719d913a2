"""The stream kernel of the Q1 plan shape (csrc/agg_stream.hip) against exact references.

The plan is exactly test_gpu_agg.q1_config(); the values are of family A (tests/exact_reference.py: every summation order gives
the same bits), so SUM and COUNT are compared exactly and AVG as float64(SUM) / COUNT (test_gpu_agg_exact.check).  Every case says
which kernel has to serve it, and qsx_debug_agg_stream_launches() proves it: the counter rises by one per update call the stream
kernel took and stays where it is for every call it must leave to the kernels that were there before it."""
import ctypes
import zlib

import numpy as np
import pytest

import exact_reference as R
from helpers import bitmap_dev, to_dev
from test_gpu_agg import q1_config
from test_gpu_agg_exact import check

pytestmark = pytest.mark.gpu

STEP_ROWS = 512                  # rows of one step of a 256-thread workgroup (two per lane)
UNROLL = 1                       # steps per tile (agg_stream.hip kStreamU)
NAMES = ["qty", "price", "disc", "tax"]


def launches(capi):
    fn = capi.lib.qsx_debug_agg_stream_launches
    fn.restype = ctypes.c_longlong
    return fn()


def rng_of(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def family_a_q1(rng, gid, groups):
    """Family A's Q1 columns (exact_reference.family_a without its FLOAT column, which needs groups of many rows)."""
    n = gid.size
    a = rng.integers(1800, 210001, size=n)
    b = rng.integers(0, 7, size=n)
    c = rng.integers(0, 6, size=n)
    cols = dict(qty=rng.integers(1, 51, size=n).astype(np.float64), price=a / 2.0, disc=b / 64.0, tax=c / 64.0)
    cols.update(R.q1_terms(cols))
    assert np.array_equal(R.assert_exact_multiples(cols["t3"], 13), a * (64 - b) * (64 + c))
    for name, e in (("qty", 0), ("price", 1), ("disc", 6), ("tax", 6), ("t1", 7), ("t3", 13)):
        R.assert_exact_sums(cols[name], e, gid, groups)
    return cols


def key_codes(rng, groups):
    """A distinct (byte, byte) key per group: Q1's four flags first, then arbitrary bytes with 0x00 and 0xFF among them."""
    codes = [ord("A") | ord("F") << 8, ord("N") | ord("F") << 8, ord("N") | ord("O") << 8, ord("R") | ord("F") << 8, 0x0000, 0xFFFF,
             0x00FF, 0xFF00]
    pool = [int(c) for c in rng.permutation(65536) if int(c) not in codes]
    return np.array((codes + pool)[:groups], dtype=np.int64)


def key_columns(codes, gid):
    return [(codes[gid] & 0xFF).astype(np.uint8), (codes[gid] >> 8).astype(np.uint8)]


def device_columns(dev, codes, gid, cols):
    return [to_dev(c, dev) for c in key_columns(codes, gid) + [cols[c] for c in NAMES]]


def finalize(st, dev, codes):
    """(group number of every output row, values, NULL flags) as test_gpu_agg_exact.check takes them."""
    cap = max(st.num_groups(), 1)
    keys, vals, nulls, found = st.finalize(dev, capacity=cap)
    g = int(found.item())
    assert 0 <= g <= cap
    k1, k2 = (k.cpu().numpy()[:g].astype(np.int64) & 0xFF for k in keys)
    number = {int(c): i for i, c in enumerate(codes)}
    got = np.array([number[int(a | b << 8)] for a, b in zip(k1, k2)], dtype=np.int64)
    return got, [v.cpu().numpy()[:g] for v in vals], [z.cpu().numpy()[:g] for z in nulls]


def run(capi, dev, gid, groups, rng, family="A", est=6, stream=True, dcols_of=None, filter_keep=None, oracle=None):
    """One state, one update call over all rows; the stream counter moves by one exactly when `stream`."""
    codes = key_codes(rng, groups)
    cols = family_a_q1(rng, gid, groups) if family == "A" else R.family_b(rng, gid, groups)
    dcols = device_columns(dev, codes, gid, cols) if dcols_of is None else dcols_of(codes, cols)
    st = capi.AggState(q1_config(est_groups=est))
    before = launches(capi)
    bitmap = None if filter_keep is None else bitmap_dev(oracle.bitmap_from_bools(filter_keep), dev)
    st.update(dcols, gid.size, filter_bitmap=bitmap)
    moved = launches(capi) - before
    assert moved == (1 if stream else 0), f"stream launches moved by {moved}"
    live = gid if filter_keep is None else np.where(filter_keep, gid, -1)
    check("Q1", family, finalize(st, dev, codes), cols, live, groups)
    st.close()


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in ("QSX_AGG_STREAM", "QSX_AGG_REG_GROUPS", "QSX_AGG_NO_SPECIALIZE"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("QSX_AGG_STREAM_MIN_ROWS", "0")        # (by default calls below 2 M rows keep the staged-tile kernel)


# ---- row counts around every boundary -------------------------------------------------------------------------------------------
ROW_COUNTS = list(dict.fromkeys([
    1, 2, 127, 128, 129, 511, 512, 513, STEP_ROWS * UNROLL - 1, STEP_ROWS * UNROLL, STEP_ROWS * UNROLL + 1, 1023, 1024, 1025,
    200_003,          # every workgroup one or two tiles, one of them ragged
    1_000_003]))      # every workgroup several iterations, then the ragged tile


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_row_counts(capi, dev, n):
    rng = rng_of(f"rows/{n}")
    run(capi, dev, rng.integers(0, 4, size=n), 4, rng)


# ---- late and rare groups --------------------------------------------------------------------------------------------------------
def test_group_that_starts_in_the_last_rows(capi, dev):
    rng = rng_of("late")
    n = 200_003
    gid = rng.integers(0, 3, size=n)
    gid[n - 100 + rng.choice(100, size=30, replace=False)] = 3
    assert not np.any(gid[:n - 100] == 3)
    run(capi, dev, gid, 4, rng)


def test_group_of_one_row(capi, dev):
    rng = rng_of("one row")
    n = 200_003
    gid = rng.integers(0, 3, size=n)
    gid[123_456] = 3
    run(capi, dev, gid, 4, rng)


def test_one_group(capi, dev):
    rng = rng_of("one group")
    run(capi, dev, np.zeros(200_003, dtype=np.int64), 1, rng)


# ---- more groups than registers, and than LDS slots -----------------------------------------------------------------------------
@pytest.mark.parametrize("skew", ["uniform", "skewed"])
@pytest.mark.parametrize("groups", [5, 9, 40])
def test_more_groups_than_a_lane_holds(capi, dev, groups, skew):
    rng = rng_of(f"groups/{groups}/{skew}")
    n = 200_003
    if skew == "uniform":
        gid = rng.integers(0, groups, size=n)
    else:                                         # 90 % of the rows in one group, the rest spread over the others
        gid = np.where(rng.random(n) < 0.9, 0, rng.integers(1, groups, size=n))
    assert np.unique(gid).size == groups
    run(capi, dev, gid, groups, rng)


# ---- NaN and Inf stay in their group -----------------------------------------------------------------------------------------------
def test_nan_and_inf_stay_in_their_group(capi, dev):
    rng = rng_of("nan")
    n, groups = 200_003, 4
    gid = rng.integers(0, groups, size=n)
    codes = key_codes(rng, groups)
    cols = family_a_q1(rng, gid, groups)
    rows = np.nonzero(gid == 0)[0]
    cols["price"][rows[10]] = np.inf
    cols["price"][rows[-10]] = np.nan
    cols.update(R.q1_terms(cols))
    st = capi.AggState(q1_config())
    before = launches(capi)
    st.update(device_columns(dev, codes, gid, cols), n)
    assert launches(capi) == before + 1
    got, vals, flags = finalize(st, dev, codes)
    st.close()
    assert np.array_equal(np.sort(got), np.arange(groups))
    order = np.argsort(got)
    cnt = np.bincount(gid, minlength=groups)
    # (SUM qty, SUM price, SUM t1, SUM t3, AVG qty, AVG price, AVG disc, COUNT)
    assert np.array_equal(vals[7][order], cnt)
    for j, name in enumerate(["qty", "price", "t1", "t3"]):
        with np.errstate(invalid="ignore"):
            want = np.bincount(gid, weights=cols[name], minlength=groups)
        assert np.array_equal(vals[j][order][1:], want[1:]), f"SUM({name}) of a group without NaN or Inf changed"
        assert np.array_equal(vals[j][order][:1], want[:1], equal_nan=True), f"SUM({name}) of group 0"
    assert np.all(np.isnan(vals[1][order][:1])) and np.all(np.isfinite(vals[0][order]))
    want_disc = np.bincount(gid, weights=cols["disc"], minlength=groups)
    assert np.array_equal(vals[6][order], want_disc / cnt)
    assert np.array_equal(vals[4][order], vals[0][order] / cnt)
    assert np.array_equal(vals[5][order], vals[1][order] / cnt, equal_nan=True)
    assert not any(np.any(z) for z in flags)


# ---- two update calls into one state; clear ----------------------------------------------------------------------------------------
def test_two_updates_and_clear(capi, dev):
    rng = rng_of("two updates")
    n, groups, cut = 200_003, 4, 77_778                           # (cut is even: the second call's views stay aligned)
    gid = rng.integers(0, groups, size=n)
    codes = key_codes(rng, groups)
    cols = family_a_q1(rng, gid, groups)
    dcols = device_columns(dev, codes, gid, cols)
    st = capi.AggState(q1_config())
    before = launches(capi)
    st.update([c[:cut] for c in dcols], cut)
    st.update([c[cut:] for c in dcols], n - cut)
    assert launches(capi) == before + 2
    check("Q1", "A", finalize(st, dev, codes), cols, gid, groups)
    st.clear()
    st.update([c[:cut] for c in dcols], cut)
    assert launches(capi) == before + 3
    check("Q1", "A", finalize(st, dev, codes), cols, np.where(np.arange(n) < cut, gid, -1), groups)
    st.close()


# ---- what the stream kernel must leave to the others -------------------------------------------------------------------------------
def test_fallback_unaligned_double_column(capi, dev):
    rng = rng_of("unaligned")

    def shifted(codes, cols):
        # price as a view one element into a longer tensor: 8-byte but not 16-byte aligned
        out = device_columns(dev, codes, gid, cols)
        longer = to_dev(np.concatenate([[0.0], cols["price"]]), dev)
        out[3] = longer[1:]
        assert out[3].data_ptr() % 16 == 8 and all(c.data_ptr() % 16 == 0 for i, c in enumerate(out) if i != 3)
        return out
    gid = rng.integers(0, 4, size=200_003)
    run(capi, dev, gid, 4, rng, stream=False, dcols_of=shifted)


def test_fallback_unaligned_key_column(capi, dev):
    rng = rng_of("unaligned key")

    def shifted(codes, cols):
        out = device_columns(dev, codes, gid, cols)
        longer = to_dev(np.concatenate([[0], key_columns(codes, gid)[1]]).astype(np.uint8), dev)
        out[1] = longer[1:]
        assert out[1].data_ptr() % 2 == 1
        return out
    gid = rng.integers(0, 4, size=200_003)
    run(capi, dev, gid, 4, rng, stream=False, dcols_of=shifted)


def test_fallback_filter_bitmap(capi, dev, oracle):
    rng = rng_of("filter")
    gid = rng.integers(0, 4, size=200_003)
    run(capi, dev, gid, 4, rng, stream=False, filter_keep=rng.random(gid.size) < 0.7, oracle=oracle)


@pytest.mark.parametrize("name,value", [("QSX_AGG_STREAM", "0"), ("QSX_AGG_NO_SPECIALIZE", "1"), ("QSX_AGG_REG_GROUPS", "1")])
def test_fallback_switches(capi, dev, monkeypatch, name, value):
    monkeypatch.setenv(name, value)
    monkeypatch.setenv("QSX_AGG_JIT_MIN_ROWS", str(1 << 60))
    rng = rng_of(f"switch/{name}")
    run(capi, dev, rng.integers(0, 4, size=200_003), 4, rng, stream=False)


def test_fallback_few_rows_by_default(capi, dev, monkeypatch):
    """Without the tests' switch a call below the row threshold keeps the staged-tile kernel; one above it streams."""
    monkeypatch.delenv("QSX_AGG_STREAM_MIN_ROWS")
    rng = rng_of("few rows")
    run(capi, dev, rng.integers(0, 4, size=200_003), 4, rng, stream=False)
    run(capi, dev, rng.integers(0, 4, size=2_000_001), 4, rng, stream=True)


def test_two_int_key_shape_keeps_its_kernel(capi, dev):
    """The other registered plan shape (two INT keys) at the same small-table geometry: not a plan the stream kernel takes."""
    from quickstep_amd import types as T
    from test_gpu_agg_exact import finalize_groups, make_config
    rng = rng_of("two int keys")
    n, groups = 200_003, 5
    gid = rng.integers(0, groups, size=n)
    cols = {"price": family_a_q1(rng, gid, groups)["price"]}
    cfg, kcols = make_config("SHAPE2", "int2", gid, T.AGG_COMPACT_KEY, est=6)
    st = capi.AggState(cfg)
    before = launches(capi)
    st.update([to_dev(c, dev) for c in kcols + [cols["price"]]], n)
    assert launches(capi) == before
    check("SHAPE2", "A", finalize_groups(st, dev, "int2"), cols, gid, groups)
    st.close()


# ---- both kernels on realistic decimals ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stream", [True, False])
def test_parity_on_family_b(capi, dev, monkeypatch, stream):
    """Family B (TPC-H-like decimals) at 200 000 rows: either kernel within exact_reference's order-independent bound tol_g."""
    if not stream:
        monkeypatch.setenv("QSX_AGG_STREAM", "0")
    rng = rng_of("family B")                      # the same rows for both
    run(capi, dev, rng.integers(0, 4, size=200_000), 4, rng, family="B", stream=stream)
