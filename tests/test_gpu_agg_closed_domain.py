"""Closed key domains: a COMPACT_KEY state whose key code has at most 16 bits holds its whole domain, never grows, and its
qsx_agg_finalize returns without waiting for the stream (include/qsx.h).

- every key of the domain present (65 536 pairs of CHAR(1), all 256 values of one CHAR(1)): COUNT and SUM of every group
  exactly a numpy group-by's, through the default kernel choice and through the stream kernel, and a second update leaves
  the exported image the size it had;
- three CHAR(1) keys (24 bits) are still a growable state: exact after growing from an estimate of 1;
- the contract on both sides: behind >= 20 ms of device work, finalize of a closed state returns with that work pending,
  finalize of a growable state returns with the stream drained;
- five steps of clear / update / finalize back to back without a host wait: every step's outputs are its own.

Integer-valued doubles throughout: every SUM is exact in any order of addition."""
import numpy as np
import pytest
import torch

from helpers import to_dev
from quickstep_amd import types as T

pytestmark = pytest.mark.gpu


def q1_config(est=6):
    """TPC-H Q1's shape (the plan the stream kernel is compiled for): two CHAR(1) keys, four doubles."""
    return T.make_agg_config(
        T.AGG_COMPACT_KEY,
        columns=[(T.CHAR, 1), (T.CHAR, 1), (T.DOUBLE, None), (T.DOUBLE, None), (T.DOUBLE, None), (T.DOUBLE, None)],
        keys=[0, 1],
        instrs=[(T.EX_SUB, 0, T.const(0), T.col(4)), (T.EX_MUL, 1, T.col(3), T.temp(0)),
                (T.EX_ADD, 2, T.const(0), T.col(5)), (T.EX_MUL, 3, T.temp(1), T.temp(2))],
        consts=[1.0],
        aggs=[(T.AGG_SUM, T.col(2)), (T.AGG_SUM, T.col(3)), (T.AGG_SUM, T.temp(1)), (T.AGG_SUM, T.temp(3)),
              (T.AGG_AVG, T.col(4)), (T.AGG_COUNT_STAR, None)],
        est_groups=est)


def q1_rows(rng, codes):
    """Host columns of Q1's shape for the given 16-bit key codes; every value an integer, so every product and sum is exact."""
    n = codes.size
    return [(codes & 0xFF).astype(np.uint8), (codes >> 8).astype(np.uint8),
            rng.integers(1, 51, size=n).astype(np.float64), rng.integers(900, 2000, size=n).astype(np.float64),
            rng.integers(0, 4, size=n).astype(np.float64), rng.integers(0, 4, size=n).astype(np.float64)]


def q1_reference(cols, times=1):
    """code -> (sum qty, sum price, sum price (1 - disc), sum price (1 - disc) (1 + tax), avg disc, count) by numpy, in
    ascending code order; `times`: the same rows were added that many times."""
    k1, k2, qty, price, disc, tax = cols
    code = k1.astype(np.int64) | (k2.astype(np.int64) << 8)
    uniq, inv = np.unique(code, return_inverse=True)
    g = uniq.size
    disc_price = price * (1.0 - disc)
    charge = disc_price * (1.0 + tax)
    count = np.bincount(inv, minlength=g) * times
    sums = [np.bincount(inv, weights=w, minlength=g) * times for w in (qty, price, disc_price, charge, disc)]
    return uniq, [sums[0], sums[1], sums[2], sums[3], sums[4] / count, count.astype(np.int64)]


def assert_q1_equals(fin, want, what, capacity=None):
    keys, vals, _, groups = fin
    uniq, want_vals = want
    g = int(groups.item())
    assert g == uniq.size, f"{what}: {g} groups, want {uniq.size}"
    code = keys[0][:g].cpu().numpy().astype(np.int64) | (keys[1][:g].cpu().numpy().astype(np.int64) << 8)
    order = np.argsort(code, kind="stable")
    assert np.array_equal(code[order], uniq), f"{what}: the keys differ"
    for a, w in enumerate(want_vals):
        got = vals[a][:g].cpu().numpy()[order]
        assert got.dtype == w.dtype and np.array_equal(got, w), f"{what}: aggregate {a} differs in {np.count_nonzero(got != w)} groups"
    if capacity is not None:
        for column in list(keys) + list(vals):
            assert not column[g:capacity].cpu().numpy().view(np.uint8).any(), f"{what}: rows behind the groups are not zero"


def slots_of(st):
    return st.image_layout()[1] - 1


# ---- every key of the domain ---------------------------------------------------------------------------------------------------
_whole_domain = {}


def whole_domain():
    """3 x 65 536 rows in which every pair of CHAR(1) values occurs three times, and their reference (computed once)."""
    if not _whole_domain:
        rng = np.random.default_rng(20)
        codes = rng.permutation(np.repeat(np.arange(65536, dtype=np.int64), 3))
        cols = q1_rows(rng, codes)
        _whole_domain.update(cols=cols, once=q1_reference(cols), twice=q1_reference(cols, times=2))
    return _whole_domain


@pytest.mark.parametrize("kernel", ["default", "stream"])
def test_whole_domain_of_two_char1_keys_is_exact(capi, dev, monkeypatch, kernel):
    if kernel == "stream":
        monkeypatch.setenv("QSX_AGG_STREAM_MIN_ROWS", "0")    # the stream kernel: its registers hold only a few groups
    else:
        monkeypatch.delenv("QSX_AGG_STREAM_MIN_ROWS", raising=False)
    data = whole_domain()
    dev_cols = [to_dev(c, dev) for c in data["cols"]]
    n = data["cols"][0].size
    st = capi.AggState(q1_config(est=6))
    assert slots_of(st) >= 2 * 65536, "a closed state holds its whole domain at load <= 1/2"
    st.update(dev_cols, n)
    assert_q1_equals(st.finalize(dev, capacity=65536), data["once"], f"{kernel}: first update", capacity=65536)
    image_bytes = st.export_bytes()
    st.update(dev_cols, n)
    assert st.export_bytes() == image_bytes, "the table of a closed state grew"
    assert_q1_equals(st.finalize(dev, capacity=65536), data["twice"], f"{kernel}: second update", capacity=65536)
    # more room than groups: the rows behind them are defined as well
    assert_q1_equals(st.finalize(dev, capacity=65536 + 1000), data["twice"], f"{kernel}: capacity beyond the groups", capacity=65536 + 1000)


def small_config(num_keys, est):
    return T.make_agg_config(T.AGG_COMPACT_KEY, columns=[(T.CHAR, 1)] * num_keys + [(T.DOUBLE, None)], keys=list(range(num_keys)),
                             aggs=[(T.AGG_COUNT_STAR, None), (T.AGG_SUM, T.col(num_keys))], est_groups=est)


def assert_counts_and_sums(fin, num_keys, codes, values, what, times=1):
    keys, vals, _, groups = fin
    uniq, inv = np.unique(codes, return_inverse=True)
    g = int(groups.item())
    assert g == uniq.size, f"{what}: {g} groups, want {uniq.size}"
    code = np.zeros(g, dtype=np.int64)
    for k in range(num_keys):
        code |= keys[k][:g].cpu().numpy().astype(np.int64) << (8 * k)
    order = np.argsort(code, kind="stable")
    assert np.array_equal(code[order], uniq), f"{what}: the keys differ"
    assert np.array_equal(vals[0][:g].cpu().numpy()[order], np.bincount(inv, minlength=g) * times), f"{what}: COUNT(*) differs"
    assert np.array_equal(vals[1][:g].cpu().numpy()[order], np.bincount(inv, weights=values, minlength=g) * times), f"{what}: SUM differs"


@pytest.mark.parametrize("kernel", ["default", "stream"])
def test_whole_domain_of_one_char1_key_is_exact(capi, dev, monkeypatch, kernel):
    if kernel == "stream":
        monkeypatch.setenv("QSX_AGG_STREAM_MIN_ROWS", "0")
    else:
        monkeypatch.delenv("QSX_AGG_STREAM_MIN_ROWS", raising=False)
    rng = np.random.default_rng(21)
    codes = rng.permutation(np.repeat(np.arange(256, dtype=np.int64), 3))
    values = rng.integers(-1000, 1000, size=codes.size).astype(np.float64)
    dev_cols = [to_dev(codes.astype(np.uint8), dev), to_dev(values, dev)]
    st = capi.AggState(small_config(1, est=6))
    assert slots_of(st) >= 2 * 256
    st.update(dev_cols, codes.size)
    assert_counts_and_sums(st.finalize(dev, capacity=256), 1, codes, values, f"{kernel}: first update")
    image_bytes = st.export_bytes()
    st.update(dev_cols, codes.size)
    assert st.export_bytes() == image_bytes, "the table of a closed state grew"
    assert_counts_and_sums(st.finalize(dev, capacity=256), 1, codes, values, f"{kernel}: second update", times=2)


def three_key_rows(seed, groups=5000):
    rng = np.random.default_rng(seed)
    distinct = rng.choice(1 << 24, size=groups, replace=False).astype(np.int64)
    codes = rng.permutation(np.repeat(distinct, 3))
    return codes, rng.integers(-1000, 1000, size=codes.size).astype(np.float64)


def three_key_columns(codes, values, dev):
    return [to_dev(((codes >> (8 * k)) & 0xFF).astype(np.uint8), dev) for k in range(3)] + [to_dev(values, dev)]


def test_three_char1_keys_are_still_growable(capi, dev):
    """24 bits of key: the table is sized from the estimate (1) and grows to hold 5 000 groups, exactly as before."""
    codes, values = three_key_rows(22)
    st = capi.AggState(small_config(3, est=1))
    created = st.export_bytes()
    st.update(three_key_columns(codes, values, dev), codes.size)
    assert_counts_and_sums(st.finalize(dev), 3, codes, values, "three keys")
    assert st.export_bytes() > created, "5 000 groups in a table made for one: it must have grown"


# ---- the contract ----------------------------------------------------------------------------------------------------------------
def enqueue_busy_ms(dev, ms):
    """At least `ms` of device work on the current stream: torch.cuda._sleep with a cycle count calibrated by events."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    probe = 2_000_000
    torch.cuda._sleep(1000)        # (first use)
    torch.cuda.synchronize()
    start.record()
    torch.cuda._sleep(probe)
    end.record()
    end.synchronize()
    cycles_per_ms = probe / max(start.elapsed_time(end), 1e-3)
    torch.cuda._sleep(int(cycles_per_ms * ms * 1.5))     # half as much again: the calibration is one sample
    return cycles_per_ms


def test_finalize_of_a_closed_state_does_not_wait_for_the_stream(capi, dev):
    rng = np.random.default_rng(23)
    cols = q1_rows(rng, rng.integers(0, 65536, size=50_000))
    dev_cols = [to_dev(c, dev) for c in cols]
    st = capi.AggState(q1_config(est=6))
    st.update(dev_cols, 50_000)                       # (first use of the kernels: nothing is compiled or loaded below)
    st.finalize(dev, capacity=65536)
    st.clear()
    torch.cuda.synchronize()
    enqueue_busy_ms(dev, 20)
    st.update(dev_cols, 50_000)
    before = torch.cuda.Event()
    before.record()
    fin = st.finalize(dev, capacity=65536)
    behind = torch.cuda.Event()
    behind.record()
    pending = (before.query(), behind.query())
    assert pending == (False, False), "qsx_agg_finalize of a closed state returned only once the stream had drained"
    torch.cuda.synchronize()
    assert_q1_equals(fin, q1_reference(cols), "closed state, read after a synchronize", capacity=65536)


def test_finalize_of_a_growable_state_still_waits_for_the_stream(capi, dev):
    """The event recorded in FRONT of the finalize is the one asked: it is complete when the call returns exactly when the
    call waited for the stream (an event recorded behind the call would race its own recording)."""
    codes, values = three_key_rows(24, groups=300)
    dev_cols = three_key_columns(codes, values, dev)
    st = capi.AggState(small_config(3, est=1024))
    st.update(dev_cols, codes.size)
    st.finalize(dev, capacity=1024)
    st.clear()
    torch.cuda.synchronize()
    enqueue_busy_ms(dev, 20)
    st.update(dev_cols, codes.size)
    before = torch.cuda.Event()
    before.record()
    fin = st.finalize(dev, capacity=1024)
    assert before.query(), "qsx_agg_finalize of a growable state returned with the stream still busy"
    assert_counts_and_sums(fin, 3, codes, values, "growable state")


def test_steps_back_to_back_without_a_host_wait(capi, dev):
    """clear, update, finalize five times with nothing between them: the host runs ahead of the device, and every step's
    outputs are that step's groups — nothing relied on the wait qsx_agg_finalize used to end in."""
    rng = np.random.default_rng(25)
    steps = []
    for step in range(5):
        cols = q1_rows(rng, rng.integers(0, 65536, size=40_000 + 1000 * step) % (200 + 50 * step))
        steps.append((cols, [to_dev(c, dev) for c in cols]))
    st = capi.AggState(q1_config(est=6))
    torch.cuda.synchronize()
    results = []
    for cols, dev_cols in steps:
        st.clear()
        st.update(dev_cols, cols[0].size)
        results.append(st.finalize(dev, capacity=512))
    torch.cuda.synchronize()
    for step, ((cols, _), fin) in enumerate(zip(steps, results)):
        assert_q1_equals(fin, q1_reference(cols), f"step {step}", capacity=512)
