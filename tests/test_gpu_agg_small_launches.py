"""The small launches around an aggregation: what qsx_agg_finalize and qsx_agg_state_clear promise, whatever kernels do it.

- finalize defines every output row: rows below the group count hold the groups (against the exact references of
  test_gpu_agg_exact.py), rows [groups, capacity) of every key, value and NULL column are zero and `groups` is written — with
  the buffers and the `groups` word full of garbage before the call (the raw binding: AggState.finalize allocates its own);
- clear brings a state back to a fresh one: MIN / MAX identities, the group directory, records left in the spill log — by the
  one-kernel clear of small tables and by the memsets above its threshold (QSX_AGG_CLEAR_ONE_KERNEL_WORDS moves it);
- finalize is enqueued before the host waits: a table with records in its spill log is grown, drained and finalized again
  inside the one call.  (The lost-rows error of that call is pinned by test_gpu_agg.py::
  test_lost_rows_are_reported_not_silently_dropped.)"""
import zlib

import numpy as np
import pytest
import torch

import exact_reference as R
from helpers import to_dev
from quickstep_amd import types as T
from test_gpu_agg_exact import PLANS, check, decode_keys, family_data, make_config

pytestmark = pytest.mark.gpu

ROWS, GROUPS = 5_003, 37
# name: keys, strategy, groups, estimate / entries, finalize partitions
STRATEGIES = {
    "single_state": dict(keys="none", strategy=T.AGG_SINGLE_STATE, groups=1, partitions=(1,)),
    "compact_key": dict(keys="int1", strategy=T.AGG_COMPACT_KEY, groups=GROUPS, est=64, partitions=(1,)),
    "generic": dict(keys="int1", strategy=T.AGG_GENERIC, groups=GROUPS, est=64, partitions=(1, 3)),
    "dense": dict(keys="dense", strategy=T.AGG_COLLISION_FREE, groups=GROUPS, entries=GROUPS + 4, partitions=(1, 3)),
}
POISON = 0xAB
_cases = {}


def case(capi, dev, name, family):
    """One state per (strategy, family), updated once and shared by the tests that only finalize it."""
    if (name, family) not in _cases:
        spec = STRATEGIES[name]
        plan = {"A": "A", "D": "D"}[family]
        rng = np.random.default_rng(zlib.crc32(f"{name}/{family}".encode()))
        gid = R.make_gids(rng, ROWS, spec["groups"])
        cols = family_data(family, plan, rng, gid, spec["groups"])
        cfg, kcols = make_config(plan, spec["keys"], gid, spec["strategy"], est=spec.get("est", 0), num_entries=spec.get("entries", 0))
        st = capi.AggState(cfg)
        st.update([to_dev(c, dev) for c in kcols + [cols[c] for c in PLANS[plan][0]]], ROWS)
        _cases[(name, family)] = (st, cfg, plan, cols, gid)
    return _cases[(name, family)]


def raw_finalize(capi, st, dev, capacity, partition=0, partitions=1):
    """qsx_agg_finalize into buffers of `capacity` rows that hold 0xAB bytes, with a `groups` word that holds garbage."""
    cfg = st.config

    def poisoned(dtype):
        width = torch.empty(0, dtype=dtype).element_size()
        return torch.full((capacity * width,), POISON, dtype=torch.uint8, device=dev).view(dtype)
    keys = [poisoned({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[cfg.column_width[cfg.key_column[k]]])
            for k in range(cfg.num_keys)]
    vals = [poisoned(getattr(torch, T.agg_output_dtype(cfg, a))) for a in range(cfg.num_aggs)]
    nulls = [poisoned(torch.uint8) for _ in range(cfg.num_aggs)]
    groups = torch.full((1,), 0x2BABABABABABABAB, dtype=torch.int64, device=dev)
    capi._check(capi.lib.qsx_agg_finalize(st._h, partition, partitions, capi._ptr_array(keys), capi._ptr_array(vals), capi._ptr_array(nulls),
                                          capacity, capi._ptr(groups), capi._stream(None)), "qsx_agg_finalize")
    return [k.cpu().numpy() for k in keys], [v.cpu().numpy() for v in vals], [z.cpu().numpy() for z in nulls], int(groups.item())


def assert_tail_is_zero(keys, vals, nulls, g, what):
    for kind, columns in (("key", keys), ("value", vals), ("null", nulls)):
        for j, c in enumerate(columns):
            tail = c[g:].view(np.uint8)
            assert not tail.any(), f"{what}: {kind} column {j} is not zero behind its {g} groups ({np.count_nonzero(tail)} bytes set)"


@pytest.mark.parametrize("family", ["A", "D"])
@pytest.mark.parametrize("name,partitions", [(n, p) for n, spec in STRATEGIES.items() for p in spec["partitions"]])
def test_finalize_defines_every_output_row(capi, dev, name, partitions, family):
    st, cfg, plan, cols, gid = case(capi, dev, name, family)
    spec = STRATEGIES[name]
    total = spec["groups"]
    # the groups of every partition, from a finalize with room to spare
    per_partition = [raw_finalize(capi, st, dev, 4 * total + 7, p, partitions)[3] for p in range(partitions)]
    assert sum(per_partition) == total and all(g > 0 for g in per_partition), per_partition
    for slack in ("g", "g + 1", "4 g + 7"):
        parts = []
        for p, g in enumerate(per_partition):
            capacity = {"g": g, "g + 1": g + 1, "4 g + 7": 4 * g + 7}[slack]
            keys, vals, nulls, found = raw_finalize(capi, st, dev, capacity, p, partitions)
            what = f"{name}, partition {p} of {partitions}, capacity {slack} = {capacity}"
            assert found == g, f"{what}: groups = {found}, want {g}"
            assert_tail_is_zero(keys, vals, nulls, g, what)
            parts.append((decode_keys(spec["keys"], [k[:g] for k in keys], g), [v[:g] for v in vals], [z[:g] for z in nulls]))
        got = (np.concatenate([p[0] for p in parts]), [np.concatenate(c) for c in zip(*[p[1] for p in parts])],
               [np.concatenate(c) for c in zip(*[p[2] for p in parts])])
        check(plan, family, got, cols, gid, total)


@pytest.mark.parametrize("name", ["compact_key", "generic", "dense"])
def test_finalize_into_less_room_than_groups(capi, dev, name):
    """As before: `groups` is the number of groups found, the rows that fit are groups of the state, nothing lies beyond."""
    st, cfg, plan, cols, gid = case(capi, dev, name, "A")
    spec = STRATEGIES[name]
    g = spec["groups"]
    fk, fv, fz, found = raw_finalize(capi, st, dev, g)
    assert found == g
    full_gid = decode_keys(spec["keys"], fk, g)
    by_gid = {int(x): r for r, x in enumerate(full_gid)}
    keys, vals, nulls, found = raw_finalize(capi, st, dev, g - 5)
    assert found == g
    some = decode_keys(spec["keys"], keys, g - 5)
    assert np.unique(some).size == g - 5
    rows = np.array([by_gid[int(x)] for x in some])
    for a in range(cfg.num_aggs):
        assert np.array_equal(vals[a].view(np.uint8), fv[a][rows].view(np.uint8)) and np.array_equal(nulls[a], fz[a][rows])


# ---- clear ----------------------------------------------------------------------------------------------------------------------
SPILL_GROUPS = 5_000
CLEARED = {
    # MIN and MAX aggregates (identities that are not zero), a group count that is not zero
    "min_max": dict(plan="D", family="D", keys="int1", strategy=T.AGG_GENERIC, est=64, groups=GROUPS, rows=ROWS, env={}),
    # a state with a group directory (csrc/aggregate.hip derive_geometry: this estimate asks for one)
    "directory": dict(plan="A", family="A", keys="int2", strategy=T.AGG_GENERIC, est=10_000, groups=900, rows=6_001,
                      env={"QSX_AGG_DIRECTORY": "1"}),
    # a 2048-slot table fed 5 000 distinct groups in one update: most of them lie in the spill log
    "spill_log": dict(plan="A", family="A", keys="int1", strategy=T.AGG_COMPACT_KEY, est=1, groups=SPILL_GROUPS, rows=2 * SPILL_GROUPS + 1, env={}),
}
ONE_KERNEL, MEMSETS = str(1 << 40), "0"


def cleared_case(kind, salt):
    spec = CLEARED[kind]
    rng = np.random.default_rng(zlib.crc32(f"clear/{kind}/{salt}".encode()))
    gid = R.make_gids(rng, spec["rows"], spec["groups"])
    cols = family_data(spec["family"], spec["plan"], rng, gid, spec["groups"])
    cfg, kcols = make_config(spec["plan"], spec["keys"], gid, spec["strategy"], est=spec["est"])
    return cfg, kcols + [cols[c] for c in PLANS[spec["plan"]][0]], cols, gid


def in_group_order(spec, fin):
    keys, vals, nulls, groups = fin
    g = int(groups.item())
    got = decode_keys(spec["keys"], [k.cpu().numpy()[:g] for k in keys], g)
    order = np.argsort(got)
    return got[order], [v.cpu().numpy()[:g][order] for v in vals], [z.cpu().numpy()[:g][order] for z in nulls]


@pytest.mark.parametrize("threshold", [None, ONE_KERNEL, MEMSETS], ids=["default", "one_kernel", "memsets"])
@pytest.mark.parametrize("kind", list(CLEARED))
def test_cleared_state_equals_a_fresh_one(capi, dev, kind, threshold, monkeypatch):
    spec = CLEARED[kind]
    monkeypatch.setenv("QSX_AGG_JIT_MIN_ROWS", str(1 << 60))
    for k, v in spec["env"].items():
        monkeypatch.setenv(k, v)
    if threshold is not None:
        monkeypatch.setenv("QSX_AGG_CLEAR_ONE_KERNEL_WORDS", threshold)
    cfg, first, _, _ = cleared_case(kind, "first")
    _, second, cols, gid = cleared_case(kind, "second")
    capacity = 2 * spec["groups"]
    used = capi.AggState(cfg)
    used.update([to_dev(c, dev) for c in first], spec["rows"])
    used.clear()
    used.update([to_dev(c, dev) for c in second], spec["rows"])
    fresh = capi.AggState(cfg)
    fresh.update([to_dev(c, dev) for c in second], spec["rows"])
    got, want = in_group_order(spec, used.finalize(dev, capacity=capacity)), in_group_order(spec, fresh.finalize(dev, capacity=capacity))
    assert np.array_equal(got[0], want[0]), "the cleared state holds other groups than a fresh one"
    for a in range(cfg.num_aggs):
        assert np.array_equal(got[1][a].view(np.uint8), want[1][a].view(np.uint8)), f"aggregate {a} differs from a fresh state's"
        assert np.array_equal(got[2][a], want[2][a]), f"NULL flags of aggregate {a} differ from a fresh state's"
    check(spec["plan"], spec["family"], got, cols, gid, spec["groups"])
    # ... and a state cleared twice in a row, or cleared while empty, is empty
    used.clear()
    used.clear()
    assert int(used.finalize(dev, capacity=4)[3].item()) == 0


# ---- finalize before the wait ---------------------------------------------------------------------------------------------------
def test_finalize_grows_drains_and_runs_again(capi, dev, monkeypatch):
    """No update, num_groups or export between the spilling update and the finalize: the call itself finds the records in the
    log behind its first kernel, grows the table, drains the log and finalizes the grown table."""
    monkeypatch.setenv("QSX_AGG_JIT_MIN_ROWS", str(1 << 60))
    spec = CLEARED["spill_log"]
    cfg, host, cols, gid = cleared_case("spill_log", "direct")
    st = capi.AggState(cfg)
    st.update([to_dev(c, dev) for c in host], spec["rows"])
    capacity = SPILL_GROUPS + 9
    keys, vals, nulls, found = raw_finalize(capi, st, dev, capacity)
    assert found == SPILL_GROUPS
    assert_tail_is_zero(keys, vals, nulls, found, "spilled state")
    got = (decode_keys(spec["keys"], [k[:found] for k in keys], found), [v[:found] for v in vals], [z[:found] for z in nulls])
    check(spec["plan"], spec["family"], got, cols, gid, SPILL_GROUPS)
    assert st.num_groups() == SPILL_GROUPS + 1          # (+ the sentinel slot) the table is at rest now: nothing left to drain
