"""Integer aggregate arguments (QSX_EX_IADD .. IDIV, include/qsx.h) on every aggregation path, against Python ints.

The paths, their switches and their proofs are those of test_gpu_agg_exact.py (PATHS); the plans, the data and the reference are
tests/int_expr_reference.py: E1 = SUM / AVG / MIN / MAX(i + j), SUM / AVG(l * 3 + i), COUNT(*) — purely integer — and
E2 = SUM(i * j), MIN / MAX(l * l), SUM(l / k), SUM((i + j) * 0.5), SUM(i), COUNT(*).  No tolerance anywhere: the output dtypes are
the reference's catalog types (int64 SUM, int32 MIN / MAX of an INT expression, int64 of a LONG one, float64 AVG and SUM of the
double node), SUM == the Python-int group sum, MIN / MAX ==, AVG through exact_reference.assert_int_avg and bit for bit equal to
float64(SUM) / COUNT of the same call, the group set and COUNT(*) exact.  After E1 every path runs PLAIN — i + j with QSX_EX_ADD
over the same columns — and wants float64 results equal to the double evaluation: what such a program returned before the integer
instructions existed; under compiled_shape that is the same process, so a shape key that does not tell IADD from ADD fails there."""
import zlib

import numpy as np
import pytest

import exact_reference as R
import int_expr_reference as X
from exact_reference import LAYOUTS
from helpers import bitmap_dev, to_dev
from quickstep_amd import types as T
from test_gpu_agg_exact import NO_JIT, NULLABLE_EDGES, PATHS, _blocks, _counter, _ragged, _two_level, finalize_groups, key_columns

pytestmark = pytest.mark.gpu

PATH_NAMES = ["single_state_1_block", "single_state_30_blocks", "interpreter", "compiled_shape", "compiled_shape_register_groups",
              "lds_flush", "growth_and_spill_log", "midsize_partitioned", "group_directory_on", "group_directory_off", "two_level",
              "collision_free_lds", "collision_free_global", "run_of_ragged_blocks", "nullable_columns", "merge_export_import"]
# the coded case: the switches of PATHS["factored_generic"], which would send a plan that factors through the factored kernels
CODED = dict(layout="few", keys="intchar", strategy=T.AGG_COMPACT_KEY, est=2, mode="coded",
             env={"QSX_AGG_FACTORED_MIN_ROWS": "0", "QSX_AGG_FACTORED_GENERIC": "1"})
CASES = [(p, plan) for p in PATH_NAMES for plan in ("E1", "E2") if not (p == "two_level" and plan == "E2")] + [("coded", "E1"), ("coded", "E2")]
NULLABLE = ("j", "k")


def _valid(live, nulls, a):
    v = live.copy()
    for c in X.OPERANDS[a]:
        if nulls is not None and c in nulls:
            v &= ~nulls[c]
    return v


def check(plan, got, cols, temps, gid, groups, nulls=None):
    """got = (group number of every output row, value columns, NULL flags); gid: -1 = filtered out; nulls: column -> bool array."""
    aggs = X.PLANS[plan]
    got_gid, vals, flags = got
    live = gid >= 0
    cnt = np.bincount(gid[live], minlength=groups)
    present = np.nonzero(cnt)[0]
    assert got_gid.size == present.size and np.array_equal(np.sort(got_gid), present), "groups lost, doubled or invented"
    order = np.argsort(got_gid)
    gg = got_gid[order]
    vals = [np.asarray(v)[order] for v in vals]
    flags = [np.asarray(z)[order].astype(bool) for z in flags]
    assert [str(v.dtype) for v in vals] == X.EXPECTED_DTYPES[plan], "output column types"
    values = dict(temps, i=(cols["i"].astype(np.int64), X.INT))
    if plan == "PLAIN":
        d0 = cols["i"].astype(np.float64) + cols["j"].astype(np.float64)
        assert np.bincount(gid[live], weights=np.abs(d0[live]), minlength=groups).max() < 2**53     # integers: every order the same sum
        values["d0"] = (d0, "double")
    sums = {}
    for j, (fn, a) in enumerate(aggs):
        if fn == "count":
            assert np.array_equal(vals[j], cnt[gg]) and not flags[j].any(), "COUNT(*)"
            continue
        valid = _valid(live, nulls, a)
        x, ty = values[a]
        x, gv = x[valid], gid[valid]
        seen = np.bincount(gv, minlength=groups)[gg]
        null = seen == 0
        assert np.array_equal(flags[j], null), f"NULL flags of {fn}({a})"
        ok = ~null
        assert not np.any(vals[j][null]), f"{fn}({a}) of a NULL group is not zero"
        if fn in ("min", "max"):
            typed = x.astype(np.int32) if ty == X.INT else x
            lo, hi, _ = R.group_min_max(typed, gv, groups)
            want = (lo if fn == "min" else hi)[gg]
            assert vals[j].dtype == want.dtype
            bad = np.nonzero(vals[j][ok] != want[ok])[0]
            assert bad.size == 0, f"{fn}({a}): group {gg[ok][bad[0]]} got {vals[j][ok][bad[0]]!r}, want {want[ok][bad[0]]!r}"
        elif ty == "double":
            want = np.bincount(gv, weights=x, minlength=groups)[gg]
            got_v = vals[j] if fn == "sum" else None
            if fn == "sum":
                bad = np.nonzero(got_v[ok] != want[ok])[0]
                assert bad.size == 0, f"SUM({a}): group {gg[ok][bad[0]]} got {got_v[ok][bad[0]]!r}, exact {want[ok][bad[0]]!r}"
            else:
                bad = np.nonzero(vals[j][ok] != want[ok] / seen[ok])[0]
                assert bad.size == 0, f"AVG({a}) is not the exact sum over the count in {bad.size} groups"
        else:
            s = R.int_group_sums(gv, x, groups)
            for r in np.nonzero(ok)[0]:
                if fn == "sum":
                    assert int(vals[j][r]) == s[gg[r]], f"SUM({a}) of group {gg[r]}: {int(vals[j][r])} != {s[gg[r]]}"
                else:
                    R.assert_int_avg(float(vals[j][r]), s[gg[r]], int(seen[r]))
        if fn == "sum":
            sums[a] = j
    for j, (fn, a) in enumerate(aggs):                 # AVG and SUM of one argument: one accumulator, so bit for bit
        if fn == "avg":
            s = vals[sums[a]]
            c = np.bincount(gid[_valid(live, nulls, a)], minlength=groups)[gg]
            ok = c > 0
            bad = np.nonzero(vals[j][ok] != s[ok].astype(np.float64) / c[ok].astype(np.float64))[0]
            assert bad.size == 0, f"AVG({a}) != SUM({a}) / COUNT in {bad.size} groups, e.g. group {gg[ok][bad[0]]}"


@pytest.mark.parametrize("path,plan", CASES)
def test_integer_aggregate_arguments_on_every_path(capi, oracle, dev, path, plan, monkeypatch):
    spec = CODED if path == "coded" else PATHS[path]
    monkeypatch.setenv("QSX_AGG_JIT_MIN_ROWS", NO_JIT)           # no compiled shape unless the path asks for one
    for k, v in spec.get("env", {}).items():
        monkeypatch.setenv(k, v)
    n, groups, order, heavy = LAYOUTS[spec["layout"]]
    rng = np.random.default_rng(zlib.crc32(f"int_expr/{path}/{plan}".encode()))
    gid = R.make_gids(rng, n, groups, order, heavy)
    if spec.get("mode") == "nullable":
        # the middle block comes without null bitmaps: no row of group 5 (whose j and k are all NULL) may lie in it
        lo, hi = NULLABLE_EDGES[1], NULLABLE_EDGES[2]
        inside = lo + np.nonzero(gid[lo:hi] == 5)[0]
        outside = np.nonzero((gid != 5) & ((np.arange(n) < lo) | (np.arange(n) >= hi)))[0][:inside.size]
        gid[inside], gid[outside] = gid[outside], 5
    cols, temps = X.int_expr_data(rng, gid, groups)
    _run_plan(capi, oracle, dev, spec, path, plan, cols, temps, gid, groups, rng)
    if plan == "E1":
        _run_plan(capi, oracle, dev, spec, path, "PLAIN", cols, temps, gid, groups, rng)


def _run_plan(capi, oracle, dev, spec, path, plan, cols, temps, gid, groups, rng):
    n = gid.size
    mode = spec.get("mode", "blocks")
    klayout, kcols = key_columns(spec["keys"], gid)
    coded = {}
    if mode == "coded":
        # k: six values, a 1-byte dictionary; i: whatever the compressed store would choose for it (often nothing)
        for c in ("k", "i"):
            comp = oracle.CompressedColumn(np.ascontiguousarray(cols[c]))
            if comp.kind != 0:
                coded[c] = comp
        assert "k" in coded and coded["k"].dictionary is not None and coded["k"].code_width == 1
    cfg = X.make_config(plan, klayout, spec["strategy"], est=spec.get("est", 0), num_entries=spec.get("entries", 0),
                        nullable=NULLABLE if mode == "nullable" else (),
                        code_widths={c: comp.code_width for c, comp in coded.items()} if coded else None)
    host = kcols + [cols[c] for c in X.NAMES]
    dcols = [to_dev(np.ascontiguousarray(c), dev) for c in host]
    partitions = spec.get("partitions", 1)
    dense = spec["strategy"] == T.AGG_COLLISION_FREE

    def done(st, g=gid, nulls=None):
        check(plan, finalize_groups(st, dev, spec["keys"], partitions, ascending=dense), cols, temps, g, groups, nulls)

    if mode == "blocks":
        for blocks in np.atleast_1d(spec["blocks"]):
            st = capi.AggState(cfg)
            for a, b in _blocks(n, int(blocks)):
                st.update([c[a:b] for c in dcols], int(b - a))
            if spec.get("proof") == "jit":
                assert capi.lib.qsx_debug_agg_jit_state(st._h, 0) == 1, "not served by a compiled run-time shape"
            done(st)
            st.close()
    elif mode == "ragged":
        st = capi.AggState(cfg)
        st.update_blocks([[c[a:b] for c in dcols] for a, b in _ragged(n)])
        done(st)
        st.close()
    elif mode == "merge":
        half = n // 2 + 17
        a, b, c = capi.AggState(cfg), capi.AggState(cfg), capi.AggState(cfg)
        a.update([x[:half] for x in dcols], half)
        b.update([x[half:] for x in dcols], n - half)
        image = b.export(dev)
        assert image.numel() * 8 == b.export_bytes()
        c.merge(a)
        c.import_merge(image)
        done(c)
    elif mode == "nullable":
        nulls = {c: (rng.random(n) < 0.2) | (gid == 5) for c in NULLABLE}      # group 5: every j and k NULL
        edges = NULLABLE_EDGES + [n]
        assert not np.any(gid[edges[1]:edges[2]] == 5)
        for c in NULLABLE:
            nulls[c][edges[1]:edges[2]] = False                   # the block without bitmaps: nothing NULL in it
        st = capi.AggState(cfg)
        for blk, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
            bms = [None] * len(kcols) + [bitmap_dev(oracle.bitmap_from_bools(nulls[c][a:b]), dev) if c in NULLABLE and blk != 1 else None
                                         for c in X.NAMES]
            st.update_nullable([x[a:b] for x in dcols], bms, int(b - a))
        done(st, nulls=nulls)
        # what group 5 must look like: COUNT(*) counts its rows, everything over j or k is NULL, the rest is not
        keys, vals, flags, found = st.finalize(dev)
        g = int(found.item())
        row = int(np.nonzero(keys[0].cpu().numpy()[:g].astype(np.int64) == 5 * 7 - 3)[0][0])
        for a_, (fn, arg) in enumerate(X.PLANS[plan]):
            over_nullable = arg is not None and any(c in NULLABLE for c in X.OPERANDS[arg])
            assert bool(flags[a_].cpu().numpy()[row]) == over_nullable, (fn, arg)
        assert int(vals[-1].cpu().numpy()[row]) == int(np.sum(gid == 5)) > 0
        st.close()
    elif mode == "coded":
        code_cols = kcols + [coded[c].codes if c in coded else cols[c] for c in X.NAMES]
        dicts = [None] * len(kcols) + [to_dev(coded[c].dictionary, dev) if c in coded and coded[c].dictionary is not None else None
                                       for c in X.NAMES]
        dcode = [to_dev(np.ascontiguousarray(c), dev) for c in code_cols]
        before = _counter(capi, "qsx_debug_agg_factored_launches")
        st = capi.AggState(cfg)
        cut = 131_072 + 5
        for a, b in ((0, cut), (cut, n)):
            st.update_coded([x[a:b] for x in dcode], dicts, b - a, sized=True)
        moved = _counter(capi, "qsx_debug_agg_factored_launches") - before
        if plan != "PLAIN":
            assert moved == 0, f"a plan with integer instructions went through the factored kernels ({moved} launches)"
        done(st)
        st.close()
    else:
        assert mode == "two_level"
        _two_level(capi, oracle, dev, cfg, dcols, done, gid, rng)
