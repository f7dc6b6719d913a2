"""Every aggregation path against exact references (tests/exact_reference.py), not against a 1e-6 tolerance.

One qsx_agg_* call can be answered by the single state, the ahead-of-time plan shapes and family, the interpreter, a compiled
run-time shape, register groups, an LDS table that flushes, the global table with its spill log, the partitioned paths, the group
directory, the two-level pieces, the dense states and the factored path over dictionary codes.  Each case below forces one of
them with the per-call switches the other tests use, proves it ran where the library has a counter, and compares:

- family A (multiples of 2^-e whose group sums every order gives bit for bit): SUM equal to np.bincount exactly;
- the subnormal variant of A: the same, with DOUBLE and FLOAT subnormals;
- family B (TPC-H-like decimals): SUM within tol_g = 2 gamma(2 n_g + k) S_g, itself below the smallest term of the group;
- family C (INT / LONG sums past 2^32 and 2^53): SUM equal to Python ints, AVG equal to the rounded Fraction;
- family D (MIN / MAX at the types' extremes and accumulator identities): == per group;

and on every case COUNT exactly, AVG(x) bit for bit equal to float64(SUM(x)) / COUNT of the same call (they share one
accumulator, agg_translate.hpp), and the NULL flags.  Only dictionary codes come from the oracle (CompressedColumn); it is never
the reference of an assertion here."""
import ctypes
import zlib

import numpy as np
import pytest

import exact_reference as R
from exact_reference import LAYOUTS
from helpers import bitmap_dev, to_dev
from quickstep_amd import types as T

pytestmark = pytest.mark.gpu

NO_JIT = str(1 << 60)


# ---- group-by keys: made from the group number of a row, and read back from finalize ------------------------------------------
def key_columns(kind, gid):
    if kind == "none":
        return [], []
    if kind == "char2":                                                       # Q1's (l_returnflag, l_linestatus)
        assert gid.max() < 4
        return [(T.CHAR, 1), (T.CHAR, 1)], [np.frombuffer(b"ANNR", np.uint8)[gid], np.frombuffer(b"FFOF", np.uint8)[gid]]
    if kind == "int1":
        return [(T.INT, None)], [(gid * 7 - 3).astype(np.int32)]
    if kind == "int2":
        return [(T.INT, None), (T.INT, None)], [(gid % 97 - 40).astype(np.int32), (gid // 97 * 3 + 1).astype(np.int32)]
    if kind == "intchar":
        return [(T.INT, None), (T.CHAR, 1)], [(gid // 2 * 5 - 1).astype(np.int32), np.frombuffer(b"FO", np.uint8)[gid % 2]]
    assert kind == "dense"
    return [(T.INT, None)], [gid.astype(np.int32)]


def decode_keys(kind, keys, rows):
    if kind == "none":
        return np.zeros(rows, dtype=np.int64)
    k = [np.asarray(x).astype(np.int64) for x in keys]
    if kind == "char2":
        table = {(ord("A"), ord("F")): 0, (ord("N"), ord("F")): 1, (ord("N"), ord("O")): 2, (ord("R"), ord("F")): 3}
        return np.array([table[(a, b)] for a, b in zip(k[0], k[1])], dtype=np.int64)
    if kind == "int1":
        assert np.all((k[0] + 3) % 7 == 0)
        return (k[0] + 3) // 7
    if kind == "int2":
        assert np.all((k[1] - 1) % 3 == 0)
        return (k[1] - 1) // 3 * 97 + k[0] + 40
    if kind == "intchar":
        assert np.all((k[0] + 1) % 5 == 0) and np.all((k[1] == ord("F")) | (k[1] == ord("O")))
        return (k[0] + 1) // 5 * 2 + (k[1] == ord("O"))
    return k[0]


# ---- plans: value columns by name, aggregates over them ------------------------------------------------------------------------
TYPES = {"qty": T.DOUBLE, "price": T.DOUBLE, "disc": T.DOUBLE, "tax": T.DOUBLE, "fl": T.FLOAT, "sd": T.DOUBLE, "sf": T.FLOAT,
         "i": T.INT, "l": T.LONG, "d": T.DOUBLE, "f": T.FLOAT}
Q1_AGGS = [("sum", "qty"), ("sum", "price"), ("sum", "t1"), ("sum", "t3"), ("avg", "qty"), ("avg", "price"), ("avg", "disc"),
           ("count", None)]
PLANS = {
    "Q1": (["qty", "price", "disc", "tax"], Q1_AGGS),                  # with char2 keys: exactly test_gpu_agg.q1_config()
    "A": (["qty", "price", "disc", "tax", "fl"], [("sum", "qty"), ("sum", "price"), ("sum", "t1"), ("sum", "t3"), ("avg", "price"),
                                                  ("sum", "fl"), ("avg", "disc"), ("count", None)]),
    "A_no_float": (["qty", "price", "disc", "tax"], [("sum", "qty"), ("sum", "price"), ("sum", "t1"), ("sum", "t3"), ("avg", "price"),
                                                     ("avg", "disc"), ("count", None)]),
    "A_doubles": (["qty", "price", "disc"], [("sum", "qty"), ("sum", "price"), ("avg", "price"), ("sum", "disc"), ("count", None)]),
    "B": (["qty", "price", "disc", "tax"], [("sum", "qty"), ("sum", "price"), ("sum", "t1"), ("sum", "t3"), ("avg", "price"),
                                            ("avg", "disc"), ("sum", "disc"), ("count", None)]),
    "SHAPE2": (["price"], [("sum", "price"), ("count", None), ("avg", "price")]),   # with int2 keys: the two-INT-key AOT shape
    "SHAPE2_SUB": (["sd"], [("sum", "sd"), ("count", None), ("avg", "sd")]),
    "SUB": (["sd", "sf"], [("sum", "sd"), ("avg", "sd"), ("sum", "sf"), ("count", None)]),
    "SUB_doubles": (["sd"], [("sum", "sd"), ("avg", "sd"), ("count", None)]),
    "SUB_coded": (["disc", "sd", "sf"], [("sum", "sd"), ("avg", "sd"), ("sum", "sf"), ("sum", "disc"), ("count", None)]),
    "C": (["i", "l"], [("sum", "i"), ("avg", "i"), ("sum", "l"), ("avg", "l"), ("count", None)]),
    "C_coded": (["disc", "i", "l"], [("sum", "i"), ("avg", "i"), ("sum", "l"), ("avg", "l"), ("sum", "disc"), ("count", None)]),
    "D": (["l", "d", "i"], [("count", None), ("min", "l"), ("max", "l"), ("min", "d"), ("max", "d"), ("min", "i"), ("max", "i")]),
    "D_float": (["f"], [("count", None), ("min", "f"), ("max", "f")]),
    # nullable arguments: every distinct NULL mask takes a counting accumulator of its own, and a state has kMaxSums of them
    # (translate_config in agg_translate.hpp refuses more): A and D split into plans that fit
    "A_nullable": (["price", "disc", "tax", "fl"], [("sum", "price"), ("avg", "price"), ("sum", "t1"), ("sum", "fl"), ("count", None)]),
    "D_nullable_long_double": (["l", "d"], [("count", None), ("min", "l"), ("max", "l"), ("min", "d"), ("max", "d")]),
    "D_nullable_int_float": (["i", "f"], [("count", None), ("min", "i"), ("max", "i"), ("min", "f"), ("max", "f")]),
}
OPERANDS = {"t1": ("price", "disc"), "t3": ("price", "disc", "tax")}     # columns an expression node reads
FN = {"sum": T.AGG_SUM, "avg": T.AGG_AVG, "min": T.AGG_MIN, "max": T.AGG_MAX, "count": T.AGG_COUNT_STAR}


def make_config(plan, key_kind, gid, strategy, est=0, num_entries=0, nullable=False, code_widths=None):
    names, aggs = PLANS[plan]
    klayout, kcols = key_columns(key_kind, gid)
    idx = {c: len(klayout) + j for j, c in enumerate(names)}
    instrs, consts = [], []
    if any(a in ("t1", "t3") for _, a in aggs):                                 # t0 = 1 - disc; t1 = price t0; t2 = 1 + tax; t3 = t1 t2
        instrs = [(T.EX_SUB, 0, T.const(0), T.col(idx["disc"])), (T.EX_MUL, 1, T.col(idx["price"]), T.temp(0)),
                  (T.EX_ADD, 2, T.const(0), T.col(idx["tax"])), (T.EX_MUL, 3, T.temp(1), T.temp(2))]
        consts = [1.0]

    def operand(a):
        return None if a is None else T.temp(1) if a == "t1" else T.temp(3) if a == "t3" else T.col(idx[a])
    widths = None if code_widths is None else [0] * len(klayout) + [code_widths.get(c, 0) for c in names]
    cfg = T.make_agg_config(strategy, klayout + [(TYPES[c], None) for c in names], keys=list(range(len(klayout))), instrs=instrs,
                            consts=consts, aggs=[(FN[f], operand(a)) for f, a in aggs], est_groups=est, num_entries=num_entries,
                            code_widths=widths, nullable=[idx[c] for c in names] if nullable else ())
    return cfg, kcols


# ---- the reference and the comparison -------------------------------------------------------------------------------------------
def check(plan, family, got, cols, gid, groups, nulls=None):
    """got = (group number of every output row, value columns, NULL flags); gid: group of every input row, -1 = filtered out;
    nulls: column name -> bool array (True = NULL)."""
    names, aggs = PLANS[plan]
    got_gid, vals, flags = got
    live = gid >= 0
    cnt = np.bincount(gid[live], minlength=groups)
    present = np.nonzero(cnt)[0]
    assert got_gid.size == present.size and np.array_equal(np.sort(got_gid), present), "groups lost, doubled or invented"
    order = np.argsort(got_gid)
    gg = got_gid[order]
    vals = [np.asarray(v)[order] for v in vals]
    flags = [np.asarray(z)[order].astype(bool) for z in flags]
    for j, (fn, a) in enumerate(aggs):                 # COUNT(*) first: every other check divides by it
        if fn == "count":
            assert vals[j].dtype == np.int64 and np.array_equal(vals[j], cnt[gg]), "COUNT(*)"
            assert not flags[j].any()
    sums = {}
    for j, (fn, a) in enumerate(aggs):
        if fn == "count":
            continue
        valid = _valid(live, nulls, a)
        x, gv = cols[a][valid], gid[valid]
        seen = np.bincount(gv, minlength=groups)[gg]
        null = seen == 0
        assert np.array_equal(flags[j], null), f"NULL flags of {fn}({a})"
        ok = ~null
        if fn in ("min", "max"):
            lo, hi, _ = R.group_min_max(x, gv, groups)
            want = (lo if fn == "min" else hi)[gg]
            assert vals[j].dtype == want.dtype
            bad = np.nonzero(vals[j][ok] != want[ok])[0]                     # == : the sign of a zero is not pinned
            assert bad.size == 0, f"{fn}({a}): group {gg[ok][bad[0]]} got {vals[j][ok][bad[0]]!r}, want {want[ok][bad[0]]!r}"
            continue
        if np.issubdtype(x.dtype, np.integer):
            s = R.int_group_sums(gv, x.astype(np.int64), groups)
            if fn == "sum":
                assert vals[j].dtype == np.int64
                for r in np.nonzero(ok)[0]:
                    assert int(vals[j][r]) == s[gg[r]], f"SUM({a}) of group {gg[r]}: {int(vals[j][r])} != {s[gg[r]]}"
            else:
                for r in np.nonzero(ok)[0]:
                    R.assert_int_avg(float(vals[j][r]), s[gg[r]], int(seen[r]))
        elif family == "B":
            k = R.FAMILY_B_ROUNDINGS[a]
            ref = R.family_b_reference(x, gv, groups)[gg]
            tol = R.family_b_tolerance(x, gv, groups, k)[gg]
            if fn == "sum":
                err = np.abs(vals[j] - ref)
                assert np.all(err[ok] <= tol[ok]), f"SUM({a}): error {err[ok].max()} beyond tol_g"
            else:
                c = np.maximum(seen, 1).astype(np.float64)
                err = np.abs(vals[j] - ref / c)
                assert np.all(err[ok] <= (tol / c + 2 * R.U * np.abs(ref / c))[ok]), f"AVG({a})"
        else:
            want = R.exact_group_sums(x, gv, groups)[gg]
            if fn == "sum":
                bad = np.nonzero(vals[j][ok] != want[ok])[0]
                assert bad.size == 0, f"SUM({a}): group {gg[ok][bad[0]]} got {vals[j][ok][bad[0]]!r}, exact {want[ok][bad[0]]!r}"
            else:
                bad = np.nonzero(vals[j][ok] != want[ok] / seen[ok])[0]
                assert bad.size == 0, (f"AVG({a}) of {bad.size} groups is not the exact sum over the count, e.g. group {gg[ok][bad[0]]}: "
                                       f"{vals[j][ok][bad[0]].hex()} != {want[ok][bad[0]].hex()} / {seen[ok][bad[0]]}")
        if fn == "sum":
            sums[a] = j
        assert not np.any(vals[j][null]), f"{fn}({a}) of a NULL group is not zero"
    for j, (fn, a) in enumerate(aggs):                 # AVG and SUM of one argument: one accumulator, so bit for bit
        if fn == "avg" and a in sums:
            s = vals[sums[a]]
            c = np.bincount(gid[_valid(live, nulls, a)], minlength=groups)[gg]
            ok = c > 0
            bad = np.nonzero(vals[j][ok] != s[ok].astype(np.float64) / c[ok].astype(np.float64))[0]
            assert bad.size == 0, f"AVG({a}) != SUM({a}) / COUNT in {bad.size} groups, e.g. group {gg[ok][bad[0]]}"


def _valid(live, nulls, a):
    """Rows that reach an aggregate over `a`: not filtered out, no operand NULL."""
    v = live.copy()
    for c in OPERANDS.get(a, (a,)):
        if nulls is not None and c in nulls:
            v &= ~nulls[c]
    return v


def finalize_groups(st, dev, key_kind, partitions=1, ascending=False):
    """Every group of the state as (group numbers, values, NULL flags), over `partitions` finalize calls."""
    out = None
    cap = max(st.num_groups(), 1)
    for p in range(partitions):
        keys, vals, nulls, groups = st.finalize(dev, p, partitions, capacity=cap)
        g = int(groups.item())
        assert 0 <= g <= cap
        part = (decode_keys(key_kind, [k.cpu().numpy()[:g] for k in keys], g), [v.cpu().numpy()[:g] for v in vals],
                [z.cpu().numpy()[:g] for z in nulls])
        if ascending:
            assert np.all(np.diff(part[0]) > 0), "a range partition of a dense state is not in ascending key order"
            if out is not None and g and out[0].size:
                assert part[0][0] > out[0][-1]
        out = part if out is None else (np.concatenate([out[0], part[0]]), [np.concatenate([a, b]) for a, b in zip(out[1], part[1])],
                                        [np.concatenate([a, b]) for a, b in zip(out[2], part[2])])
    return out


# ---- family data ----------------------------------------------------------------------------------------------------------------
def family_data(family, plan, rng, gid, groups):
    if family == "A":
        return R.family_a(rng, gid, groups)
    if family == "B":
        return R.family_b(rng, gid, groups)
    if family == "SUB":
        cols = R.family_a_subnormal(rng, gid, groups)
        if plan in ("Q1", "SUB_coded", "C_coded"):
            # Q1's columns: qty and price subnormal, disc = tax = 0 (so that t1 = t3 = price exactly); a coded plan: A's disc
            other = R.family_a_subnormal(rng, gid, groups)
            cols.update(qty=cols["sd"], price=other["sd"], disc=np.zeros(gid.size), tax=np.zeros(gid.size))
            if plan != "Q1":
                cols["disc"] = R.family_a(rng, gid, groups)["disc"]
            cols.update(R.q1_terms(cols))
        assert R.subnormal_groups_with_normal_sums(cols, gid, groups).size > 0 or np.bincount(gid).max() < 8192
        return cols
    if family == "C":
        cols = R.family_c(rng, gid, groups)
        if groups > 1:
            R.assert_family_c_ranges(cols, gid, groups)
        if plan == "C_coded":
            cols["disc"] = R.family_a(rng, gid, groups)["disc"]
        return cols
    assert family == "D"
    return R.family_d(rng, gid, groups)


# ---- the paths ------------------------------------------------------------------------------------------------------------------
def _counter(capi, name):
    fn = getattr(capi.lib, name)
    fn.restype = ctypes.c_longlong
    return fn()


STD = {"A": ["A"], "SUB": ["SUB"], "B": ["B"], "C": ["C"], "D": ["D", "D_float"]}
DOUBLES = {"A": ["A_doubles"], "SUB": ["SUB_doubles"], "B": ["A_doubles"]}
PATHS = {
    # name: layout, keys, strategy, environment, plans per family, how rows arrive, proof that the path ran
    "single_state_1_block": dict(layout="single", keys="none", strategy=T.AGG_SINGLE_STATE, plans=STD, blocks=1),
    "single_state_30_blocks": dict(layout="single", keys="none", strategy=T.AGG_SINGLE_STATE, plans=STD, blocks=30),
    "q1_fixed_shape": dict(layout="q1", keys="char2", strategy=T.AGG_COMPACT_KEY, est=6, blocks=3, proof="shape",
                           plans={"A": ["Q1"], "SUB": ["Q1"], "B": ["Q1"]}),
    "q1_fixed_shape_register_groups": dict(layout="q1", keys="char2", strategy=T.AGG_COMPACT_KEY, est=6, blocks=3, proof="shape",
                                           env={"QSX_AGG_REG_GROUPS": "1"}, plans={"A": ["Q1"], "SUB": ["Q1"], "B": ["Q1"]}),
    "q1_fixed_shape_run_of_blocks": dict(layout="q1", keys="char2", strategy=T.AGG_COMPACT_KEY, est=6, mode="ragged", proof="shape",
                                         plans={"A": ["Q1"], "SUB": ["Q1"]}),
    "two_int_key_shape": dict(layout="few", keys="int2", strategy=T.AGG_COMPACT_KEY, est=64, blocks=2, proof="shape",
                              plans={"A": ["SHAPE2"], "SUB": ["SHAPE2_SUB"], "B": ["SHAPE2"]}),
    "aot_family_compact_two_keys": dict(layout="few", keys="intchar", strategy=T.AGG_COMPACT_KEY, est=64, blocks=2, proof="family",
                                        env={"QSX_AGG_JIT": "0"}, plans=DOUBLES),
    "aot_family_generic_one_key": dict(layout="few", keys="int1", strategy=T.AGG_GENERIC, est=64, blocks=2, proof="family",
                                       env={"QSX_AGG_JIT": "0"}, plans=DOUBLES),
    "interpreter": dict(layout="few", keys="int1", strategy=T.AGG_GENERIC, est=64, blocks=2, env={"QSX_AGG_NO_SPECIALIZE": "1"},
                        plans=STD),
    "compiled_shape": dict(layout="few", keys="int1", strategy=T.AGG_GENERIC, est=64, blocks=2, proof="jit",
                           env={"QSX_AGG_JIT_MIN_ROWS": "0"}, plans={f: STD[f] for f in ("A", "SUB", "C", "D")}),
    "compiled_shape_register_groups": dict(layout="five", keys="int1", strategy=T.AGG_COMPACT_KEY, est=8, blocks=2, proof="jit",
                                           env={"QSX_AGG_JIT_MIN_ROWS": "0", "QSX_AGG_REG_GROUPS": "1"},
                                           plans={f: STD[f] for f in ("A", "SUB", "C", "D")}),
    "lds_flush": dict(layout="lds_flush", keys="int1", strategy=T.AGG_GENERIC, est=100_000, blocks=1, plans=STD),
    "growth_and_spill_log": dict(layout="growth", keys="int1", strategy=T.AGG_COMPACT_KEY, est=4, blocks=(1, 7),
                                 plans={f: STD[f] for f in ("A", "SUB", "C", "D")}),
    "midsize_partitioned": dict(layout="midsize", keys="int2", strategy=T.AGG_COMPACT_KEY, est=3_000, blocks=3, partitions=7,
                                env={"QSX_AGG_PARTITION_MIN_ROWS": "0"}, plans={f: STD[f] for f in ("A", "SUB", "C", "D")}),
    "group_directory_on": dict(layout="directory", keys="int2", strategy=T.AGG_GENERIC, est=10_000, blocks=1,
                               env={"QSX_AGG_DIRECTORY": "1", "QSX_AGG_PARTITION_MIN_ROWS": "100000"},
                               plans={f: STD[f] for f in ("A", "SUB", "C", "D")}),
    "group_directory_off": dict(layout="directory", keys="int2", strategy=T.AGG_GENERIC, est=10_000, blocks=1,
                                env={"QSX_AGG_DIRECTORY": "0", "QSX_AGG_PARTITION_MIN_ROWS": "100000"},
                                plans={f: STD[f] for f in ("A", "SUB", "C", "D")}),
    # two_level_plan (aggregate.hip) takes SUM over DOUBLE / INT / LONG and MIN / MAX over DOUBLE / INT / LONG only: no FLOAT
    # argument, so A without its FLOAT column, the subnormal DOUBLEs alone and D without its FLOAT plan
    "two_level": dict(layout="two_level", keys="int1", strategy=T.AGG_GENERIC, est=120_000, mode="two_level",
                      env={"QSX_AGG_PARTITION_MIN_ROWS": "100000", "QSX_AGG_TWO_LEVEL_MIN_GROUPS": "100000"},
                      plans={"A": ["A_no_float"], "SUB": ["SUB_doubles"], "B": ["B"], "C": ["C"], "D": ["D"]}),
    "collision_free_lds": dict(layout="dense", keys="dense", strategy=T.AGG_COLLISION_FREE, entries=5_000, blocks=4, partitions=3,
                               env={"QSX_AGG_DENSE_LDS": "1"}, plans={f: STD[f] for f in ("A", "SUB", "C", "D")}),
    "collision_free_global": dict(layout="dense", keys="dense", strategy=T.AGG_COLLISION_FREE, entries=5_000, blocks=4, partitions=3,
                                  env={"QSX_AGG_DENSE_LDS": "0"}, plans={f: STD[f] for f in ("A", "SUB", "C", "D")}),
    # MIN / MAX do not factor (the "minmax" plan of test_gpu_compressed.py is answered by the decoding kernels): no family D
    "factored_direct": dict(layout="q1_small", keys="char2", strategy=T.AGG_COMPACT_KEY, est=6, mode="coded", proof="factored",
                            coded=("qty", "disc", "tax"), env={"QSX_AGG_FACTORED_MIN_ROWS": "0"}, plans={"A": ["Q1"], "B": ["Q1"]}),
    # (est = 2: the workgroup's table takes a handful of groups, the rows of the others take the per-row path; a larger table
    # leaves factored_plan in aggregate.hip)
    "factored_generic": dict(layout="few", keys="intchar", strategy=T.AGG_COMPACT_KEY, est=2, mode="coded", proof="factored",
                             coded=("qty", "disc", "tax"), env={"QSX_AGG_FACTORED_MIN_ROWS": "0", "QSX_AGG_FACTORED_GENERIC": "1"},
                             plans={"A": ["Q1"], "B": ["Q1"], "SUB": ["SUB_coded"], "C": ["C_coded"]}),
    "factored_unsized_calls": dict(layout="q1_small", keys="char2", strategy=T.AGG_COMPACT_KEY, est=6, mode="coded_unsized",
                                   proof="not_factored", coded=("qty", "disc", "tax"), env={"QSX_AGG_FACTORED_MIN_ROWS": "0"},
                                   plans={"A": ["Q1"], "B": ["Q1"]}),
    "run_of_ragged_blocks": dict(layout="few", keys="int1", strategy=T.AGG_GENERIC, est=64, mode="ragged",
                                 plans={f: STD[f] for f in ("A", "SUB", "C", "D")}),
    "nullable_columns": dict(layout="few", keys="int1", strategy=T.AGG_GENERIC, est=64, mode="nullable",
                             plans={"A": ["A_nullable"], "SUB": ["SUB"], "C": ["C"], "D": ["D_nullable_long_double", "D_nullable_int_float"]}),
    "merge_export_import": dict(layout="few", keys="int1", strategy=T.AGG_GENERIC, est=64, mode="merge",
                                plans={f: STD[f] for f in ("A", "SUB", "C", "D")}),
}
CASES = [(p, f) for p, spec in PATHS.items() for f in ("A", "SUB", "B", "C", "D") if f in spec["plans"]]


NULLABLE_EDGES = [0, 100_032, 200_064]         # block starts of the nullable path (bitmaps are sliced by 64-row word)


def _blocks(n, k):
    edges = np.linspace(0, n, k + 1).astype(np.int64)
    return list(zip(edges[:-1], edges[1:]))


def _ragged(n):
    sizes = [0, 1, 1023, 1025, 70_001, 0, 333, 100_000]
    sizes.append(n - sum(sizes))
    edges = np.concatenate([[0], np.cumsum(sizes)])
    return list(zip(edges[:-1], edges[1:]))


@pytest.mark.parametrize("path,family", CASES)
def test_aggregation_path_against_exact_reference(capi, oracle, dev, path, family, monkeypatch, capfd):
    spec = PATHS[path]
    monkeypatch.setenv("QSX_AGG_JIT_MIN_ROWS", NO_JIT)           # no compiled shape unless the path asks for one
    for k, v in spec.get("env", {}).items():
        monkeypatch.setenv(k, v)
    if spec.get("proof") == "shape":
        monkeypatch.setenv("QSX_DEBUG_LAUNCH", "1")
    n, groups, order, heavy = LAYOUTS[spec["layout"]]
    rng = np.random.default_rng(zlib.crc32(f"{path}/{family}".encode()))
    gid = R.make_gids(rng, n, groups, order, heavy)
    if spec.get("mode") == "nullable":
        # the middle block comes without null bitmaps: no row of group 5 (whose arguments are all NULL) may lie in it
        lo, hi = NULLABLE_EDGES[1], NULLABLE_EDGES[2]
        inside = lo + np.nonzero(gid[lo:hi] == 5)[0]
        outside = np.nonzero((gid != 5) & ((np.arange(n) < lo) | (np.arange(n) >= hi)))[0][:inside.size]
        gid[inside], gid[outside] = gid[outside], 5
    for plan in spec["plans"][family]:
        cols = family_data(family, plan, rng, gid, groups)
        _run_plan(capi, oracle, dev, spec, path, plan, family, cols, gid, groups, rng, capfd)
    if path.startswith("single_state") and family == "D":
        # a single state whose every row is one accumulator identity (INT64_MAX / INT64_MIN, +-inf): that value, not NULL
        small = np.zeros(3, dtype=np.int64)
        for which in range(4):
            for plan in spec["plans"]["D"]:
                cols = R.family_d(rng, small, 1, identity_only=which)
                _run_plan(capi, oracle, dev, dict(spec, blocks=1), path, plan, family, cols, small, 1, rng, capfd)


def _run_plan(capi, oracle, dev, spec, path, plan, family, cols, gid, groups, rng, capfd):
    n = gid.size
    names = PLANS[plan][0]
    mode = spec.get("mode", "blocks")
    coded = {}
    if mode.startswith("coded"):
        for c in names:
            if c in spec["coded"]:
                comp = oracle.CompressedColumn(np.ascontiguousarray(cols[c]))
                assert comp.dictionary is not None, f"{c}: the test wants a dictionary-coded column"
                coded[c] = comp
    cfg, kcols = make_config(plan, spec["keys"], gid, spec["strategy"], est=spec.get("est", 0), num_entries=spec.get("entries", 0),
                             nullable=mode == "nullable", code_widths={c: comp.code_width for c, comp in coded.items()} if coded else None)
    if path.startswith("q1_fixed_shape"):
        from test_gpu_agg import q1_config
        assert bytes(cfg) == bytes(q1_config()), "not exactly the plan of the fixed Q1 shape"
    host = kcols + [cols[c] for c in names]
    dcols = [to_dev(np.ascontiguousarray(c), dev) for c in host]
    partitions = spec.get("partitions", 1)
    dense = spec["strategy"] == T.AGG_COLLISION_FREE
    capfd.readouterr()

    def done(st, g=gid, nulls=None):
        check(plan, family, finalize_groups(st, dev, spec["keys"], partitions, ascending=dense), cols, g, groups, nulls)

    if mode == "blocks":
        for blocks in np.atleast_1d(spec["blocks"]):
            before = _counter(capi, "qsx_debug_agg_family_launches")
            st = capi.AggState(cfg)
            for a, b in _blocks(n, int(blocks)):
                st.update([c[a:b] for c in dcols], int(b - a))
            if spec.get("proof") == "family":
                assert _counter(capi, "qsx_debug_agg_family_launches") == before + int(blocks), "not served by the AOT family"
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
        nulls = {c: rng.random(n) < 0.2 for c in names}
        for c in names:
            nulls[c] |= gid == 5                                   # group 5: every argument NULL, so every SUM / AVG / MIN / MAX too
        edges = NULLABLE_EDGES + [n]
        assert not np.any(gid[edges[1]:edges[2]] == 5)
        for c in names:
            nulls[c][edges[1]:edges[2]] = False                   # the block without bitmaps: nothing NULL in it
        st = capi.AggState(cfg)
        for blk, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
            bms = [None] * len(kcols) + [None if blk == 1 else bitmap_dev(oracle.bitmap_from_bools(nulls[c][a:b]), dev) for c in names]
            st.update_nullable([x[a:b] for x in dcols], bms, int(b - a))
        done(st, nulls=nulls)
    elif mode.startswith("coded"):
        sized = mode == "coded"
        code_cols = kcols + [coded[c].codes if c in coded else cols[c] for c in names]
        dicts = [None] * len(kcols) + [to_dev(coded[c].dictionary, dev) if c in coded else None for c in names]
        dcode = [to_dev(np.ascontiguousarray(c), dev) for c in code_cols]
        before = _counter(capi, "qsx_debug_agg_factored_launches")
        st = capi.AggState(cfg)
        cut = 131_072 + 5
        for a, b in ((0, cut), (cut, n)):
            st.update_coded([x[a:b] for x in dcode], dicts, b - a, sized=sized)
        moved = _counter(capi, "qsx_debug_agg_factored_launches") - before
        assert moved == (2 if spec["proof"] == "factored" else 0), f"factored launches moved by {moved}"
        done(st)
    else:
        assert mode == "two_level"
        _two_level(capi, oracle, dev, cfg, dcols, done, gid, rng)
    if spec.get("proof") == "shape":
        assert "[qsx] shape launch" in capfd.readouterr().err, "the fixed AOT shape did not launch"


def _two_level(capi, oracle, dev, cfg, dcols, done, gid, rng):
    n = gid.size
    two = lambda: _counter(capi, "qsx_debug_agg_two_level_updates")               # noqa: E731
    comp = lambda: _counter(capi, "qsx_debug_agg_filtered_compactions")           # noqa: E731
    runs = lambda: _counter(capi, "qsx_debug_agg_run_concats")                    # noqa: E731
    before = two()
    st = capi.AggState(cfg)
    st.update(dcols, n)
    assert two() == before + 1, "the call did not take the two-level pieces"
    done(st)
    st.close()
    # under a filter: the survivors compacted, then the two passes
    keep = rng.random(n) < 0.7
    before, compactions = two(), comp()
    st = capi.AggState(cfg)
    st.update(dcols, n, filter_bitmap=bitmap_dev(oracle.bitmap_from_bools(keep), dev))
    assert comp() == compactions + 1 and two() == before + 1, "the filtered call did not compact and take the pieces"
    done(st, g=np.where(keep, gid, -1))
    st.close()
    # a run of blocks (ragged, one empty) laid end to end, then the two passes
    before, concats = two(), runs()
    st = capi.AggState(cfg)
    edges = [0, 100_000, 100_000, 250_001, 400_000, n]
    st.update_blocks([[c[a:b] for c in dcols] for a, b in zip(edges[:-1], edges[1:])])
    assert runs() == concats + 1 and two() == before + 1, "the run was not laid end to end through the pieces"
    done(st)
    st.close()


@pytest.mark.parametrize("strategy", [T.AGG_SINGLE_STATE, T.AGG_GENERIC, T.AGG_COLLISION_FREE])
def test_avg_of_subnormal_sums_is_rounded_once(capi, dev, strategy, monkeypatch):
    """AVG = SUM / COUNT rounded once, ties to even, also where the quotient is subnormal: sums of k c + c / 2 units of 2^-1074
    over c rows (c even) are exact ties, the others are not.  The hardware divide rounds such a quotient twice
    (aggregate.hip avg_quotient).  Reference: Fraction, rounded by float()."""
    from fractions import Fraction
    monkeypatch.setenv("QSX_AGG_JIT_MIN_ROWS", NO_JIT)
    rng = np.random.default_rng(1074)
    groups = 1 if strategy == T.AGG_SINGLE_STATE else 300
    counts = np.array([98] if groups == 1 else [2 * (g % 50 + 1) for g in range(groups)])
    units, parts, gids = [], [], []
    for g, c in enumerate(counts):
        k = int(rng.integers(1, 2**30))
        s = (k * int(c) + int(c) // 2) * (1 if g % 4 else -1) if g % 2 == 0 else int(rng.integers(-2**36, 2**36))
        p = rng.integers(-2**40, 2**40, size=int(c))
        p[-1] = s - int(p[:-1].sum())
        assert abs(int(p[-1])) < 2**52 and int(p.sum()) == s
        units.append(s)
        parts.append(p)
        gids.append(np.full(int(c), g))
    gid = np.concatenate(gids)
    order = rng.permutation(gid.size)
    gid, x = gid[order], np.ldexp(np.concatenate(parts).astype(np.float64), -1074)[order]
    keys = [] if groups == 1 else [gid.astype(np.int32)]
    layout = ([] if groups == 1 else [(T.INT, None)]) + [(T.DOUBLE, None)]
    v = len(keys)
    cfg = T.make_agg_config(strategy, layout, keys=list(range(v)), aggs=[(T.AGG_AVG, T.col(v)), (T.AGG_SUM, T.col(v)), (T.AGG_COUNT_STAR, None)],
                            est_groups=groups, num_entries=groups if strategy == T.AGG_COLLISION_FREE else 0)
    st = capi.AggState(cfg)
    st.update([to_dev(c, dev) for c in keys + [x]], gid.size)
    k_, vals, nulls, found = st.finalize(dev)
    f = int(found.item())
    got_gid = np.zeros(1, dtype=np.int64) if groups == 1 else k_[0].cpu().numpy()[:f].astype(np.int64)
    assert f == groups and np.array_equal(np.sort(got_gid), np.arange(groups))
    avg, total, cnt = (v_.cpu().numpy()[:f] for v_ in vals)
    for r, g in enumerate(got_gid):
        assert cnt[r] == counts[g] and total[r] == np.ldexp(float(units[g]), -1074)
        want = float(Fraction(units[g], int(counts[g])) / 2**1074)
        assert avg[r] == want, f"group {g}: AVG {avg[r].hex()} != {want.hex()} (sum {units[g]} x 2^-1074 over {counts[g]} rows)"
