#!/usr/bin/env python3
"""Integer aggregate arguments (QSX_EX_IADD .. IDIV) against the same plan evaluated in double (QSX_EX_ADD ..).

100 M rows (argv[1]), one INT key with 4 groups and with 10^6 groups, columns i, j INT and l LONG; the plan
SUM(i + j), MIN(i + j), SUM(l * 3 + i), SUM(l * l), COUNT(*) once with plain ops and once with integer ops, alternating in one
process after a warm-up of each, 7 timed calls each (argv[2]), HIP events around every call; the compiled run-time shape and the
interpreter separately, the fused one-pass kernel (two-level pieces switched off) and, for 10^6 groups, the two-level pieces.
One JSON line per configuration: median, min, max in ms and the share of the 8 TB/s HBM peak by algorithmic bytes (key + operand
columns = 20 bytes per row).  On a library without the integer ops only the plain lines are printed."""
import json
import os
import statistics
import sys

import torch

os.environ.setdefault("QSX_AGG_JIT_SYNC", "1")   # time the run-time plan shape, not the interpreter that covers its compile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quickstep_amd.capi as capi  # noqa: E402
from quickstep_amd import types as T  # noqa: E402

dev = torch.device("cuda:0")
n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 7
BYTES_PER_ROW = 4 + 4 + 4 + 8
HAS_INT = hasattr(T, "EX_IADD")


def config(integer, groups):
    add, mul = (T.EX_IADD, T.EX_IMUL) if integer else (T.EX_ADD, T.EX_MUL)
    i, j, l = T.col(1), T.col(2), T.col(3)
    return T.make_agg_config(T.AGG_GENERIC, [(T.INT, None), (T.INT, None), (T.INT, None), (T.LONG, None)], keys=[0],
                             instrs=[(add, 0, i, j), (mul, 1, l, T.const(0)), (add, 2, T.temp(1), i), (mul, 3, l, l)], consts=[3.0],
                             aggs=[(T.AGG_SUM, T.temp(0)), (T.AGG_MIN, T.temp(0)), (T.AGG_SUM, T.temp(2)), (T.AGG_SUM, T.temp(3)),
                                   (T.AGG_COUNT_STAR, None)], est_groups=groups)


def time_call(st, cols):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    st.update(cols, n)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


gen = torch.Generator(device=dev)
gen.manual_seed(20)
i_col = torch.randint(-2**31, 2**31 - 1, (n,), dtype=torch.int64, device=dev, generator=gen).to(torch.int32)
j_col = torch.randint(-2**31, 2**31 - 1, (n,), dtype=torch.int64, device=dev, generator=gen).to(torch.int32)
l_col = torch.randint(-2**41, 2**41, (n,), dtype=torch.int64, device=dev, generator=gen)
MODES = {
    "compiled_shape": {"QSX_AGG_JIT_MIN_ROWS": "0", "QSX_AGG_TWO_LEVEL_MIN_GROUPS": "0"},
    "interpreter": {"QSX_AGG_NO_SPECIALIZE": "1", "QSX_AGG_JIT_MIN_ROWS": str(1 << 60), "QSX_AGG_TWO_LEVEL_MIN_GROUPS": "0"},
    "two_level": {"QSX_AGG_JIT_MIN_ROWS": str(1 << 60)},
}
for groups in (4, 1_000_000):
    key = torch.randint(0, groups, (n,), dtype=torch.int64, device=dev, generator=gen).to(torch.int32)
    cols = [key, i_col, j_col, l_col]
    for mode, env in MODES.items():
        if mode == "two_level" and groups < 1_000_000:
            continue
        for k in ("QSX_AGG_JIT_MIN_ROWS", "QSX_AGG_NO_SPECIALIZE", "QSX_AGG_TWO_LEVEL_MIN_GROUPS"):
            os.environ.pop(k, None)
        os.environ.update(env)
        forms = ["double"] + (["integer"] if HAS_INT else [])
        states = {f: capi.AggState(config(f == "integer", groups)) for f in forms}
        for f in forms:                                   # warm-up of each shape (the compile, the table's growth)
            time_call(states[f], cols)
            time_call(states[f], cols)
        ms = {f: [] for f in forms}
        for _ in range(calls):                            # alternating
            for f in forms:
                ms[f].append(time_call(states[f], cols))
        for f in forms:
            med = statistics.median(ms[f])
            print(json.dumps({"tool": "agg_int_expr", "rows": n, "groups": groups, "mode": mode, "form": f, "calls": calls,
                              "median_ms": round(med, 3), "min_ms": round(min(ms[f]), 3), "max_ms": round(max(ms[f]), 3),
                              "hbm_peak_share": round(BYTES_PER_ROW * n / (med * 1e-3) / 8e12, 4)}), flush=True)
            states[f].close()
    del key, cols
