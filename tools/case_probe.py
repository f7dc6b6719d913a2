#!/usr/bin/env python3
"""Searched CASE on an MI355X: ms per call, one JSON line per configuration.

  * the yardstick, existing code: qsx_eval_expression on x * (1 - y) over two DOUBLE stripes, measured three times in the
    session (first, in the middle, last) so that the spread between repeated medians is on record;
  * qsx_eval_case on CASE WHEN w THEN x * (1 - y) ELSE 0 END over the same stripes with one WHEN at selectivity 1/6, the same
    with three WHENs (1/6 each, overlapping, the same THEN: a disjunction written as WHENs), and the one-WHEN call writing a
    null bitmap as well;
  * a LONG leg: CASE WHEN w THEN l + i ELSE 0 END over a LONG and an INT stripe next to qsx_eval_expression_long on l + i.

Every line carries the algorithmic bytes of the call (operand stripes + output + bitmaps) and those bytes over the 8 TB/s peak.

usage: case_probe.py [rows_millions] [out.jsonl]      (100 M rows by default; the lines go to stdout and, when given, the file)"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import quickstep_amd.capi as capi  # noqa: E402
from quickstep_amd import types as T  # noqa: E402

dev = torch.device("cuda", 0)
n = int(float(sys.argv[1]) * 1e6) if len(sys.argv) > 1 else 100_000_000
out_path = sys.argv[2] if len(sys.argv) > 2 else None
g = torch.Generator(device=dev)
g.manual_seed(11)
lines = []


def emit(line):
    lines.append(line)
    print(json.dumps(line), flush=True)


def timed(fn, reps=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def line(call, what, bytes_per_row, timing, **more):
    med, lo, hi = timing
    d = {"call": call, "what": what, "rows": n, "ms": round(med, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4),
         "bytes_per_row": round(bytes_per_row, 4), "bytes_over_hbm_peak_ms": round(bytes_per_row * n / 8e12 * 1e3, 4),
         "achieved_tb_per_s": round(bytes_per_row * n / (med * 1e-3) / 1e12, 3)}
    d.update(more)
    emit(d)
    return med


x = (torch.rand(n, device=dev, generator=g, dtype=torch.float64) * 104100.0 + 900.0)
y = torch.randint(0, 11, (n,), device=dev, generator=g).to(torch.float64) / 100.0
whens = [capi.select_cmp(torch.randint(0, 6, (n,), device=dev, generator=g, dtype=torch.int32), T.EQ, 0)[0] for _ in range(3)]
program = [(T.EX_SUB, 0, T.const(0), T.col(1)), (T.EX_MUL, 1, T.col(0), T.temp(0))]
consts = [1.0, 0.0] + [0.0] * 6
out = torch.empty(n, dtype=torch.float64, device=dev)


def yardstick(label):
    return line("qsx_eval_expression", f"x * (1 - y), {label}", 24.0, timed(lambda: capi.eval_expression([x, y], program, consts, T.temp(1))))


def unpack(bitmap):
    """bool per row of an MSB-first bitmap (for the value check only)."""
    shifts = torch.arange(63, -1, -1, device=dev, dtype=torch.int64)
    return (((bitmap.view(-1, 1) >> shifts) & 1) != 0).view(-1)[:n]


first = yardstick("first")
one = [T.temp(1), T.const(1)]
med1 = line("qsx_eval_case", "1 WHEN (1/6), ELSE 0, no null bitmap", 24.0 + 1 / 8,
            timed(lambda: capi.eval_case([x, y], program, consts, one, whens[:1], T.DOUBLE, want_nulls=False, out=out)))
want = torch.where(unpack(whens[0]), x * (1.0 - y), torch.zeros((), dtype=torch.float64, device=dev))
lines[-1]["values_ok"] = bool(torch.equal(out, want))
del want
three = [T.temp(1), T.temp(1), T.temp(1), T.const(1)]
middle = yardstick("middle")
med3 = line("qsx_eval_case", "3 WHENs (1/6 each), ELSE 0, no null bitmap", 24.0 + 3 / 8,
            timed(lambda: capi.eval_case([x, y], program, consts, three, whens, T.DOUBLE, want_nulls=False, out=out)))
line("qsx_eval_case", "1 WHEN (1/6), ELSE 0, null bitmap written", 24.0 + 2 / 8,
     timed(lambda: capi.eval_case([x, y], program, consts, one, whens[:1], T.DOUBLE, want_nulls=True, out=out)))
del x, y
# the LONG leg
l = torch.randint(-2 ** 40, 2 ** 40, (n,), device=dev, generator=g, dtype=torch.int64)
i = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), device=dev, generator=g, dtype=torch.int64).to(torch.int32)
iprogram = [(T.EX_IADD, 0, T.col(0), T.col(1))]
out_long = torch.empty(n, dtype=torch.int64, device=dev)
yard_long = line("qsx_eval_expression_long", "l + i (LONG + INT)", 20.0,
                 timed(lambda: capi.eval_expression_long([l, i], iprogram, [0] * 8, T.temp(0))))
med_long = line("qsx_eval_case", "LONG: 1 WHEN (1/6) THEN l + i ELSE 0, no null bitmap", 20.0 + 1 / 8,
                timed(lambda: capi.eval_case([l, i], iprogram, consts, [T.temp(0), T.const(1)], whens[:1], T.LONG, want_nulls=False, out=out_long)))
lines[-1]["values_ok"] = bool(torch.equal(out_long, torch.where(unpack(whens[0]), l + i.to(torch.int64), torch.zeros((), dtype=torch.int64, device=dev))))
del l, i
x = (torch.rand(n, device=dev, generator=g, dtype=torch.float64) * 104100.0 + 900.0)
y = torch.randint(0, 11, (n,), device=dev, generator=g).to(torch.float64) / 100.0
last = yardstick("last")
yard = sorted([first, middle, last])
emit({"summary": "aim: a CASE leg costs no more than the yardstick scaled by its byte ratio plus the yardstick's own spread",
      "yardstick_medians_ms": [round(v, 4) for v in (first, middle, last)], "yardstick_spread_ms": round(yard[-1] - yard[0], 4),
      "case_1when_over_yardstick": round(med1 / yard[1], 4), "byte_ratio_1when": round((24 + 1 / 8) / 24, 4),
      "case_3whens_over_yardstick": round(med3 / yard[1], 4), "byte_ratio_3whens": round((24 + 3 / 8) / 24, 4),
      "case_long_over_yardstick_long": round(med_long / yard_long, 4), "byte_ratio_long": round((20 + 1 / 8) / 20, 4)})
if out_path:
    with open(out_path, "w") as f:
        for entry in lines:
            f.write(json.dumps(entry) + "\n")
