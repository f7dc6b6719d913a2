#!/usr/bin/env python3
"""EXTRACT and SUBSTRING on an MI355X: ms per call, one JSON line per configuration.  Every pair is measured in one process,
its two calls alternating, 10 timed calls each after a warm-up; a line holds the median, the minimum and the maximum, and
the bytes the call moves over the 8 TB/s peak.

  * qsx_eval_date_extract (8 bytes in, 4 out per row) next to qsx_eval_expression_long over one LONG column with out_width 4
    (the yardstick: an existing kernel that moves exactly the same bytes);
  * qsx_eval_substring CHAR(15) -> 2 and CHAR(25) -> 5 (w + m bytes per row) next to qsx_select_like with a `lit%` pattern of
    m bytes over the same stripe (it reads the same bytes, walks as far into the row and writes 1 bit instead of m bytes);
  * EXTRACT over a dictionary-coded date (2-byte codes): extract over the dictionary + qsx_decode_codes into INTs, next to
    qsx_decode_codes into 8-byte dates + extract.

usage: unary_probe.py [rows_millions] [out.jsonl]      (100 M rows by default; the lines go to stdout and, when given, the file)"""
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
g.manual_seed(5)
lines = []
HBM_PEAK = 8e12


def emit(line):
    lines.append(line)
    print(json.dumps(line), flush=True)


def timed_alternating(fns, reps=10):
    """fns: the calls of one comparison.  Returns (median, min, max) ms per call, the calls taking turns."""
    for _ in range(3):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times[i].append(a.elapsed_time(b))
    out = []
    for t in times:
        t.sort()
        out.append((t[len(t) // 2], t[0], t[-1]))
    return out


def stats(t, moved_bytes):
    return {"ms": round(t[0], 4), "min_ms": round(t[1], 4), "max_ms": round(t[2], 4), "bytes_over_hbm_peak_ms": round(moved_bytes / HBM_PEAK * 1e3, 4)}


def random_dates(count):
    year = torch.randint(1992, 1999, (count,), device=dev, generator=g, dtype=torch.int64)
    month = torch.randint(1, 13, (count,), device=dev, generator=g, dtype=torch.int64)
    day = torch.randint(1, 29, (count,), device=dev, generator=g, dtype=torch.int64)
    return year | (month << 32) | (day << 40)


# ---- EXTRACT against the expression kernel moving the same bytes
dates = random_dates(n)
for unit, name in ((T.DATE_YEAR, "YEAR"), (T.DATE_MONTH, "MONTH")):
    ours, yard = timed_alternating([lambda: capi.eval_date_extract(unit, dates),
                                    lambda: capi.eval_expression_long([dates], [], [], T.col(0), out_dtype=torch.int32)])
    want = (dates & 0xFFFFFFFF) if unit == T.DATE_YEAR else ((dates >> 32) & 0xFF)
    ok = bool(torch.equal(capi.eval_date_extract(unit, dates).long(), want))
    emit(dict({"call": "qsx_eval_date_extract", "unit": name, "rows": n, "values_ok": ok}, **stats(ours, 12 * n)))
    emit(dict({"call": "qsx_eval_expression_long", "beside": "EXTRACT " + name, "columns": "1 LONG", "out_width": 4, "rows": n}, **stats(yard, 12 * n)))
    emit({"compare": "EXTRACT " + name + " / yardstick", "ratio_of_medians": round(ours[0] / yard[0], 4),
          "median_difference_ms": round(ours[0] - yard[0], 4), "yardstick_spread_ms": round(yard[2] - yard[1], 4)})
del want

# ---- EXTRACT over a dictionary-coded date: 2-byte codes
num_codes = 2500
dictionary = random_dates(num_codes)
codes = torch.randint(0, num_codes, (n,), device=dev, generator=g, dtype=torch.int32).to(torch.int16)
fields = torch.zeros(num_codes + 1, dtype=torch.int32, device=dev)      # one entry more: the NULL code's


def on_codes():
    capi.eval_date_extract(T.DATE_YEAR, dictionary, out=fields[:num_codes])
    return capi.decode_codes(codes, fields, torch.int32)


def decoded_first():
    return capi.eval_date_extract(T.DATE_YEAR, capi.decode_codes(codes, dictionary, torch.int64))


a, b = timed_alternating([on_codes, decoded_first])
ok = bool(torch.equal(on_codes(), decoded_first()))
emit(dict({"call": "qsx_eval_date_extract(dictionary) + qsx_decode_codes", "code_width": 2, "num_codes": num_codes, "rows": n, "values_ok": ok},
          **stats(a, 6 * n)))
emit(dict({"call": "qsx_decode_codes + qsx_eval_date_extract", "code_width": 2, "num_codes": num_codes, "rows": n}, **stats(b, (2 + 8 + 8 + 4) * n)))
del dates, codes

# ---- SUBSTRING against LIKE 'lit%' with a literal of m bytes
for width, m in ((15, 2), (25, 5)):
    prefixes = torch.randint(ord("0"), ord("9") + 1, (n, width), device=dev, generator=g, dtype=torch.uint8)
    col = prefixes.contiguous()
    del prefixes
    pattern = bytes(col[0, :m].cpu().tolist()) + b"%"
    ours, yard = timed_alternating([lambda: capi.eval_substring(col, 0, m), lambda: capi.select_like(col, pattern, want_count=False)])
    ok = bool(torch.equal(capi.eval_substring(col, 0, m), col[:, :m]))
    emit(dict({"call": "qsx_eval_substring", "width": width, "start": 0, "length": m, "rows": n, "values_ok": ok}, **stats(ours, (width + m) * n)))
    emit(dict({"call": "qsx_select_like", "pattern": "<%d bytes>%%" % m, "width": width, "rows": n}, **stats(yard, width * n + n // 8)))
    emit({"compare": "SUBSTRING CHAR(%d) -> %d / LIKE" % (width, m), "ratio_of_medians": round(ours[0] / yard[0], 4)})
    del col
if out_path:
    with open(out_path, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
