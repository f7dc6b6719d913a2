#!/usr/bin/env python3
"""Predicates over a unary operation on an MI355X: the fused call against the two-call sequence of existing entry points that
computes the same bitmap, ms per call, one JSON line per variant.

  * a 7-literal IN over SUBSTRING(CHAR(15), 0, 2):  qsx_select_in_unary  against  qsx_eval_substring + qsx_select_in_char;
  * EXTRACT(YEAR) = literal over plain dates:       qsx_select_cmp_unary  against  qsx_eval_date_extract + qsx_select_cmp;
  * the run forms: 64 blocks in one launch (qsx_select_in_unary_blocks, qsx_select_cmp_unary_blocks) against 64 launches.

The two variants of a pair ALTERNATE inside one timed loop (fused, two-call, fused, ...) after a warm-up of both, so that whatever
else the machine does falls on both alike; a line reports the median, the minimum, the maximum and the spread (max - min) of its
variant's samples, and the pair's verdict: the fused form counts as faster only when the difference of the medians is more
than the larger of the two spreads.  Every fused result is compared with the two-call result before it is timed.

usage: unary_predicate_probe.py [rows_millions] [out.jsonl]   (100 M rows by default; the lines go to stdout and, when given, the file)"""
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
g.manual_seed(22)
lines = []
WARMUP, REPS = 3, 15
HBM_PEAK = 8e12      # bytes per second


def emit(line):
    lines.append(line)
    print(json.dumps(line), flush=True)


def alternate(first, second):
    """-> (samples of first, samples of second) in ms: both warmed up, then timed in turn."""
    for _ in range(WARMUP):
        first()
        second()
    torch.cuda.synchronize()
    samples = ([], [])
    for _ in range(REPS):
        for fn, into in ((first, samples[0]), (second, samples[1])):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            into.append(a.elapsed_time(b))
    return samples


def stats(samples):
    s = sorted(samples)
    return {"ms": round(s[len(s) // 2], 4), "min_ms": round(s[0], 4), "max_ms": round(s[-1], 4), "spread_ms": round(s[-1] - s[0], 4)}


def pair(what, fused, baseline, same, fused_bytes, baseline_bytes, **more):
    a, b = alternate(fused[1], baseline[1])
    sa, sb = stats(a), stats(b)
    faster_by = sb["ms"] - sa["ms"]
    verdict = {"fused_faster_by_ms": round(faster_by, 4), "beyond_spread": bool(faster_by > max(sa["spread_ms"], sb["spread_ms"]))}
    emit(dict({"what": what, "call": fused[0], "variant": "fused", "equals_two_calls": same, "bytes_over_hbm_peak_ms": round(fused_bytes / HBM_PEAK * 1e3, 4)},
              **sa, **verdict, **more))
    emit(dict({"what": what, "call": baseline[0], "variant": "two calls", "bytes_over_hbm_peak_ms": round(baseline_bytes / HBM_PEAK * 1e3, 4)}, **sb, **more))


CODES = [b"13", b"31", b"23", b"29", b"30", b"18", b"17"]
SUB = T.substring_of(0, 2)
YEAR = T.date_field(T.DATE_YEAR)


def phones(rows):
    """CHAR(15) 'CC-ddd-ddd-dddd' with 25 country codes."""
    digits = torch.randint(0, 10, (rows, 15), device=dev, generator=g, dtype=torch.int32).to(torch.uint8) + 48
    code = torch.randint(10, 35, (rows,), device=dev, generator=g, dtype=torch.int32)
    digits[:, 0] = (code // 10 + 48).to(torch.uint8)
    digits[:, 1] = (code % 10 + 48).to(torch.uint8)
    digits[:, 2] = digits[:, 6] = digits[:, 10] = 45
    return digits.contiguous()


def dates(rows):
    year = torch.randint(1992, 1999, (rows,), device=dev, generator=g, dtype=torch.int64)
    month = torch.randint(1, 13, (rows,), device=dev, generator=g, dtype=torch.int64)
    day = torch.randint(1, 29, (rows,), device=dev, generator=g, dtype=torch.int64)
    return (year | (month << 32) | (day << 40)).contiguous()


# ---- single stripes
col = phones(n)
prefix = torch.empty((n, 2), dtype=torch.uint8, device=dev)
out_a, out_b = capi.new_bitmap(n, dev), capi.new_bitmap(n, dev)


def sub_fused():
    return capi.select_in_unary(SUB, col, CODES, out_bitmap=out_a)


def sub_two_calls():
    capi.eval_substring(col, 0, 2, out=prefix)
    return capi.select_in_char(prefix, CODES, out_bitmap=out_b)


(fa, ca), (fb, cb) = sub_fused(), sub_two_calls()
pair("7-literal IN over SUBSTRING(CHAR(15), 0, 2)", ("qsx_select_in_unary", sub_fused), ("qsx_eval_substring + qsx_select_in_char", sub_two_calls),
     bool(torch.equal(fa, fb)) and int(ca.item()) == int(cb.item()), 15 * n + n // 8, 15 * n + 2 * n + 2 * n + n // 8, rows=n, matches=int(ca.item()))
del col, prefix

dcol = dates(n)
years = torch.empty(n, dtype=torch.int32, device=dev)


def year_fused():
    return capi.select_cmp_unary(YEAR, dcol, T.EQ, 1995, out_bitmap=out_a)


def year_two_calls():
    capi.eval_date_extract(T.DATE_YEAR, dcol, out=years)
    return capi.select_cmp(years, T.EQ, 1995, out_bitmap=out_b)


(fa, ca), (fb, cb) = year_fused(), year_two_calls()
pair("EXTRACT(YEAR) = 1995 over plain dates", ("qsx_select_cmp_unary", year_fused), ("qsx_eval_date_extract + qsx_select_cmp", year_two_calls),
     bool(torch.equal(fa, fb)) and int(ca.item()) == int(cb.item()), 8 * n + n // 8, 8 * n + 4 * n + 4 * n + n // 8, rows=n, matches=int(ca.item()))
del dcol, years, out_a, out_b

# ---- the run forms: 64 blocks in one launch against 64 launches
BLOCKS = 64
block_rows = max(n // BLOCKS // 64 * 64, 64)
pblocks = [phones(block_rows) for _ in range(BLOCKS)]
dblocks = [dates(block_rows) for _ in range(BLOCKS)]


def sub_run():
    return capi.select_in_unary_blocks(SUB, pblocks, CODES)


def sub_per_block():
    return [capi.select_in_unary(SUB, blk, CODES)[0] for blk in pblocks]      # (both variants allocate their outputs)


run_outs, _ = sub_run()
same = all(bool(torch.equal(a[:(block_rows + 63) // 64], b[:(block_rows + 63) // 64])) for a, b in zip(run_outs, sub_per_block()))
a, b = alternate(sub_run, sub_per_block)
emit(dict({"what": "7-literal IN over SUBSTRING(CHAR(15), 0, 2), 64 blocks", "call": "qsx_select_in_unary_blocks", "variant": "one launch", "blocks": BLOCKS,
           "block_rows": block_rows, "equals_per_block": same}, **stats(a)))
emit(dict({"what": "7-literal IN over SUBSTRING(CHAR(15), 0, 2), 64 blocks", "call": "64 x qsx_select_in_unary", "variant": "64 launches", "blocks": BLOCKS,
           "block_rows": block_rows}, **stats(b)))


def year_run():
    return capi.select_cmp_unary_blocks(YEAR, dblocks, T.EQ, 1995)


def year_per_block():
    return [capi.select_cmp_unary(YEAR, blk, T.EQ, 1995)[0] for blk in dblocks]


run_outs, _ = year_run()
same = all(bool(torch.equal(a[:(block_rows + 63) // 64], b[:(block_rows + 63) // 64])) for a, b in zip(run_outs, year_per_block()))
a, b = alternate(year_run, year_per_block)
emit(dict({"what": "EXTRACT(YEAR) = 1995, 64 blocks", "call": "qsx_select_cmp_unary_blocks", "variant": "one launch", "blocks": BLOCKS, "block_rows": block_rows,
           "equals_per_block": same}, **stats(a)))
emit(dict({"what": "EXTRACT(YEAR) = 1995, 64 blocks", "call": "64 x qsx_select_cmp_unary", "variant": "64 launches", "blocks": BLOCKS, "block_rows": block_rows},
          **stats(b)))

if out_path:
    with open(out_path, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
