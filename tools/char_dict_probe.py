#!/usr/bin/env python3
"""Interning CHAR(n) group-by keys on an MI355X (qsx_char_dict_*): ms per call, one JSON line per configuration.

Per stripe — CHAR(10) with 7 values, CHAR(15) with 5, CHAR(25) with 25, CHAR(25) with 10^6 distinct values:
  * qsx_select_cmp_char with = on the same stripe (the yardstick: an existing kernel that walks each text once out of LDS) and
    the stripe's bytes over the 8 TB/s peak;
  * intern into a warm dictionary (every value present: the steady state of a scan) and into a cleared one, with the
    per-workgroup LDS cache and without it (QSX_CHAR_DICT_LDS_CACHE=0 when the dictionary is created);
  * intern + qsx_agg_update of SUM(DOUBLE), COUNT(*) grouped by the ids, end to end.
Then the dictionary-coded route: intern 7 dictionary values + qsx_decode_codes of 1-byte codes through the id array.

usage: char_dict_probe.py [rows_millions] [out.jsonl]      (100 M rows by default; the lines go to stdout and, when given, the file)"""
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
g.manual_seed(7)
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
    return {"ms": round(times[len(times) // 2], 4), "min_ms": round(times[0], 4), "max_ms": round(times[-1], 4)}


def table_of(values, width):
    words = torch.zeros((len(values), width), dtype=torch.uint8, device=dev)
    for i, v in enumerate(values):
        words[i, :len(v)] = torch.tensor(list(v[:width]), dtype=torch.uint8, device=dev)
    return words


def numbered(count, width):
    """count distinct texts of 7 digits."""
    idx = torch.arange(count, device=dev)
    words = torch.zeros((count, width), dtype=torch.uint8, device=dev)
    for d in range(7):
        words[:, d] = (48 + (idx // 10 ** d) % 10).to(torch.uint8)
    return words


def dictionary(width, capacity, lds_cache):
    os.environ["QSX_CHAR_DICT_LDS_CACHE"] = "1" if lds_cache else "0"
    return capi.CharDict(width, capacity)


MODES = [b"MAIL", b"SHIP", b"AIR", b"REG AIR", b"TRUCK", b"RAIL", b"FOB"]
PRIORITIES = [b"1-URGENT", b"2-HIGH", b"3-MEDIUM", b"4-NOT SPECIFIED", b"5-LOW"]
NATIONS = [b"NATION NUMBER %02d" % i for i in range(25)]
STRIPES = (("l_shipmode", 10, table_of(MODES, 10)), ("o_orderpriority", 15, table_of(PRIORITIES, 15)), ("n_name", 25, table_of(NATIONS, 25)),
           ("distinct", 25, numbered(1_000_000, 25)))
x = torch.randint(0, 1000, (n,), device=dev, generator=g).to(torch.float64)
for name, width, table in STRIPES:
    values = table.shape[0]
    col = table[torch.randint(0, values, (n,), device=dev, generator=g)].contiguous()
    base = {"stripe": name, "width": width, "values": values, "rows": n, "stripe_bytes_over_hbm_peak_ms": round(width * n / 8e12 * 1e3, 4)}
    emit({**base, "call": "qsx_select_cmp_char =", **timed(lambda: capi.select_cmp_char(col, T.EQ, bytes(table[0].cpu().numpy()).rstrip(b"\0")))})
    ids = torch.empty(n, dtype=torch.int32, device=dev)
    capacity = max(16, 2 * values)
    for lds_cache in (True, False):
        d = dictionary(width, capacity, lds_cache)
        d.intern(col, out=ids)
        size, dropped = d.size()
        emit({**base, "call": "qsx_char_dict_intern, warm", "lds_cache": lds_cache, "size": size, "dropped": dropped,
              **timed(lambda: d.intern(col, out=ids))})

        def cleared():
            d.clear()
            d.intern(col, out=ids)
        emit({**base, "call": "qsx_char_dict_clear + qsx_char_dict_intern", "lds_cache": lds_cache, **timed(cleared)})
        if lds_cache:
            try:
                cfg = T.make_agg_config(T.AGG_COMPACT_KEY, [(T.INT, None), (T.DOUBLE, None)], keys=[0],
                                        aggs=[(T.AGG_SUM, T.col(1)), (T.AGG_COUNT_STAR, None)], est_groups=capacity)
                state = capi.AggState(cfg)

                def grouped():
                    d.intern(col, out=ids)
                    state.update([ids, x])
                emit({**base, "call": "qsx_char_dict_intern + qsx_agg_update SUM(DOUBLE), COUNT(*)", "lds_cache": True, **timed(grouped)})
                emit({**base, "call": "qsx_agg_update SUM(DOUBLE), COUNT(*) on the ids alone", **timed(lambda: state.update([ids, x]))})
                state.close()
            except capi.QsxError as e:
                emit({**base, "call": "qsx_char_dict_intern + qsx_agg_update", "error": str(e)})
        d.close()
    del col, ids

# the dictionary-coded route: the block's dictionary is interned, the code stripe mapped through the id array
codes = torch.randint(0, len(MODES), (n,), device=dev, generator=g, dtype=torch.int32).to(torch.uint8)
d = dictionary(10, 16, True)
table = table_of(MODES, 10)
ids = torch.empty(n, dtype=torch.int32, device=dev)


def coded():
    id_array = d.intern(table)
    capi.decode_codes(codes, id_array, torch.int32, out=ids)


emit({"call": "qsx_char_dict_intern of 7 dictionary values + qsx_decode_codes of 1-byte codes", "rows": n,
      "stripe_bytes_over_hbm_peak_ms": round(n / 8e12 * 1e3, 4), **timed(coded)})
d.close()
if out_path:
    with open(out_path, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
