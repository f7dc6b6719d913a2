#!/usr/bin/env python3
"""LIKE and code membership on an MI355X: ms per call, one JSON line per configuration.

  * qsx_select_like for PROMO%, %BRASS, %green%, %special%requests% over CHAR(25) and CHAR(55) stripes, next to
    qsx_select_cmp_char with = on the same stripe (the yardstick: an existing kernel) and the stripe's bytes over the 8 TB/s peak;
  * qsx_select_codes_in_set over 1- and 2-byte codes next to qsx_select_codes with QSX_CODE_EQ.

usage: like_probe.py [rows_millions] [out.jsonl]      (100 M rows by default; the lines go to stdout and, when given, the file)"""
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


VALUES = [b"PROMO BRUSHED BRASS", b"STANDARD PLATED TIN", b"MEDIUM POLISHED COPPER", b"ECONOMY ANODIZED BRASS",
          b"dark green forest lime", b"special packages requests", b"no special deposits; requests", b"almond antique blue"]
for width in (25, 55):
    words = torch.zeros((len(VALUES), width), dtype=torch.uint8, device=dev)
    for i, w in enumerate(VALUES):
        raw = list(w[:width])
        words[i, :len(raw)] = torch.tensor(raw, dtype=torch.uint8, device=dev)
    col = words[torch.randint(0, len(VALUES), (n,), device=dev, generator=g)].contiguous()
    floor_ms = width * n / 8e12 * 1e3
    med, lo, hi = timed(lambda: capi.select_cmp_char(col, T.EQ, VALUES[0][:width]))
    emit({"call": "qsx_select_cmp_char", "op": "=", "width": width, "rows": n, "ms": round(med, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4),
          "stripe_bytes_over_hbm_peak_ms": round(floor_ms, 4)})
    for pattern in (b"PROMO%", b"%BRASS", b"%green%", b"%special%requests%"):
        med, lo, hi = timed(lambda: capi.select_like(col, pattern))
        _, count = capi.select_like(col, pattern)
        emit({"call": "qsx_select_like", "pattern": pattern.decode(), "width": width, "rows": n, "ms": round(med, 4), "min_ms": round(lo, 4),
              "max_ms": round(hi, 4), "stripe_bytes_over_hbm_peak_ms": round(floor_ms, 4), "matches": int(count.item())})
    del col
for dtype, num_codes in ((torch.uint8, 150), (torch.int16, 20000)):
    codes = torch.randint(0, num_codes, (n,), device=dev, generator=g, dtype=torch.int32).to(dtype)
    members = torch.rand(num_codes, device=dev, generator=g) < 0.3
    padded = torch.zeros((num_codes + 63) // 64 * 64, dtype=torch.int64, device=dev)
    padded[:num_codes] = members
    shifts = torch.arange(63, -1, -1, device=dev, dtype=torch.int64)
    code_set = (padded.view(-1, 64) << shifts).sum(dim=1)          # bit i = bit 63 - i % 64 of word i / 64
    floor_ms = codes.element_size() * n / 8e12 * 1e3
    med, lo, hi = timed(lambda: capi.select_codes(codes, T.CODE_EQ, 7))
    emit({"call": "qsx_select_codes", "op": "QSX_CODE_EQ", "code_width": codes.element_size(), "rows": n, "ms": round(med, 4), "min_ms": round(lo, 4),
          "max_ms": round(hi, 4), "stripe_bytes_over_hbm_peak_ms": round(floor_ms, 4)})
    med, lo, hi = timed(lambda: capi.select_codes_in_set(codes, code_set, num_codes))
    _, count = capi.select_codes_in_set(codes, code_set, num_codes)
    want = int(members[codes.long()].sum().item())
    emit({"call": "qsx_select_codes_in_set", "code_width": codes.element_size(), "num_codes": num_codes, "rows": n, "ms": round(med, 4),
          "min_ms": round(lo, 4), "max_ms": round(hi, 4), "stripe_bytes_over_hbm_peak_ms": round(floor_ms, 4), "count_ok": int(count.item()) == want})
    del codes
if out_path:
    with open(out_path, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
