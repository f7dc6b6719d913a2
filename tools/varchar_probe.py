#!/usr/bin/env python3
"""VARCHAR entry points on an MI355X: ms per call and achieved bytes/s, one JSON line per configuration.

  (a) qsx_select_like_var over ONE variable-length dictionary of texts shaped like o_comment (VARCHAR(79), lengths spread over
      19..78) next to qsx_select_like over the same texts held as a fixed CHAR(79) dictionary — the kernel a caller had before —
      for %special%requests% and PROMO%.  The two are timed alternately in one process; their match counts must agree.
      bytes = what the kernel has to read: value bytes + 4 bytes of offset per entry, against 79 bytes per entry.
  (b) qsx_decode_codes_var next to qsx_decode_codes.  qsx_decode_codes knows 4- and 8-byte values only, so the comparable case
      is texts of at most 8 bytes decoded into 8-byte fields from either dictionary; the o_comment shape (79-byte fields) is
      timed for qsx_decode_codes_var alone.  bytes = codes read + fields written (the dictionary reads come on top).
  (c) qsx_select_like_var_blocks over 64 dictionaries of ~40 K entries in one launch, next to 64 qsx_select_like_var calls.

usage: varchar_probe.py [entries_millions] [out.jsonl]   (10 M entries by default; the lines go to stdout and, when given, the file)"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import quickstep_amd.capi as capi  # noqa: E402

dev = torch.device("cuda", 0)
n = int(float(sys.argv[1]) * 1e6) if len(sys.argv) > 1 else 10_000_000
out_path = sys.argv[2] if len(sys.argv) > 2 else None
g = torch.Generator(device=dev)
g.manual_seed(5)
lines = []


def emit(line):
    lines.append(line)
    print(json.dumps(line), flush=True)


def timed_pair(fns, reps=10):
    """The calls of `fns` alternately: (median, min, max) ms of each."""
    for _ in range(3):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times[k].append(a.elapsed_time(b))
    return [(sorted(t)[len(t) // 2], min(t), max(t)) for t in times]


def make_texts(count, width, low, high):
    """count texts of low..high bytes as a fixed (count, width) matrix, NUL-padded; some hold 'special .. requests', some start
    with PROMO.  And the same texts as a variable-length dictionary: (offsets int32, value bytes with the terminators)."""
    fixed = torch.randint(97, 123, (count, width), device=dev, generator=g, dtype=torch.int32).to(torch.uint8)
    fixed[torch.rand((count, width), device=dev, generator=g) < 0.15] = 32
    kind = torch.rand(count, device=dev, generator=g)
    if width >= 20:
        rows = kind < 0.02
        fixed[rows, 2:9] = torch.tensor(list(b"special"), dtype=torch.uint8, device=dev)
        fixed[rows, 10:18] = torch.tensor(list(b"requests"), dtype=torch.uint8, device=dev)
    if width >= 5:
        fixed[(kind >= 0.02) & (kind < 0.07), 0:5] = torch.tensor(list(b"PROMO"), dtype=torch.uint8, device=dev)
    length = torch.randint(low, high + 1, (count,), device=dev, generator=g)
    at = torch.arange(width, device=dev).unsqueeze(0)
    fixed[at >= length.unsqueeze(1)] = 0
    padded = torch.cat([fixed, torch.zeros((count, 1), dtype=torch.uint8, device=dev)], dim=1)      # room for a text of `width` bytes
    values = padded[torch.arange(width + 1, device=dev).unsqueeze(0) <= length.unsqueeze(1)]         # text + its terminator, back to back
    ends = torch.cumsum(length + 1, dim=0)
    assert int(ends[-1].item()) == values.numel() < 2 ** 31
    offsets = (ends - (length + 1)).to(torch.int32)
    return fixed.contiguous(), offsets.contiguous(), values.contiguous()


def rate(nbytes, ms):
    return round(nbytes / (ms * 1e-3) / 1e12, 3)


# ---- (a) one dictionary ---------------------------------------------------------------------------------------------------------
fixed, offsets, values = make_texts(n, 79, 19, 78)
var_bytes, fixed_bytes = values.numel() + 4 * n, 79 * n
for pattern in (b"%special%requests%", b"PROMO%"):
    (v, vlo, vhi), (f, flo, fhi) = timed_pair([lambda: capi.select_like_var(offsets, values, 79, pattern), lambda: capi.select_like(fixed, pattern)])
    _, var_count = capi.select_like_var(offsets, values, 79, pattern)
    _, fixed_count = capi.select_like(fixed, pattern)
    emit({"measure": "a", "pattern": pattern.decode(), "entries": n, "matches": int(var_count.item()), "counts_agree": int(var_count.item()) == int(fixed_count.item()),
          "qsx_select_like_var": {"ms": round(v, 4), "min_ms": round(vlo, 4), "max_ms": round(vhi, 4), "bytes": var_bytes, "TB_per_s": rate(var_bytes, v)},
          "qsx_select_like_char79": {"ms": round(f, 4), "min_ms": round(flo, 4), "max_ms": round(fhi, 4), "bytes": fixed_bytes, "TB_per_s": rate(fixed_bytes, f)}})

# ---- (b) decode -------------------------------------------------------------------------------------------------------------------
rows = 4 * n
codes = torch.randint(0, n, (rows,), device=dev, generator=g, dtype=torch.int32)
out79 = torch.empty((rows, 79), dtype=torch.uint8, device=dev)
(v, vlo, vhi), = timed_pair([lambda: capi.decode_codes_var(codes, offsets, values, 79, out=out79)])
emit({"measure": "b", "shape": "VARCHAR(79), lengths 19..78", "rows": rows, "entries": n,
      "qsx_decode_codes_var": {"ms": round(v, 4), "min_ms": round(vlo, 4), "max_ms": round(vhi, 4), "bytes": rows * (4 + 79), "TB_per_s": rate(rows * (4 + 79), v)}})
del out79, fixed, offsets, values
fixed8, offsets8, values8 = make_texts(n, 8, 1, 7)
dict8 = fixed8.view(torch.int64).reshape(-1)
out8 = torch.empty((rows, 8), dtype=torch.uint8, device=dev)
out8_fixed = torch.empty(rows, dtype=torch.int64, device=dev)
(v, vlo, vhi), (f, flo, fhi) = timed_pair([lambda: capi.decode_codes_var(codes, offsets8, values8, 8, out=out8),
                                           lambda: capi.decode_codes(codes, dict8, torch.int64, out=out8_fixed)])
emit({"measure": "b", "shape": "texts of 1..7 bytes in 8-byte fields", "rows": rows, "entries": n,
      "fields_agree": bool(torch.equal(out8.view(torch.int64).reshape(-1), out8_fixed)),
      "qsx_decode_codes_var": {"ms": round(v, 4), "min_ms": round(vlo, 4), "max_ms": round(vhi, 4), "bytes": rows * 12, "TB_per_s": rate(rows * 12, v)},
      "qsx_decode_codes": {"ms": round(f, 4), "min_ms": round(flo, 4), "max_ms": round(fhi, 4), "bytes": rows * 12, "TB_per_s": rate(rows * 12, f)}})
del codes, out8, out8_fixed, fixed8, offsets8, values8

# ---- (c) a run of dictionaries -------------------------------------------------------------------------------------------------------
dictionaries = [make_texts(40_000 + 37 * b, 79, 19, 78)[1:] for b in range(64)]
offs, vals = [d[0] for d in dictionaries], [d[1] for d in dictionaries]
pattern = b"%special%requests%"


def per_dictionary():
    for o, v_ in zip(offs, vals):
        capi.select_like_var(o, v_, 79, pattern, want_count=False)


(r, rlo, rhi), (s, slo, shi) = timed_pair([lambda: capi.select_like_var_blocks(offs, vals, 79, pattern), per_dictionary])
_, run_counts = capi.select_like_var_blocks(offs, vals, 79, pattern)
single = [int(capi.select_like_var(o, v_, 79, pattern)[1].item()) for o, v_ in zip(offs, vals)]
emit({"measure": "c", "dictionaries": 64, "entries_each": "40000 + 37 b", "pattern": pattern.decode(), "counts_agree": run_counts.cpu().tolist() == single,
      "one_blocks_launch": {"ms": round(r, 4), "min_ms": round(rlo, 4), "max_ms": round(rhi, 4)},
      "64_launches": {"ms": round(s, 4), "min_ms": round(slo, 4), "max_ms": round(shi, 4)}})
if out_path:
    with open(out_path, "w") as f_:
        for line in lines:
            f_.write(json.dumps(line) + "\n")
