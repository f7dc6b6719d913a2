#!/usr/bin/env python3
"""qsx_select_cmp_columns_blocks on an MI355X, DATE < DATE: ms per call (median, min, max of 15 after 3 warm-ups; device events
around the call), the bytes the call has to move and their share of 8 TB/s.  One JSON line per leg:

  (a) plain aligned stripes of all rows as ONE block through the new entry point, and through qsx_select_cmp_columns on the same
      stripes (unchanged code: the baseline).  The two alternate in one process; the baseline's min..max is its spread.
  (b) both sides as 2-byte codes behind a 2,526-entry dictionary per block, blocks of 40,000 rows (a lineitem block's size), all
      blocks in one launch.
  (c) the same data decoded first: qsx_decode_codes twice over the whole stripes, then qsx_select_cmp_columns — three launches,
      the cheapest way to decode (every block's dictionary has the same contents here, so one decode call serves all blocks
      and (b) and (c) must give the same bitmap: checked).
  (d) a run of 64 plain blocks in one launch against 64 launches (of the new entry point with one block each, and of
      qsx_select_cmp_columns).

The arguments of every call are built before the clock starts; what the entry point does on the host (the run table, its
upload) is inside.

usage: cmp_columns_probe.py [rows_millions] [out.jsonl]   (100 M rows by default; the lines go to stdout and, when given, the file)"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import quickstep_amd.capi as capi  # noqa: E402
from quickstep_amd import types as T  # noqa: E402

dev = torch.device("cuda", 0)
BLOCK_ROWS = 40_000
ENTRIES = 2_526
n = int(float(sys.argv[1]) * 1e6) if len(sys.argv) > 1 else 100_000_000
n -= n % BLOCK_ROWS
assert n >= 64 * BLOCK_ROWS, "leg (d) takes 64 blocks"
out_path = sys.argv[2] if len(sys.argv) > 2 else None
HBM_PEAK = 8e12
lines = []
lib = capi.lib


def emit(line):
    lines.append(line)
    print(json.dumps(line), flush=True)


def timed(fns, reps=15):
    """Median / min / max ms of every function in fns, the functions taking turns."""
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


def report(leg, call, med_lo_hi, bytes_moved, **more):
    med, lo, hi = med_lo_hi
    emit(dict({"leg": leg, "call": call, "rows": n, "ms": round(med, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4), "bytes_moved": int(bytes_moved),
               "fraction_of_8TBps": round(bytes_moved / (med * 1e-3) / HBM_PEAK, 4)}, **more))


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def check(rc, what):
    if rc != T.OK:
        raise capi.QsxError(rc, what)


def blocks_call(lhs_ptrs, rhs_ptrs, rows, outs, counts, lhs_coding=None, rhs_coding=None):
    """A closure that calls qsx_select_cmp_columns_blocks(DATE < DATE) with arguments prepared once."""
    nb = len(rows)
    c_rows = (C.c_int64 * nb)(*rows)
    lptr, rptr, optr = (C.c_void_p * nb)(*lhs_ptrs), (C.c_void_p * nb)(*rhs_ptrs), (C.c_void_p * nb)(*outs)
    lcod, lkeep = capi._operand_coding(lhs_coding, nb)
    rcod, rkeep = capi._operand_coding(rhs_coding, nb)
    cptr = C.c_void_p(counts.data_ptr())

    def call():
        check(lib.qsx_select_cmp_columns_blocks(T.DATE, T.DATE, nb, c_rows, lptr, lcod, rptr, rcod, T.LT, None, optr, cptr, stream()),
              "qsx_select_cmp_columns_blocks")
    call.keep = (c_rows, lptr, rptr, optr, lkeep, rkeep, counts)
    return call


def columns_call(lhs_ptr, rhs_ptr, rows, out_ptr, count):
    cptr = C.c_void_p(count.data_ptr())

    def call():
        check(lib.qsx_select_cmp_columns(T.DATE, C.c_void_p(lhs_ptr), C.c_void_p(rhs_ptr), rows, T.LT, None, C.c_void_p(out_ptr), cptr, stream()),
              "qsx_select_cmp_columns")
    return call


# ---- the data: one dictionary of ENTRIES ascending dates, two code stripes, and the stripes decoded -----------------------------
days = np.arange(ENTRIES)
dictionary_np = np.array([T.date_raw(1992 + d // 372, 1 + (d % 372) // 31, 1 + d % 31) for d in days], dtype=np.int64)
dictionary = torch.from_numpy(dictionary_np).to(dev)
g = torch.Generator(device=dev)
g.manual_seed(12)
codes_l = torch.randint(0, ENTRIES, (n,), dtype=torch.int16, device=dev, generator=g)
codes_r = torch.randint(0, ENTRIES, (n,), dtype=torch.int16, device=dev, generator=g)
plain_l = dictionary[codes_l.long()]
plain_r = dictionary[codes_r.long()]
nb = n // BLOCK_ROWS
dictionaries = dictionary.repeat(2 * nb, 1).contiguous()        # every block and side its own copy (2 x nb x 20 KB)
words = (n + 63) // 64
bitmap_bytes = words * 8

# ---- (a) plain stripes: one block through the new entry point / the baseline --------------------------------------------------
out_new, out_base = capi.new_bitmap(n, dev), capi.new_bitmap(n, dev)
count_new, count_base = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
new_one = blocks_call([plain_l.data_ptr()], [plain_r.data_ptr()], [n], [out_new.data_ptr()], count_new)
base_one = columns_call(plain_l.data_ptr(), plain_r.data_ptr(), n, out_base.data_ptr(), count_base)
new_one()
base_one()
torch.cuda.synchronize()
same = bool(torch.equal(out_new[:words], out_base[:words])) and int(count_new.item()) == int(count_base.item())
plain_bytes = 16 * n + bitmap_bytes
t_base, t_new = timed([base_one, new_one])
report("a", "qsx_select_cmp_columns (baseline)", t_base, plain_bytes, matches=int(count_base.item()))
report("a", "qsx_select_cmp_columns_blocks, 1 block", t_new, plain_bytes, equals_baseline=same,
       slower_than_baseline_by_more_than_its_spread=bool(t_new[0] > t_base[2]))

# ---- (b) 2-byte codes on both sides, a dictionary per block, all blocks in one launch ------------------------------------------
rows_b = [BLOCK_ROWS] * nb
outs_b = capi.new_bitmap(n, dev)          # BLOCK_ROWS is a multiple of 64: the blocks' bitmaps lie back to back
counts_b = torch.zeros(nb, dtype=torch.int64, device=dev)
row_bytes = dictionaries.stride(0) * 8
coded = blocks_call([codes_l.data_ptr() + 2 * b * BLOCK_ROWS for b in range(nb)], [codes_r.data_ptr() + 2 * b * BLOCK_ROWS for b in range(nb)], rows_b,
                    [outs_b.data_ptr() + (b * BLOCK_ROWS // 64) * 8 for b in range(nb)], counts_b,
                    lhs_coding=[(2, dictionaries[2 * b], ENTRIES) for b in range(nb)], rhs_coding=[(2, dictionaries[2 * b + 1], ENTRIES) for b in range(nb)])
assert BLOCK_ROWS % 64 == 0 and row_bytes == ENTRIES * 8
coded()
torch.cuda.synchronize()
coded_same = bool(torch.equal(outs_b[:words], out_base[:words])) and int(counts_b.sum().item()) == int(count_base.item())

# ---- (c) decode both stripes, then the baseline ----------------------------------------------------------------------------------
dec_l, dec_r = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
out_c, count_c = capi.new_bitmap(n, dev), torch.zeros(1, dtype=torch.int64, device=dev)
cmp_decoded = columns_call(dec_l.data_ptr(), dec_r.data_ptr(), n, out_c.data_ptr(), count_c)


def decode_then_compare():
    check(lib.qsx_decode_codes(2, C.c_void_p(codes_l.data_ptr()), n, C.c_void_p(dictionary.data_ptr()), 8, C.c_void_p(dec_l.data_ptr()), stream()), "qsx_decode_codes")
    check(lib.qsx_decode_codes(2, C.c_void_p(codes_r.data_ptr()), n, C.c_void_p(dictionary.data_ptr()), 8, C.c_void_p(dec_r.data_ptr()), stream()), "qsx_decode_codes")
    cmp_decoded()


decode_then_compare()
torch.cuda.synchronize()
decoded_same = bool(torch.equal(out_c[:words], out_base[:words]))
t_coded, t_decoded = timed([coded, decode_then_compare])
report("b", f"qsx_select_cmp_columns_blocks, {nb} blocks of {BLOCK_ROWS} rows, 2-byte codes on both sides", t_coded, 4 * n + bitmap_bytes,
       equals_plain_result=coded_same, dictionary_entries=ENTRIES, dictionary_bytes_per_block_and_side=ENTRIES * 8)
report("c", "2 x qsx_decode_codes + qsx_select_cmp_columns", t_decoded, 2 * (2 + 8) * n + 16 * n + bitmap_bytes, equals_plain_result=decoded_same)

# ---- (d) 64 plain blocks: one launch / 64 launches --------------------------------------------------------------------------------
k = 64
rows_d = [BLOCK_ROWS] * k
lp = [plain_l.data_ptr() + 8 * b * BLOCK_ROWS for b in range(k)]
rp = [plain_r.data_ptr() + 8 * b * BLOCK_ROWS for b in range(k)]
op = [out_new.data_ptr() + (b * BLOCK_ROWS // 64) * 8 for b in range(k)]
counts_d = torch.zeros(k, dtype=torch.int64, device=dev)
one_launch = blocks_call(lp, rp, rows_d, op, counts_d)
per_block_new = [blocks_call([lp[b]], [rp[b]], [BLOCK_ROWS], [op[b]], counts_d[b:b + 1]) for b in range(k)]
per_block_base = [columns_call(lp[b], rp[b], BLOCK_ROWS, op[b], counts_d[b:b + 1]) for b in range(k)]


def launches_new():
    for call in per_block_new:
        call()


def launches_base():
    for call in per_block_base:
        call()


t_one, t_many_new, t_many_base = timed([one_launch, launches_new, launches_base])
bytes_d = k * BLOCK_ROWS * 16 + k * BLOCK_ROWS // 8
n_all, n = n, k * BLOCK_ROWS
report("d", f"qsx_select_cmp_columns_blocks, {k} blocks of {BLOCK_ROWS} rows in one launch", t_one, bytes_d)
report("d", f"{k} x qsx_select_cmp_columns_blocks with one block", t_many_new, bytes_d)
report("d", f"{k} x qsx_select_cmp_columns", t_many_base, bytes_d)
n = n_all

if out_path:
    with open(out_path, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
