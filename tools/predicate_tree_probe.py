#!/usr/bin/env python3
"""IN lists and the boolean evaluator on an MI355X: ms per call (median of 10 after 3 warm-ups), one JSON line per configuration.

  * qsx_select_in / qsx_select_in_char with K = 1, 2, 4, 7, 32 literals over INT, CHAR(2) and CHAR(10) stripes, and over 1-byte
    codes through the code set (the list against a 150-entry dictionary, then qsx_select_codes_in_set);
  * beside each: ONE qsx_select_cmp / qsx_select_cmp_char / qsx_select_codes with = on the same stripe (the yardstick: an existing
    kernel reading the same bytes) and the composition without IN lists: K equality calls plus K - 1 qsx_bitmap_combine;
  * a 20-leaf Q19-shaped program through qsx_bitmap_eval next to 19 qsx_bitmap_combine calls;
  * qsx_bitmap_eval_blocks over 64 blocks of 120 K rows next to 64 qsx_bitmap_eval calls.

Every IN result is checked against the composition's bitmap before it is timed.

usage: predicate_tree_probe.py [rows_millions] [out.jsonl]   (100 M rows by default; the lines go to stdout and, when given, the file)"""
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
KS = (1, 2, 4, 7, 32)


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


def report(call, med_lo_hi, **more):
    med, lo, hi = med_lo_hi
    emit(dict({"call": call, "rows": n, "ms": round(med, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4)}, **more))


def composed(equal, literals, scratch):
    """K equality calls and K - 1 unions: what a caller without IN lists runs."""
    acc = equal(literals[0])
    for lit in literals[1:]:
        acc = capi.bitmap_combine(1, acc, equal(lit), n, out=scratch)
    return acc


def in_list_block(name, one_equal, in_call, literals_of, floor_ms, **more):
    scratch = capi.new_bitmap(n, dev)
    report(one_equal[0], timed(lambda: one_equal[1](literals_of(1)[0])), stripe_bytes_over_hbm_peak_ms=round(floor_ms, 4), **more)
    for k in KS:
        literals = literals_of(k)
        want = composed(one_equal[1], literals, scratch).clone()
        got, count = in_call(literals)
        same = bool(torch.equal(got, want))
        ms_in = timed(lambda: in_call(literals))
        ms_composed = timed(lambda: composed(one_equal[1], literals, scratch))
        report(name, ms_in, k=k, matches=int(count.item()), equals_composition=same, stripe_bytes_over_hbm_peak_ms=round(floor_ms, 4), **more)
        report(f"{k} x {one_equal[0]} + {k - 1} x qsx_bitmap_combine", ms_composed, k=k, **more)


# ---- INT
col = torch.randint(0, 50, (n,), device=dev, generator=g, dtype=torch.int32)
in_list_block("qsx_select_in", ("qsx_select_cmp", lambda lit: capi.select_cmp(col, T.EQ, lit)[0]), lambda lits: capi.select_in(col, lits),
              lambda k: [(7 * i + 3) % 64 for i in range(k)], 4 * n / 8e12 * 1e3, type="INT")
del col

# ---- CHAR(2) (a phone prefix) and CHAR(10) (l_shipmode)
VALUES = {2: [b"%02d" % i for i in range(10, 35)], 10: [b"MAIL", b"SHIP", b"AIR", b"REG AIR", b"TRUCK", b"RAIL", b"FOB"]}
MISSES = {2: [b"%02d" % i for i in range(40, 72)], 10: [b"miss%02d" % i for i in range(32)]}
for width in (2, 10):
    words = torch.zeros((len(VALUES[width]), width), dtype=torch.uint8, device=dev)
    for i, w in enumerate(VALUES[width]):
        words[i, :len(w)] = torch.tensor(list(w), dtype=torch.uint8, device=dev)
    ccol = words[torch.randint(0, len(VALUES[width]), (n,), device=dev, generator=g)].contiguous()

    def char_literals(k, width=width):   # half of them present in the column
        return [(VALUES[width][i // 2 % len(VALUES[width])] if i % 2 == 0 else MISSES[width][i]) for i in range(k)]

    in_list_block("qsx_select_in_char", ("qsx_select_cmp_char", lambda lit: capi.select_cmp_char(ccol, T.EQ, lit)[0]),
                  lambda lits: capi.select_in_char(ccol, lits), char_literals, width * n / 8e12 * 1e3, width=width)
    del ccol

# ---- 1-byte codes through the code set
NUM_CODES = 150
dictionary = torch.zeros((NUM_CODES, 10), dtype=torch.uint8, device=dev)
for i in range(NUM_CODES):
    text = b"value%03d" % i
    dictionary[i, :len(text)] = torch.tensor(list(text), dtype=torch.uint8, device=dev)
codes = torch.randint(0, NUM_CODES, (n,), device=dev, generator=g, dtype=torch.int32).to(torch.uint8)


def in_through_code_set(codes_of_literals):
    code_set, _ = capi.select_in_char(dictionary, [b"value%03d" % c for c in codes_of_literals], want_count=False)
    return capi.select_codes_in_set(codes, code_set, NUM_CODES)


in_list_block("qsx_select_in_char(dictionary) + qsx_select_codes_in_set", ("qsx_select_codes", lambda code: capi.select_codes(codes, T.CODE_EQ, code)[0]),
              in_through_code_set, lambda k: [(11 * i + 5) % NUM_CODES for i in range(k)], n / 8e12 * 1e3, code_width=1, num_codes=NUM_CODES)
del codes

# ---- the evaluator: a Q19-shaped program of 20 leaves (three OR-ed conjunctions of 6, 7 and 7 leaves), at n and at 4 n rows (the
# difference of the two is what the rows cost; the rest is the call: the table's upload and the launch)
program, at = [], 0
for group, size in enumerate((6, 7, 7)):
    for k in range(size):
        program += [at] + ([T.BOOL_AND] if k else [])
        at += 1
    program += [T.BOOL_OR] if group else []
for rows_here in (n, 4 * n):
    words_here = (rows_here + 63) // 64
    leaves = [torch.randint(-2**62, 2**62, (words_here,), device=dev, generator=g, dtype=torch.int64) for _ in range(20)]
    out = capi.new_bitmap(rows_here, dev)
    a, b = capi.new_bitmap(rows_here, dev), capi.new_bitmap(rows_here, dev)

    def nineteen_combines():
        at = 0
        for group, size in enumerate((6, 7, 7)):
            acc = leaves[at]
            for k in range(1, size):
                acc = capi.bitmap_combine(0, acc, leaves[at + k], rows_here, out=a)
            at += size
            if group:
                capi.bitmap_combine(1, b, a, rows_here, out=b)
            else:
                b.copy_(a)
        return b

    got, count = capi.bitmap_eval(leaves, program, rows_here, out_bitmap=out)
    same = bool(torch.equal(got, nineteen_combines()))
    leaf_bytes_ms = 21 * words_here * 8 / 8e12 * 1e3       # 20 leaves read, one bitmap written
    med = timed(lambda: capi.bitmap_eval(leaves, program, rows_here, out_bitmap=out))
    emit({"call": "qsx_bitmap_eval", "rows": rows_here, "leaves": 20, "instrs": len(program), "ms": round(med[0], 4), "min_ms": round(med[1], 4),
          "max_ms": round(med[2], 4), "equals_composition": same, "bytes_over_hbm_peak_ms": round(leaf_bytes_ms, 4)})
    med = timed(nineteen_combines)
    emit({"call": "19 x qsx_bitmap_combine (+ 1 copy)", "rows": rows_here, "leaves": 20, "ms": round(med[0], 4), "min_ms": round(med[1], 4),
          "max_ms": round(med[2], 4)})
    del leaves, out, a, b

# ---- the evaluator over a run: 64 blocks of 120 K rows
BLOCKS, BLOCK_ROWS = 64, 120_000
block_leaves = [[torch.randint(-2**62, 2**62, ((BLOCK_ROWS + 63) // 64,), device=dev, generator=g, dtype=torch.int64) for _ in range(20)]
                for _ in range(BLOCKS)]
outs = [capi.new_bitmap(BLOCK_ROWS, dev) for _ in range(BLOCKS)]
rows = [BLOCK_ROWS] * BLOCKS


def per_block():
    for b in range(BLOCKS):
        capi.bitmap_eval(block_leaves[b], program, BLOCK_ROWS, out_bitmap=outs[b])


run_outs, run_counts = capi.bitmap_eval_blocks(block_leaves, program, rows, dev)
per_block()
same = all(bool(torch.equal(a, b)) for a, b in zip(run_outs, outs))
med = timed(lambda: capi.bitmap_eval_blocks(block_leaves, program, rows, dev, out_bitmaps=outs))
emit({"call": "qsx_bitmap_eval_blocks", "blocks": BLOCKS, "block_rows": BLOCK_ROWS, "leaves": 20, "ms": round(med[0], 4), "min_ms": round(med[1], 4),
      "max_ms": round(med[2], 4), "equals_per_block": same})
med = timed(per_block)
emit({"call": "64 x qsx_bitmap_eval", "blocks": BLOCKS, "block_rows": BLOCK_ROWS, "leaves": 20, "ms": round(med[0], 4), "min_ms": round(med[1], 4),
      "max_ms": round(med[2], 4)})

if out_path:
    with open(out_path, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
