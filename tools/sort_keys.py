#!/usr/bin/env python3
"""ORDER BY with NULL ordering and CHAR(n) keys (qsx_sort_permutation_keys / qsx_sort_top_k_keys) next to the plain entry points.

  sort_keys.py [rows] [calls]              measurements 1-3 below, one JSON line each
  sort_keys.py --ab OTHER_LIB [rows] [calls]   the plain entry points of this build and of another libqsx.so (the parent
                                               commit's), alternating in one process: the regression check

1. `rows` (12.8 M) rows ordered by DOUBLE DESC, DATE (the Q3 shape, NULL-free): qsx_sort_permutation and
   qsx_sort_permutation_keys on the same data, and the two top-k calls with k = 10.
2. The same with 10 % NULLs in key 0, NULLS FIRST and NULLS LAST.
3. 10 M rows (rows / 1.28) ordered by a CHAR(15) key with 5 distinct values and by a CHAR(25) key of random names, each with the
   digit skipping and without it (the library's qsx_debug_sort_keys_skip_digits hook).
HIP events around every call, two warm-up calls per form, then `calls` (7) timed calls per form, the forms of one measurement
alternating; median, min and max in ms.  `launches` is the number of kernel launches of one call: counted by the library for
the *_keys calls (qsx_debug_sort_keys_launches: a digit pass = 3, the top-k selection's launches included), computed for
qsx_sort_permutation (1 + per key 1 + 3 x ceil(bits / 6)), not stated (-1) for qsx_sort_top_k."""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quickstep_amd.capi as capi  # noqa: E402
from quickstep_amd import types as T  # noqa: E402

args = sys.argv[1:]
other_lib = None
if args and args[0] == "--ab":
    other_lib, args = args[1], args[2:]
n = int(args[0]) if len(args) > 0 else 12_800_000
calls = int(args[1]) if len(args) > 1 else 7
dev = torch.device("cuda:0")
rng = np.random.default_rng(31)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


capi.lib.qsx_debug_sort_keys_launches.restype = C.c_longlong
capi.lib.qsx_debug_sort_keys_skip_digits.restype = C.c_int
capi.lib.qsx_debug_sort_keys_skip_digits.argtypes = [C.c_int]


def measure(what, rows, forms):
    """forms: name -> (callable, launches or None = the library's count for the call, digit skipping on / off)."""
    ms = {name: [] for name in forms}
    outs, launches = {}, {}
    for rounds in (2, calls):
        for _ in range(rounds):
            for name, (fn, count, skip) in forms.items():
                capi.lib.qsx_debug_sort_keys_skip_digits(1 if skip else 0)
                before = capi.lib.qsx_debug_sort_keys_launches()
                t, outs[name] = timed(fn)
                launches[name] = capi.lib.qsx_debug_sort_keys_launches() - before if count is None else count
                capi.lib.qsx_debug_sort_keys_skip_digits(1)
                if rounds == calls:
                    ms[name].append(t)
    first = next(iter(outs.values()))
    for name in forms:
        assert torch.equal(outs[name], first), (what, name)            # every form of a measurement gives the same permutation
        line = {"tool": "sort_keys", "measurement": what, "form": name, "rows": rows, "calls": calls, "launches": launches[name],
                "median_ms": round(statistics.median(ms[name]), 3), "min_ms": round(min(ms[name]), 3), "max_ms": round(max(ms[name]), 3)}
        print(json.dumps(line), flush=True)


def bitmap(nulls):
    bits = np.zeros((nulls.size + 63) // 64 * 64, dtype=np.uint8)
    bits[:nulls.size] = nulls
    return torch.from_numpy(np.packbits(bits).view(">u8").astype(np.uint64).view(np.int64)).to(dev)


def plain_launches(bits_per_key):
    return 1 + sum(1 + 3 * ((b + 5) // 6) for b in bits_per_key)


revenue = torch.from_numpy(np.round(rng.uniform(1000, 500000, size=n), 4)).to(dev)
orderdate = torch.from_numpy((rng.integers(1992, 1999, size=n).astype(np.int64)) | (rng.integers(1, 13, size=n).astype(np.int64) << 32)
                             | (rng.integers(1, 29, size=n).astype(np.int64) << 40)).to(dev)
q3_cols, q3_types, q3_desc = [revenue, orderdate], [T.DOUBLE, T.DATE], [True, False]

if other_lib is not None:
    # ---- 4. the plain entry points of two builds, alternating ----------------------------------------------------------
    libs = {"this commit": C.CDLL(capi.LIB_PATH), "parent commit": C.CDLL(other_lib)}
    ws_bytes = capi.lib.qsx_sort_workspace_bytes(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty(n, dtype=torch.int32, device=dev)
    ptrs = (C.c_void_p * 2)(revenue.data_ptr(), orderdate.data_ptr())
    types, desc = (C.c_int32 * 2)(*q3_types), (C.c_int32 * 2)(1, 0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(lib, top_k):
        def run():
            if top_k:
                rc = lib.qsx_sort_top_k(2, ptrs, types, desc, C.c_int64(n), C.c_int64(10), C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()),
                                        C.c_size_t(ws_bytes), stream)
            else:
                rc = lib.qsx_sort_permutation(2, ptrs, types, desc, C.c_int64(n), C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()),
                                              C.c_size_t(ws_bytes), stream)
            assert rc == 0, rc
            return out[:10].clone() if top_k else out.clone()
        return run
    measure("q3 shape, qsx_sort_permutation, two builds", n, {name: (call(lib, False), plain_launches([64, 64]), True) for name, lib in libs.items()})
    measure("q3 shape, qsx_sort_top_k k=10, two builds", n, {name: (call(lib, True), -1, True) for name, lib in libs.items()})
    sys.exit(0)

# ---- 1. the Q3 shape without NULLs -----------------------------------------------------------------------------------
plain_keys = [capi.SortKeySpec(c, t, 0, d) for c, t, d in zip(q3_cols, q3_types, q3_desc)]
measure("q3 shape, no NULLs", n, {
    "qsx_sort_permutation": (lambda: capi.sort_permutation(q3_cols, q3_desc, types=q3_types), plain_launches([64, 64]), True),
    "qsx_sort_permutation_keys": (lambda: capi.sort_permutation_keys(plain_keys), None, True),
    "qsx_sort_permutation_keys, no digit skipping": (lambda: capi.sort_permutation_keys(plain_keys), None, False),
})
measure("q3 shape, no NULLs, top 10", n, {
    "qsx_sort_top_k": (lambda: capi.sort_top_k(q3_cols, 10, q3_desc, types=q3_types), -1, True),
    "qsx_sort_top_k_keys": (lambda: capi.sort_top_k_keys(plain_keys, 10), None, True),
})

# ---- 2. 10 % NULLs in key 0 ----------------------------------------------------------------------------------------------
nulls = bitmap(rng.random(n) < 0.1)
forms = {}
for first in (True, False):
    keys = [capi.SortKeySpec(revenue, T.DOUBLE, 0, True, first, nulls), plain_keys[1]]
    forms["NULLS FIRST" if first else "NULLS LAST"] = (lambda keys=keys: capi.sort_permutation_keys(keys), None, True)
for name, form in forms.items():                      # (two orders: two results, one measurement each)
    measure("q3 shape, 10 % NULLs in key 0", n, {name: form})
for first in (True, False):
    keys = [capi.SortKeySpec(revenue, T.DOUBLE, 0, True, first, nulls), plain_keys[1]]
    measure("q3 shape, 10 % NULLs in key 0, top 10", n, {"NULLS FIRST" if first else "NULLS LAST": (lambda keys=keys: capi.sort_top_k_keys(keys, 10), None, True)})
del revenue, orderdate, nulls

# ---- 3. CHAR keys, with and without the digit skipping -------------------------------------------------------------------
m = int(n / 1.28)
priorities = np.zeros((5, 15), dtype=np.uint8)
for i, text in enumerate((b"1-URGENT", b"2-HIGH", b"3-MEDIUM", b"4-NOT SPECIFIED", b"5-LOW")):
    priorities[i, :len(text)] = np.frombuffer(text, dtype=np.uint8)
orderpriority = torch.from_numpy(priorities[rng.integers(0, 5, size=m)].reshape(-1)).to(dev)
names = np.zeros((m, 25), dtype=np.uint8)
names[:, :9] = np.frombuffer(b"Supplier#", dtype=np.uint8)
digits = rng.integers(0, 10, size=(m, 9)).astype(np.uint8) + ord("0")
names[:, 9:18] = digits
s_name = torch.from_numpy(names.reshape(-1)).to(dev)
for what, col, width in (("char(15), 5 distinct values", orderpriority, 15), ("char(25), random names", s_name, 25)):
    keys = [capi.SortKeySpec(col, T.CHAR, width)]
    measure(what, m, {
        "digit skipping": (lambda keys=keys: capi.sort_permutation_keys(keys), None, True),
        "no digit skipping": (lambda keys=keys: capi.sort_permutation_keys(keys), None, False),
    })
