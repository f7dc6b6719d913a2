#!/usr/bin/env python3
"""qsx_agg_state_clear through the memsets and through the one-kernel clear, over table sizes: where is the threshold?

    python tools/agg_clear_threshold.py profiles/clear_threshold.jsonl

50 clears back to back per size and path (QSX_AGG_CLEAR_ONE_KERNEL_WORDS is read per call), us per clear between two events."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quickstep_amd.capi as capi
from quickstep_amd import types as T

dev = torch.device("cuda:0")
out = open(sys.argv[1], "w")
for est in (6, 100, 1000, 4000, 16000, 64000, 250000, 1000000):
    cfg = T.make_agg_config(T.AGG_GENERIC, [(T.INT, None), (T.DOUBLE, None)], keys=[0],
                            aggs=[(T.AGG_SUM, T.col(1)), (T.AGG_MIN, T.col(1)), (T.AGG_COUNT_STAR, None)], est_groups=est)
    st = capi.AggState(cfg)
    dense, header, per_col, kinds = st.image_layout()
    words = header + per_col * len(kinds)
    line = {"est_groups": est, "image_words": words}
    for name, env in (("memsets", "0"), ("one_kernel", str(1 << 40))):
        os.environ["QSX_AGG_CLEAR_ONE_KERNEL_WORDS"] = env
        for _ in range(5):
            st.clear()
        torch.cuda.synchronize()
        # back to back: the device time of the clears as the stream sees them (launch-bound when the fills are small)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(50):
            st.clear()
        b.record()
        torch.cuda.synchronize()
        line[name + "_us"] = a.elapsed_time(b) * 1e3 / 50
    print(json.dumps(line), file=out, flush=True)
    print(json.dumps(line))
    st.close()
