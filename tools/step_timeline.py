#!/usr/bin/env python3
"""The device timeline of one headline step, from a rocprofv3 trace.

    rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d OUT -o trace -- python bench.py --gpus 1 --steps 20 --warmup 5
    python tools/step_timeline.py OUT/trace_kernel_trace.csv [OUT/trace_memory_copy_trace.csv] > profiles/NAME.md

Lists every device operation from the end of one launch of the anchor kernel (the Q1 aggregation update) to the end of the next:
start and end relative to the first anchor's end, duration, and the idle gap in front of the operation (start minus the latest
end seen so far).  The step taken is the one before the last anchor pair (--step counts back from the end), a timed step."""
import argparse
import csv
import re


def short(name):
    name = re.sub(r"^void ", "", name)
    name = re.sub(r"\(anonymous namespace\)::", "", name)
    m = re.match(r"(at::native::)?([\w:]+)<(.*)", name)
    if m and m.group(1):                                        # a torch elementwise kernel: keep the functor
        f = re.search(r"at::native::(\w*Functor<\w+>)", name)
        return "torch " + m.group(2) + ("<" + f.group(1) + ">" if f else "")
    name = re.sub(r"\(.*$", "", name)
    return name if len(name) <= 70 else name[:67] + "..."


def rows_of(path, kind):
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            if kind == "kernel":
                yield int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"]), r["Grid_Size_X"], r["Workgroup_Size_X"]
            else:
                yield int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "copy " + r.get("Direction", "") + " " + r.get("Bytes", "") + " B", "", ""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("kernel_trace")
    ap.add_argument("memory_copy_trace", nargs="?")
    ap.add_argument("--anchor", default="agg_stream_kernel", help="substring of the kernel that delimits a step")
    ap.add_argument("--step", type=int, default=2, help="which step, counted back from the last (1 = the last)")
    args = ap.parse_args()
    ops = list(rows_of(args.kernel_trace, "kernel"))
    if args.memory_copy_trace:
        ops += list(rows_of(args.memory_copy_trace, "copy"))
    ops.sort()
    anchors = [i for i, o in enumerate(ops) if args.anchor in o[2]]
    assert len(anchors) > args.step, f"fewer than {args.step + 1} launches of a kernel named *{args.anchor}*"
    first, second = anchors[-args.step - 1], anchors[-args.step]
    t0 = ops[first][1]
    latest_end = t0
    print(f"| # | operation | work-items x workgroup | start us | end us | duration us | idle before us |")
    print(f"|---|---|---|---|---|---|---|")
    busy = 0
    for n, (start, end, name, grid, block) in enumerate(ops[first + 1:second + 1], 1):
        gap = max(0, start - latest_end)
        shape = f"{grid} x {block}" if grid else ""
        print(f"| {n} | `{name}` | {shape} | {(start - t0) / 1e3:.1f} | {(end - t0) / 1e3:.1f} | {(end - start) / 1e3:.1f} | {gap / 1e3:.1f} |")
        busy += end - max(start, latest_end) if end > latest_end else 0
        latest_end = max(latest_end, end)
    span = ops[second][1] - t0
    print()
    print(f"{second - first} operations, {span / 1e3:.1f} us from the end of one `{args.anchor}` to the end of the next; "
          f"the device is busy for {busy / 1e3:.1f} us of them and idle for {(span - busy) / 1e3:.1f} us.")


if __name__ == "__main__":
    main()
