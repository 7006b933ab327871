#!/usr/bin/env python3
"""Where a sampler-lane launch of one kernel spends its time, from a rocprofv3 *kernel_trace.csv of the two-lane loop.
For every launch of <kernel> at <grid> workgroups (the lane shape): its duration; the gap from the end of the previous kernel on the same
stream to its start; and how much of [start, end] the other stream's kernels cover, in total and by the other lane's <other> kernel
(default: the attention).  The trace stamps say when a dispatch starts and ends, not when its first workgroup ran, so the gap is the queue's
latency and what the duration holds beyond the kernel's isolated time is the wait for CUs that the other lane's workgroups hold.
usage: trace_lanes.py <dir or file> [kernel] [grid] [other]   (default: d3pm_layer_h2_kernel<true, false> 256 d3pm_attention_v4_kernel)
-> one CSV row of medians and means over the launches"""
import bisect
import csv
import glob
import os
import statistics
import sys

root = sys.argv[1]
kern = sys.argv[2] if len(sys.argv) > 2 else "d3pm_layer_h2_kernel<true, false>"
grid = int(sys.argv[3]) if len(sys.argv) > 3 else 256
other = sys.argv[4] if len(sys.argv) > 4 else "d3pm_attention_v4_kernel"
files = [root] if os.path.isfile(root) else glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True)
rows = []
for f in files:
    for r in csv.DictReader(open(f)):
        wgs = (int(r["Grid_Size_X"]) // max(int(r["Workgroup_Size_X"]), 1)) * int(r["Grid_Size_Y"]) * int(r["Grid_Size_Z"])
        rows.append((r["Stream_Id"], int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], wgs))
by_stream = {}
for s, t0, t1, name, wgs in sorted(rows, key=lambda x: x[1]):
    by_stream.setdefault(s, []).append((t0, t1, name, wgs))


def covered(ivs, a, b):
    """time of [a, b] covered by the union of the (sorted by start) intervals ivs"""
    tot, cur = 0, a
    for t0, t1 in ivs:
        if t1 <= cur:
            continue
        if t0 >= b:
            break
        lo, hi = max(t0, cur), min(t1, b)
        if hi > lo:
            tot += hi - lo
            cur = hi
    return tot


dur, gap, cov_any, cov_other = [], [], [], []
for s, ks in by_stream.items():
    others = [(t0, t1, n) for s2, ks2 in by_stream.items() if s2 != s for t0, t1, n, _ in ks2]
    others.sort()
    starts = [o[0] for o in others]
    for i, (t0, t1, name, wgs) in enumerate(ks):
        if kern not in name or wgs != grid:
            continue
        dur.append((t1 - t0) / 1e3)
        if i > 0:
            gap.append((t0 - ks[i - 1][1]) / 1e3)
        j0 = max(bisect.bisect_left(starts, t0) - 64, 0)            # earlier starts that may still run at t0
        near = [o for o in others[j0:] if o[0] < t1]
        cov_any.append(covered([(a, b) for a, b, _ in near], t0, t1) / 1e3)
        cov_other.append(covered([(a, b) for a, b, n in near if other in n], t0, t1) / 1e3)
if not dur:
    sys.exit(f"no launches of {kern} at grid {grid}")
print("kernel,grid_workgroups,launches,duration_med_us,duration_mean_us,gap_after_prev_on_stream_med_us,"
      "overlap_other_stream_med_us,overlap_other_kernel_med_us,overlap_other_kernel_mean_us")
print(f"{kern.replace(', ', ';')},{grid},{len(dur)},{statistics.median(dur):.1f},{statistics.mean(dur):.1f},"
      f"{statistics.median(gap):.1f},{statistics.median(cov_any):.1f},{statistics.median(cov_other):.1f},{statistics.mean(cov_other):.1f}")
