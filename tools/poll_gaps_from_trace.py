#!/usr/bin/env python3
"""Where the device stands empty inside a K-pivot solve call, from a rocprofv3 --kernel-trace CSV
(the stamps tools/hop_from_trace.py reads): every stretch with NO kernel running between the first
and the last k_ov2 kernel of a call, with the number of working sweeps before it.  A host poll that
lets the queue run dry shows as one long stretch; an ordinary step boundary as the hand-over hop.
python tools/poll_gaps_from_trace.py <kernel_trace.csv> [idle_us_listed=25] [min_sweeps=10]"""
import csv
import json
import statistics
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
listed_us = float(sys.argv[2]) if len(sys.argv) > 2 else 25.0
min_sweeps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
name_key = "Kernel_Name" if "Kernel_Name" in rows[0] else "Name"
ks = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r[name_key]) for r in rows)

# calls: runs of kernels in which consecutive k_ov2 kernels start less than 2 ms apart
calls, cur, last = [], [], None
for s, e, nm in ks:
    if "k_ov2_" in nm:
        if last is not None and s - last > 2_000_000:
            calls.append(cur)
            cur = []
        last = s
    if "k_ov2_" in nm or cur:
        cur.append((s, e, nm))
if cur:
    calls.append(cur)

out = []
for c in calls:
    while c and "k_ov2_" not in c[-1][2]:
        c.pop()  # (copies after the last step belong to the final poll)
    work = [(s, e) for s, e, nm in c if "k_ov2_sweep" in nm and e - s >= 100_000]
    if len(work) < min_sweeps:
        continue
    idle, hops, busy_to, nwork = [], [], c[0][1], 0
    for s, e, nm in c:
        if s > busy_to:
            gap = (s - busy_to) / 1e3
            hops.append(gap)
            if gap >= listed_us:
                idle.append({"after_working_sweeps": nwork, "idle_us": round(gap, 1)})
        if "k_ov2_sweep" in nm and e - s >= 100_000:
            nwork += 1
        busy_to = max(busy_to, e)
    span = (c[-1][1] - c[0][0]) / 1e3
    out.append({"working_sweeps": len(work), "heads": sum("k_ov2_heads" in nm for _, _, nm in c),
                "sweeps": sum("k_ov2_sweep" in nm for _, _, nm in c),
                "copies": sum("copyBuffer" in nm for _, _, nm in c),
                "span_us": round(span, 1), "idle_stretches": len(hops),
                "idle_median_us": round(statistics.median(hops), 2) if hops else None,
                "idle_total_us": round(sum(hops), 1),
                "listed": idle, "listed_total_us": round(sum(i["idle_us"] for i in idle), 1),
                "listed_share_of_call": round(sum(i["idle_us"] for i in idle) / span, 4)})
print(json.dumps(out))
