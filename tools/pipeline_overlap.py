#!/usr/bin/env python3
"""Steady state of the headline pipeline from a rocprofv3 kernel trace: medians of the row reduction's and the resolver's durations
and of the period (resolver end to resolver end), over the second half of the trace.
usage: python tools/pipeline_overlap.py <tag> <kernel_trace.csv>   (one line)"""
import csv
import sys
from statistics import median

rows = list(csv.DictReader(open(sys.argv[2])))
ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].split("(")[0].replace("void ", "")) for r in rows)
ev = [e for e in ev if e[2].startswith("k_bulk") or e[2] == "k_resolve"]
ev = ev[len(ev) // 2:]
red = [e for e in ev if e[2].startswith("k_bulk")]
res = [e for e in ev if e[2] == "k_resolve"]
per = [(b[1] - a[1]) / 1e3 for a, b in zip(res[:-1], res[1:])]
ovl = [max(0, a[1] - b[0]) / 1e3 for a, b in zip(red[:-1], red[1:])]
# a reduction starts behind the resolver two sweeps back (same stream): the gap between the last resolver end before it and its start
ends = sorted(e[1] for e in res)
gap = []
for e in red:
    before = [x for x in ends if x <= e[0]]
    if before:
        gap.append((e[0] - before[-1]) / 1e3)
print(f"{sys.argv[1]} launches {len(red)} ({red[0][2]}) period med {median(per):.1f} us reduction med {median((e[1] - e[0]) / 1e3 for e in red):.1f} us "
      f"overlap of consecutive reductions med {median(ovl):.1f} us resolver med {median((e[1] - e[0]) / 1e3 for e in res):.1f} us "
      f"resolver end to next reduction start med {median(gap) if gap else float('nan'):.1f} us")
