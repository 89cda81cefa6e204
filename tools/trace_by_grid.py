#!/usr/bin/env python3
"""rocprofv3 --kernel-trace CSV -> per (kernel, workgroups): calls, avg / min / max duration in microseconds.
   python tools/trace_by_grid.py <kernel_trace.csv>
   python tools/trace_by_grid.py --signature <kernel_trace.csv>
--signature prints no timings: the multiset of (kernel with its template arguments, workgroups, workgroup size,
LDS_Block_Size) with call counts, one sorted line each -- two runs launched the same work when these outputs are equal."""
import collections
import csv
import re
import sys

signature = "--signature" in sys.argv[1:]
path = [a for a in sys.argv[1:] if a != "--signature"][0]
rows = list(csv.DictReader(open(path)))
agg = collections.defaultdict(list)
for r in rows:
    name = r["Kernel_Name"].replace("void ", "").replace("(anonymous namespace)::", "")
    if not signature:
        name = re.sub(r"\(.*$", "", name)
    wg = max(1, int(r["Workgroup_Size_X"]) * int(r.get("Workgroup_Size_Y") or 1) * int(r.get("Workgroup_Size_Z") or 1))
    wgs = int(r["Grid_Size_X"]) * int(r.get("Grid_Size_Y") or 1) * int(r.get("Grid_Size_Z") or 1) // wg
    key = (name, wgs, wg, int(r.get("LDS_Block_Size") or 0)) if signature else (name, wgs)
    agg[key].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
for key, v in sorted(agg.items()):
    if signature:
        print("%s wgs=%d wg=%d lds=%d calls=%d" % (key + (len(v),)))
    else:
        print("%-44s wgs=%6d calls=%4d avg=%9.2f min=%9.2f max=%9.2f" % (key[0][:44], key[1], len(v), sum(v) / len(v), min(v), max(v)))
