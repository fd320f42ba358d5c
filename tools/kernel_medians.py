"""Durations per kernel and grid from a rocprofv3 --kernel-trace --output-format csv directory: launches, median, min and max in us (End - Start), the first
two launches of every (kernel, grid) dropped.  usage: python tools/kernel_medians.py <dir> [substring of the kernel names to keep]"""
import csv, glob, statistics, sys
f = glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)[0]
keep = sys.argv[2] if len(sys.argv) > 2 else "vstab"
runs = {}
for r in csv.DictReader(open(f)):
    if keep in r["Kernel_Name"]:
        name = r["Kernel_Name"].split("(")[0].split("::")[-1]
        grid = int(r.get("Grid_Size") or r.get("Grid_Size_X") or 0)
        runs.setdefault((name, grid), []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
for (name, grid), v in sorted(runs.items()):
    d = [(e - s) / 1000.0 for s, e in sorted(v)][2:]
    if d:
        print(f"{name:32s} grid {grid:9d}  launches {len(d):4d}  median {statistics.median(d):8.2f}  min {min(d):8.2f}  max {max(d):8.2f} us")
