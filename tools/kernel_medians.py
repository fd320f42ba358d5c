"""Durations per kernel and grid from a rocprofv3 --kernel-trace --output-format csv directory: launches, median, min and max in us (End - Start), the first
two launches of every (kernel, grid) dropped.  usage: python tools/kernel_medians.py <dir> [substring of the kernel names to keep] [rounds]
   rounds: the same per ROUND instead -- a round is a run of consecutive launches of one (kernel, grid) among the kept kernels, in start
           order (tools/detect_time.py --harris alternates a kernel and its sibling); the first two launches of a round are dropped"""
import csv, glob, statistics, sys
f = glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)[0]
keep = sys.argv[2] if len(sys.argv) > 2 else "vstab"
by_round = len(sys.argv) > 3 and sys.argv[3] == "rounds"
runs, order = {}, []
for r in csv.DictReader(open(f)):
    if keep in r["Kernel_Name"]:
        name = r["Kernel_Name"].split("(")[0].split("::")[-1]
        grid = int(r.get("Grid_Size") or r.get("Grid_Size_X") or 0)
        runs.setdefault((name, grid), []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
        order.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name, grid))


def line(name, grid, d, tag=""):
    print(f"{tag}{name:32s} grid {grid:9d}  launches {len(d):4d}  median {statistics.median(d):8.2f}  min {min(d):8.2f}  max {max(d):8.2f} us")


if by_round:
    rounds = []
    for s, e, name, grid in sorted(order):
        if not rounds or rounds[-1][0] != (name, grid):
            rounds.append(((name, grid), []))
        rounds[-1][1].append((e - s) / 1000.0)
    seen = {}
    for (name, grid), d in rounds:
        seen[(name, grid)] = seen.get((name, grid), 0) + 1
        if len(d) > 2:
            line(name, grid, d[2:], "round %d  " % seen[(name, grid)])
else:
    for (name, grid), v in sorted(runs.items()):
        d = [(e - s) / 1000.0 for s, e in sorted(v)][2:]
        if d:
            line(name, grid, d)
