#!/usr/bin/env python3
"""Keeps the screen kernel's rows of a rocprofv3 --pmc run's counter CSVs and prints the per-launch means.
    python tools/pmc_screen_rows.py DIR OUT.csv"""
import csv
import glob
import json
import os
import sys

rows, head = [], None
for p in glob.glob(os.path.join(sys.argv[1], "**", "*counter_collection.csv"), recursive=True):
    with open(p, newline="") as f:
        r = csv.reader(f)
        h = next(r)
        head = head or h
        ki = h.index("Kernel_Name")
        rows += [x for x in r if "pair_fp6_screen2w_kernel" in x[ki]]
if not rows:
    print("no screen kernel rows under", sys.argv[1])
    sys.exit(1)
gi = head.index("Grid_Size")  # (the whole-list launches: the sample run's grid is smaller)
g = max(int(x[gi]) for x in rows)
rows = [x for x in rows if int(x[gi]) == g]
with open(sys.argv[2], "w", newline="") as f:
    w = csv.writer(f, quoting=csv.QUOTE_NONNUMERIC)
    w.writerow(head)
    w.writerows(rows)
ci, vi, di = head.index("Counter_Name"), head.index("Counter_Value"), head.index("Dispatch_Id")
out = {}
for x in rows:
    out.setdefault(x[ci], []).append(float(x[vi]))
print(json.dumps({"kernel": rows[0][head.index("Kernel_Name")].split("(")[0], "launches": len({x[di] for x in rows}),
                  **{k: sum(v) / len(v) for k, v in sorted(out.items())}}))
