"""FETCH_SIZE / WRITE_SIZE per kernel of the captured PPO update, from two rocprofv3 counter
passes (one counter each, no tracing beside them) over tools/probes/update_time.py: the mean
over a kernel's dispatches, in MB per launch as the counters report them (KiB x 1024).  No
calibration copy is run here (tools/pmc_summary.py does that for one kernel): on gfx950
FETCH_SIZE counts a wide streaming read at half its bytes, so the read column is a lower bound
and comparable between builds, not an absolute figure.
usage: python tools/pmc_update_bytes.py <fetch_dir> <write_dir>"""
import collections
import csv
import glob
import os
import sys


def load(d):
    acc = collections.defaultdict(list)
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            acc[r["Kernel_Name"]].append(float(r["Counter_Value"]))
    return acc


def main(fetch, write):
    f, w = load(fetch), load(write)
    rows = []
    for k in sorted(set(f) | set(w)):
        fm = sum(f[k]) / len(f[k]) * 1024 / 1e6 if f.get(k) else 0.0
        wm = sum(w[k]) / len(w[k]) * 1024 / 1e6 if w.get(k) else 0.0
        rows.append((fm + wm, fm, wm, len(f.get(k, ())), k))
    print("FETCH_SIZE MB  WRITE_SIZE MB  dispatches  kernel")
    for _, fm, wm, n, k in sorted(rows, reverse=True)[:14]:
        print(f"{fm:13.2f}  {wm:13.2f}  {n:10d}  {k[:150]}")


if __name__ == "__main__":
    main(*sys.argv[1:3])
