"""What each launch edge of a C2 pass costs, from a per-dispatch kernel trace:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python3 tools/roofline_run.py c2
    python3 tools/launch_edges.py DIR/.../t_kernel_trace.csv

A pass of the one-launch sweep is assemble_first_kernel followed by one slab_step_kernel per
64-column step.  For every launch of a pass, as medians over the passes of the trace: its
duration, the gap to the next launch of the pass, T (the step's tile rows; workgroups =
T (T + 1) / 2) and the bytes it stores -- tiles, solved rows, factor.  The steps that have a next
factor share workgroup 0's path, so a straight line through (stored MB, duration + gap) over
them has the cost of the other workgroups' stores as its slope, in us per MB.

Stored bytes of a step at T (slab.h): T (T - 1) / 2 off-diagonal tiles of 32 KiB, the ten lower
16 x 16 blocks of every diagonal tile that is not workgroup 0's (all T of them in the last
step), T solved row blocks of 32 KiB, and workgroup 0's factor: the lower triangle of a 64 x 64
block, 64 reciprocal pivots and four 16 x 16 block inverses.  Of the assembly: every 128 x 64
tile that touches the lower triangle, and the scratch column.
"""
import csv
import sys

import numpy as np

TILE = 64 * 64 * 8
DIAG = 10 * 16 * 16 * 8
FACTOR = (64 * 65 // 2 + 64 + 4 * 256) * 8


def step_bytes(T, last):
    tiles = T * (T - 1) // 2 * TILE + (T if last else T - 1) * DIAG
    return tiles, T * TILE, 0 if last else FACTOR


def assembly_bytes(ntot):
    tiles = sum(1 for bi in range((ntot + 127) // 128) for bj in range(ntot // 64)
                if 64 * bj <= 128 * bi + 127)
    return tiles * 2 * TILE + (ntot - 64) * 64 * 8, 0, FACTOR


def passes(path):
    rows = [r for r in csv.DictReader(open(path))
            if "assemble_first_kernel" in r["Kernel_Name"] or "slab_step_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out = []
    for r in rows:
        first = "assemble_first_kernel" in r["Kernel_Name"]
        if first:
            out.append([])
        if out:
            wgs = (int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"])) * int(r["Grid_Size_Y"])
            out[-1].append((first, wgs, int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    n = max(len(p) for p in out)
    return [p for p in out if len(p) == n]


def main():
    ps = passes(sys.argv[1])
    skip = int(sys.argv[2]) if len(sys.argv) > 2 else 2  # (the first passes capture the graph)
    ps = ps[skip:] if len(ps) > skip + 2 else ps
    n = len(ps[0])
    dur = np.array([[(e - s) / 1e3 for _, _, s, e in p] for p in ps])
    gap = np.array([[(p[k + 1][2] - p[k][3]) / 1e3 for k in range(n - 1)] + [np.nan] for p in ps])
    tot = np.array([(p[-1][3] - p[0][2]) / 1e3 for p in ps])
    print("# %d passes of %d launches; us; medians over passes (spread: max - min over passes)"
          % (len(ps), n))
    print("# launch   T  workgroups  duration   gap_next  dur+gap  spread   tiles_KB  rows_KB  "
          "factor_KB  stored_MB")
    xs, ys, sp = [], [], []
    T0 = None
    for k in range(n):
        first, wgs = ps[0][k][0], ps[0][k][1]
        T = 0  # (the assembly's: from the first step, below)
        if not first:
            T = int(((8 * wgs + 1) ** 0.5 - 1) / 2 + 0.5)
            if T0 is None:
                T0 = T
        last = k == n - 1
        b = step_bytes(T, last) if not first else None
        both = dur[:, k] + gap[:, k]
        row = (k, T, wgs, np.median(dur[:, k]), np.median(gap[:, k]), np.median(both),
               (np.max(both) - np.min(both)) if not last else np.max(dur[:, k]) - np.min(dur[:, k]))
        ps[0][k] = ps[0][k] + (row,)
        if not first:
            print("  %4d  %3d  %8d  %9.2f  %9.2f  %7.2f  %6.2f  %9.0f  %7.0f  %9.1f  %9.3f"
                  % (row + (b[0] / 1024, b[1] / 1024, b[2] / 1024, sum(b) / 1e6)))
            if not last:
                xs.append(sum(b) / 1e6), ys.append(row[5]), sp.append(row[6])
    # (the assembly's line last: its T is the first step's + 1 row blocks)
    ntot = 64 * (T0 + 1)
    b = assembly_bytes(ntot)
    row = ps[0][0][-1]
    print("# assembly (ntot = %d):" % ntot)
    print("  %4d  %3d  %8d  %9.2f  %9.2f  %7.2f  %6.2f  %9.0f  %7.0f  %9.1f  %9.3f"
          % (row[0], T0 + 1, row[2], row[3], row[4], row[5], row[6], b[0] / 1024, b[1] / 1024,
             b[2] / 1024, sum(b) / 1e6))
    xs, ys = np.array(xs), np.array(ys)
    slope, icpt = np.polyfit(xs, ys, 1)
    # per pass, for the slope's own spread
    sl = [np.polyfit(xs, (dur[i, 1:n - 1] + gap[i, 1:n - 1]), 1)[0] for i in range(len(ps))]
    print("# fit over the %d steps with a next factor: dur+gap = %.3f us + %.4f us/MB * stored_MB"
          % (len(xs), icpt, slope))
    print("# slope per pass: median %.4f  min %.4f  max %.4f us/MB" % (np.median(sl), min(sl), max(sl)))
    print("# largest - smallest step (T = %d against T = %d): %.2f us; median spread of a step "
          "between passes %.2f us" % (T0, T0 - len(xs) + 1, ys[0] - ys[-1], float(np.median(sp))))
    print("# stored per pass: %.1f MB steps + %.1f MB assembly; slope x steps' MB = %.2f us"
          % (xs.sum() + sum(step_bytes(T0 - len(xs), True)) / 1e6, sum(b) / 1e6, slope * xs.sum()))
    print("# pass (first start to last end): median %.2f us, min %.2f, max %.2f"
          % (np.median(tot), tot.min(), tot.max()))


if __name__ == "__main__":
    main()
