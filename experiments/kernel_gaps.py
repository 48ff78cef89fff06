"""Inter-kernel gaps of the BA iteration from a rocprofv3 --kernel-trace CSV: for every consecutive pair of dispatches (by begin
time), gap = begin(next) - end(prev); medians per (prev kernel -> next kernel) pair."""
import csv
import statistics
import sys


def short(n):
    n = n.split("(")[0]
    n = n.replace("void ", "")
    return n.split("<")[0].strip()


def main(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
    rows.sort()
    gaps, durs = {}, {}
    for (s0, e0, n0), (s1, e1, n1) in zip(rows, rows[1:]):
        gaps.setdefault((n0, n1), []).append(s1 - e0)
    for s, e, n in rows:
        durs.setdefault(n, []).append(e - s)
    print("dispatches: %d" % len(rows))
    print("%-34s %6s %10s %10s" % ("kernel", "calls", "median ns", "mean ns"))
    for n, d in sorted(durs.items(), key=lambda kv: -sum(kv[1])):
        if n.startswith("ba_") or n.startswith("chol_"):
            print("%-34s %6d %10.0f %10.0f" % (n, len(d), statistics.median(d), sum(d) / len(d)))
    print()
    print("%-34s -> %-30s %6s %10s %8s %8s" % ("end of", "begin of", "count", "median ns", "p10", "p90"))
    for (a, b), g in sorted(gaps.items(), key=lambda kv: -len(kv[1])):
        if len(g) < 5 or not (a.startswith("ba_") or a.startswith("chol_")):
            continue
        g = sorted(g)
        print("%-34s -> %-30s %6d %10.0f %8d %8d" % (a, b, len(g), statistics.median(g), g[len(g) // 10], g[(9 * len(g)) // 10]))


if __name__ == "__main__":
    main(sys.argv[1])
