"""Per-kernel launch times of rocprofv3 kernel traces, one row per build and kernel: the median, the shortest and the
longest of the kernel's 16 longest launches (with `bench.py --lanes 1 --steps 2` those are the 256 MiB blocks).
    python3 tools/kernel_medians.py [--pmc] out.csv name=dir ...
dir: what `rocprofv3 --kernel-trace --output-format csv -d dir -- ...` wrote (searched for *kernel_trace.csv).
--pmc: dir holds a counter run (*counter_collection.csv); the row is then the median over the kernel's 16 launches with the
most waves of every counter (wave-instructions per launch)."""
import collections
import csv
import glob
import os
import re
import statistics
import sys


def short(n):
    return re.sub(r"\(.*", "", n.replace("(anonymous namespace)::", "").replace("void ", "")).replace(",", ";")


def newest(d, pat):
    found = sorted(glob.glob(os.path.join(d, "**", pat), recursive=True), key=os.path.getmtime)
    assert found, (d, pat)
    return found[-1]


def times(d):
    by = collections.defaultdict(list)
    for r in csv.DictReader(open(newest(d, "*kernel_trace.csv"))):
        by[short(r["Kernel_Name"])].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    rows = []
    for k, t in by.items():
        top = sorted(t)[-16:]
        rows.append((k, len(top), statistics.median(top), min(top), max(top)))
    return sorted(rows, key=lambda r: -r[2] * r[1])


def counters(d):
    per = collections.defaultdict(lambda: collections.defaultdict(dict))   # kernel -> dispatch -> counter -> value
    for r in csv.DictReader(open(newest(d, "*counter_collection.csv"))):
        c = per[short(r["Kernel_Name"])][r["Dispatch_Id"]]
        c[r["Counter_Name"]] = c.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
    rows = []
    for k, disp in per.items():
        top = sorted(disp.values(), key=lambda c: c.get("SQ_WAVES", 0.0))[-16:]
        names = sorted({n for c in top for n in c})
        rows.append((k, len(top), {n: statistics.median(c.get(n, 0.0) for c in top) for n in names}))
    return sorted(rows, key=lambda r: -sum(v for n, v in r[2].items() if n.startswith("SQ_INSTS")))


def main():
    args = sys.argv[1:]
    pmc = args[0] == "--pmc"
    out, builds = args[1 if pmc else 0], [a.split("=", 1) for a in args[(2 if pmc else 1):]]
    with open(out, "w") as f:
        if pmc:
            cols = None
            for name, d in builds:
                for k, n, c in counters(d):
                    if cols is None:
                        cols = sorted(c)
                        f.write("build,kernel,launches," + ",".join("median_" + x for x in cols) + "\n")
                    f.write("%s,%s,%d,%s\n" % (name, k, n, ",".join("%.5g" % c.get(x, 0.0) for x in cols)))
        else:
            f.write("build,kernel,launches,median_us_of_16_longest,min_us,max_us\n")
            for name, d in builds:
                for k, n, med, lo, hi in times(d):
                    f.write("%s,%s,%d,%.1f,%.1f,%.1f\n" % (name, k, n, med, lo, hi))


if __name__ == "__main__":
    main()
