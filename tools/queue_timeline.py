"""Which hardware queues the kernels of a run went through and how many ran at a time, from a rocprofv3 kernel trace.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 bench.py
    python3 tools/queue_timeline.py DIR [--idle-us 100] [--gap-us 20]
DIR (or a file) is searched for `*kernel_trace.csv`.  The timed region is taken to be the BURST with the most launches: the
trace is cut wherever no kernel runs for more than --idle-us (a host wait: bench.py waits behind its warm-up and behind its
timed steps, never between them).  Printed for that region:
  - the distinct queue ids seen, with launches and streams per queue (streams only where the trace has a Stream_Id column);
  - the share of the region's time with 0 / 1 / 2 / >= 3 kernels running;
  - hand-overs: launches that start within --gap-us behind the end of the kernel that ended last on the SAME queue where
    that kernel belongs to ANOTHER stream -- a stream that waited for a queue, not for its own work.  Streams number in the
    order of creation and a lane creates its two in one go, so streams (s, s+1) of one pair are one lane; hand-overs
    between the two streams of a lane are counted apart from those between lanes."""
import argparse
import csv
import glob
import os
import sys
from collections import Counter, defaultdict


def find_trace(path):
    if os.path.isfile(path):
        return path
    hits = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))
    if not hits:
        sys.exit("no *kernel_trace.csv under %s" % path)
    return hits[-1]


def load(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append({"q": r.get("Queue_Id", "?"), "s": r.get("Stream_Id"), "name": r.get("Kernel_Name", ""),
                         "b": int(r["Start_Timestamp"]), "e": int(r["End_Timestamp"])})
    rows.sort(key=lambda r: r["b"])
    return rows


def bursts(rows, idle_ns):
    """Maximal runs of launches with no gap above idle_ns in which nothing runs."""
    out, cur, end = [], [], None
    for r in rows:
        if cur and r["b"] - end > idle_ns:
            out.append(cur)
            cur = []
            end = None
        cur.append(r)
        end = r["e"] if end is None else max(end, r["e"])
    if cur:
        out.append(cur)
    return out


def concurrency(rows):
    """ns of the region with k kernels running, k = 0, 1, 2, 3 (3: three or more)."""
    ev = []
    for r in rows:
        ev.append((r["b"], 1))
        ev.append((r["e"], -1))
    ev.sort()
    share, k, t = [0, 0, 0, 0], 0, ev[0][0]
    for at, d in ev:
        share[min(k, 3)] += at - t
        t = at
        k += d
    return share


def lane_of(stream_ids):
    """stream id -> lane: the streams of the region in order of their ids, two by two."""
    order = sorted(stream_ids, key=lambda s: (len(s), s))
    return {s: i // 2 for i, s in enumerate(order)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--idle-us", type=float, default=100.0)
    ap.add_argument("--gap-us", type=float, default=20.0)
    args = ap.parse_args()
    path = find_trace(args.trace)
    rows = load(path)
    if not rows:
        sys.exit("%s holds no launches" % path)
    region = max(bursts(rows, args.idle_us * 1e3), key=len)
    t0, t1 = region[0]["b"], max(r["e"] for r in region)
    print("trace: %s" % os.path.basename(path))
    print("launches: %d in the trace, %d in the timed region (%.3f ms)" % (len(rows), len(region), (t1 - t0) / 1e6))
    have_streams = region[0]["s"] is not None
    per_q = defaultdict(list)
    for r in region:
        per_q[r["q"]].append(r)
    print("distinct queue ids in the region: %d  (%s)" % (len(per_q), " ".join(sorted(per_q, key=lambda q: (len(q), q)))))
    for q in sorted(per_q, key=lambda q: (len(q), q)):
        ss = sorted({r["s"] for r in per_q[q]}, key=lambda s: (len(s), s)) if have_streams else []
        print("  queue %-4s %5d launches%s" % (q, len(per_q[q]), ("  streams: " + " ".join(ss)) if have_streams else ""))
    share = concurrency(region)
    tot = float(sum(share)) or 1.0
    print("kernels running at a time, share of the region: 0: %.1f %%  1: %.1f %%  2: %.1f %%  >=3: %.1f %%"
          % tuple(100.0 * s / tot for s in share))
    if not have_streams:
        print("hand-overs: the trace has no Stream_Id column")
        return
    lanes = lane_of({r["s"] for r in region})
    gap = args.gap_us * 1e3
    kinds = Counter()
    for q, rs in per_q.items():
        last = None   # the launch of this queue that ended last so far
        for r in rs:  # (in start order)
            if last is not None and last["s"] != r["s"] and 0 <= r["b"] - last["e"] <= gap:
                kinds["other lane" if lanes[last["s"]] != lanes[r["s"]] else "same lane"] += 1
            if last is None or r["e"] >= last["e"]:
                last = r
    print("hand-overs (start within %.0f us behind the end of another stream's kernel on the same queue): "
          "%d from another lane, %d from the lane's other stream, of %d launches (%.1f %%)"
          % (args.gap_us, kinds["other lane"], kinds["same lane"], len(region), 100.0 * sum(kinds.values()) / len(region)))


if __name__ == "__main__":
    main()
