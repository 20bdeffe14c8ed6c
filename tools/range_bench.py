"""Restores of a record range (fqc_tool d --records A:B) against the full restore, on one synthetic archive:
writes a configs[1]-like FASTQ file (150 bp reads, Phred ~ N(34, 5)), compresses it in 256 MiB blocks with decode
indexes of 1 Mi and of 64 Ki symbols per stride (the .fqc files are the same; only the .fqx sidecars differ) and
without, and times
  one read in the middle of the archive, 10,000 reads across a block boundary, the whole archive.
    python tools/range_bench.py [--gib 4] [--threads 4] [--dir DIR]
Prints one JSON line per restore (fqc_tool's clock: the worker threads, tables and handles built before; the range
restore's clock includes the size queries of its edge blocks) and leaves DIR/ranges.json, the archives and the input
in DIR for a profiling run of its own."""
import argparse
import json
import os
import struct
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fqcomp28_amd as F  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--gib", type=float, default=4)
ap.add_argument("--threads", type=int, default=4)
ap.add_argument("--dir", default="/tmp/range_bench")
args = ap.parse_args()

exe = os.path.join(ROOT, "tools", "_build", "fqc_tool")
if not os.path.exists(exe):
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O2", "-o", exe, os.path.join(ROOT, "tools", "fqc_tool.cpp"), "-L" + os.path.join(ROOT, "fqcomp28_amd"),
                    "-lfqgpu", "-Wl,-rpath," + os.path.join(ROOT, "fqcomp28_amd"), "-lpthread"], check=True)
os.makedirs(args.dir, exist_ok=True)
src = os.path.join(args.dir, "in.fastq")
size = int(args.gib * (1 << 30))
if not os.path.exists(src) or os.path.getsize(src) < size - (64 << 20):
    done, next_id = 0, 0
    with open(src, "wb") as f:
        while done < size:
            raw, n = F.synth_fastq(min(64 << 20, size - done), 2, seed=28, first_read_id=next_id)
            raw.tofile(f)
            next_id += n
            done += 64 << 20


def tool(*a):
    t0 = time.time()
    r = subprocess.run([exe] + [str(x) for x in a], capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit("fqc_tool %s failed: %s" % (" ".join(str(x) for x in a), r.stderr))
    return json.loads(r.stdout.strip().splitlines()[-1]), time.time() - t0


def record_counts(arc):
    """records per block in input order: the second word of every block (the index sits at the end of the file)"""
    with open(arc, "rb") as f:
        (n,) = struct.unpack("<I", f.read(4))
        f.seek(-16 * n, 2)
        idx = [struct.unpack_from("<qI", f.read(16)) for _ in range(n)]
        counts = {}
        for off, k in idx:
            f.seek(off)
            counts[k] = struct.unpack("<II", f.read(8))[1]
    return [counts[k] for k in range(n)]


arcs = {}
for name, opts in (("index_1Mi", ["--index"]), ("index_64Ki", ["--index", "--index-stride", 64])):
    arc = os.path.join(args.dir, name + ".fqc")
    c, _ = tool("c", src, arc, "-t", args.threads, "-R", 256, *opts)
    arcs[name] = arc
plain = os.path.join(args.dir, "no_index.fqc")
if os.path.exists(plain):
    os.remove(plain)
os.link(arcs["index_1Mi"], plain)  # the same .fqc without a sidecar
arcs["no_index"] = plain

counts = record_counts(plain)
edges = [0]
for c in counts:
    edges.append(edges[-1] + c)
n = edges[-1]
mid_block = len(counts) // 2
ranges = {"one_read_mid": (n // 2, n // 2 + 1), "10k_across_boundary": (edges[mid_block] - 5000, edges[mid_block] + 5000)}
with open(os.path.join(args.dir, "ranges.json"), "w") as f:
    json.dump({"archives": arcs, "ranges": ranges, "blocks": len(counts), "records": n}, f)
out = os.path.join(args.dir, "out.fastq")
for name, arc in arcs.items():
    for what, (a, b) in list(ranges.items()) + [("full", (0, None))]:
        rec = ["--records", "%d:%d" % (a, b)] if b is not None else []
        rep, wall = tool("d", arc, out, "-t", args.threads, *rec)
        line = {"archive": name, "restore": what, "records": rep["records"], "raw_bytes": rep["raw_bytes"],
                "seconds": round(rep["seconds"], 4), "wall_s": round(wall, 3), "blocks_decoded": sum(rep["blocks_per_worker"]),
                "blocks": len(counts), "threads": args.threads}
        if what == "full":
            line["roundtrip_equal"] = subprocess.run(["cmp", "-s", src, out]).returncode == 0
        os.remove(out)
        print(json.dumps(line), flush=True)
