"""The FASTA restore (fqc_tool d --fasta) against the FASTQ restore (fqc_tool d) of the same archive, in the same session:
writes a configs[1]-like FASTQ file (synthetic mode 2: 150 bp reads, Phred ~ N(34, 5)), compresses it in 256 MiB blocks
with decode indexes, and times both restores with the `.fqx` sidecar and without it -- every run a fresh process under a
time limit of its own, `--runs` of each with the two forms taking turns, the median reported with the spread (max - min)
beside it.
    python tools/fasta_bench.py [--gib 4] [--threads 16] [--runs 3] [--dir DIR] [--tool PATH] [--limit SECONDS]
Prints one JSON line per run and one summary line per (sidecar, form): seconds by fqc_tool's clock (the worker threads;
tables and handles built before), wall seconds, bytes read of the archive (the FASTQ restore reads every block whole:
the archive's size less its tables and index), bytes written.  --tool PATH --forms fastq: the FASTQ restore of another
build's fqc_tool (one that does not know --fasta), to confirm the FASTQ figure against it.
The first failing run ends the script: nothing more is started on the GPU after it."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fqcomp28_amd as F  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--gib", type=float, default=4)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--dir", default="/tmp/fasta_bench")
ap.add_argument("--tool", default=None)
ap.add_argument("--limit", type=int, default=240, help="seconds one fqc_tool run may take")
ap.add_argument("--forms", default="fastq,fasta")
args = ap.parse_args()

exe = args.tool or os.path.join(ROOT, "tools", "_build", "fqc_tool")
if not args.tool and not os.path.exists(exe):
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
    """one fresh process under its own time limit -> (its JSON line, wall seconds)"""
    t0 = time.time()
    r = subprocess.run(["timeout", "-k", "10", str(args.limit), exe] + [str(x) for x in a], capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit("fqc_tool %s failed (exit %d): %s" % (" ".join(str(x) for x in a), r.returncode, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1]), time.time() - t0


arc = os.path.join(args.dir, "indexed.fqc")
if not os.path.exists(arc) or not os.path.exists(arc + ".fqx"):
    tool("c", src, arc, "-t", args.threads, "-R", 256, "--index")
plain = os.path.join(args.dir, "no_index.fqc")
if os.path.exists(plain):
    os.remove(plain)
os.link(arc, plain)  # the same .fqc without a sidecar
arc_bytes = os.path.getsize(arc)
print(json.dumps({"input_bytes": os.path.getsize(src), "archive_bytes": arc_bytes, "fqx_bytes": os.path.getsize(arc + ".fqx"),
                  "threads": args.threads, "tool": exe}), flush=True)

for sidecar, path in (("fqx", arc), ("none", plain)):
    forms = args.forms.split(",")
    runs = {form: [] for form in forms}
    for k in range(args.runs):  # the forms take turns, so that what else the box does meets both alike
        for form in forms:
            out = os.path.join(args.dir, "out." + form)
            rep, wall = tool("d", path, out, "-t", args.threads, *(["--fasta"] if form == "fasta" else []))
            line = {"sidecar": sidecar, "form": form, "run": k, "seconds": round(rep["seconds"], 4), "wall_s": round(wall, 3),
                    "records": rep["records"], "out_bytes": os.path.getsize(out), "index": rep["index"],
                    "archive_bytes_read": rep.get("archive_bytes_read")}
            os.remove(out)
            runs[form].append(line)
            print(json.dumps(line), flush=True)
    for form in forms:
        secs, walls = [r["seconds"] for r in runs[form]], [r["wall_s"] for r in runs[form]]
        print(json.dumps({"summary": True, "sidecar": sidecar, "form": form, "median_s": statistics.median(secs),
                          "spread_s": round(max(secs) - min(secs), 4), "median_wall_s": statistics.median(walls),
                          "spread_wall_s": round(max(walls) - min(walls), 3), "out_bytes": runs[form][0]["out_bytes"],
                          "archive_bytes_read": runs[form][0]["archive_bytes_read"], "archive_bytes": arc_bytes}), flush=True)
