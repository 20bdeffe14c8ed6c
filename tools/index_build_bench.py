"""What building a decode index for an existing archive costs and buys, on one archive written WITHOUT --index:
seconds of
  d (plain: every stream by one lane from its end), x (index only), d --index (restore and index in one pass),
then, with the built sidecar beside the archive, d again and a one-record --records restore; finally d with the
sidecar an encode with --index leaves for the same archive (same bytes: the same pace, or the wrong path ran).
    python tools/index_build_bench.py [--gib 1] [--threads 4] [--block-mib 256] [--mode 2] [--stride-ki 1024] [--input FILE] [--dir DIR]
--input: a FASTQ file of real reads instead of the synthetic one.  Prints one JSON line per step (fqc_tool's clock: the
worker threads, tables and handles built before) and leaves the archives and the input in DIR."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fqcomp28_amd as F  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--gib", type=float, default=1)
ap.add_argument("--threads", type=int, default=4)
ap.add_argument("--block-mib", type=int, default=256)
ap.add_argument("--mode", type=int, default=2)
ap.add_argument("--stride-ki", type=int, default=1024)
ap.add_argument("--input", default=None)
ap.add_argument("--dir", default="/tmp/index_build_bench")
args = ap.parse_args()

exe = os.path.join(ROOT, "tools", "_build", "fqc_tool")
src_cpp = os.path.join(ROOT, "tools", "fqc_tool.cpp")
if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src_cpp):
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O2", "-o", exe, src_cpp, "-L" + os.path.join(ROOT, "fqcomp28_amd"),
                    "-lfqgpu", "-Wl,-rpath," + os.path.join(ROOT, "fqcomp28_amd"), "-lpthread"], check=True)
os.makedirs(args.dir, exist_ok=True)
src = args.input or os.path.join(args.dir, "in_mode%d.fastq" % args.mode)
size = int(args.gib * (1 << 30))
if not args.input and (not os.path.exists(src) or os.path.getsize(src) < size - (64 << 20)):
    done, next_id = 0, 0
    with open(src, "wb") as f:
        while done < size:
            raw, n = F.synth_fastq(min(64 << 20, size - done), args.mode, seed=28, first_read_id=next_id)
            raw.tofile(f)
            next_id += n
            done += 64 << 20


def tool(*a):
    t0 = time.time()
    r = subprocess.run([exe] + [str(x) for x in a], capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit("fqc_tool %s failed: %s" % (" ".join(str(x) for x in a), r.stderr))
    return json.loads(r.stdout.strip().splitlines()[-1]), time.time() - t0


stride = ["--index-stride", args.stride_ki]
arc = os.path.join(args.dir, "plain.fqc")
enc = os.path.join(args.dir, "encoded_index.fqc")
side, out = arc + ".fqx", os.path.join(args.dir, "out.fastq")
common = ["-t", args.threads, "-R", args.block_mib]
c, _ = tool("c", src, arc, *common)
tool("c", src, enc, *common, "--index", *stride)
n_records = c["records"]


def step(what, *a, check=True):
    rep, wall = tool(*a)
    line = {"step": what, "seconds": round(rep["seconds"], 4), "wall_s": round(wall, 3), "raw_bytes": rep["raw_bytes"],
            "index": rep.get("index"), "indexed_blocks": rep.get("indexed_blocks"), "index_bytes": rep.get("index_bytes"),
            "blocks": c["blocks"], "threads": args.threads, "stride_ki": args.stride_ki}
    if rep["raw_bytes"] and rep["seconds"] > 0:
        line["MBps"] = round(rep["raw_bytes"] / rep["seconds"] / 1e6, 1)
    if check and os.path.exists(out):
        line["roundtrip_equal"] = subprocess.run(["cmp", "-s", src, out]).returncode == 0
    if os.path.exists(out):
        os.remove(out)
    print(json.dumps(line), flush=True)
    return rep


def drop_sidecar():
    if os.path.exists(side):
        os.remove(side)


drop_sidecar()
step("d plain", "d", arc, out, "-t", args.threads)
step("x", "x", arc, "-t", args.threads, *stride)
drop_sidecar()
step("d --index", "d", arc, out, "-t", args.threads, "--index", *stride)
step("d with the built sidecar", "d", arc, out, "-t", args.threads)
step("one record with the built sidecar", "d", arc, out, "-t", args.threads, "--records", "%d:%d" % (n_records // 2, n_records // 2 + 1), check=False)
# the same archive bytes under the sidecar an encode left: its identity is the archive's own
if open(arc, "rb").read(1 << 16) == open(enc, "rb").read(1 << 16) and os.path.getsize(arc) == os.path.getsize(enc):
    shutil.copy(enc + ".fqx", side)
    step("d with the encoder's sidecar", "d", arc, out, "-t", args.threads)
else:
    step("d of the archive encoded with --index", "d", enc, out, "-t", args.threads)
