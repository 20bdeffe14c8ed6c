"""What the read summaries cost (Read summaries), measured in fresh processes.
    python tools/stats_bench.py kernel [MiB, default 256] [calls, default 20]
        for synth modes 2, 4 and 5, each in a process of its own: one block on the device, the median wall time of
        `calls` fqgpu_dblock_stats calls at P = 512 beside that of as many fqgpu_dblock_crc32 calls on the same block, and
        the device time of both kernel groups (HIP events).
        (the child alone: python tools/stats_bench.py kernel_one <mode> [MiB] [calls] -- the form to put behind
        `rocprofv3 --kernel-trace --stats --`; tools/rocprof_kernel_table.py makes the table.)
    python tools/stats_bench.py farm [MiB, default 4096] [workers, default 16] [rounds, default 3]
        mode-2 input: fqc_tool c against c --stats, t against s (archive written with --index --checksum), the variants
        alternating, every run a fresh process (worker seconds of every run)"""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fqcomp28_amd as F  # noqa: E402
from checksum_bench import build_tool, seconds, write_input  # noqa: E402


def kernel_one(mode, mib, calls):
    raw, _ = F.synth_fastq(mib << 20, mode, seed=28)
    recs = F.parse_fastq(raw)
    sft, qft = F.freq_tables(raw[: min(raw.size, 32 << 20)], recs[: max(1, len(recs) * min(raw.size, 32 << 20) // raw.size - 1)])
    ctx = F.Context(sft, qft)
    b = ctx.dblock(raw, recs)
    b.stats(512); b.crc32(); ctx.sync()   # (allocations, tables)
    ctx.enable_timing(True)
    wall = {"stats": [], "crc32": []}
    for _ in range(calls):
        for name, call in (("stats", lambda: b.stats(512)), ("crc32", b.crc32)):
            t0 = time.perf_counter()
            call()
            wall[name].append((time.perf_counter() - t0) * 1e3)
    _, spans = ctx.last_timing()
    print(json.dumps({"mode": mode, "block_MiB": round(raw.size / 2 ** 20, 1), "records": len(recs), "calls": calls,
                      "wall_ms_median": {n: round(statistics.median(v), 4) for n, v in wall.items()},
                      "kernel_ms_per_call": {n: round(ms / c, 4) for n, ms, c in spans}}), flush=True)
    b.close(); ctx.close()


def kernel(mib, calls):
    for mode in (2, 4, 5):
        subprocess.run([sys.executable, os.path.abspath(__file__), "kernel_one", str(mode), str(mib), str(calls)], check=True, timeout=600)


def farm(mib, workers, rounds):
    exe = build_tool()
    with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
        src, arc, rep_c, rep_s = (os.path.join(tmp, n) for n in ("in.fastq", "a.fqc", "c.tsv", "s.tsv"))
        write_input(src, mib)
        t = ["-t", str(workers)]
        made = ["--index", "--checksum"]
        variants = [("c", [exe, "c", src, arc] + t + made), ("c --stats", [exe, "c", src, arc] + t + made + ["--stats", rep_c]),
                    ("t", [exe, "t", arc] + t), ("s", [exe, "s", arc, rep_s] + t)]
        out = {name: [] for name, _ in variants}
        seconds(variants[0][1])  # (page cache: a warm-up of the box, and the archive t and s read)
        for _ in range(rounds):
            for name, cmd in variants:
                out[name].append(round(seconds(cmd)["seconds"], 3))
        assert open(rep_c, "rb").read() == open(rep_s, "rb").read(), "the two reports of one file differ"
        med = {n: statistics.median(v) for n, v in out.items()}
        print(json.dumps({"farm_MiB": mib, "workers": workers, "worker_seconds": out,
                          "slowdown_percent": {"c --stats": round(100 * (med["c --stats"] / med["c"] - 1), 1), "s": round(100 * (med["s"] / med["t"] - 1), 1)},
                          "spread_percent_of_plain": {n: round(100 * (max(out[n]) - min(out[n])) / med[n], 1) for n in ("c", "t")}}), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    nums = [int(x) for x in sys.argv[2:]]
    if what == "kernel_one":
        kernel_one(*(nums + [2, 256, 20][len(nums):]))
    elif what == "kernel":
        kernel(*(nums + [256, 20][len(nums):]))
    else:
        farm(*(nums + [4096, 16, 3][len(nums):]))
