"""What read trimming costs (Read trimming), measured in fresh processes.
    python tools/trim_bench.py kernel [MiB, default 256] [calls, default 20]
        for synth modes 2 and 4, each in a process of its own: one block on the device; for a trim that cuts nothing,
        cut_front 5 + cut_tail 5, q_front = q_tail = 20 and q_tail 30 + crop 100 (no filter) the median wall time and the "trim"
        device time (HIP events) of `calls` size-query fqgpu_dblock_trim calls (out == NULL: the judge alone) and, separately,
        of as many calls with `out` given (judge, scan, gather and the copy of the kept bytes into page-locked memory) --
        beside `calls` fqgpu_dblock_filter calls for each of three filters (one that keeps everything by reading the quality
        lines, min_mean_q = 1; one that keeps everything by length alone, min_len = 1: the yardstick of the trim that cuts
        nothing; and min_mean_q = 34) and `calls` fqgpu_dblock_crc32 calls on the same block in the same process.
        (the child alone: python tools/trim_bench.py kernel_one <mode> [MiB] [calls] -- the form to put behind
        `rocprofv3 --kernel-trace --stats --`; tools/rocprof_kernel_table.py makes the table.)
    python tools/trim_bench.py farm [MiB, default 4096] [workers, default 16] [rounds, default 3]
        mode-2 input, archive written with --index: fqc_tool d against d --min-mean-q 34 and d --trim-q3 30 --trim-q5 30,
        alternating, every run a fresh process: worker seconds and bytes written of every run"""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fqcomp28_amd as F  # noqa: E402
from fqcomp28_amd import binding as B  # noqa: E402
from checksum_bench import build_tool, seconds, write_input  # noqa: E402


def kernel_one(mode, mib, calls):
    raw, _ = F.synth_fastq(mib << 20, mode, seed=28)
    recs = F.parse_fastq(raw)
    sft, qft = F.freq_tables(raw[: min(raw.size, 32 << 20)], recs[: max(1, len(recs) * min(raw.size, 32 << 20) // raw.size - 1)])
    ctx = F.Context(sft, qft)
    b = ctx.dblock(raw, recs)
    lib = F.lib()
    out = F.pinned_empty(raw.size)
    report = np.zeros(B.TRIM_REPORT_WORDS, dtype=np.uint64)
    n = C.c_size_t(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    trims = [("cuts nothing", B.read_trim()), ("cut_front 5, cut_tail 5", B.read_trim(cut_front=5, cut_tail=5)),
             ("q_front 20, q_tail 20", B.read_trim(q_front=20, q_tail=20)), ("q_tail 30, crop 100", B.read_trim(q_tail=30, crop=100))]
    filters = [("keeps everything", B.read_filter(min_mean_q=1)), ("keeps everything, by length", B.read_filter(min_len=1)),
               ("min_mean_q 34", B.read_filter(min_mean_q=34))]

    def trim(t, with_out):
        rc = lib.fqgpu_dblock_trim(ctx.h, b.h, p(t), None, p(out) if with_out else None, out.size, C.byref(n), p(report), None, None)
        assert rc == 0, rc

    def filt(f, with_out):
        rc = lib.fqgpu_dblock_filter(ctx.h, b.h, p(f), p(out) if with_out else None, out.size, C.byref(n), p(report), None)
        assert rc == 0, rc

    def timed(fn):
        ctx.enable_timing(True)
        wall = []
        for _ in range(calls):
            t0 = time.perf_counter()
            fn()
            wall.append((time.perf_counter() - t0) * 1e3)
        _, spans = ctx.last_timing()
        return {"wall_ms_median": round(statistics.median(wall), 4), "kernel_ms_per_call": {name: round(ms / calls, 4) for name, ms, _ in spans}}

    b.crc32(); filt(filters[0][1], True); trim(trims[2][1], True); ctx.sync()   # (allocations, tables)
    res = {"mode": mode, "block_MiB": round(raw.size / 2 ** 20, 1), "records": len(recs), "calls": calls, "crc32": timed(b.crc32),
           "filter": [], "trim": []}
    for name, f in filters:
        query = timed(lambda: filt(f, False))
        full = timed(lambda: filt(f, True))
        res["filter"].append({"filter": name, "kept_percent": round(100 * int(report[1]) / len(recs), 1), "kept_MiB": round(n.value / 2 ** 20, 1),
                              "size_query": query, "with_out": full})
    for name, t in trims:
        query = timed(lambda: trim(t, False))
        full = timed(lambda: trim(t, True))
        res["trim"].append({"trim": name, "trimmed_percent": round(100 * int(report[10]) / len(recs), 1),
                            "emptied_percent": round(100 * int(report[13]) / len(recs), 2), "kept_MiB": round(n.value / 2 ** 20, 1),
                            "size_query": query, "with_out": full})
    print(json.dumps(res), flush=True)
    b.close(); ctx.close()


def kernel(mib, calls):
    for mode in (2, 4):
        subprocess.run([sys.executable, os.path.abspath(__file__), "kernel_one", str(mode), str(mib), str(calls)], check=True, timeout=600)


def farm(mib, workers, rounds):
    exe = build_tool()
    with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
        src, arc, plain, kept, cut = (os.path.join(tmp, n) for n in ("in.fastq", "a.fqc", "plain.fastq", "kept.fastq", "trimmed.fastq"))
        write_input(src, mib)
        t = ["-t", str(workers)]
        seconds([exe, "c", src, arc] + t + ["--index"])
        variants = [("d", [exe, "d", arc, plain] + t, plain), ("d --min-mean-q 34", [exe, "d", arc, kept] + t + ["--min-mean-q", "34"], kept),
                    ("d --trim-q3 30 --trim-q5 30", [exe, "d", arc, cut] + t + ["--trim-q3", "30", "--trim-q5", "30"], cut)]
        out = {name: [] for name, _, _ in variants}
        written = {}
        seconds(variants[0][1])  # (page cache: a warm-up of the box, and the archive both read)
        for _ in range(rounds):
            for name, cmd, path in variants:
                out[name].append(round(seconds(cmd)["seconds"], 3))
                written[name] = os.path.getsize(path)
        med = {name: statistics.median(v) for name, v in out.items()}
        print(json.dumps({"farm_MiB": mib, "workers": workers, "worker_seconds": out, "bytes_written": written,
                          "filtered_against_plain_percent": round(100 * (med["d --min-mean-q 34"] / med["d"] - 1), 1),
                          "trimmed_against_plain_percent": round(100 * (med["d --trim-q3 30 --trim-q5 30"] / med["d"] - 1), 1),
                          "spread_percent_of_plain": round(100 * (max(out["d"]) - min(out["d"])) / med["d"], 1)}), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    nums = [int(x) for x in sys.argv[2:]]
    if what == "kernel_one":
        kernel_one(*(nums + [2, 256, 20][len(nums):]))
    elif what == "kernel":
        kernel(*(nums + [256, 20][len(nums):]))
    else:
        farm(*(nums + [4096, 16, 3][len(nums):]))
