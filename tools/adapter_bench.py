"""What adapter clipping costs (Adapter clipping), measured in fresh processes.
    python tools/adapter_bench.py kernel [MiB, default 256] [calls, default 20]
        one mode-2 block on the device, in a process of its own; the median wall time and the device time (HIP events; the
        span "clip" is k_adapter_find and the judge, "trim" / "filter" the judge alone) of `calls` calls each of
          - the clip alone as a size query (out == NULL), against the max_n filter as a size query: both read exactly the
            sequence lines;
          - the same clip against the trim q_front = q_tail = 20 as a size query, which reads the quality lines;
          - the clip plus q_tail = 20 with `out` given (search, judge, scan, gather, the copy of the kept bytes into page-locked
            memory) against that trim alone with `out`.
        The adapter is the 33-base TruSeq adapter, which no synthetic read holds, and -- to see the cost of what is found -- the
        same block with it written over the 3' end of every fourth read.
        (the child alone: python tools/adapter_bench.py kernel_one [MiB] [calls] -- the form to put behind
        `rocprofv3 --kernel-trace --stats --`; tools/rocprof_kernel_table.py makes the table.)
    python tools/adapter_bench.py farm [MiB, default 4096] [workers, default 16] [rounds, default 3]
        mode-2 input, archive written with --index: fqc_tool d against d --trim-q3 20 and d --adapter ... --trim-q3 20,
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

TRUSEQ = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"


def kernel_one(mib, calls):
    raw, _ = F.synth_fastq(mib << 20, 2, seed=28)
    recs = F.parse_fastq(raw)
    sft, qft = F.freq_tables(raw[: min(raw.size, 32 << 20)], recs[: max(1, len(recs) * min(raw.size, 32 << 20) // raw.size - 1)])
    ctx = F.Context(sft, qft)
    lib = F.lib()
    out = F.pinned_empty(raw.size)
    report = np.zeros(B.TRIM_REPORT_WORDS, dtype=np.uint64)
    n = C.c_size_t(0)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    adapter = B.read_adapter(TRUSEQ)
    q_both, q_tail = B.read_trim(q_front=20, q_tail=20), B.read_trim(q_tail=20)
    res = {"block_MiB": round(raw.size / 2 ** 20, 1), "records": len(recs), "calls": calls, "adapter_bases": len(TRUSEQ), "blocks": []}
    for planted in (False, True):
        if planted:      # the adapter's first 20 bases over the 3' end of every fourth read
            raw = raw.copy()
            a = np.frombuffer(TRUSEQ[:20].encode(), dtype=np.uint8)
            for r in recs[::4]:
                k = min(20, int(r["len"]))
                raw[int(r["seq_off"]) + int(r["len"]) - k:int(r["seq_off"]) + int(r["len"])] = a[:k]
        b = ctx.dblock(raw, recs)

        def clip(t, with_out):
            rc = lib.fqgpu_dblock_clip(ctx.h, b.h, p(adapter), p(t), None, p(out) if with_out else None, out.size, C.byref(n), p(report), None, None)
            assert rc == 0, rc

        def trim(t, with_out):
            rc = lib.fqgpu_dblock_trim(ctx.h, b.h, p(t), None, p(out) if with_out else None, out.size, C.byref(n), p(report), None, None)
            assert rc == 0, rc

        def filt(f):
            rc = lib.fqgpu_dblock_filter(ctx.h, b.h, p(f), None, 0, C.byref(n), p(report), None)
            assert rc == 0, rc

        def timed(fn):
            ctx.enable_timing(True)
            wall = []
            for _ in range(calls):
                t0 = time.perf_counter()
                fn()
                wall.append((time.perf_counter() - t0) * 1e3)
            _, spans = ctx.last_timing()
            return {"wall_ms_median": round(statistics.median(wall), 4), "kernel_ms_per_call": {name: round(ms / calls, 4) for name, ms, _ in spans},
                    "with_adapter_percent": round(100 * int(report[14]) / len(recs), 2), "kept_MiB": round(n.value / 2 ** 20, 1)}

        clip(q_tail, True); trim(q_tail, True); filt(B.read_filter(max_n=0)); ctx.sync()   # (allocations, tables)
        res["blocks"].append({
            "planted": planted,
            "clip alone, size query": timed(lambda: clip(None, False)),
            "filter max_n 0, size query": timed(lambda: filt(B.read_filter(max_n=0))),
            "trim q_front 20 q_tail 20, size query": timed(lambda: trim(q_both, False)),
            "clip + q_tail 20, with out": timed(lambda: clip(q_tail, True)),
            "trim q_tail 20, with out": timed(lambda: trim(q_tail, True)),
        })
        b.close()
    print(json.dumps(res), flush=True)
    ctx.close()


def kernel(mib, calls):
    subprocess.run([sys.executable, os.path.abspath(__file__), "kernel_one", str(mib), str(calls)], check=True, timeout=600)


def farm(mib, workers, rounds):
    exe = build_tool()
    with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
        src, arc, plain, cut, clipped = (os.path.join(tmp, n) for n in ("in.fastq", "a.fqc", "plain.fastq", "trimmed.fastq", "clipped.fastq"))
        write_input(src, mib)
        t = ["-t", str(workers)]
        seconds([exe, "c", src, arc] + t + ["--index"])
        variants = [("d", [exe, "d", arc, plain] + t, plain), ("d --trim-q3 20", [exe, "d", arc, cut] + t + ["--trim-q3", "20"], cut),
                    ("d --adapter --trim-q3 20", [exe, "d", arc, clipped] + t + ["--adapter", TRUSEQ, "--trim-q3", "20"], clipped)]
        out = {name: [] for name, _, _ in variants}
        written = {}
        seconds(variants[0][1])  # (page cache: a warm-up of the box, and the archive both read)
        for _ in range(rounds):
            for name, cmd, path in variants:
                out[name].append(round(seconds(cmd)["seconds"], 3))
                written[name] = os.path.getsize(path)
        med = {name: statistics.median(v) for name, v in out.items()}
        print(json.dumps({"farm_MiB": mib, "workers": workers, "worker_seconds": out, "bytes_written": written,
                          "trimmed_against_plain_percent": round(100 * (med["d --trim-q3 20"] / med["d"] - 1), 1),
                          "clipped_against_trimmed_percent": round(100 * (med["d --adapter --trim-q3 20"] / med["d --trim-q3 20"] - 1), 1),
                          "spread_percent_of_plain": round(100 * (max(out["d"]) - min(out["d"])) / med["d"], 1)}), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    nums = [int(x) for x in sys.argv[2:]]
    if what == "kernel_one":
        kernel_one(*(nums + [256, 20][len(nums):]))
    elif what == "kernel":
        kernel(*(nums + [256, 20][len(nums):]))
    else:
        farm(*(nums + [4096, 16, 3][len(nums):]))
