"""What the tail trims cost (Tail trims), measured in fresh processes.
    python tools/tail_bench.py kernel [MiB, default 256] [calls, default 20]
        one mode-2 block on the device, in a process of its own; the median wall time and the device time (HIP events; the
        span "tailtrim" is k_adapter_find where an adapter is given, k_tail_find and the judge, "clip" k_adapter_find and the
        judge, "trim" the judge alone) of `calls` calls each, as size queries (out == NULL), of
          - poly-G alone against the adapter clip alone: both read exactly the sequence lines;
          - the window 4:20 alone against the trim q_tail = 20 alone: both read exactly the quality lines;
          - adapter + poly-G + window 4:20 against adapter + q_tail = 20;
        and the last pair once more with `out` given (search, judge, scan, gather, the copy of the kept bytes into page-locked
        memory).  The block is the synthetic one, in which next to nothing is found, and -- to see the cost of what is found --
        the same block with a tail of 20 G written over the 3' end of every fourth read and a drop of four qualities to Phred 2
        in the middle of every fourth.
        (the child alone: python tools/tail_bench.py kernel_one [MiB] [calls] -- the form to put behind
        `rocprofv3 --kernel-trace --stats --`; tools/rocprof_kernel_table.py makes the table.)
    python tools/tail_bench.py farm [MiB, default 4096] [workers, default 16] [rounds, default 3]
        mode-2 input, archive written with --index: fqc_tool d against d --adapter and d --adapter --poly-g --window 4:20,
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
    report = np.zeros(B.TAIL_REPORT_WORDS, dtype=np.uint64)
    n = C.c_size_t(0)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    adapter = B.read_adapter(TRUSEQ)
    q_tail = B.read_trim(q_tail=20)
    poly, window, both = B.read_tail("G"), B.read_tail(window_len=4, window_q=20), B.read_tail("G", window_len=4, window_q=20)
    res = {"block_MiB": round(raw.size / 2 ** 20, 1), "records": len(recs), "calls": calls, "blocks": []}
    for planted in (False, True):
        if planted:
            raw = raw.copy()
            for r in recs[::4]:
                so, qo, L = int(r["seq_off"]), int(r["qual_off"]), int(r["len"])
                raw[so + L - min(20, L):so + L] = ord("G")
                raw[qo + L // 2:qo + min(L // 2 + 4, L)] = 33 + 2
        b = ctx.dblock(raw, recs)

        def tail(a, x, t, with_out):
            rc = lib.fqgpu_dblock_tailtrim(ctx.h, b.h, p(a), p(x), p(t), None, p(out) if with_out else None, out.size, C.byref(n), p(report), None,
                                           None, None)
            assert rc == 0, rc

        def clip(t, with_out):
            rc = lib.fqgpu_dblock_clip(ctx.h, b.h, p(adapter), p(t), None, p(out) if with_out else None, out.size, C.byref(n), p(report), None, None)
            assert rc == 0, rc

        def trim(t):
            rc = lib.fqgpu_dblock_trim(ctx.h, b.h, p(t), None, None, out.size, C.byref(n), p(report), None, None)
            assert rc == 0, rc

        def timed(fn):
            report[:] = 0
            ctx.enable_timing(True)
            wall = []
            for _ in range(calls):
                t0 = time.perf_counter()
                fn()
                wall.append((time.perf_counter() - t0) * 1e3)
            _, spans = ctx.last_timing()
            return {"wall_ms_median": round(statistics.median(wall), 4), "kernel_ms_per_call": {name: round(ms / calls, 4) for name, ms, _ in spans},
                    "poly_percent": round(100 * int(report[16]) / len(recs), 2), "window_percent": round(100 * int(report[18]) / len(recs), 2),
                    "kept_MiB": round(n.value / 2 ** 20, 1)}

        tail(adapter, both, None, True); clip(q_tail, True); trim(q_tail); ctx.sync()   # (allocations, tables)
        res["blocks"].append({
            "planted": planted,
            "poly-G alone, size query": timed(lambda: tail(None, poly, None, False)),
            "clip alone, size query": timed(lambda: clip(None, False)),
            "window 4:20 alone, size query": timed(lambda: tail(None, window, None, False)),
            "trim q_tail 20, size query": timed(lambda: trim(q_tail)),
            "clip + poly-G + window 4:20, size query": timed(lambda: tail(adapter, both, None, False)),
            "clip + q_tail 20, size query": timed(lambda: clip(q_tail, False)),
            "clip + poly-G + window 4:20, with out": timed(lambda: tail(adapter, both, None, True)),
            "clip + q_tail 20, with out": timed(lambda: clip(q_tail, True)),
        })
        b.close()
    print(json.dumps(res), flush=True)
    ctx.close()


def kernel(mib, calls):
    subprocess.run([sys.executable, os.path.abspath(__file__), "kernel_one", str(mib), str(calls)], check=True, timeout=600)


def farm(mib, workers, rounds):
    exe = build_tool()
    with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
        src, arc, plain, clipped, tailed = (os.path.join(tmp, n) for n in ("in.fastq", "a.fqc", "plain.fastq", "clipped.fastq", "tailed.fastq"))
        write_input(src, mib)
        t = ["-t", str(workers)]
        seconds([exe, "c", src, arc] + t + ["--index"])
        variants = [("d", [exe, "d", arc, plain] + t, plain), ("d --adapter", [exe, "d", arc, clipped] + t + ["--adapter", TRUSEQ], clipped),
                    ("d --adapter --poly-g --window 4:20", [exe, "d", arc, tailed] + t + ["--adapter", TRUSEQ, "--poly-g", "--window", "4:20"], tailed)]
        out = {name: [] for name, _, _ in variants}
        written = {}
        seconds(variants[0][1])  # (page cache: a warm-up of the box, and the archive both read)
        for _ in range(rounds):
            for name, cmd, path in variants:
                out[name].append(round(seconds(cmd)["seconds"], 3))
                written[name] = os.path.getsize(path)
        med = {name: statistics.median(v) for name, v in out.items()}
        print(json.dumps({"farm_MiB": mib, "workers": workers, "worker_seconds": out, "bytes_written": written,
                          "clipped_against_plain_percent": round(100 * (med["d --adapter"] / med["d"] - 1), 1),
                          "tailed_against_clipped_percent": round(100 * (med["d --adapter --poly-g --window 4:20"] / med["d --adapter"] - 1), 1),
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
