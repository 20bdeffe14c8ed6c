"""What a paired restore costs (Paired restores), measured in fresh processes.
    python tools/pair_bench.py kernel [MiB, default 256] [calls, default 20]
        one mode-2 block on the device, in a process of its own; the median wall time and the device time (HIP events; the span
        "select_marked" is the marked call's kernels -- the tail call's and k_select_mark --, "tailtrim" the tail call's,
        "pair_names" k_pair_names, "filter" the judge alone) of `calls` calls each of
          - fqgpu_dblock_select_marked over the whole block with a mark of all ones against fqgpu_dblock_tailtrim with the same
            adapter, tail and trim, both as size queries (out == NULL): the difference is the mark's upload and k_select_mark;
          - the same pair with `out` given, and the marked call once more with a mark that drops every other read;
          - fqgpu_dblock_pair_names of the block against a second copy of itself against the size query of the filter
            max_n = 0, which reads the sequence lines -- about five times the bytes -- in the same scattered pattern.
        (the child alone: python tools/pair_bench.py kernel_one [MiB] [calls])
    python tools/pair_bench.py farm [MiB, default 4096] [workers, default 16] [rounds, default 3]
        two mode-2 inputs of that size whose records are mates (the same read ids, other bases), archives written with --index:
        fqc_tool d --mate --min-mean-q 34 against the two single runs d --min-mean-q 34, alternating, every run a fresh process
        -- once with both archives cut at the same records, once with mate 2 written at half the block size: worker seconds of
        every run, the blocks of both archives and the chunk decodes of archive 2, the spread of the plain runs"""
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
from checksum_bench import build_tool, seconds  # noqa: E402

TRUSEQ = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"


def kernel_one(mib, calls):
    raw, _ = F.synth_fastq(mib << 20, 2, seed=28)
    recs = F.parse_fastq(raw)
    n_recs = len(recs)
    sft, qft = F.freq_tables(raw[: min(raw.size, 32 << 20)], recs[: max(1, n_recs * min(raw.size, 32 << 20) // raw.size - 1)])
    ctx = F.Context(sft, qft)
    lib = F.lib()
    out = F.pinned_empty(raw.size)
    report = np.zeros(B.TAIL_REPORT_WORDS, dtype=np.uint64)
    n, mismatch = C.c_size_t(0), C.c_size_t(0)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    adapter, q_tail, both = B.read_adapter(TRUSEQ), B.read_trim(q_tail=20), B.read_tail("G", window_len=4, window_q=20)
    no_n = B.read_filter(max_n=0)
    ones, half = np.full((n_recs + 7) // 8, 0xFF, dtype=np.uint8), np.full((n_recs + 7) // 8, 0x55, dtype=np.uint8)
    b, mate = ctx.dblock(raw, recs), ctx.dblock(raw, recs)

    def tail(with_out):
        rc = lib.fqgpu_dblock_tailtrim(ctx.h, b.h, p(adapter), p(both), p(q_tail), None, p(out) if with_out else None, out.size, C.byref(n), p(report),
                                       None, None, None)
        assert rc == 0, rc

    def marked(mark, with_out):
        rc = lib.fqgpu_dblock_select_marked(ctx.h, b.h, p(adapter), p(both), p(q_tail), None, 0, n_recs, p(mark), p(out) if with_out else None, out.size,
                                            C.byref(n), p(report), None, None, None)
        assert rc == 0, rc

    def names():
        rc = lib.fqgpu_dblock_pair_names(ctx.h, b.h, 0, mate.h, 0, n_recs, C.byref(mismatch))
        assert rc == 0 and mismatch.value == B.NO_MISMATCH, (rc, mismatch.value)

    def max_n():
        rc = lib.fqgpu_dblock_filter(ctx.h, b.h, p(no_n), None, 0, C.byref(n), p(report), None)
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
                "kept_MiB": round(n.value / 2 ** 20, 1)}

    tail(True); marked(ones, True); names(); max_n(); ctx.sync()   # (allocations, tables)
    res = {"block_MiB": round(raw.size / 2 ** 20, 1), "records": n_recs, "calls": calls,
           "tailtrim, size query": timed(lambda: tail(False)),
           "select_marked, mark of ones, size query": timed(lambda: marked(ones, False)),
           "select_marked, no mark, size query": timed(lambda: marked(None, False)),
           "tailtrim, with out": timed(lambda: tail(True)),
           "select_marked, mark of ones, with out": timed(lambda: marked(ones, True)),
           "select_marked, every other read marked, with out": timed(lambda: marked(half, True)),
           "pair_names": timed(names),
           "filter max_n 0, size query": timed(max_n)}
    print(json.dumps(res), flush=True)
    b.close()
    mate.close()
    ctx.close()


def kernel(mib, calls):
    subprocess.run([sys.executable, os.path.abspath(__file__), "kernel_one", str(mib), str(calls)], check=True, timeout=600)


def write_mates(path1, path2, mib):
    """two mode-2 files with the same read ids: mate 2's records are those of another seed under mate 1's header lines (a
    mode-2 header line holds the read's number and its length, 150 in both)"""
    done, next_id = 0, 0
    with open(path1, "wb") as f1, open(path2, "wb") as f2:
        while done < mib << 20:
            want = min(64 << 20, (mib << 20) - done)
            one, n = F.synth_fastq(want, 2, seed=28, first_read_id=next_id)
            two, m = F.synth_fastq(want, 2, seed=29, first_read_id=next_id)
            assert n == m and one.size == two.size
            one.tofile(f1); two.tofile(f2); next_id += n; done += 64 << 20


def farm(mib, workers, rounds):
    exe = build_tool()
    with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
        path = lambda name: os.path.join(tmp, name)  # noqa: E731
        write_mates(path("m1.fastq"), path("m2.fastq"), mib)
        t, flt = ["-t", str(workers)], ["--min-mean-q", "34"]
        seconds([exe, "c", path("m1.fastq"), path("m1.fqc")] + t + ["--index"])
        seconds([exe, "c", path("m2.fastq"), path("m2.fqc")] + t + ["--index"])
        seconds([exe, "c", path("m2.fastq"), path("m2half.fqc")] + t + ["--index", "-R", "128"])
        single1 = [exe, "d", path("m1.fqc"), path("s1.fastq")] + t + flt
        res = {"farm_MiB_per_mate": mib, "workers": workers}
        seconds(single1)  # (page cache: a warm-up of the box)
        for what, arc2 in (("cut at the same records", "m2.fqc"), ("mate 2 at half the block size", "m2half.fqc")):
            single2 = [exe, "d", path(arc2), path("s2.fastq")] + t + flt
            paired = [exe, "d", path("m1.fqc"), path("p1.fastq"), "--mate", path(arc2), path("p2.fastq")] + t + flt
            runs = {"d mate 1": [], "d mate 2": [], "d --mate": []}
            last = {}
            for _ in range(rounds):
                runs["d mate 1"].append(round(seconds(single1)["seconds"], 3))
                runs["d mate 2"].append(round(seconds(single2)["seconds"], 3))
                last = seconds(paired)
                runs["d --mate"].append(round(last["seconds"], 3))
            singles = [a + b for a, b in zip(runs["d mate 1"], runs["d mate 2"])]
            res[what] = {"worker_seconds": runs, "two_single_runs": [round(s, 3) for s in singles], "pairs": last["pairs"],
                         "blocks1": last["blocks1"], "blocks2": last["blocks2"], "decodes2": last["decodes2"],
                         "bytes_written": [os.path.getsize(path("p1.fastq")), os.path.getsize(path("p2.fastq"))],
                         "paired_against_two_singles_percent": round(100 * (statistics.median(runs["d --mate"]) / statistics.median(singles) - 1), 1),
                         "spread_percent_of_two_singles": round(100 * (max(singles) - min(singles)) / statistics.median(singles), 1)}
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    nums = [int(x) for x in sys.argv[2:]]
    if what == "kernel_one":
        kernel_one(*(nums + [256, 20][len(nums):]))
    elif what == "kernel":
        kernel(*(nums + [256, 20][len(nums):]))
    else:
        farm(*(nums + [4096, 16, 3][len(nums):]))
