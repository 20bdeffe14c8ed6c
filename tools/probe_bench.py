"""What adapter content costs (Adapter content), measured in fresh processes.
    python tools/probe_bench.py kernel [MiB, default 256] [calls, default 20]
        one mode-2 block on the device, in a process of its own; the median wall time and the device time (HIP events; the
        span "probe" is k_adapter_find's probe form, "clip" its single-adapter form and the judge) of `calls` calls each of
          - the probe call with one probe against one fqgpu_dblock_clip size query (out == NULL) of the same adapter;
          - the probe call with sixteen probes against sixteen such size queries, one per probe, one after another;
        the probes are the nine built-ins and seven drawn ones of 12 .. 64 bases.  The block is the synthetic one, in which
        next to nothing is found, and -- to see the cost of the counters -- the same block with a built-in adapter written at
        a random place of every fourth read.
        (the child alone: python tools/probe_bench.py kernel_one [MiB] [calls] -- the form to put behind
        `rocprofv3 --kernel-trace --stats --`; tools/rocprof_kernel_table.py makes the table.)
    python tools/probe_bench.py farm [MiB, default 4096] [workers, default 16] [rounds, default 3]
        mode-2 input, archive written with --index: fqc_tool s against s --adapters all, and c --stats against
        c --stats --adapters all, alternating, every run a fresh process: worker seconds of every run"""
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

BUILTIN = ["AGATCGGAAGAGC", "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA", "AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT", "CTGTCTCTTATACACATCT", "TGGAATTCTCGG",
           "GATCGTCGGACT", "CGCCTTGGCCGT", "A" * 20, "G" * 20]
POSITIONS = 512


def sixteen():
    rng = np.random.default_rng(16)
    drawn = ["".join("ACGT"[i] for i in rng.integers(0, 4, m)) for m in (12, 20, 31, 32, 33, 48, 64)]
    return [B.read_adapter(s) for s in BUILTIN + drawn]


def kernel_one(mib, calls):
    raw, _ = F.synth_fastq(mib << 20, 2, seed=28)
    recs = F.parse_fastq(raw)
    sft, qft = F.freq_tables(raw[: min(raw.size, 32 << 20)], recs[: max(1, len(recs) * min(raw.size, 32 << 20) // raw.size - 1)])
    ctx = F.Context(sft, qft)
    lib = F.lib()
    report = np.zeros(B.TRIM_REPORT_WORDS, dtype=np.uint64)
    n = C.c_size_t(0)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    adapters = sixteen()
    one, many = B.read_probes(adapters[1:2]), B.read_probes(adapters)
    out = np.zeros(B.probe_words(16, POSITIONS), dtype=np.uint64)
    res = {"block_MiB": round(raw.size / 2 ** 20, 1), "records": len(recs), "calls": calls, "positions": POSITIONS, "blocks": []}
    for planted in (False, True):
        if planted:      # a built-in adapter, as much of it as fits, at a random place of every fourth read
            raw = raw.copy()
            rng = np.random.default_rng(4)
            at = rng.integers(0, 1 << 30, len(recs))
            for i, r in enumerate(recs[::4]):
                a = np.frombuffer(BUILTIN[i % len(BUILTIN)].encode(), dtype=np.uint8)
                so, L = int(r["seq_off"]), int(r["len"])
                q = int(at[i]) % L
                raw[so + q:so + q + min(a.size, L - q)] = a[:min(a.size, L - q)]
        b = ctx.dblock(raw, recs)

        def probe(probes):
            rc = lib.fqgpu_dblock_probe(ctx.h, b.h, p(probes), POSITIONS, p(out), out.size, None)
            assert rc == 0, rc

        def clips(which):
            for a in which:
                rc = lib.fqgpu_dblock_clip(ctx.h, b.h, p(a), None, None, None, 0, C.byref(n), p(report), None, None)
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

        probe(many); clips(adapters[:2]); ctx.sync()   # (allocations)
        rows = {"planted": planted,
                "probe, 1 probe": timed(lambda: probe(one)),
                "clip size query, the same adapter": timed(lambda: clips(adapters[1:2])),
                "probe, 16 probes": timed(lambda: probe(many)),
                "16 clip size queries": timed(lambda: clips(adapters))}
        rows["reads_with_any_percent"] = round(100 * int(B.probe_view(out)["tables"][16, 0]) / len(recs), 2)
        for a, b_ in (("probe, 1 probe", "clip size query, the same adapter"), ("probe, 16 probes", "16 clip size queries")):
            rows["%s / %s" % (a, b_)] = {k: round(rows[a][k] / rows[b_][k], 3) for k in ("wall_ms_median",)}
            rows["%s / %s" % (a, b_)]["kernel_ms"] = round(sum(rows[a]["kernel_ms_per_call"].values()) / sum(rows[b_]["kernel_ms_per_call"].values()), 3)
        res["blocks"].append(rows)
        b.close()
    print(json.dumps(res), flush=True)
    ctx.close()


def kernel(mib, calls):
    subprocess.run([sys.executable, os.path.abspath(__file__), "kernel_one", str(mib), str(calls)], check=True, timeout=900)


def farm(mib, workers, rounds):
    exe = build_tool()
    with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
        src, arc, arc2, rep = (os.path.join(tmp, n) for n in ("in.fastq", "a.fqc", "b.fqc", "r.tsv"))
        write_input(src, mib)
        t = ["-t", str(workers)]
        seconds([exe, "c", src, arc] + t + ["--index"])
        probes = ["--adapters", "all"]
        variants = [("s", [exe, "s", arc, rep] + t), ("s --adapters all", [exe, "s", arc, rep] + t + probes),
                    ("c --stats", [exe, "c", src, arc2] + t + ["--stats", rep]), ("c --stats --adapters all", [exe, "c", src, arc2] + t + ["--stats", rep] + probes)]
        out = {name: [] for name, _ in variants}
        seconds(variants[0][1])  # (page cache: a warm-up of the box, and the archive all read)
        for _ in range(rounds):
            for name, cmd in variants:
                out[name].append(round(seconds(cmd)["seconds"], 3))
        med = {name: statistics.median(v) for name, v in out.items()}
        print(json.dumps({"farm_MiB": mib, "workers": workers, "worker_seconds": out,
                          "s_adapters_against_s_percent": round(100 * (med["s --adapters all"] / med["s"] - 1), 1),
                          "c_adapters_against_c_percent": round(100 * (med["c --stats --adapters all"] / med["c --stats"] - 1), 1),
                          "spread_percent_of_s": round(100 * (max(out["s"]) - min(out["s"])) / med["s"], 1),
                          "spread_percent_of_c": round(100 * (max(out["c --stats"]) - min(out["c --stats"])) / med["c --stats"], 1)}), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    nums = [int(x) for x in sys.argv[2:]]
    if what == "kernel_one":
        kernel_one(*(nums + [256, 20][len(nums):]))
    elif what == "kernel":
        kernel(*(nums + [256, 20][len(nums):]))
    else:
        farm(*(nums + [4096, 16, 3][len(nums):]))
