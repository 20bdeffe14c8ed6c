"""What the mate overlap costs (Mate overlap), measured in fresh processes.
    python tools/overlap_bench.py kernel [MiB, default 256] [calls, default 20] [rounds, default 3]
        one mode-2 block and its mate block (the same read ids, the bases of another seed: mode 2's uniform bases give pairs
        without a hit, which is the search's full cost) on the device, each measurement in a process of its own: the median
        wall time and the device time (HIP events; the span "pair_overlap" is k_pair_overlap, "clip" k_adapter_find and the
        judge) of `calls` calls of
          - fqgpu_dblock_pair_overlap at the defaults (30, 5, 20), and at min_overlap 1 with max_mism 65535 and 50 per cent,
            where no walk ends early;
          - fqgpu_dblock_clip as a size query on each of the two blocks, which reads the same lines: with this library and,
            when FQGPU_PARENT_LIB names the parent commit's library, with that one, alternately, `rounds` runs each.
        (the children alone: python tools/overlap_bench.py overlap_one | clip_one [MiB] [calls])
    python tools/overlap_bench.py farm [MiB, default 4096] [workers, default 16] [rounds, default 3]
        two mode-2 inputs of that size whose records are mates, archives written with --index: fqc_tool d --mate against
        d --mate --overlap-trim, alternating, every run a fresh process: worker seconds of every run and the overlap's counts"""
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
from fqcomp28_amd import binding as B  # noqa: E402

NEW = [name for name in B._PROTOS if "overlap" in name or "select_limited" in name]
if os.environ.get("FQGPU_LIB"):  # (a library from before the overlap has everything the clip figure needs)
    have = C.CDLL(os.environ["FQGPU_LIB"])
    for name in NEW:
        if not hasattr(have, name):
            del B._PROTOS[name]
import fqcomp28_amd as F  # noqa: E402

TRUSEQ = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"


def blocks(mib):
    one, n = F.synth_fastq(mib << 20, 2, seed=28)
    two, m = F.synth_fastq(mib << 20, 2, seed=29)
    assert n == m and one.size == two.size
    recs1, recs2 = F.parse_fastq(one), F.parse_fastq(two)
    head = min(one.size, 32 << 20)
    sft, qft = F.freq_tables(one[:head], recs1[: max(1, n * head // one.size - 1)])
    ctx = F.Context(sft, qft)
    return ctx, ctx.dblock(one, recs1), ctx.dblock(two, recs2), n, one.size


def timed(ctx, fn, calls):
    fn()
    ctx.sync()  # (allocations)
    ctx.enable_timing(True)
    wall = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
    _, spans = ctx.last_timing()
    return {"wall_ms_median": round(statistics.median(wall), 4), "kernel_ms_per_call": {name: round(ms / calls, 4) for name, ms, _ in spans}}


def overlap_one(mib, calls):
    ctx, b1, b2, n, size = blocks(mib)
    res = {"block_MiB": round(size / 2 ** 20, 1), "pairs": n, "calls": calls}
    for what, spec in (("defaults (30, 5, 20)", B.read_overlap()), ("no early end (1, 65535, 50)", B.read_overlap(1, 65535, 50))):
        got = {}

        def call():
            got.update(b1.pair_overlap(0, b2, 0, n, spec, want_arrays=True))
            assert got["rc"] == 0, got["rc"]

        res[what] = timed(ctx, call, calls)
        res[what]["pairs_overlapped"] = int(got["out"][1])
    print(json.dumps(res), flush=True)


def clip_one(mib, calls):
    ctx, b1, b2, n, size = blocks(mib)
    adapter = B.read_adapter(TRUSEQ)
    res = {"library": F.lib_path(), "block_MiB": round(size / 2 ** 20, 1), "records": n, "calls": calls}
    for what, b in (("clip, size query, mate 1", b1), ("clip, size query, mate 2", b2)):
        def call():
            assert b.clip(adapter, query=True, want_win=False, want_keep=False)["rc"] == 0

        res[what] = timed(ctx, call, calls)
    print(json.dumps(res), flush=True)


def child(what, mib, calls, lib=None):
    env = dict(os.environ)
    if lib:
        env["FQGPU_LIB"] = lib
    else:
        env.pop("FQGPU_LIB", None)
    subprocess.run([sys.executable, os.path.abspath(__file__), what, str(mib), str(calls)], check=True, timeout=900, env=env)


def kernel(mib, calls, rounds):
    child("overlap_one", mib, calls)
    parent = os.environ.get("FQGPU_PARENT_LIB")
    for _ in range(rounds):
        child("clip_one", mib, calls)
        if parent:
            child("clip_one", mib, calls, parent)


def farm(mib, workers, rounds):
    from checksum_bench import build_tool, seconds
    from pair_bench import write_mates
    exe = build_tool()
    with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
        path = lambda name: os.path.join(tmp, name)  # noqa: E731
        note = lambda what: print(what, file=sys.stderr, flush=True)  # noqa: E731
        write_mates(path("m1.fastq"), path("m2.fastq"), mib)
        note("inputs written")
        t = ["-t", str(workers)]
        seconds([exe, "c", path("m1.fastq"), path("m1.fqc")] + t + ["--index"])
        seconds([exe, "c", path("m2.fastq"), path("m2.fqc")] + t + ["--index"])
        note("archives written")
        plain = [exe, "d", path("m1.fqc"), path("p1.fastq"), "--mate", path("m2.fqc"), path("p2.fastq")] + t
        seconds(plain)  # (page cache: a warm-up of the box)
        runs = {"d --mate": [], "d --mate --overlap-trim": []}
        last = {}
        for _ in range(rounds):
            runs["d --mate"].append(round(seconds(plain)["seconds"], 3))
            last = seconds(plain + ["--overlap-trim"])
            runs["d --mate --overlap-trim"].append(round(last["seconds"], 3))
            note("round done")
        a, b = statistics.median(runs["d --mate"]), statistics.median(runs["d --mate --overlap-trim"])
        print(json.dumps({"farm_MiB_per_mate": mib, "workers": workers, "worker_seconds": runs, "overlap": last["overlap"],
                          "overlap_trim_against_plain_percent": round(100 * (b / a - 1), 1),
                          "spread_percent_of_plain": round(100 * (max(runs["d --mate"]) - min(runs["d --mate"])) / a, 1)}), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    nums = [int(x) for x in sys.argv[2:]]
    if what == "overlap_one":
        overlap_one(*(nums + [256, 20][len(nums):]))
    elif what == "clip_one":
        clip_one(*(nums + [256, 20][len(nums):]))
    elif what == "kernel":
        kernel(*(nums + [256, 20, 3][len(nums):]))
    else:
        farm(*(nums + [4096, 16, 3][len(nums):]))
