"""What the overlap correction costs (Overlap correction), measured in fresh processes.
    python tools/correct_bench.py kernel [MiB, default 256] [calls, default 20] [rounds, default 3]
        one mode-2 block and a mate block built from it -- every read's reverse complement with fresh qualities, so that every
        pair overlaps at d = 0 and nothing disagrees -- on the device: the median wall time and the device time (HIP events;
        the span "pair_correct" is both launches of k_pair_correct, "pair_overlap" is k_pair_overlap) of `calls` calls of
        fqgpu_dblock_pair_correct
          (a) with inserts all 0;
          (b) with every pair's insert, nothing to correct: one launch;
          (c) as (b) with a substitution planted in every fourth pair, a poor base against a confident one: two launches.
              A correction is applied once, so the two blocks are built afresh in front of every call;
        each beside fqgpu_dblock_pair_overlap at the defaults on the same blocks in the same process.  Then, when
        FQGPU_PARENT_LIB names the parent commit's library, fqgpu_dblock_pair_overlap alone with this library and with that
        one, alternately, `rounds` runs each: that kernel must not have moved.
        (the children alone: python tools/correct_bench.py correct_one | overlap_one [MiB] [calls])
    python tools/correct_bench.py farm [MiB, default 4096] [workers, default 16] [rounds, default 3]
        two mode-2 inputs of that size whose records are mates, archives written with --index: fqc_tool d --mate
        --overlap-report against d --mate --overlap-report --overlap-correct, alternating, every run a fresh process: worker
        seconds of every run beside the plain runs' spread, and the correction's counts"""
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

NEW = [name for name in B._PROTOS if "correct" in name]
if os.environ.get("FQGPU_LIB"):  # (the parent's library has everything the overlap figure needs)
    have = C.CDLL(os.environ["FQGPU_LIB"])
    for name in NEW:
        if not hasattr(have, name):
            del B._PROTOS[name]
import fqcomp28_amd as F  # noqa: E402

COMP = np.zeros(256, dtype=np.uint8)
COMP[list(b"ACGTN")] = list(b"TGCAN")
OTHER = np.zeros(256, dtype=np.uint8)
OTHER[list(b"ACGTN")] = list(b"CATGA")   # another base, never the same one


def mates(mib):
    """-> (raw1, recs, raw2, planted raw1, planted raw2, inserts): raw2 is raw1 with every sequence line reverse-complemented
    and fresh qualities; the planted pair has, in every fourth record, another base of Phred 0 in the middle of mate 2 against
    a base of Phred 40 in mate 1"""
    raw1, n = F.synth_fastq(mib << 20, 2, seed=28)
    recs = F.parse_fastq(raw1)
    L = recs["len"].astype(np.int64)
    assert int(L.max()) <= B.OVERLAP_MAX_LEN and int(L.min()) >= 3
    so, qo = recs["seq_off"].astype(np.int64), recs["qual_off"].astype(np.int64)
    raw2 = raw1.copy()
    rng = np.random.default_rng(29)
    for length in np.unique(L):   # (mode 2 has few lengths: a gather per length)
        rows = np.flatnonzero(L == length)
        k = np.arange(length)
        raw2[so[rows, None] + k] = COMP[raw1[so[rows, None] + (length - 1 - k)]]
        raw2[qo[rows, None] + k] = rng.integers(33, 75, (rows.size, int(length)), dtype=np.uint8)
    fourth = np.arange(0, n, 4)
    at = L[fourth] // 2                      # place j of mate 2 stands beside place L - 1 - j of mate 1
    plant1, plant2 = raw1.copy(), raw2.copy()
    plant2[so[fourth] + at] = OTHER[raw2[so[fourth] + at]]
    plant2[qo[fourth] + at] = 33
    plant1[qo[fourth] + L[fourth] - 1 - at] = 33 + 40
    not_n = raw1[so[fourth] + L[fourth] - 1 - at] != ord("N")
    return raw1, recs, raw2, plant1, plant2, L.astype(np.uint16), int(not_n.sum())


def context(raw, recs):
    head = min(raw.size, 32 << 20)
    sft, qft = F.freq_tables(raw[:head], recs[: max(1, len(recs) * head // raw.size - 1)])
    return F.Context(sft, qft)


def timed(ctx, fn, calls, before=None):
    if before:
        before()
    fn()
    ctx.sync()  # (allocations)
    wall, device = [], {}
    for _ in range(calls):
        if before:
            before()
            ctx.sync()
        ctx.enable_timing(True)
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        for name, ms, _ in ctx.last_timing()[1]:
            device.setdefault(name, []).append(ms)
        ctx.enable_timing(False)
    return {"wall_ms_median": round(statistics.median(wall), 4), "device_ms_median": {k: round(statistics.median(v), 4) for k, v in device.items()}}


def correct_one(mib, calls):
    raw1, recs, raw2, plant1, plant2, ins, plantable = mates(mib)
    n = len(recs)
    ctx = context(raw1, recs)
    res = {"block_MiB": round(raw1.size / 2 ** 20, 1), "pairs": n, "calls": calls}
    blocks = {}

    def build(a, b):
        def go():
            for blk in blocks.values():
                blk.close()
            blocks["a"], blocks["b"] = ctx.dblock(a, recs), ctx.dblock(b, recs)
        return go

    got = {}

    def correct(inserts):
        def go():
            got.update(blocks["a"].pair_correct(0, blocks["b"], 0, n, inserts, B.read_correct(), want_arrays=True))
            assert got["rc"] == 0, got["rc"]
        return go

    def overlap():
        got.update(blocks["a"].pair_overlap(0, blocks["b"], 0, n, B.read_overlap(), want_arrays=True))
        assert got["rc"] == 0, got["rc"]

    build(raw1, raw2)()
    res["overlap, clean mates"] = timed(ctx, overlap, calls)
    res["pairs that overlap at d = 0"] = int((got["insert"] == ins).sum())
    res["(a) inserts all 0"] = timed(ctx, correct(np.zeros(n, dtype=np.uint16)), calls)
    assert got["report"].tolist() == [n, 0, 0, 0, 0, 0, 0, 0]
    res["(b) every pair, nothing disagrees"] = timed(ctx, correct(ins), calls)
    assert got["report"][1:6].tolist() == [n, 0, 0, 0, 0], got["report"].tolist()
    build(plant1, plant2)()
    res["overlap, planted mates"] = timed(ctx, overlap, calls)
    res["(c) a substitution in every fourth pair"] = timed(ctx, correct(ins), calls, before=build(plant1, plant2))
    assert got["report"][1:5].tolist() == [n, plantable, 0, plantable], got["report"].tolist()
    res["(c) bases corrected"] = plantable
    ov = res["overlap, clean mates"]["device_ms_median"]["pair_overlap"]
    res["(a) / overlap"] = round(res["(a) inserts all 0"]["device_ms_median"]["pair_correct"] / ov, 3)
    res["(b) / overlap"] = round(res["(b) every pair, nothing disagrees"]["device_ms_median"]["pair_correct"] / ov, 3)
    res["(c) / overlap"] = round(res["(c) a substitution in every fourth pair"]["device_ms_median"]["pair_correct"] /
                                 res["overlap, planted mates"]["device_ms_median"]["pair_overlap"], 3)
    print(json.dumps(res), flush=True)


def overlap_one(mib, calls):
    raw1, recs, raw2, _, _, ins, _ = mates(mib)
    n = len(recs)
    ctx = context(raw1, recs)
    b1, b2 = ctx.dblock(raw1, recs), ctx.dblock(raw2, recs)

    def call():
        assert b1.pair_overlap(0, b2, 0, n, B.read_overlap(), want_arrays=True)["rc"] == 0

    res = timed(ctx, call, calls)
    print(json.dumps({"library": F.lib_path(), "pairs": n, "pair_overlap": res}), flush=True)


def child(what, mib, calls, lib=None):
    env = dict(os.environ)
    if lib:
        env["FQGPU_LIB"] = lib
    else:
        env.pop("FQGPU_LIB", None)
    subprocess.run([sys.executable, os.path.abspath(__file__), what, str(mib), str(calls)], check=True, timeout=900, env=env)


def kernel(mib, calls, rounds):
    child("correct_one", mib, calls)
    parent = os.environ.get("FQGPU_PARENT_LIB")
    for _ in range(rounds if parent else 0):
        child("overlap_one", mib, calls)
        child("overlap_one", mib, calls, parent)


def farm(mib, workers, rounds):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
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
        plain = [exe, "d", path("m1.fqc"), path("p1.fastq"), "--mate", path("m2.fqc"), path("p2.fastq"), "--overlap-report", path("ov.tsv")] + t
        seconds(plain)  # (page cache: a warm-up of the box)
        runs = {"d --mate --overlap-report": [], "d --mate --overlap-report --overlap-correct": []}
        last = {}
        for _ in range(rounds):
            runs["d --mate --overlap-report"].append(round(seconds(plain)["seconds"], 3))
            last = seconds(plain + ["--overlap-correct"])
            runs["d --mate --overlap-report --overlap-correct"].append(round(last["seconds"], 3))
            note("round done")
        a, b = (statistics.median(v) for v in runs.values())
        plain_runs = runs["d --mate --overlap-report"]
        print(json.dumps({"farm_MiB_per_mate": mib, "workers": workers, "worker_seconds": runs, "overlap": last["overlap"],
                          "overlap_correct_against_plain_percent": round(100 * (b / a - 1), 1),
                          "spread_percent_of_plain": round(100 * (max(plain_runs) - min(plain_runs)) / a, 1)}), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    nums = [int(x) for x in sys.argv[2:]]
    if what == "correct_one":
        correct_one(*(nums + [256, 20][len(nums):]))
    elif what == "overlap_one":
        overlap_one(*(nums + [256, 20][len(nums):]))
    elif what == "kernel":
        kernel(*(nums + [256, 20, 3][len(nums):]))
    else:
        farm(*(nums + [4096, 16, 3][len(nums):]))
