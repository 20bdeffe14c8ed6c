"""What the mate merge costs (Mate merging), measured in fresh processes.
    python tools/merge_bench.py kernel [MiB, default 256] [calls, default 20]
        one mode-2 block and a mate block built from it -- every read's reverse complement with fresh qualities, so that every
        pair overlaps at d = 0 -- on the device: the median wall time and the device time (HIP events; the span "pair_merge"
        is k_merge_size, the scan and k_merge_emit) of `calls` calls of fqgpu_dblock_pair_merge
          (a) with inserts all 0;
          (b) with every pair's insert: every pair merged;
          (c) with every fourth pair's insert;
        each beside fqgpu_dblock_pair_correct with every pair's insert and nothing to correct (correct_bench.py's case (b)) and
        fqgpu_dblock_select_marked of mate 1 with `out`, on the same blocks in the same process, and fqgpu_dblock_pair_overlap
        at the defaults.
        (the child alone: python tools/merge_bench.py merge_one [MiB] [calls])
    python tools/merge_bench.py farm [MiB, default 1024] [workers, default 16] [rounds, default 3]
        two mode-2 inputs of that size whose records are overlapping mates, archives written with --index: fqc_tool d --mate
        --overlap-report against the same with --merge, alternating, every run a fresh process: worker seconds of every run
        beside the plain runs' spread, and the merge's counts"""
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fqcomp28_amd import binding as B  # noqa: E402
import fqcomp28_amd as F  # noqa: E402
from correct_bench import COMP, context, timed  # noqa: E402


def mates(mib, seed=28, first_read_id=0):
    """-> (raw1, recs, raw2, inserts): raw2 is raw1 with every sequence line reverse-complemented and fresh qualities"""
    raw1, n = F.synth_fastq(mib << 20, 2, seed=seed, first_read_id=first_read_id)
    recs = F.parse_fastq(raw1)
    L = recs["len"].astype(np.int64)
    assert int(L.max()) <= B.OVERLAP_MAX_LEN and int(L.min()) >= 3
    so, qo = recs["seq_off"].astype(np.int64), recs["qual_off"].astype(np.int64)
    raw2 = raw1.copy()
    rng = np.random.default_rng(seed + 1)
    for length in np.unique(L):   # (mode 2 has few lengths: a gather per length)
        rows = np.flatnonzero(L == length)
        k = np.arange(length)
        raw2[so[rows, None] + k] = COMP[raw1[so[rows, None] + (length - 1 - k)]]
        raw2[qo[rows, None] + k] = rng.integers(33, 75, (rows.size, int(length)), dtype=np.uint8)
    return raw1, recs, raw2, L.astype(np.uint16)


def merge_one(mib, calls):
    raw1, recs, raw2, ins = mates(mib)
    n = len(recs)
    ctx = context(raw1, recs)
    b1, b2 = ctx.dblock(raw1, recs), ctx.dblock(raw2, recs)
    res = {"block_MiB": round(raw1.size / 2 ** 20, 1), "pairs": n, "calls": calls}
    got = {}
    out = np.zeros(raw1.size, dtype=np.uint8)   # (a pair merged at d = 0 is no longer than mate 1's record)

    def merge(inserts):
        def go():
            got.update(b1.pair_merge(0, b2, 0, n, inserts, None, B.read_merge(), out=out))
            assert got["rc"] == 0, got["rc"]
        return go

    def correct():
        got.update(b1.pair_correct(0, b2, 0, n, ins, B.read_correct(), want_arrays=True))
        assert got["rc"] == 0, got["rc"]

    def overlap():
        got.update(b1.pair_overlap(0, b2, 0, n, B.read_overlap(), want_arrays=True))
        assert got["rc"] == 0, got["rc"]

    def select():
        got.update(b1.select_marked(0, n))
        assert got["rc"] == 0 and got["out_len"] == raw1.size, got["rc"]

    res["overlap"] = timed(ctx, overlap, calls)
    res["pairs that overlap at d = 0"] = int((got["insert"] == ins).sum())
    res["correct, every pair, nothing disagrees"] = timed(ctx, correct, calls)
    assert got["report"][1:6].tolist() == [n, 0, 0, 0, 0], got["report"].tolist()
    res["select_marked with out"] = timed(ctx, select, calls)
    res["(a) inserts all 0"] = timed(ctx, merge(np.zeros(n, dtype=np.uint16)), calls)
    assert got["report"].tolist() == [n] + [0] * 15
    res["(b) every pair merged"] = timed(ctx, merge(ins), calls)
    assert got["report"][1:4].tolist() == [n, n, int(ins.astype(np.int64).sum())] and int(got["report"][6]) == 0, got["report"].tolist()
    res["(b) bytes_out"] = int(got["out_len"])
    fourth = np.where(np.arange(n) % 4 == 0, ins, 0).astype(np.uint16)
    res["(c) every fourth pair merged"] = timed(ctx, merge(fourth), calls)
    assert got["report"][1:3].tolist() == [(n + 3) // 4, (n + 3) // 4], got["report"].tolist()
    dev = lambda key, span: res[key]["device_ms_median"][span]  # noqa: E731
    both = dev("correct, every pair, nothing disagrees", "pair_correct") + sum(res["select_marked with out"]["device_ms_median"].values())
    res["(b) / (correct + select_marked)"] = round(dev("(b) every pair merged", "pair_merge") / both, 3)
    res["(a) / overlap"] = round(dev("(a) inserts all 0", "pair_merge") / dev("overlap", "pair_overlap"), 3)
    print(json.dumps(res), flush=True)


def write_overlapping_mates(path1, path2, mib):
    done, next_id = 0, 0
    with open(path1, "wb") as f1, open(path2, "wb") as f2:
        while done < mib:
            raw1, recs, raw2, _ = mates(min(64, mib - done), first_read_id=next_id)
            raw1.tofile(f1); raw2.tofile(f2); next_id += len(recs); done += 64


def farm(mib, workers, rounds):
    from checksum_bench import build_tool, seconds
    exe = build_tool()
    with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
        path = lambda name: os.path.join(tmp, name)  # noqa: E731
        note = lambda what: print(what, file=sys.stderr, flush=True)  # noqa: E731
        write_overlapping_mates(path("m1.fastq"), path("m2.fastq"), mib)
        note("inputs written")
        t = ["-t", str(workers)]
        seconds([exe, "c", path("m1.fastq"), path("m1.fqc")] + t + ["--index"])
        seconds([exe, "c", path("m2.fastq"), path("m2.fqc")] + t + ["--index"])
        note("archives written")
        plain = [exe, "d", path("m1.fqc"), path("p1.fastq"), "--mate", path("m2.fqc"), path("p2.fastq"), "--overlap-report", path("ov.tsv")] + t
        seconds(plain)  # (page cache: a warm-up of the box)
        runs = {"d --mate --overlap-report": [], "d --mate --overlap-report --merge": []}
        last = {}
        for _ in range(rounds):
            runs["d --mate --overlap-report"].append(round(seconds(plain)["seconds"], 3))
            last = seconds(plain + ["--merge", path("mg.fastq")])
            runs["d --mate --overlap-report --merge"].append(round(last["seconds"], 3))
            note("round done")
        a, b = (statistics.median(v) for v in runs.values())
        plain_runs = runs["d --mate --overlap-report"]
        print(json.dumps({"farm_MiB_per_mate": mib, "workers": workers, "worker_seconds": runs, "pairs": last["pairs"], "merge": last["merge"],
                          "merge_against_plain_percent": round(100 * (b / a - 1), 1),
                          "spread_percent_of_plain": round(100 * (max(plain_runs) - min(plain_runs)) / a, 1)}), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    nums = [int(x) for x in sys.argv[2:]]
    if what == "merge_one":
        merge_one(*(nums + [256, 20][len(nums):]))
    elif what == "kernel":
        mib, calls = nums + [256, 20][len(nums):]
        subprocess.run([sys.executable, os.path.abspath(__file__), "merge_one", str(mib), str(calls)], check=True, timeout=900)
    else:
        farm(*(nums + [1024, 16, 3][len(nums):]))
