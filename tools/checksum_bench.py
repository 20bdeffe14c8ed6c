"""What the chunk checksums cost, measured in fresh processes, the variants alternating.
    python tools/checksum_bench.py kernel
        one 256 MiB block: encoded three times, digested three times; prints the device time of every kernel group
        (HIP events).  Under `rocprofv3 --kernel-trace --stats -- python tools/checksum_bench.py kernel` the trace
        holds k_crc_slices / k_crc_fold beside k_tile_hist2.
    python tools/checksum_bench.py compress [MiB, default 4096] [workers, default 16] [rounds, default 3]
        fqc_tool c without and with --checksum (worker seconds of every run)
    python tools/checksum_bench.py restore [MiB, default 1024] [workers, default 4] [rounds, default 3]
        -R 256, without and with decode indexes: d without a sums file, d with one, t
CHECKSUM_BENCH_PARENT=<fqc_tool of the parent commit, linked to its own library> adds that tool's c / d as the baseline."""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fqcomp28_amd as F  # noqa: E402


def build_tool():
    exe = os.path.join(ROOT, "tools", "_build", "fqc_tool")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O2", "-o", exe, os.path.join(ROOT, "tools", "fqc_tool.cpp"), "-L" + os.path.join(ROOT, "fqcomp28_amd"),
                    "-lfqgpu", "-Wl,-rpath," + os.path.join(ROOT, "fqcomp28_amd"), "-lpthread"], check=True)
    return exe


def write_input(path, mib):
    done, next_id = 0, 0
    with open(path, "wb") as f:
        while done < mib << 20:
            raw, n = F.synth_fastq(min(64 << 20, (mib << 20) - done), 2, seed=28, first_read_id=next_id)
            raw.tofile(f); next_id += n; done += 64 << 20


def seconds(cmd):
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, (cmd, run.stderr[-500:])
    return json.loads(run.stdout.splitlines()[-1])


def kernel():
    raw, _ = F.synth_fastq(256 << 20, 2, seed=28)
    recs = F.parse_fastq(raw)
    sft, qft = F.freq_tables(raw[: 32 << 20], recs[: len(recs) // 8])
    ctx = F.Context(sft, qft)
    b = ctx.dblock(raw, recs)
    b.encode(); b.crc32(); ctx.sync()   # (allocations, tables)
    ctx.enable_timing(True)
    for _ in range(3):
        b.encode()
        ctx.sync()
        b.crc32()
    total, spans = ctx.last_timing()
    print(json.dumps({"block_MiB": raw.size >> 20, "kernel_ms_per_call": {n: round(ms / calls, 4) for n, ms, calls in spans}}))
    b.close(); ctx.close()


def compress(mib, workers, rounds):
    exe, parent = build_tool(), os.environ.get("CHECKSUM_BENCH_PARENT")
    with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
        src, arc = os.path.join(tmp, "in.fastq"), os.path.join(tmp, "a.fqc")
        write_input(src, mib)
        variants = ([("parent c", parent, [])] if parent else []) + [("c", exe, []), ("c --checksum", exe, ["--checksum"])]
        out = {name: [] for name, _, _ in variants}
        seconds([exe, "c", src, arc, "-t", str(workers)])  # (page cache, pin cache of nobody: a warm-up of the box)
        for _ in range(rounds):
            for name, tool, opts in variants:
                out[name].append(round(seconds([tool, "c", src, arc, "-t", str(workers)] + opts)["seconds"], 3))
        print(json.dumps({"compress_MiB": mib, "workers": workers, "worker_seconds": out}))


def restore(mib, workers, rounds):
    exe, parent = build_tool(), os.environ.get("CHECKSUM_BENCH_PARENT")
    with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
        src, back = os.path.join(tmp, "in.fastq"), os.path.join(tmp, "back.fastq")
        write_input(src, mib)
        for index in ([], ["--index"]):
            plain, sums = os.path.join(tmp, "plain.fqc"), os.path.join(tmp, "sums.fqc")
            seconds([exe, "c", src, plain, "-t", str(workers), "-R", "256"] + index)
            seconds([exe, "c", src, sums, "-t", str(workers), "-R", "256", "--checksum"] + index)
            variants = ([("parent d", [parent, "d", plain, back])] if parent else []) + \
                       [("d, no sums file", [exe, "d", plain, back]), ("d, verified", [exe, "d", sums, back]), ("t", [exe, "t", sums])]
            out = {name: [] for name, _ in variants}
            for _ in range(rounds):
                for name, cmd in variants:
                    rep = seconds(cmd + ["-t", str(workers)])
                    assert name not in ("d, verified", "t") or rep["verified"] > 0
                    out[name].append(round(rep["seconds"], 3))
            print(json.dumps({"restore_MiB": mib, "workers": workers, "decode_index": bool(index), "worker_seconds": out}), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    nums = [int(x) for x in sys.argv[2:]]
    if what == "kernel":
        kernel()
    elif what == "compress":
        compress(*(nums + [4096, 16, 3][len(nums):]))
    else:
        restore(*(nums + [1024, 4, 3][len(nums):]))
