"""`fqc_tool s` and `fqc_tool c --stats`: the read summary of a whole file through the farm (process.hpp), against the
rendered numpy restatement (stats_ref.py) of the file, byte for byte."""
import json
import os
import shutil
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import oracle_lib as O
import stats_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import fqc_archive as A  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    if F.device_count() < 1:
        pytest.fail("no GPU visible: the product path has no CPU fallback")
    return F


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stats_farm_tool") / "fqc_tool")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-o", exe, os.path.join(ROOT, "tools", "fqc_tool.cpp"),
                    "-L" + os.path.join(ROOT, "fqcomp28_amd"), "-lfqgpu", "-Wl,-rpath," + os.path.join(ROOT, "fqcomp28_amd"),
                    "-lpthread"], check=True)
    return exe


def run_any(tool, *args):
    return subprocess.run([tool] + [str(a) for a in args], capture_output=True, text=True, timeout=600)


def run_tool(tool, *args):
    r = run_any(tool, *args)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def farm(F, tool, tmp_path_factory):
    """about 6 MiB of mode 4 compressed with -R 1 -t 3: plain, and with --stats (which also gets --index --checksum)"""
    d = tmp_path_factory.mktemp("stats_farm")
    raw, _ = F.synth_fastq(6 << 20, 4, seed=37)
    recs = F.parse_fastq(raw)
    src = d / "in.fastq"
    raw.tofile(src)
    common = ["-t", 3, "-R", 1, "-S", 1, "--index", "--checksum"]
    plain = run_tool(tool, "c", src, d / "plain.fqc", *common)
    rep = run_tool(tool, "c", src, d / "stats.fqc", *common, "--stats", d / "c.tsv")
    return dict(dir=d, raw=raw, recs=recs, plain=plain, rep=rep, want=R.stats_of(raw, recs, 512))


def test_c_stats_reports_the_input_and_leaves_the_archive_alone(farm):
    d, want, rep = farm["dir"], farm["want"], farm["rep"]
    assert rep["blocks"] >= 5
    assert (d / "c.tsv").read_bytes() == R.render(want)
    assert not os.path.exists(str(d / "c.tsv") + ".part")
    # the same blocks (they lie in completion order in the file: compared block by block), the same size
    x, y = A.read_archive(str(d / "plain.fqc")), A.read_archive(str(d / "stats.fqc"))
    key = lambda p: (p.idx, p.total, p.n_records, p.seq, p.qual, p.readlens, p.n_count, p.n_pos, p.fields)  # noqa: E731
    assert x[:3] == y[:3] and [key(p) for p in x[3]] == [key(p) for p in y[3]]
    assert os.path.getsize(d / "plain.fqc") == os.path.getsize(d / "stats.fqc")
    # the JSON line
    phred_sum = int((R.view(want)["qual_pos"].sum(axis=0) * np.arange(64, dtype=np.uint64)).sum())
    assert rep["stats"] == str(d / "c.tsv") and rep["records"] == int(want[0]) and rep["bases"] == int(want[1])
    assert rep["mean_quality"] == float("%.6f" % (phred_sum / int(want[1])))
    assert "stats" not in farm["plain"] and "bases" not in farm["plain"]


def test_c_stats_with_one_worker_writes_the_same_archive(F, tool, farm, tmp_path):
    """(with one worker the blocks are written in order: the two archives are the same bytes)"""
    d = farm["dir"]
    run_tool(tool, "c", d / "in.fastq", tmp_path / "a.fqc", "-t", 1, "-R", 1, "-S", 1)
    run_tool(tool, "c", d / "in.fastq", tmp_path / "b.fqc", "-t", 1, "-R", 1, "-S", 1, "--stats", tmp_path / "b.tsv", "--positions", 100)
    assert (tmp_path / "a.fqc").read_bytes() == (tmp_path / "b.fqc").read_bytes()
    assert (tmp_path / "b.tsv").read_bytes() == R.render(R.stats_of(farm["raw"], farm["recs"], 100))


def test_s_gives_the_same_bytes_whatever_the_workers_and_the_index(tool, farm, tmp_path):
    d, want = farm["dir"], R.render(farm["want"])
    arc = tmp_path / "a.fqc"
    for ext in ("", ".fqx", ".fqs"):
        shutil.copy(str(d / "stats.fqc") + ext, str(arc) + ext)
    for with_index in (True, False):
        if not with_index:
            os.remove(str(arc) + ".fqx")
        for t in (1, 3):
            out = tmp_path / "s.tsv"
            before = sorted(os.listdir(tmp_path))
            rep = run_tool(tool, "s", arc, out, "-t", t)
            assert out.read_bytes() == want, (with_index, t)
            assert sorted(os.listdir(tmp_path)) == sorted(before + ["s.tsv"]), "the report and nothing else"
            assert rep["index"] == ("used" if with_index else "none") and rep["sums"] == "used" and rep["verified"] == farm["rep"]["blocks"]
            assert rep["stats"] == str(out) and rep["records"] == int(farm["want"][0]) and rep["bases"] == int(farm["want"][1])
            assert rep["mean_quality"] == farm["rep"]["mean_quality"]
            os.remove(out)


def test_more_workers_than_blocks(F, tool, tmp_path, golden_dir):
    """workers that never get a chunk hold an empty summary, which merges as nothing"""
    raw, recs = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_1.fastq"))
    src = tmp_path / "in.fastq"
    raw.tofile(src)
    want = R.render(R.stats_of(raw, recs, 512))
    rep = run_tool(tool, "c", src, tmp_path / "one.fqc", "-t", 4, "--stats", tmp_path / "c.tsv")
    assert rep["blocks"] == 1 and sorted(rep["blocks_per_worker"]) == [0, 0, 0, 1]
    assert (tmp_path / "c.tsv").read_bytes() == want
    rep = run_tool(tool, "s", tmp_path / "one.fqc", tmp_path / "s.tsv", "-t", 4)
    assert sorted(rep["blocks_per_worker"]) == [0, 0, 0, 1] and rep["records"] == len(recs)
    assert (tmp_path / "s.tsv").read_bytes() == want


def test_s_on_an_archive_of_the_independent_writer(F, tool, tmp_path, golden_dir):
    import test_archive as TA
    raw, recs = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_1.fastq"))
    arc = tmp_path / "o.fqc"
    TA.oracle_archive(F, str(arc), raw, recs, 3, order=[2, 0, 1])
    rep = run_tool(tool, "s", arc, tmp_path / "o.tsv", "-t", 2)
    assert (tmp_path / "o.tsv").read_bytes() == R.render(R.stats_of(raw, recs, 512))
    assert rep["sums"] == "none" and rep["records"] == len(recs)
    # --positions 64 on reads of 100: row 64 collects the rest
    run_tool(tool, "s", arc, tmp_path / "o64.tsv", "-t", 2, "--positions", 64)
    text = (tmp_path / "o64.tsv").read_bytes()
    want = R.stats_of(raw, recs, 64)
    assert text == R.render(want)
    assert b"\nlen\t64\t%d\n" % len(recs) in text and b"\nbase\t64\t" in text and b"\nbase\t65\t" not in text
    assert int(R.view(R.parse(text))["base_pos"][64].sum()) == 36 * len(recs)


def test_a_failed_s_leaves_no_report(F, tool, farm, tmp_path):
    d = farm["dir"]
    first_header, sft, qft, blocks, _ = A.read_archive(str(d / "stats.fqc"))
    # a damaged quality stream (most single bits are refused by the decoder: take the first archive that is)
    bad = tmp_path / "bad.fqc"
    out = tmp_path / "bad.tsv"
    k = 2
    good_qual = blocks[k].qual
    for at in range(len(good_qual) // 2, len(good_qual) // 2 + 64):
        q = bytearray(good_qual)
        q[at] ^= 0x10
        blocks[k].qual = bytes(q)
        A.write_archive(str(bad), first_header, sft, qft, blocks)
        r = run_any(tool, "s", bad, out, "-t", 3)
        if r.returncode != 0:
            break
    assert r.returncode == 1 and r.stderr, r.stdout
    assert not os.path.exists(out) and not os.path.exists(str(out) + ".part")
    # a well-formed sums file that records another digest for one chunk (layout: archive.hpp, ChunkSumsFile)
    arc = tmp_path / "a.fqc"
    shutil.copy(d / "stats.fqc", arc)
    data = bytearray(open(str(d / "stats.fqc") + ".fqs", "rb").read())
    n = struct.unpack_from("<I", data, 4)[0]
    sums = [list(struct.unpack_from("<III", data, 8 + 12 * i)) for i in range(n)]
    sums[k][0] ^= 1
    file_crc = 0
    for i, (crc, length, _) in enumerate(sums):
        struct.pack_into("<III", data, 8 + 12 * i, *sums[i])
        file_crc = F.crc32_combine(file_crc, crc, length)
    at = 8 + 12 * n
    struct.pack_into("<I", data, at, file_crc)
    struct.pack_into("<I", data, at + 28, zlib.crc32(bytes(data[:at + 28])))
    open(str(arc) + ".fqs", "wb").write(data)
    r = run_any(tool, "s", arc, out, "-t", 3)
    assert r.returncode == 1 and "checksum of chunk %d does not hold" % k in r.stderr, (r.stdout, r.stderr)
    assert not os.path.exists(out) and not os.path.exists(str(out) + ".part")
    assert run_any(tool, "t", arc, "-t", 3).returncode == 1, "the exit code of t"
