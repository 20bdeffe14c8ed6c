"""`fqc_tool d --fasta` on a real GPU: the farm behind it (processArchiveFasta in fqcomp28_amd/csrc/process.hpp) restores
names and bases of a multi-block archive in input order, with and without the decode index file, whole or by record
range, and neither reads nor decodes a quality stream.  The expected FASTA is made here from the input FASTQ."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import fqc_archive as A  # noqa: E402
from test_gpu_fasta import fasta_records  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    assert F.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return F


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fasta_farm") / "fqc_tool")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-o", exe, os.path.join(ROOT, "tools", "fqc_tool.cpp"),
                    "-L" + os.path.join(ROOT, "fqcomp28_amd"), "-lfqgpu", "-Wl,-rpath," + os.path.join(ROOT, "fqcomp28_amd"),
                    "-lpthread"], check=True)
    return exe


def run(tool, *args):
    """(under a time limit of its own: a farm that waits for a piece that never comes must not outlive the test)"""
    return subprocess.run(["timeout", "-k", "10", "300", tool] + [str(x) for x in args], capture_output=True, text=True, timeout=400)


def report(r):
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def archive(F, tool, tmp_path_factory):
    """a multi-block archive with its decode index file, the input's expected FASTA record by record"""
    d = tmp_path_factory.mktemp("fasta_in")
    raw, _ = F.synth_fastq(40 << 20, 4, seed=19)
    fq = d / "in.fastq"
    raw.tofile(fq)
    arc = d / "a.fqc"
    report(run(tool, "c", fq, arc, "-t", 4, "-R", 4, "-S", 4, "--index", "--index-stride", 64))
    recs = F.parse_fastq(raw)
    counts = [b.n_records for b in A.read_archive(str(arc))[3]]
    assert len(counts) >= 8 and sum(counts) == len(recs)
    return d, arc, raw, fasta_records(raw, recs), counts


def restore(tool, arc, out, want, *extra):
    rep = report(run(tool, "d", arc, out, "--fasta", "-t", 3, *extra))
    got = open(out, "rb").read()
    assert got == want, (len(got), len(want))
    assert rep["form"] == "fasta" and rep["raw_bytes"] == len(want) and rep["sums"] == "none" and rep["verified"] == 0
    assert not os.path.exists(str(out) + ".part")
    os.remove(out)
    return rep


def test_farm_restores_the_fasta_with_and_without_the_index_file(F, tool, archive, tmp_path):
    d, arc, raw, want, counts = archive
    n = len(want)
    e = np.concatenate([[0], np.cumsum(counts)]).astype(int)
    ranges = [(e[1] + 7, e[4] - 9), (e[2] + 10, e[2] + 50), (0, 1), (n - 1, n), (e[3], e[4])]  # the first: across two block borders and more
    size = os.path.getsize(arc)
    quals = sum(len(b.qual) for b in A.read_archive(str(arc))[3])
    local = tmp_path / "a.fqc"
    os.symlink(arc, local)
    os.symlink(str(arc) + ".fqx", str(local) + ".fqx")
    for indexed in (True, False):
        if not indexed:
            os.remove(str(local) + ".fqx")
        rep = restore(tool, local, tmp_path / "all.fasta", b"".join(want))
        assert rep["records"] == n and sum(rep["blocks_per_worker"]) == len(counts)
        assert rep["index"] == ("used" if indexed else "none") and rep["indexed_blocks"] == (len(counts) if indexed else 0)
        # what was read of the archive: everything but the quality streams (and the tables, the index and the size words around)
        assert rep["archive_bytes_read"] <= size - quals + 64 * len(counts)
        for a, b in ranges:
            rep = restore(tool, local, tmp_path / "r.fasta", b"".join(want[a:b]), "--records", "%d:%d" % (a, b))
            overlap = sum(1 for k in range(len(counts)) if e[k] < b and e[k + 1] > a)
            assert rep["records"] == b - a and sum(rep["blocks_per_worker"]) == overlap, (a, b)
        restore(tool, local, tmp_path / "tail.fasta", b"".join(want[e[5] + 3:]), "--records", "%d:" % (e[5] + 3))
    # and the FASTQ restore is what it was: no word of the form in its report
    rep = report(run(tool, "d", local, tmp_path / "back.fastq", "-t", 3))
    assert "form" not in rep and "archive_bytes_read" not in rep
    assert open(tmp_path / "back.fastq", "rb").read() == raw.tobytes()


def rewrite(arc, out, change):
    first, sft, qft, blocks, _ = A.read_archive(str(arc))
    for b in blocks:
        change(b)
    A.write_archive(str(out), first, sft, qft, blocks)


def test_farm_neither_reads_nor_decodes_the_qualities(F, tool, archive, tmp_path):
    d, arc, raw, want, counts = archive
    bad = tmp_path / "noqual.fqc"

    def no_qualities(b):
        b.qual = b"\0" * 5

    rewrite(arc, bad, no_qualities)
    rep = restore(tool, bad, tmp_path / "all.fasta", b"".join(want))
    assert rep["records"] == len(want)
    out = tmp_path / "back.fastq"
    r = run(tool, "d", bad, out, "-t", 3)
    assert r.returncode == 1 and "fqc_tool:" in r.stderr, r.stdout + r.stderr
    assert not os.path.exists(out) and not os.path.exists(str(out) + ".part")


def test_farm_damaged_sequence_stream_ends_the_command_and_leaves_no_file(F, tool, archive, tmp_path):
    """one run of an input the coder reports as corrupt (as the damaged-block test of the FASTQ restore): block 2 of 10
    or so, so that workers with later pieces are waiting in the writer when it is found"""
    d, arc, raw, want, counts = archive
    bad = tmp_path / "badseq.fqc"

    def damage(b):
        if b.idx == 2:
            s = bytearray(b.seq)
            mid = len(s) // 2
            for i in range(mid, mid + 32):
                s[i] ^= 0x5A
            b.seq = bytes(s)

    rewrite(arc, bad, damage)
    out = tmp_path / "bad.fasta"
    r = run(tool, "d", bad, out, "--fasta", "-t", 3)
    assert r.returncode == 1, (r.returncode, r.stdout, r.stderr)  # (124: it hung and was ended)
    line = [x for x in r.stderr.splitlines() if x.startswith("fqc_tool:")]
    assert line and "chunk 2" in line[-1], r.stderr
    assert not os.path.exists(out) and not os.path.exists(str(out) + ".part")
