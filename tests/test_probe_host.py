"""The host side of adapter content, no GPU: the reference (tests/probe_ref.py) against adapter_ref's clip, probe by probe,
fqgpu_probe_words, fqgpu_probes_check, the fingerprint, fqgpu_probe_merge, the device calls' answer without a device, and
the tool's usage errors."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

import adapter_ref as AR
import filter_ref as FR
import probe_ref as PR
import test_trim_host as TH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_OVERFLOW, E_ARG, E_NO_DEVICE = -1, -4, -5
TRUSEQ = b"AGATCGGAAGAGC"


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    F.lib()
    return F


def chunk(seed, n=400, probes=()):
    """reads of 1 .. 199 bases with N, in half of them one of the probes' sequences planted somewhere (over the end or not)"""
    rng = np.random.default_rng(seed)
    bases = np.frombuffer(b"ACGTN", dtype=np.uint8)
    parts = []
    for i, L in enumerate(rng.integers(1, 200, n).tolist()):
        s = bases[rng.choice(5, L, p=[0.24, 0.24, 0.24, 0.24, 0.04])].copy()
        if probes and rng.random() < 0.5:
            A = np.frombuffer(probes[int(rng.integers(0, len(probes)))], dtype=np.uint8)
            p = int(rng.integers(0, L))
            s[p:p + min(A.size, L - p)] = A[:min(A.size, L - p)]
        parts.append(TH.record(b"r%d" % i, s.tobytes(), [30] * L))
    raw = np.frombuffer(b"".join(parts), dtype=np.uint8)
    return raw, FR.parse(raw)


SEQS = [TRUSEQ, b"CTGTCTCTTATACACATCT", b"A" * 20, b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA", b"G"]
SET = [AR.adp(TRUSEQ), AR.adp(SEQS[1], 3, 20), AR.adp(SEQS[2], 20, 0), AR.adp(SEQS[3], 5, 10), AR.adp(SEQS[4], 1, 0), AR.adp(TRUSEQ)]


def test_every_probe_is_the_clip_with_that_adapter_alone():
    raw, recs = chunk(11, probes=SEQS)
    p = PR.prb(SET)
    w, places = PR.probe_of(raw, recs, p, 64)
    v = PR.view(w)
    lens = recs["len"].astype(np.int64)
    assert v["n_records"] == len(recs) and v["n_bases"] == int(lens.sum()) and v["n"] == len(SET) and v["positions"] == 64
    for k, a in enumerate(SET):
        _, report, _, _, clip = AR.clip_records(raw, recs, a)
        assert int(v["tables"][k, 0]) == int(report[AR.READS_WITH_ADAPTER]) > 0
        assert int(v["tables"][k, 1]) == int(report[AR.BASES_CUT_ADAPTER])
        assert places[:, k].tolist() == clip.tolist()
        assert int(v["rows"][k].sum()) == int(v["tables"][k, 0])
        assert int(v["tables"][k, 3]) == int((clip == 0).sum())
        assert int(v["tables"][k, 2]) == int((clip + AR.fields(a)[1] <= lens).sum())
        assert not v["tables"][k, 4:].any()
    # "any" is the leftmost cut of all; equal probes give equal tables; the long TruSeq probe shows whole less often
    a = places.min(axis=1)
    assert [int(x) for x in v["tables"][len(SET), :4]] == [int((a < lens).sum()), int((lens - a).sum()), 0, int((a == 0).sum())]
    assert v["rows"][len(SET)].tolist() == np.bincount(np.minimum(a[a < lens], 64), minlength=65).tolist()
    assert v["tables"][0].tolist() == v["tables"][5].tolist() and v["rows"][0].tolist() == v["rows"][5].tolist()
    assert int(v["tables"][3, 2]) < int(v["tables"][0, 2])
    assert int(v["rows"][0, 64]) > 0, "places at and beyond P share the last row"


def test_probe_words(F):
    B = F.binding
    for n, P in ((1, 1), (1, 65535), (16, 1), (16, 65535), (3, 512)):
        assert B.probe_words(n, P) == PR.words(n, P) == 8 + (n + 1) * (8 + P + 1)
    for n, P in ((0, 5), (17, 5), (1, 0), (1, 65536), (0, 0)):
        assert B.probe_words(n, P) == PR.words(n, P) == 0
    assert B.PROBES_MAX == PR.PROBES_MAX and B.PROBE_WINDOW_ROWS == PR.WINDOW_ROWS
    assert {"fqgpu_probe_words", "fqgpu_probes_check", "fqgpu_chunk_probe", "fqgpu_dblock_probe", "fqgpu_probe_merge"} <= set(B.EXPORTS)


ONE = [AR.adp(TRUSEQ)]
GOOD = [dict(adapters=ONE), dict(adapters=SET), dict(adapters=ONE * 16), dict(adapters=[AR.adp("A", 1), AR.adp("ACGT" * 16, 64, 50)])]
BAD = [dict(adapters=[]), dict(adapters=ONE * 16, n=17), dict(adapters=ONE, reserved=(1, 0, 0)), dict(adapters=ONE, reserved=(0, 0, 1)),
       dict(adapters=[AR.adp(TRUSEQ), AR.adp(TRUSEQ, 14)]), dict(adapters=[AR.adp("ACGTN")]), dict(adapters=[AR.adp(TRUSEQ, reserved=1)]),
       dict(adapters=ONE * 2, n=1), dict(adapters=ONE, n=2), dict(adapters=ONE, n=0)]


def test_probes_check(F):
    B = F.binding
    for kw in GOOD:
        assert B.probes_check(PR.prb(**kw)) == 0 and PR.check(PR.prb(**kw)), kw
        assert B.read_probes(**kw).tolist() == PR.prb(**kw).tolist()
    for kw in BAD:
        assert B.probes_check(PR.prb(**kw)) == E_ARG and not PR.check(PR.prb(**kw)), kw
    spoilt = PR.prb(ONE)
    spoilt.view(np.uint8)[-1] = 1      # the last byte of probe[15]
    assert B.probes_check(spoilt) == E_ARG and not PR.check(spoilt)
    spoilt = PR.prb(ONE)
    spoilt[4 + AR.ADAPTER_WORDS] = 1   # the first byte behind probe[0]
    assert B.probes_check(spoilt) == E_ARG and not PR.check(spoilt)
    assert F.lib().fqgpu_probes_check(None) == E_ARG
    assert B.read_probes(ONE).nbytes == 16 + 16 * 80


def _merge(B, dst, src):
    dst = dst.copy()
    return B.probe_merge(dst, src), dst


def test_probe_merge_and_the_fingerprint(F):
    B = F.binding
    raw, recs = chunk(12, probes=SEQS)
    p = PR.prb(SET)
    P = 37
    whole, _ = PR.probe_of(raw, recs, p, P)
    assert int(whole[4]) == PR.fingerprint(p) == zlib.crc32(p[4:4 + len(SET) * 20].tobytes()) == zlib.crc32(b"".join(a.tobytes() for a in SET))
    half = len(recs) // 2
    a, b = PR.probe_of(raw, recs[:half], p, P)[0], PR.probe_of(raw, recs[half:], p, P)[0]
    rc, got = _merge(B, a, b)
    assert rc == 0 and got.tolist() == whole.tolist() == PR.merge(a, b).tolist(), "two halves give the whole"
    rc, got = _merge(B, np.zeros_like(a), b)
    assert rc == 0 and got.tolist() == b.tolist(), "a dst of all zeros is empty"
    empty = PR.probe_of(raw, recs[:0], p, P)[0]
    assert empty[0] == 0 and int(empty[4]) == PR.fingerprint(p)
    rc, got = _merge(B, empty, b)
    assert rc == 0 and got.tolist() == b.tolist(), "an empty dst becomes a copy"
    rc, got = _merge(B, a, empty)
    assert rc == 0 and got.tolist() == a.tolist(), "an empty src adds nothing"
    # refusals leave dst as it is
    other_n = PR.probe_of(raw, recs[half:], PR.prb(SET[:5]), P)[0]
    other_P = PR.probe_of(raw, recs[half:], p, P + 1)[0]
    other_set = PR.probe_of(raw, recs[half:], PR.prb(SET[:5] + [AR.adp(TRUSEQ, 6)]), P)[0]
    assert other_set.size == b.size and other_set[4] != b[4]
    for src in (other_n, other_P, other_set, b[:-1]):
        rc, got = _merge(B, a, np.ascontiguousarray(src))
        assert rc == E_ARG and got.tolist() == a.tolist()
    for dst in (other_n, other_P, other_set):
        empty_dst = dst.copy()
        empty_dst[0] = 0     # an empty result of another probe set is still another probe set
        assert B.probe_merge(empty_dst, b) == E_ARG
    lib = F.lib()
    assert lib.fqgpu_probe_merge(None, 0, None, 0) == E_ARG
    short = np.zeros(4, dtype=np.uint64)
    assert B.probe_merge(short, short.copy()) == E_ARG
    spoilt = b.copy()
    spoilt[2] = 99
    assert B.probe_merge(a.copy(), spoilt) == E_ARG


def test_the_device_calls_say_no_device_without_one(F):
    """(with a device in the machine the same calls get as far as their arguments: no handle, FQGPU_E_ARG)"""
    want = E_NO_DEVICE if F.device_count() == 0 else E_ARG
    lib = F.lib()
    p = PR.prb(ONE)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    out = np.full(PR.words(1, 8), 7, dtype=np.uint64)
    assert lib.fqgpu_chunk_probe(None, ptr(p), 8, ptr(out), out.size, None) == want
    assert lib.fqgpu_dblock_probe(None, None, ptr(p), 8, ptr(out), out.size, None) == want
    assert lib.fqgpu_chunk_probe(None, None, 0, None, 0, None) == want, "said before any argument is looked at"
    assert lib.fqgpu_dblock_probe(None, None, None, 0, None, 0, None) == want
    if want == E_NO_DEVICE:
        assert (out == 7).all(), "nothing is looked at"


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("probe_tool") / "fqc_tool")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tools", "fqc_tool.cpp"),
                    "-L" + os.path.join(ROOT, "fqcomp28_amd"), "-lfqgpu", "-Wl,-rpath," + os.path.join(ROOT, "fqcomp28_amd"),
                    "-lpthread"], check=True)
    return exe


ALL = ["--adapters", "all"]


@pytest.mark.parametrize("args", [
    # --adapters with d, x or t, or without a report to write
    ["d", "in.fqc", "out.fastq"] + ALL,
    ["x", "in.fqc"] + ALL,
    ["t", "in.fqc"] + ALL,
    ["c", "in.fastq", "out.fqc"] + ALL,
    ["d", "in.fqc", "out.fastq", "--adapter", "AGATCGGAAGAGC"] + ALL,
    # an item that is neither a built-in name nor valid
    ["s", "in.fqc", "report.tsv", "--adapters", "truseq,illumina"],
    ["s", "in.fqc", "report.tsv", "--adapters", "agatcggaagagc"],
    ["s", "in.fqc", "report.tsv", "--adapters", "x=AGATNGGAAGAGC"],
    ["s", "in.fqc", "report.tsv", "--adapters", "x=" + "ACGT" * 16 + "A"],
    ["s", "in.fqc", "report.tsv", "--adapters", "x="],
    ["s", "in.fqc", "report.tsv", "--adapters", "=ACGT"],
    ["s", "in.fqc", "report.tsv", "--adapters", ""],
    ["s", "in.fqc", "report.tsv", "--adapters", "truseq,,nextera"],
    ["c", "in.fastq", "out.fqc", "--stats", "report.tsv", "--adapters", "ALL"],
    ["s", "in.fqc", "report.tsv"] + ALL + ["--adapter-overlap", "0"],
    ["s", "in.fqc", "report.tsv"] + ALL + ["--adapter-err", "51"],
    ["s", "in.fqc", "report.tsv"] + ALL + ["--adapter-err", "x"],
    ["s", "in.fqc", "report.tsv", "--adapters"],
    # more than 16 probes after expansion
    ["s", "in.fqc", "report.tsv", "--adapters", "all,truseq,nextera,solid,poly-a,poly-g,ACGTACGT,x=ACGTACGA,truseq-r1"],
    ["c", "in.fastq", "out.fqc", "--stats", "report.tsv", "--adapters", ",".join(["ACGTAC"] * 17)],
    # --adapter together with s or c
    ["s", "in.fqc", "report.tsv", "--adapter", "AGATCGGAAGAGC"] + ALL,
    ["c", "in.fastq", "out.fqc", "--stats", "report.tsv", "--adapter", "AGATCGGAAGAGC"] + ALL,
    # the other adapter options without --adapters
    ["s", "in.fqc", "report.tsv", "--adapter-overlap", "5"],
    ["c", "in.fastq", "out.fqc", "--stats", "report.tsv", "--adapter-err", "10"],
])
def test_usage_errors_are_said_before_any_file_or_device_is_touched(tool, tmp_path, args):
    r = subprocess.run([tool] + args, capture_output=True, text=True, cwd=tmp_path, timeout=60)
    assert r.returncode == 2 and r.stdout == "" and r.stderr, (args, r.stderr)
    assert os.listdir(tmp_path) == []


def test_a_good_list_gets_as_far_as_the_archive(tool, tmp_path):
    """sixteen probes, names and bare sequences: no usage error -- the missing archive is what ends the command"""
    r = subprocess.run([tool, "s", "in.fqc", "report.tsv", "--adapters", "all,ACGTACGT,x=ACGTACGA,truseq,nextera,solid,poly-a,poly-g",
                        "--adapter-overlap", "7", "--adapter-err", "0", "--positions", "40"], capture_output=True, text=True, cwd=tmp_path, timeout=60)
    assert r.returncode == 1 and r.stdout == "" and "in.fqc" in r.stderr
    assert os.listdir(tmp_path) == []
