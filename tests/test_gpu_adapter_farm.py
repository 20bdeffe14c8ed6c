"""`fqc_tool d ... --adapter SEQ [--adapter-overlap N] [--adapter-err PCT]`: the clipped restore of a whole archive through the
farm (process.hpp: processArchiveSelected), against the numpy restatement (adapter_ref.py) of the input file, byte for byte."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import adapter_ref as AR
import filter_ref as FR
import oracle_lib as O
import test_gpu_trim_farm as TF
import trim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

ADAPTER = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"     # TruSeq, 33 bases
CLIP_WORDS = dict(TF.TRIM_WORDS, reads_with_adapter=AR.READS_WITH_ADAPTER, bases_cut_adapter=AR.BASES_CUT_ADAPTER)
OPTIONS = ["--adapter", ADAPTER.decode(), "--trim-q3", 20, "--min-len", 20]


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    if F.device_count() < 1:
        pytest.fail("no GPU visible: the product path has no CPU fallback")
    return F


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("adapter_farm_tool") / "fqc_tool")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-o", exe, os.path.join(ROOT, "tools", "fqc_tool.cpp"),
                    "-L" + os.path.join(ROOT, "fqcomp28_amd"), "-lfqgpu", "-Wl,-rpath," + os.path.join(ROOT, "fqcomp28_amd"),
                    "-lpthread"], check=True)
    return exe


def planted_file(golden_dir, tiles=12):
    """SRR065390_sub_1.fastq `tiles` times over (about 3 MiB), the adapter written over the bases of a quarter of the reads from
    a random place on, its first 5 .. 20 bases over the 3' end of another quarter, one substitution in half of these"""
    one, _ = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_1.fastq"))
    raw = np.tile(one, tiles)
    recs = FR.parse(raw)
    rng = np.random.default_rng(33)
    a = np.frombuffer(ADAPTER, dtype=np.uint8)
    for r in recs:
        kind, at, L = int(rng.integers(0, 4)), int(r["seq_off"]), int(r["len"])
        if kind > 1:
            continue
        k = min(int(rng.integers(5, 21)), L)
        p = int(rng.integers(0, L)) if kind == 0 else L - k
        k = min(len(a), L - p) if kind == 0 else k
        raw[at + p:at + p + k] = a[:k]
        if rng.random() < 0.5:
            raw[at + p + int(rng.integers(0, k))] = ord("T")
    return raw, recs


@pytest.fixture(scope="module")
def farm(F, tool, tmp_path_factory, golden_dir):
    """the planted file compressed with -R 1 -t 3 --index --checksum, and what the reference makes of it"""
    d = tmp_path_factory.mktemp("adapter_farm")
    raw, recs = planted_file(golden_dir)
    src = d / "in.fastq"
    raw.tofile(src)
    rep = TF.run_tool(tool, "c", src, d / "a.fqc", "-t", 3, "-R", 1, "-S", 1, "--index", "--checksum")
    want = AR.clip_records(raw, recs, AR.adp(ADAPTER), R.trm(q_tail=20), FR.flt(min_len=20))
    n = len(recs)
    assert rep["blocks"] >= 3 and 0.3 * n < int(want[1][AR.READS_WITH_ADAPTER]) < 0.7 * n and 0 < int(want[1][R.N_KEPT]) < n
    assert int(want[1][R.BASES_CUT_TAIL]) > int(want[1][AR.BASES_CUT_ADAPTER]) > 0, "the quality trim cuts beyond the clip"
    return dict(dir=d, raw=raw, recs=recs, rep=rep, want=want)


def report_matches(rep, want):
    assert rep["trim"] == {k: int(want[1][w]) for k, w in CLIP_WORDS.items()}
    assert rep["records"] == int(want[1][R.N_KEPT]) and rep["raw_bytes"] == int(want[1][R.BYTES_KEPT])


def test_the_clipped_restore_is_what_the_reference_makes(tool, farm, tmp_path):
    d, want = farm["dir"], farm["want"]
    arc = tmp_path / "a.fqc"
    for ext in ("", ".fqx", ".fqs"):
        shutil.copy(str(d / "a.fqc") + ext, str(arc) + ext)
    for with_index in (True, False):
        if not with_index:
            os.remove(str(arc) + ".fqx")
        for t in (1, 3):
            out = tmp_path / "out.fastq"
            listing = sorted(os.listdir(tmp_path))
            rep = TF.run_tool(tool, "d", arc, out, "-t", t, *OPTIONS)
            assert out.read_bytes() == want[0].tobytes(), (with_index, t)
            assert sorted(os.listdir(tmp_path)) == sorted(listing + ["out.fastq"]), "the output and nothing else"
            assert rep["index"] == ("used" if with_index else "none") and rep["sums"] == "used" and rep["verified"] == farm["rep"]["blocks"]
            report_matches(rep, want)
            assert rep["filter"]["kept"] == rep["trim"]["kept"], "printed as for a filtered restore"
            os.remove(out)


def test_the_adapter_alone_and_its_two_options(tool, farm, tmp_path):
    d, raw, recs = farm["dir"], farm["raw"], farm["recs"]
    for options, a in ((["--adapter", ADAPTER.decode()], AR.adp(ADAPTER)),
                       (["--adapter", ADAPTER[:13].decode(), "--adapter-overlap", 8, "--adapter-err", 0], AR.adp(ADAPTER[:13], 8, 0)),
                       (["--adapter", "ACGT", "--adapter-overlap", 30, "--adapter-err", 25], AR.adp(b"ACGT", 4, 25))):
        want = AR.clip_records(raw, recs, a)
        rep = TF.run_tool(tool, "d", d / "a.fqc", tmp_path / "o.fastq", "-t", 3, *options)
        assert (tmp_path / "o.fastq").read_bytes() == want[0].tobytes(), options
        report_matches(rep, want)
        assert "filter" not in rep and rep["trim"]["reads_with_adapter"] > 0


def test_runs_without_an_adapter_print_what_they_printed(tool, farm, tmp_path):
    d, raw = farm["dir"], farm["raw"]
    plain = TF.run_tool(tool, "d", d / "a.fqc", tmp_path / "plain.fastq", "-t", 3)
    assert "trim" not in plain and "filter" not in plain and (tmp_path / "plain.fastq").read_bytes() == raw.tobytes()
    rep = TF.run_tool(tool, "d", d / "a.fqc", tmp_path / "t.fastq", "-t", 3, "--trim-q3", 20)
    want = R.trim_records(raw, farm["recs"], R.trm(q_tail=20))
    assert (tmp_path / "t.fastq").read_bytes() == want[0].tobytes()
    TF.report_matches(rep, want, False)
    assert set(rep["trim"]) == set(TF.TRIM_WORDS), "no adapter keys"
    assert "adapter" not in json.dumps(rep)
