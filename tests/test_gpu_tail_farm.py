"""`fqc_tool d ... [--poly-g [N] | --poly-x [N]] [--poly-every K] [--poly-mism M] [--window W:Q]`: the restore of a whole archive
with the tail trims through the farm (process.hpp: processArchiveSelected), against the numpy restatement (tail_ref.py) of
the input file, byte for byte."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import adapter_ref as AR
import filter_ref as FR
import oracle_lib as O
import tail_ref as TR
import test_gpu_adapter_farm as AF
import test_gpu_trim_farm as TF
import trim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

ADAPTER = AF.ADAPTER
TAIL_KEYS = dict(reads_with_poly_tail=TR.READS_WITH_POLY, bases_cut_poly=TR.BASES_CUT_POLY, reads_window_cut=TR.READS_WINDOW_CUT,
                 bases_cut_window=TR.BASES_CUT_WINDOW)
TAIL_WORDS = dict(TF.TRIM_WORDS, **TAIL_KEYS)
OPTIONS = ["--poly-g", "--window", "4:20"]


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    if F.device_count() < 1:
        pytest.fail("no GPU visible: the product path has no CPU fallback")
    return F


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tail_farm_tool") / "fqc_tool")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-o", exe, os.path.join(ROOT, "tools", "fqc_tool.cpp"),
                    "-L" + os.path.join(ROOT, "fqcomp28_amd"), "-lfqgpu", "-Wl,-rpath," + os.path.join(ROOT, "fqcomp28_amd"),
                    "-lpthread"], check=True)
    return exe


def planted_file(golden_dir):
    """test_gpu_adapter_farm's planted file (about 3 MiB, adapters in half of the reads); over it, in a third of the reads, a
    tail of 8 .. 40 G with one base in twenty wrong and high qualities, in front of the adapter where there is one and at the
    3' end elsewhere, and in a third a drop of 2 .. 6 qualities to Phred 2 somewhere in the read"""
    raw, recs = AF.planted_file(golden_dir)
    clip = AR.clip_records(raw, recs, AR.adp(ADAPTER))[4]
    rng = np.random.default_rng(44)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)
    for r, end in zip(recs, clip.tolist()):
        so, qo, L = int(r["seq_off"]), int(r["qual_off"]), int(r["len"])
        if rng.random() < 0.33 and end >= 8:
            k = min(int(rng.integers(8, 41)), end)
            tail = np.full(k, ord("G"), dtype=np.uint8)
            wrong = rng.random(k) < 0.05
            tail[wrong] = bases[rng.integers(0, 4, int(wrong.sum()))]
            raw[so + end - k:so + end] = tail
            raw[qo + end - k:qo + end] = 33 + 38
        if rng.random() < 0.33:
            at = int(rng.integers(0, L))
            raw[qo + at:qo + min(at + int(rng.integers(2, 7)), L)] = 33 + 2
    return raw, recs


@pytest.fixture(scope="module")
def farm(F, tool, tmp_path_factory, golden_dir):
    """the planted file compressed with -R 1 -t 3 --index --checksum, and what the reference makes of it"""
    d = tmp_path_factory.mktemp("tail_farm")
    raw, recs = planted_file(golden_dir)
    src = d / "in.fastq"
    raw.tofile(src)
    rep = TF.run_tool(tool, "c", src, d / "a.fqc", "-t", 3, "-R", 1, "-S", 1, "--index", "--checksum")
    want = TR.tail_records(raw, recs, None, TR.tl("G", window_len=4, window_q=20))
    n = len(recs)
    assert rep["blocks"] >= 3 and 0.1 * n < int(want[1][TR.READS_WITH_POLY]) < 0.6 * n and 0.2 * n < int(want[1][TR.READS_WINDOW_CUT]) < n
    return dict(dir=d, raw=raw, recs=recs, rep=rep, want=want)


def report_matches(rep, want, words):
    assert rep["trim"] == {k: int(want[1][w]) for k, w in words.items()}
    assert rep["records"] == int(want[1][R.N_KEPT]) and rep["raw_bytes"] == int(want[1][R.BYTES_KEPT])


def test_the_restore_with_the_tail_trims_is_what_the_reference_makes(tool, farm, tmp_path):
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
            report_matches(rep, want, TAIL_WORDS)
            assert "filter" not in rep and "reads_with_adapter" not in rep["trim"], "no adapter, no filter: neither is printed"
            os.remove(out)


def test_beside_the_adapter_the_trim_and_the_filter(tool, farm, tmp_path):
    d, raw, recs = farm["dir"], farm["raw"], farm["recs"]
    a = AR.adp(ADAPTER)
    for options, args in (
            (["--adapter", ADAPTER.decode(), "--poly-g", "--window", "4:20", "--trim-q3", 20, "--min-len", 20],
             (a, TR.tl("G", window_len=4, window_q=20), R.trm(q_tail=20), FR.flt(min_len=20))),
            (["--poly-x", 8, "--poly-every", 4, "--poly-mism", 2, "--cut-front", 2], (None, TR.tl("ACGT", 8, 4, 2), R.trm(cut_front=2), None)),
            (["--window", "17:25", "--adapter", ADAPTER.decode(), "--max-n", 0], (a, TR.tl(window_len=17, window_q=25), None, FR.flt(max_n=0))),
            (["--poly-g", 12], (None, TR.tl("G", 12), None, None))):
        want = TR.tail_records(raw, recs, *args)
        rep = TF.run_tool(tool, "d", d / "a.fqc", tmp_path / "o.fastq", "-t", 3, *options)
        assert (tmp_path / "o.fastq").read_bytes() == want[0].tobytes(), options
        words = dict(AF.CLIP_WORDS, **TAIL_KEYS) if args[0] is not None else TAIL_WORDS
        report_matches(rep, want, words)
        assert ("filter" in rep) == (args[3] is not None) and list(rep["trim"]) == list(words), "the new keys stand last"
        assert 0 < int(want[1][R.N_KEPT]) < len(recs) or args[3] is None


def test_runs_without_the_new_options_print_what_they_printed(tool, farm, tmp_path):
    d, raw, recs = farm["dir"], farm["raw"], farm["recs"]
    plain = TF.run_tool(tool, "d", d / "a.fqc", tmp_path / "plain.fastq", "-t", 3)
    assert "trim" not in plain and "filter" not in plain and (tmp_path / "plain.fastq").read_bytes() == raw.tobytes()
    rep = TF.run_tool(tool, "d", d / "a.fqc", tmp_path / "t.fastq", "-t", 3, "--trim-q3", 20)
    want = R.trim_records(raw, recs, R.trm(q_tail=20))
    assert (tmp_path / "t.fastq").read_bytes() == want[0].tobytes()
    TF.report_matches(rep, want, False)
    assert list(rep["trim"]) == list(TF.TRIM_WORDS), "the trim's keys, in their order"
    rep = TF.run_tool(tool, "d", d / "a.fqc", tmp_path / "c.fastq", "-t", 3, "--adapter", ADAPTER.decode(), "--trim-q3", 20, "--min-len", 20)
    want = AR.clip_records(raw, recs, AR.adp(ADAPTER), R.trm(q_tail=20), FR.flt(min_len=20))
    assert (tmp_path / "c.fastq").read_bytes() == want[0].tobytes()
    AF.report_matches(rep, want)
    assert list(rep["trim"]) == list(AF.CLIP_WORDS), "the clip's keys, in their order"
    for r in (plain, rep):
        assert "poly" not in json.dumps(r) and "window" not in json.dumps(r)
