"""`fqc_tool d <in1.fqc> <out1.fastq> --mate <in2.fqc> <out2.fastq> --merge <merged.fastq>`: the mate merge through the farm
(process.hpp: processArchivePaired with Selection::merge) against the composition of the existing restatements with
merge_ref.py -- all three outputs, the JSON line and the report's text, byte for byte, whatever -t -- on
test_gpu_overlap_farm's archives, whose mate 2 is written at another -R so that a unit has several pieces of mate 2; the usage
errors; a run that fails; and a run without the option, which writes what it wrote before."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import correct_ref as CR
import filter_ref as FR
import merge_ref as MR
import oracle_lib as O
import overlap_ref as OR
import pair_ref as PR
import test_gpu_overlap_farm as OF
import test_gpu_pair_farm as PF
import test_gpu_tail_farm as GF
import test_gpu_trim_farm as TF
import test_merge_host as HM
import trim_ref as R

pytestmark = pytest.mark.gpu

COPIES = OF.COPIES
COMBINATIONS = ((2, 1), (1, 2), (1, 1))   # -R of mate 1's and of mate 2's archive: a unit of two pieces, a chunk of mate 2 decoded twice, the same cuts
MERGE_KEYS = dict(pairs_merged=MR.PAIRS_MERGED, bases_merged=MR.BASES_MERGED, bytes_merged=MR.BYTES_OUT, overlap_bases=MR.OVERLAP_BASES,
                  places_disagree=MR.PLACES_DISAGREE, places_n=MR.PLACES_N, pairs_too_short=MR.PAIRS_TOO_SHORT)
PAIR_KEYS = PF.PAIR_KEYS + ("merged",)

F = GF.F
tool = GF.tool


@pytest.fixture(scope="module")
def farm(F, tool, tmp_path_factory, golden_dir):
    """test_gpu_overlap_farm's recipe: the fixture's two files COPIES times over, each compressed with -R 1 and -R 2, and the
    overlap of the two files (once: the slow part of every answer)"""
    d = tmp_path_factory.mktemp("merge_farm")
    files = []
    for m in (1, 2):
        raw, _ = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_%d.fastq" % m))
        raw = np.tile(raw, COPIES)
        files.append((raw, FR.parse(raw)))
    for name, (raw, recs) in zip(("m1", "m2"), files):
        for R_mib in (1, 2):
            PF.compress(tool, d, "%s_r%d" % (name, R_mib), raw, R_mib)
    overlap = OR.overlap_records(*files[0], 0, *files[1], 0, len(files[0][1]), OR.spec())
    return dict(dir=d, files=files, overlap=overlap)


def run(tool, d, tmp_path, r1, r2, t, *options, any_exit=False):
    args = ("d", d / ("m1_r%d.fqc" % r1), tmp_path / "o1.fastq", "--mate", d / ("m2_r%d.fqc" % r2), tmp_path / "o2.fastq", "-t", t, *options)
    return TF.run_any(tool, *args) if any_exit else TF.run_tool(tool, *args)


def outputs(tmp_path):
    return tuple((tmp_path / name).read_bytes() for name in ("o1.fastq", "o2.fastq", "mg.fastq"))


def holds(rep, want, what):
    out1, out2, merged, rep1, rep2, counters, summary, creport, mreport = want
    assert rep["pairs"] == counters and tuple(rep["pairs"]) == PAIR_KEYS, what
    assert counters["pairs"] == counters["kept"] + counters["merged"] + counters["dropped_mate1_only"] + counters["dropped_mate2_only"] + counters["dropped_both"]
    assert rep["merge"] == {k: int(mreport[w]) for k, w in MERGE_KEYS.items()} and list(rep["merge"]) == list(MERGE_KEYS), what
    assert rep["records"] == counters["kept"] and rep["raw_bytes"] == out1.size and rep["raw_bytes2"] == out2.size, what


def test_the_merge_alone_and_behind_the_correction(tool, farm, tmp_path):
    d = farm["dir"]
    for correct in (False, True):
        want = MR.pair_records_merged(*farm["files"][0], *farm["files"][1], OR.spec(), MR.spec(), c=CR.spec() if correct else None, overlap=farm["overlap"])
        assert want[5] == dict(pairs=1000 * COPIES, kept=889 * COPIES, dropped_mate1_only=0, dropped_mate2_only=0, dropped_both=0, merged=111 * COPIES)
        assert want[0].tobytes().count(b"\n") == 4 * 889 * COPIES == want[1].tobytes().count(b"\n") and want[2].tobytes().count(b"\n") == 4 * 111 * COPIES
        options = ["--merge", tmp_path / "mg.fastq"] + (["--overlap-correct"] if correct else [])
        for r1, r2 in COMBINATIONS:
            for t in (1, 3):
                rep = run(tool, d, tmp_path, r1, r2, t, *options)
                got = outputs(tmp_path)
                assert got == tuple(w.tobytes() for w in want[:3]), (correct, r1, r2, t, [len(g) for g in got])
                assert sorted(os.listdir(tmp_path)) == ["mg.fastq", "o1.fastq", "o2.fastq"]
                holds(rep, want, (correct, r1, r2, t))
                assert "mate1" not in rep and ("pairs_corrected" in rep["overlap"]) == correct
                assert (rep["blocks1"], rep["blocks2"], rep["decodes2"]) == (3 - r1, 3 - r2, 2), "no chunk is decoded more often than without"


def test_the_merge_with_a_filter_and_with_a_quality_trim(tool, farm, tmp_path):
    d = farm["dir"]
    summary = farm["overlap"][0]
    rows = [(int(r), int(summary[OR.HEAD + r])) for r in np.flatnonzero(summary[OR.HEAD:])]
    for what, options, selection, spec in (
        ("a filter", ["--min-mean-q", 20], dict(f=FR.flt(min_mean_q=20)), MR.spec()),
        ("a quality trim, the limits and the correction", ["--overlap-trim", "--overlap-correct", "--merge-min-len", 60, "--merge-floor-q", 0] + OF.OPTIONS,
         dict(OF.SELECTION, overlap_trim=True, c=CR.spec()), MR.spec(0, 60)),
    ):
        want = MR.pair_records_merged(*farm["files"][0], *farm["files"][1], OR.spec(), spec, overlap=farm["overlap"], **selection)
        counters, mreport = want[5], want[8]
        assert 0 < counters["merged"] < 111 * COPIES and counters["kept"] + counters["merged"] < 1000 * COPIES, what + ": a degenerate selection"
        text = HM.report_text((30, 5, 20), summary[:8].tolist(), rows, (30, 14) if "c" in selection else None, None if want[7] is None else want[7].tolist(),
                              (int(spec[0]), int(spec[1])), mreport.tolist())
        for (r1, r2), t in zip(COMBINATIONS, (1, 3, 2)):
            rep = run(tool, d, tmp_path, r1, r2, t, "--merge", tmp_path / "mg.fastq", "--overlap-report", tmp_path / "ov.tsv", *options)
            got = outputs(tmp_path)
            assert got == tuple(w.tobytes() for w in want[:3]), (what, r1, r2, t, [len(g) for g in got])
            assert (tmp_path / "ov.tsv").read_text() == text, (what, r1, r2, t)
            assert sorted(os.listdir(tmp_path)) == ["mg.fastq", "o1.fastq", "o2.fastq", "ov.tsv"]
            holds(rep, want, (what, r1, r2, t))
            # in "mate1" / "mate2" a merged pair shows under dropped_unmarked
            assert rep["mate1"]["dropped_unmarked"] == int(want[3][PR.DROPPED_UNMARKED]) >= counters["merged"]
            assert rep["mate2"]["dropped_unmarked"] == int(want[4][PR.DROPPED_UNMARKED]) >= counters["merged"]
            assert rep["mate1"]["kept"] == counters["kept"] == rep["mate2"]["kept"]
            os.remove(tmp_path / "ov.tsv")


def test_without_the_option_nothing_is_new(tool, farm, tmp_path):
    d = farm["dir"]
    want = OR.pair_records_trimmed(*farm["files"][0], *farm["files"][1], OR.spec(), **OF.SELECTION)
    rep = run(tool, d, tmp_path, 2, 1, 3, "--overlap-trim", "--overlap-report", tmp_path / "ov.tsv", *OF.OPTIONS)
    assert (tmp_path / "o1.fastq").read_bytes() == want[0].tobytes() and (tmp_path / "o2.fastq").read_bytes() == want[1].tobytes()
    assert sorted(os.listdir(tmp_path)) == ["o1.fastq", "o2.fastq", "ov.tsv"]
    assert "merge" not in rep and tuple(rep["pairs"]) == PF.PAIR_KEYS and rep["pairs"] == want[4]
    text = (tmp_path / "ov.tsv").read_text()
    assert not any(("\n" + name + "\t") in text for name in HM.MERGE_LINES) and text.rstrip("\n").rsplit("\n", 1)[1].startswith("insert\t")
    plain = run(tool, d, tmp_path, 1, 2, 2)
    (raw1, _), (raw2, _) = farm["files"]
    assert (tmp_path / "o1.fastq").read_bytes() == raw1.tobytes() and (tmp_path / "o2.fastq").read_bytes() == raw2.tobytes() and "merge" not in plain


def test_usage_errors_are_refused(tool, farm, tmp_path):
    d = farm["dir"]
    for options in (["--merge-min-len", 30], ["--merge-floor-q", 2], ["--merge", tmp_path / "mg.fastq", "--merge-min-len", 0],
                    ["--merge", tmp_path / "mg.fastq", "--merge-floor-q", 64], ["--merge", tmp_path / "mg.fastq", "--cut-front", 3],
                    ["--merge", tmp_path / "mg.fastq", "--cut-tail", 3], ["--merge", tmp_path / "mg.fastq", "--crop", 90]):
        r = run(tool, d, tmp_path, 1, 1, 2, *options, any_exit=True)
        assert r.returncode == 2 and r.stdout == "" and r.stderr, options
        assert os.listdir(tmp_path) == []
    r = TF.run_any(tool, "d", d / "m1_r1.fqc", tmp_path / "o1.fastq", "--merge", tmp_path / "mg.fastq")
    assert r.returncode == 2 and os.listdir(tmp_path) == [], "--merge without --mate"


def test_a_run_that_fails_leaves_none_of_the_three_outputs(tool, farm, tmp_path):
    d = farm["dir"]
    raw2, recs2 = farm["files"][1]
    starts = PR.header_starts(recs2)
    end = lambda r: int(recs2["qual_off"][r]) + int(recs2["len"][r]) + 1  # noqa: E731
    at = 2 * 1000 + 321   # two records of mate 2 swapped, in the third copy: the units in front of it have delivered their pieces
    swapped = np.concatenate((raw2[:starts[at]], raw2[starts[at + 1]:end(at + 1)], raw2[starts[at]:end(at)], raw2[end(at + 1):]))
    assert swapped.size == raw2.size and PR.first_mismatch(*farm["files"][0], 0, swapped, FR.parse(swapped), 0, len(recs2)) == at
    PF.compress(tool, tmp_path, "swapped", swapped)
    before = sorted(os.listdir(tmp_path))
    for t in (1, 3):
        r = TF.run_any(tool, "d", d / "m1_r1.fqc", tmp_path / "o1.fastq", "--mate", tmp_path / "swapped.fqc", tmp_path / "o2.fastq", "-t", t,
                       "--merge", tmp_path / "mg.fastq", "--overlap-report", tmp_path / "ov.tsv")
        assert r.returncode == 1 and r.stdout == "" and ("record %d:" % at) in r.stderr and "read ids" in r.stderr, r.stderr
        PF.nothing_left(tmp_path, before)
