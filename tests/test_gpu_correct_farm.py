"""`fqc_tool d <in1.fqc> <out1.fastq> --mate <in2.fqc> <out2.fastq> --overlap-correct`: the overlap correction through the farm
(process.hpp: processArchivePaired with Selection::correct) against the restatement in correct_ref.py -- both outputs, the
JSON line and the report's text, byte for byte, whatever -t -- on test_gpu_overlap_farm's archives, whose mate 2 is written at
another -R so that a unit has several pieces of mate 2 and a chunk of mate 2 is patched by two units; and without the option,
which leaves every key and every line what it was."""
import os

import numpy as np
import pytest

import correct_ref as CR
import filter_ref as FR
import overlap_ref as OR
import oracle_lib as O
import test_correct_host as HC
import test_gpu_overlap_farm as OF
import test_gpu_pair_farm as PF
import test_gpu_tail_farm as GF
import test_gpu_trim_farm as TF

pytestmark = pytest.mark.gpu

COPIES = OF.COPIES
OPTIONS = ["--overlap-trim"] + OF.OPTIONS
CORRECT_KEYS = dict(pairs_corrected=CR.PAIRS_CORRECTED, bases_corrected_1=CR.FIXED_A, bases_corrected_2=CR.FIXED_B, n_resolved=CR.N_RESOLVED)
COMBINATIONS = ((2, 1), (1, 2), (1, 1))

F = GF.F
tool = GF.tool


@pytest.fixture(scope="module")
def farm(F, tool, tmp_path_factory, golden_dir):
    """test_gpu_overlap_farm's recipe: the fixture's two files COPIES times over, each compressed with -R 1 and -R 2; the
    reference's answers with the correction alone and with the limits, a trim and a filter behind it"""
    d = tmp_path_factory.mktemp("correct_farm")
    files = []
    for m in (1, 2):
        raw, _ = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_%d.fastq" % m))
        raw = np.tile(raw, COPIES)
        files.append((raw, FR.parse(raw)))
    for name, (raw, recs) in zip(("m1", "m2"), files):
        for R_mib in (1, 2):
            PF.compress(tool, d, "%s_r%d" % (name, R_mib), raw, R_mib)
    overlap = OR.overlap_records(*files[0], 0, *files[1], 0, len(files[0][1]), OR.spec())   # (once: the slow part of every answer)
    alone = CR.pair_records_corrected(*files[0], *files[1], OR.spec(), CR.spec(), overlap=overlap)
    full = CR.pair_records_corrected(*files[0], *files[1], OR.spec(), CR.spec(), overlap_trim=True, overlap=overlap, **OF.SELECTION)
    # levels that no quality of the fixture meets: the restore without a correction
    none = CR.pair_records_corrected(*files[0], *files[1], OR.spec(), CR.spec(63, 0), overlap_trim=True, overlap=overlap, **OF.SELECTION)
    assert not none[6][2:6].any()
    return dict(dir=d, files=files, alone=alone, full=full, none=none, overlap=overlap)


def run(tool, d, tmp_path, r1, r2, t, *options):
    return TF.run_tool(tool, "d", d / ("m1_r%d.fqc" % r1), tmp_path / "o1.fastq", "--mate", d / ("m2_r%d.fqc" % r2), tmp_path / "o2.fastq", "-t", t, *options)


def test_the_correction_alone(tool, farm, tmp_path):
    d = farm["dir"]
    out1, out2, _, _, counters, summary, creport = farm["alone"]
    assert creport[:5].tolist() == [1000 * COPIES, 111 * COPIES, 36 * COPIES, 34 * COPIES, 28 * COPIES]
    (raw1, _), (raw2, _) = farm["files"]
    assert out1.size == raw1.size and out2.size == raw2.size, "every pair is kept whole"
    assert int((out1 != raw1).sum()) + int((out2 != raw2).sum()) == 2 * (34 + 28) * COPIES, "one base byte and one quality byte per correction"
    for r1, r2 in COMBINATIONS:
        for t in (1, 4):
            rep = run(tool, d, tmp_path, r1, r2, t, "--overlap-correct")
            assert (tmp_path / "o1.fastq").read_bytes() == out1.tobytes() and (tmp_path / "o2.fastq").read_bytes() == out2.tobytes(), (r1, r2, t)
            assert sorted(os.listdir(tmp_path)) == ["o1.fastq", "o2.fastq"]
            assert rep["pairs"] == counters and counters["kept"] == 1000 * COPIES and "mate1" not in rep
            want = dict({k: int(summary[w]) for k, w in OF.OVERLAP_KEYS.items()}, **{k: int(creport[w]) for k, w in CORRECT_KEYS.items()})
            assert rep["overlap"] == want and list(rep["overlap"]) == list(OF.OVERLAP_KEYS) + list(CORRECT_KEYS)
            assert (rep["blocks1"], rep["blocks2"], rep["decodes2"]) == (3 - r1, 3 - r2, 2)
    # other levels reach the device, and a pair of levels nothing meets corrects nothing
    rep = run(tool, d, tmp_path, 2, 1, 2, "--overlap-correct", "--correct-q", "63:0")
    assert rep["overlap"]["pairs_corrected"] == 0 and (tmp_path / "o1.fastq").read_bytes() == raw1.tobytes() and (tmp_path / "o2.fastq").read_bytes() == raw2.tobytes()
    other = CR.pair_records_corrected(*farm["files"][0], *farm["files"][1], OR.spec(), CR.spec(25, 10), overlap=farm["overlap"])
    rep = run(tool, d, tmp_path, 1, 2, 3, "--overlap-correct", "--correct-q", "25:10", "--overlap-min", 30, "--overlap-mism", 5, "--overlap-err", 20)
    assert (tmp_path / "o1.fastq").read_bytes() == other[0].tobytes() and (tmp_path / "o2.fastq").read_bytes() == other[1].tobytes()
    assert {k: rep["overlap"][k] for k in CORRECT_KEYS} == {k: int(other[6][w]) for k, w in CORRECT_KEYS.items()} and other[6].tolist() != creport.tolist()


def test_the_correction_in_front_of_the_limits_a_trim_and_a_filter(tool, farm, tmp_path):
    d = farm["dir"]
    out1, out2, rep1, rep2, counters, summary, creport = farm["full"]
    uncorrected = farm["none"]
    assert out1.tobytes() != uncorrected[0].tobytes() and out2.tobytes() != uncorrected[1].tobytes(), "the correction shows behind the trim"
    rows = [(int(r), int(summary[OR.HEAD + r])) for r in np.flatnonzero(summary[OR.HEAD:])]
    text = HC.report_text((30, 5, 20), summary[:8].tolist(), rows, (30, 14), creport.tolist())
    assert text.count("\n") == OF.HO.report_text((30, 5, 20), summary[:8].tolist(), rows).count("\n") + 6
    base = run(tool, d, tmp_path, 2, 1, 2, *OPTIONS)
    for r1, r2 in COMBINATIONS:
        for t in (1, 4):
            rep = run(tool, d, tmp_path, r1, r2, t, "--overlap-correct", "--overlap-report", tmp_path / "ov.tsv", *OPTIONS)
            assert (tmp_path / "o1.fastq").read_bytes() == out1.tobytes() and (tmp_path / "o2.fastq").read_bytes() == out2.tobytes(), (r1, r2, t)
            assert (tmp_path / "ov.tsv").read_text() == text, (r1, r2, t)
            assert sorted(os.listdir(tmp_path)) == ["o1.fastq", "o2.fastq", "ov.tsv"]
            assert rep["pairs"] == counters
            want = dict({k: int(summary[w]) for k, w in OF.OVERLAP_KEYS.items()}, **{k: int(creport[w]) for k, w in CORRECT_KEYS.items()})
            assert rep["overlap"] == want and list(rep["overlap"])[-4:] == list(CORRECT_KEYS)
            assert rep["mate1"] == {k: int(rep1[w]) for k, w in OF.LIMIT_WORDS.items()} and rep["mate2"] == {k: int(rep2[w]) for k, w in OF.LIMIT_WORDS.items()}
            assert list(rep) == list(base), "the line's keys and their order are what they are without the option"
            assert (rep["blocks1"], rep["blocks2"], rep["decodes2"]) == (3 - r1, 3 - r2, 2), "what they are without the option"
            os.remove(tmp_path / "ov.tsv")


def test_without_the_option_nothing_is_new(tool, farm, tmp_path):
    d = farm["dir"]
    rep = run(tool, d, tmp_path, 2, 1, 3, "--overlap-report", tmp_path / "ov.tsv", *OPTIONS)
    assert list(rep["overlap"]) == list(OF.OVERLAP_KEYS)
    text = (tmp_path / "ov.tsv").read_text()
    assert not any(name in text for name in HC.CORRECT_LINES) and text.rstrip("\n").rsplit("\n", 1)[1].startswith("insert\t")
    want = farm["none"]
    assert (tmp_path / "o1.fastq").read_bytes() == want[0].tobytes() and (tmp_path / "o2.fastq").read_bytes() == want[1].tobytes()
