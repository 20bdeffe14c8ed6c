"""`fqc_tool d <in1.fqc> <out1.fastq> --mate <in2.fqc> <out2.fastq> --overlap-trim --overlap-report <file.tsv>`: the mate overlap
through the farm (process.hpp: processArchivePaired with an overlap spec) against the restatement in overlap_ref.py -- both
outputs, the JSON line and the report's text, byte for byte, whatever -t -- on archives of the fixture's pairs whose mate 2 is
written at another -R, so that a unit has several pieces of mate 2; and the report alone, which leaves both outputs what
plain `d --mate` makes them."""
import os

import numpy as np
import pytest

import filter_ref as FR
import overlap_ref as OR
import oracle_lib as O
import pair_ref as PR
import test_gpu_pair_farm as PF
import test_gpu_tail_farm as GF
import test_gpu_trim_farm as TF
import test_overlap_host as HO
import trim_ref as R

pytestmark = pytest.mark.gpu

COPIES = 4     # of the fixture's 1 000 pairs: a little over 1 MiB a file
OPTIONS = ["--trim-q3", 20, "--min-len", 40]
SELECTION = dict(t=R.trm(q_tail=20), f=FR.flt(min_len=40))
OVERLAP_KEYS = dict(pairs_overlapped=OR.OVERLAPPED, pairs_read_through=OR.READ_THROUGH, bases_behind_1=OR.BEHIND_A, bases_behind_2=OR.BEHIND_B,
                    pairs_not_analysed=OR.NOT_ANALYSED)
LIMIT_WORDS = dict(PF.MATE_WORDS, reads_cut_limit=OR.READS_CUT_LIMIT, bases_cut_limit=OR.BASES_CUT_LIMIT)

F = GF.F
tool = GF.tool


@pytest.fixture(scope="module")
def farm(F, tool, tmp_path_factory, golden_dir):
    """the fixture's two files COPIES times over; mate 1 compressed with -R 1 and with -R 2, mate 2 the same: the pairs
    (m1 at -R 2, m2 at -R 1) and (m1 at -R 1, m2 at -R 2) give a unit two pieces / a chunk of mate 2 two decodes"""
    d = tmp_path_factory.mktemp("overlap_farm")
    files = []
    for m in (1, 2):
        raw, _ = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_%d.fastq" % m))
        raw = np.tile(raw, COPIES)
        files.append((raw, FR.parse(raw)))
    reps = {}
    for name, (raw, recs) in zip(("m1", "m2"), files):
        for R_mib in (1, 2):
            reps[name, R_mib] = PF.compress(tool, d, "%s_r%d" % (name, R_mib), raw, R_mib)
    assert reps["m1", 1]["blocks"] == reps["m2", 1]["blocks"] == 2 and reps["m1", 2]["blocks"] == reps["m2", 2]["blocks"] == 1
    want = OR.pair_records_trimmed(*files[0], *files[1], OR.spec(), **SELECTION)
    plain = PR.pair_records(*files[0], *files[1], **SELECTION)
    return dict(dir=d, files=files, want=want, plain=plain)


def test_overlap_trim_with_several_pieces_a_unit(tool, farm, tmp_path):
    d = farm["dir"]
    out1, out2, rep1, rep2, counters, summary = farm["want"]
    assert int(summary[OR.OVERLAPPED]) == 111 * COPIES and int(summary[OR.READ_THROUGH]) == 36 * COPIES
    assert out1.size < farm["plain"][0].size and out2.size < farm["plain"][1].size, "the limits cut something"
    rows = [(int(r), int(summary[OR.HEAD + r])) for r in np.flatnonzero(summary[OR.HEAD:])]
    text = HO.report_text((30, 5, 20), summary[:8].tolist(), rows)
    seen = set()
    for r1, r2, decodes2 in ((2, 1, 2), (1, 2, 2), (1, 1, 2)):
        for t in (1, 4):
            rep = TF.run_tool(tool, "d", d / ("m1_r%d.fqc" % r1), tmp_path / "o1.fastq", "--mate", d / ("m2_r%d.fqc" % r2), tmp_path / "o2.fastq", "-t", t,
                              "--overlap-trim", "--overlap-report", tmp_path / "ov.tsv", *OPTIONS)
            assert (tmp_path / "o1.fastq").read_bytes() == out1.tobytes() and (tmp_path / "o2.fastq").read_bytes() == out2.tobytes(), (r1, r2, t)
            assert (tmp_path / "ov.tsv").read_text() == text, (r1, r2, t)
            assert sorted(os.listdir(tmp_path)) == ["o1.fastq", "o2.fastq", "ov.tsv"]
            assert rep["pairs"] == counters and rep["overlap"] == {k: int(summary[w]) for k, w in OVERLAP_KEYS.items()}
            assert rep["mate1"] == {k: int(rep1[w]) for k, w in LIMIT_WORDS.items()} and rep["mate2"] == {k: int(rep2[w]) for k, w in LIMIT_WORDS.items()}
            assert list(rep["mate1"])[-2:] == ["reads_cut_limit", "bases_cut_limit"] and rep["mate1"]["reads_cut_limit"] > 0
            assert (rep["blocks1"], rep["blocks2"], rep["decodes2"]) == (3 - r1, 3 - r2, decodes2), "no chunk is decoded more often than without"
            seen.add((rep["blocks1"], rep["blocks2"]))
            for name in ("o1.fastq", "o2.fastq", "ov.tsv"):
                os.remove(tmp_path / name)
    assert seen == {(1, 2), (2, 1), (2, 2)}
    # other limits of the overlap reach the device: nothing overlaps over 101 bases of reads of 100
    rep = TF.run_tool(tool, "d", d / "m1_r2.fqc", tmp_path / "o1.fastq", "--mate", d / "m2_r1.fqc", tmp_path / "o2.fastq", "--overlap-trim",
                      "--overlap-min", 101, *OPTIONS)
    assert rep["overlap"]["pairs_overlapped"] == 0 and (tmp_path / "o1.fastq").read_bytes() == farm["plain"][0].tobytes()
    assert rep["mate1"]["reads_cut_limit"] == 0 == rep["mate2"]["bases_cut_limit"]


def test_the_report_alone_leaves_both_outputs_as_they_are(tool, farm, tmp_path):
    d = farm["dir"]
    summary = farm["want"][5]
    for options, plain in ((OPTIONS, farm["plain"]), ([], None)):
        base = TF.run_tool(tool, "d", d / "m1_r2.fqc", tmp_path / "p1.fastq", "--mate", d / "m2_r1.fqc", tmp_path / "p2.fastq", "-t", 3, *options)
        rep = TF.run_tool(tool, "d", d / "m1_r2.fqc", tmp_path / "o1.fastq", "--mate", d / "m2_r1.fqc", tmp_path / "o2.fastq", "-t", 3,
                          "--overlap-report", tmp_path / "ov.tsv", "--overlap-err", 20, *options)
        assert (tmp_path / "o1.fastq").read_bytes() == (tmp_path / "p1.fastq").read_bytes() and (tmp_path / "o2.fastq").read_bytes() == (tmp_path / "p2.fastq").read_bytes()
        if plain is not None:
            assert (tmp_path / "o1.fastq").read_bytes() == plain[0].tobytes() and (tmp_path / "o2.fastq").read_bytes() == plain[1].tobytes()
        else:
            assert (tmp_path / "o1.fastq").read_bytes() == farm["files"][0][0].tobytes() and "mate1" not in rep
        assert "overlap" not in base and rep["overlap"] == {k: int(summary[w]) for k, w in OVERLAP_KEYS.items()}
        assert {k: v for k, v in rep.items() if k not in ("overlap", "seconds", "blocks_per_worker")} == \
               {k: v for k, v in base.items() if k not in ("seconds", "blocks_per_worker")}, "every other key is what it was"
        assert all("reads_cut_limit" not in rep.get(m, {}) for m in ("mate1", "mate2"))
        assert (tmp_path / "ov.tsv").read_text().startswith("#fqgpu-overlap 1\nmin_overlap\t30\n") and "pairs_overlapped\t%d\n" % (111 * COPIES) in (tmp_path / "ov.tsv").read_text()
