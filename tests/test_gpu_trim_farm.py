"""`fqc_tool d ... --cut-front / --cut-tail / --trim-q5 / --trim-q3 / --crop`: the trimmed restore of a whole archive through
the farm (process.hpp: processArchiveSelected), against the numpy restatement (trim_ref.py) of the input file, byte for byte."""
import json
import os
import shutil
import subprocess

import pytest

import filter_ref as FR
import oracle_lib as O
import trim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

TRIM_WORDS = dict(records=R.N_RECORDS, kept=R.N_KEPT, bases_in=R.BASES_IN, bases_kept=R.BASES_KEPT, bytes_kept=R.BYTES_KEPT,
                  dropped_short=R.DROPPED_SHORT, dropped_long=R.DROPPED_LONG, dropped_n=R.DROPPED_N, dropped_mean_q=R.DROPPED_MEAN_Q,
                  dropped_low_q=R.DROPPED_LOW_Q, reads_trimmed=R.READS_TRIMMED, bases_cut_front=R.BASES_CUT_FRONT,
                  bases_cut_tail=R.BASES_CUT_TAIL, reads_emptied=R.READS_EMPTIED)
FILTER_WORDS = {k: w for k, w in TRIM_WORDS.items() if w <= R.DROPPED_LOW_Q and k != "bytes_kept"}


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    if F.device_count() < 1:
        pytest.fail("no GPU visible: the product path has no CPU fallback")
    return F


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("trim_farm_tool") / "fqc_tool")
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


TRIM = dict(cut_front=3, q_front=30, q_tail=34, crop=100)
TRIM_OPTIONS = ["--cut-front", 3, "--trim-q5", 30, "--trim-q3", 34, "--crop", 100]
FILTER = dict(max_n=0, min_len=30)
FILTER_OPTIONS = ["--max-n", 0, "--min-len", 30]


@pytest.fixture(scope="module")
def farm(F, tool, tmp_path_factory):
    """about 6 MiB of mode 4 compressed with -R 1 -t 3 --index --checksum, and what the reference makes of the input"""
    d = tmp_path_factory.mktemp("trim_farm")
    raw, _ = F.synth_fastq(6 << 20, 4, seed=37)
    src = d / "in.fastq"
    raw.tofile(src)
    rep = run_tool(tool, "c", src, d / "a.fqc", "-t", 3, "-R", 1, "-S", 1, "--index", "--checksum")
    trimmed = R.trim_chunk(raw, R.trm(**TRIM))
    both = R.trim_chunk(raw, R.trm(**TRIM), FR.flt(**FILTER))
    n = int(both[1][R.N_RECORDS])
    assert rep["blocks"] >= 5 and 0.5 * n < int(trimmed[1][R.READS_TRIMMED]) and 0 < int(trimmed[1][R.READS_EMPTIED]) < 0.1 * n
    assert 0.02 * n < int(both[1][R.N_KEPT]) < 0.98 * n and int(both[1][R.DROPPED_N]) > 0 and int(both[1][R.DROPPED_SHORT]) > int(both[1][R.READS_EMPTIED])
    return dict(dir=d, raw=raw, rep=rep, trimmed=trimmed, both=both)


def report_matches(rep, want, filtered):
    assert rep["trim"] == {k: int(want[1][w]) for k, w in TRIM_WORDS.items()}
    assert rep["records"] == int(want[1][R.N_KEPT]) and rep["raw_bytes"] == int(want[1][R.BYTES_KEPT])
    if filtered:
        assert rep["filter"] == {k: int(want[1][w]) for k, w in FILTER_WORDS.items()}, "printed as for a filtered restore"
    else:
        assert "filter" not in rep


def test_the_trimmed_restore_is_what_the_reference_makes(tool, farm, tmp_path):
    d = farm["dir"]
    arc = tmp_path / "a.fqc"
    for ext in ("", ".fqx", ".fqs"):
        shutil.copy(str(d / "a.fqc") + ext, str(arc) + ext)
    before = {ext: open(str(arc) + ext, "rb").read() for ext in ("", ".fqx", ".fqs")}
    for with_index in (True, False):
        if not with_index:
            os.remove(str(arc) + ".fqx")
        for t in (4, 1):
            for options, want, filtered in ((TRIM_OPTIONS, farm["trimmed"], False), (TRIM_OPTIONS + FILTER_OPTIONS, farm["both"], True)):
                out = tmp_path / "out.fastq"
                listing = sorted(os.listdir(tmp_path))
                rep = run_tool(tool, "d", arc, out, "-t", t, *options)
                assert out.read_bytes() == want[0].tobytes(), (with_index, t, filtered)
                assert sorted(os.listdir(tmp_path)) == sorted(listing + ["out.fastq"]), "the output and nothing else"
                assert rep["index"] == ("used" if with_index else "none") and rep["sums"] == "used" and rep["verified"] == farm["rep"]["blocks"]
                report_matches(rep, want, filtered)
                os.remove(out)
    for ext in ("", ".fqs"):
        assert open(str(arc) + ext, "rb").read() == before[ext], "the archive and its files are not touched"
    os.remove(str(arc) + ".fqs")
    rep = run_tool(tool, "d", arc, tmp_path / "plain.fastq", "-t", 4, *TRIM_OPTIONS)
    assert (tmp_path / "plain.fastq").read_bytes() == farm["trimmed"][0].tobytes() and rep["sums"] == "none" and rep["verified"] == 0


def test_every_option_through_the_tool(tool, farm, tmp_path):
    d, raw = farm["dir"], farm["raw"]
    for options, t, f in ((["--cut-tail", 20], dict(cut_tail=20), None),
                          (["--crop", 75, "--min-mean-q", 30], dict(crop=75), dict(min_mean_q=30)),
                          (["--trim-q3", 30, "--trim-q5", 30], dict(q_front=30, q_tail=30), None),
                          (["--cut-front", 10, "--cut-tail", 10, "--trim-q3", 35, "--max-low-q", "30:20", "--max-len", 150],
                           dict(cut_front=10, cut_tail=10, q_tail=35), dict(low_q=30, max_low_pct=20, max_len=150))):
        want = R.trim_chunk(raw, R.trm(**t), None if f is None else FR.flt(**f))
        assert 0 < int(want[1][R.READS_TRIMMED]) and 0 < int(want[1][R.N_KEPT]), (t, f)
        rep = run_tool(tool, "d", d / "a.fqc", tmp_path / "o.fastq", "-t", 3, *options)
        assert (tmp_path / "o.fastq").read_bytes() == want[0].tobytes(), (t, f)
        report_matches(rep, want, f is not None)


def test_a_trim_that_empties_everything_and_one_that_cuts_nothing(tool, farm, tmp_path):
    d, raw = farm["dir"], farm["raw"]
    rep = run_tool(tool, "d", d / "a.fqc", tmp_path / "none.fastq", "-t", 3, "--cut-front", 65535)
    assert os.path.getsize(tmp_path / "none.fastq") == 0 and not os.path.exists(str(tmp_path / "none.fastq") + ".part")
    assert rep["trim"]["kept"] == 0 and rep["trim"]["reads_emptied"] == rep["trim"]["dropped_short"] == rep["trim"]["records"] > 0
    assert rep["trim"]["bases_cut_tail"] == rep["trim"]["bases_in"] and rep["raw_bytes"] == 0
    rep = run_tool(tool, "d", d / "a.fqc", tmp_path / "all.fastq", "-t", 3, "--crop", 65535)
    assert (tmp_path / "all.fastq").read_bytes() == raw.tobytes()
    assert rep["trim"]["kept"] == rep["trim"]["records"] and rep["trim"]["reads_trimmed"] == 0 and rep["raw_bytes"] == raw.size
    plain = run_tool(tool, "d", d / "a.fqc", tmp_path / "plain.fastq", "-t", 3)
    assert "trim" not in plain and "filter" not in plain and (tmp_path / "plain.fastq").read_bytes() == raw.tobytes()


def test_a_damaged_archive_leaves_no_output(F, tool, farm, tmp_path):
    """One byte of the archive flipped inside some block's streams: either the decoder refuses the stream or the chunk's
    digest does not hold."""
    d = farm["dir"]
    good = open(d / "a.fqc", "rb").read()
    bad, out = tmp_path / "bad.fqc", tmp_path / "bad.fastq"
    for ext in (".fqx", ".fqs"):
        shutil.copy(str(d / "a.fqc") + ext, str(bad) + ext)
    for at in (len(good) // 2, len(good) // 3):
        assert at > (64 << 10)
        data = bytearray(good)
        data[at] ^= 0x10
        open(bad, "wb").write(data)
        for t in (3, 1):
            r = run_any(tool, "d", bad, out, "-t", t, *TRIM_OPTIONS)
            assert r.returncode == 1 and r.stdout == "" and r.stderr, (at, t, r.stdout)
            assert not os.path.exists(out) and not os.path.exists(str(out) + ".part"), (at, t)
    # the same archive, whole: the command works
    open(bad, "wb").write(good)
    assert run_tool(tool, "d", bad, out, "-t", 3, *TRIM_OPTIONS)["sums"] == "used"
    assert open(out, "rb").read() == farm["trimmed"][0].tobytes()


def test_an_archive_of_the_independent_writer(F, tool, tmp_path, golden_dir):
    import test_archive as TA
    raw, recs = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_1.fastq"))
    arc = tmp_path / "o.fqc"
    TA.oracle_archive(F, str(arc), raw, recs, 3, order=[2, 0, 1])
    want = R.trim_chunk(raw, R.trm(q_front=20, q_tail=20), FR.flt(max_n=0, min_len=20))
    assert 0 < int(want[1][R.N_KEPT]) < len(recs) and int(want[1][R.READS_TRIMMED]) > 0
    rep = run_tool(tool, "d", arc, tmp_path / "o.fastq", "-t", 2, "--trim-q5", 20, "--trim-q3", 20, "--max-n", 0, "--min-len", 20)
    assert (tmp_path / "o.fastq").read_bytes() == want[0].tobytes()
    assert rep["sums"] == "none" and rep["index"] == "none"
    report_matches(rep, want, True)
