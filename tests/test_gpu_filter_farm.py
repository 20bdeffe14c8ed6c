"""`fqc_tool d ... --max-n / --min-mean-q / ...`: the filtered restore of a whole archive through the farm (process.hpp:
processArchiveSelected), against the numpy restatement (filter_ref.py) of the input file, byte for byte."""
import json
import os
import shutil
import subprocess

import pytest

import filter_ref as R
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

JSON_WORDS = dict(records=R.N_RECORDS, kept=R.N_KEPT, bases_in=R.BASES_IN, bases_kept=R.BASES_KEPT, dropped_short=R.DROPPED_SHORT,
                  dropped_long=R.DROPPED_LONG, dropped_n=R.DROPPED_N, dropped_mean_q=R.DROPPED_MEAN_Q, dropped_low_q=R.DROPPED_LOW_Q)


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    if F.device_count() < 1:
        pytest.fail("no GPU visible: the product path has no CPU fallback")
    return F


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("filter_farm_tool") / "fqc_tool")
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


FILTER = dict(max_n=0, min_mean_q=33)
OPTIONS = ["--max-n", 0, "--min-mean-q", 33]


@pytest.fixture(scope="module")
def farm(F, tool, tmp_path_factory):
    """about 6 MiB of mode 4 compressed with -R 1 -t 3 --index --checksum, and what the reference keeps of the input"""
    d = tmp_path_factory.mktemp("filter_farm")
    raw, _ = F.synth_fastq(6 << 20, 4, seed=37)
    src = d / "in.fastq"
    raw.tofile(src)
    rep = run_tool(tool, "c", src, d / "a.fqc", "-t", 3, "-R", 1, "-S", 1, "--index", "--checksum")
    want = R.filter_chunk(raw, R.flt(**FILTER))
    assert rep["blocks"] >= 5 and 0.02 < int(want[1][R.N_KEPT]) / int(want[1][R.N_RECORDS]) < 0.98
    return dict(dir=d, raw=raw, rep=rep, want=want)


def report_matches(rep, want):
    assert {k: rep["filter"][k] for k in JSON_WORDS} == {k: int(want[1][w]) for k, w in JSON_WORDS.items()}
    assert rep["records"] == int(want[1][R.N_KEPT]) and rep["raw_bytes"] == int(want[1][R.BYTES_KEPT])


def test_the_filtered_restore_is_what_the_reference_keeps(tool, farm, tmp_path):
    d, want = farm["dir"], farm["want"]
    sizes = {p: os.path.getsize(str(d / "a.fqc") + p) for p in ("", ".fqx", ".fqs")}
    arc = tmp_path / "a.fqc"
    for ext in ("", ".fqx", ".fqs"):
        shutil.copy(str(d / "a.fqc") + ext, str(arc) + ext)
    before = {ext: open(str(arc) + ext, "rb").read() for ext in ("", ".fqx", ".fqs")}
    for with_index in (True, False):
        if not with_index:
            os.remove(str(arc) + ".fqx")
        for t in (3, 1, 16):   # (16: more workers than blocks)
            out = tmp_path / "out.fastq"
            listing = sorted(os.listdir(tmp_path))
            rep = run_tool(tool, "d", arc, out, "-t", t, *OPTIONS)
            assert out.read_bytes() == want[0].tobytes(), (with_index, t)
            assert sorted(os.listdir(tmp_path)) == sorted(listing + ["out.fastq"]), "the output and nothing else"
            assert rep["index"] == ("used" if with_index else "none") and rep["sums"] == "used" and rep["verified"] == farm["rep"]["blocks"]
            report_matches(rep, want)
            os.remove(out)
    for ext in ("", ".fqs"):
        assert open(str(arc) + ext, "rb").read() == before[ext], "the archive and its files are not touched"
    os.remove(str(arc) + ".fqs")
    rep = run_tool(tool, "d", arc, tmp_path / "plain.fastq", "-t", 3, *OPTIONS)
    assert (tmp_path / "plain.fastq").read_bytes() == want[0].tobytes() and rep["sums"] == "none" and rep["verified"] == 0
    assert sizes[""] == os.path.getsize(d / "a.fqc")


def test_every_criterion_through_the_tool(tool, farm, tmp_path):
    d, raw = farm["dir"], farm["raw"]
    for options, kw in ((["--min-len", 100, "--max-len", 200], dict(min_len=100, max_len=200)),
                        (["--max-low-q", "30:20"], dict(low_q=30, max_low_pct=20)),
                        (["--min-len", 80, "--max-n", 1, "--min-mean-q", 34, "--max-low-q", "30:20"],
                         dict(min_len=80, max_n=1, min_mean_q=34, low_q=30, max_low_pct=20))):
        want = R.filter_chunk(raw, R.flt(**kw))
        assert 0 < int(want[1][R.N_KEPT]) < int(want[1][R.N_RECORDS]), kw
        rep = run_tool(tool, "d", d / "a.fqc", tmp_path / "o.fastq", "-t", 3, *options)
        assert (tmp_path / "o.fastq").read_bytes() == want[0].tobytes(), kw
        report_matches(rep, want)


def test_a_filter_that_keeps_nothing_and_one_that_keeps_everything(tool, farm, tmp_path):
    d, raw = farm["dir"], farm["raw"]
    rep = run_tool(tool, "d", d / "a.fqc", tmp_path / "none.fastq", "-t", 3, "--min-mean-q", 63)
    assert os.path.getsize(tmp_path / "none.fastq") == 0 and not os.path.exists(str(tmp_path / "none.fastq") + ".part")
    assert rep["filter"]["kept"] == 0 and rep["filter"]["dropped_mean_q"] == rep["filter"]["records"] > 0 and rep["raw_bytes"] == 0
    plain = run_tool(tool, "d", d / "a.fqc", tmp_path / "plain.fastq", "-t", 3)
    assert "filter" not in plain and (tmp_path / "plain.fastq").read_bytes() == raw.tobytes()
    rep = run_tool(tool, "d", d / "a.fqc", tmp_path / "all.fastq", "-t", 3, "--min-len", 1)
    assert (tmp_path / "all.fastq").read_bytes() == (tmp_path / "plain.fastq").read_bytes()
    assert rep["filter"]["kept"] == rep["filter"]["records"] == plain["records"] and rep["raw_bytes"] == raw.size


def test_a_damaged_archive_leaves_no_output(F, tool, farm, tmp_path):
    """One byte of the archive flipped, well behind the 64 KiB the sums file knows the archive by and far from the index at its
    end: inside some block's streams.  Either the decoder refuses the stream or the chunk's digest does not hold."""
    d = farm["dir"]
    good = open(d / "a.fqc", "rb").read()
    bad, out = tmp_path / "bad.fqc", tmp_path / "bad.fastq"
    for ext in (".fqx", ".fqs"):
        shutil.copy(str(d / "a.fqc") + ext, str(bad) + ext)
    said = set()
    for at in (len(good) // 2, len(good) // 3, len(good) // 2 + 12345):
        assert at > (64 << 10)
        data = bytearray(good)
        data[at] ^= 0x10
        open(bad, "wb").write(data)
        for t in (3, 1):
            r = run_any(tool, "d", bad, out, "-t", t, *OPTIONS)
            assert r.returncode == 1 and r.stdout == "" and r.stderr, (at, t, r.stdout)
            assert not os.path.exists(out) and not os.path.exists(str(out) + ".part"), (at, t)
            said.add("checksum" if "checksum of chunk" in r.stderr else "decode")
    assert said <= {"checksum", "decode"}
    # the same archive, whole: the command works
    open(bad, "wb").write(good)
    assert run_tool(tool, "d", bad, out, "-t", 3, *OPTIONS)["sums"] == "used"
    assert open(out, "rb").read() == farm["want"][0].tobytes()


def test_an_archive_of_the_independent_writer(F, tool, tmp_path, golden_dir):
    import test_archive as TA
    raw, recs = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_1.fastq"))
    arc = tmp_path / "o.fqc"
    TA.oracle_archive(F, str(arc), raw, recs, 3, order=[2, 0, 1])
    want = R.filter_chunk(raw, R.flt(max_n=0, min_mean_q=18))
    assert 0 < int(want[1][R.N_KEPT]) < len(recs)
    rep = run_tool(tool, "d", arc, tmp_path / "o.fastq", "-t", 2, "--max-n", 0, "--min-mean-q", 18)
    assert (tmp_path / "o.fastq").read_bytes() == want[0].tobytes()
    assert rep["sums"] == "none" and rep["index"] == "none"
    report_matches(rep, want)
