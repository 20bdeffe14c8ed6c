"""`fqc_tool d <in1.fqc> <out1.fastq> --mate <in2.fqc> <out2.fastq>`: two archives of mates restored in step through the farm
(process.hpp: processArchivePaired) against the numpy restatement (pair_ref.py) of the two input files, byte for byte: archives
whose chunks hold different records because the mates' reads have different lengths, archives cut at the same records,
archives written with different block sizes; no selection option; and the runs that must fail and leave nothing behind."""
import os
import shutil

import numpy as np
import pytest

import adapter_ref as AR
import filter_ref as FR
import pair_ref as PR
import tail_ref as TR
import test_gpu_tail_farm as GF
import test_gpu_trim_farm as TF
import trim_ref as R

pytestmark = pytest.mark.gpu

ADAPTER1 = GF.ADAPTER
ADAPTER2 = b"AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"     # TruSeq, read 2
OPTIONS = ["--adapter", ADAPTER1.decode(), "--adapter2", ADAPTER2.decode(), "--poly-g", "--window", "4:20", "--trim-q3", 20, "--min-len", 30]
SELECTION = dict(a1=AR.adp(ADAPTER1), a2=AR.adp(ADAPTER2), x=TR.tl("G", window_len=4, window_q=20), t=R.trm(q_tail=20), f=FR.flt(min_len=30))
MATE_WORDS = dict(GF.AF.CLIP_WORDS, **GF.TAIL_KEYS, dropped_unmarked=PR.DROPPED_UNMARKED)
PAIR_KEYS = ("pairs", "kept", "dropped_mate1_only", "dropped_mate2_only", "dropped_both")

F = GF.F
tool = GF.tool


def mate_of(raw, recs, crop):
    """mate 2 of a file: the same header lines, every read reversed -- bases and qualities -- and cropped to `crop` bases, and
    its own adapter over the 3' end of a third of the reads from a drawn place on -> (raw, recs)"""
    rng = np.random.default_rng(91)
    a = np.frombuffer(ADAPTER2, dtype=np.uint8)
    parts = []
    for line, r in zip(PR.header_lines(raw, recs), recs):
        so, qo, L = int(r["seq_off"]), int(r["qual_off"]), int(r["len"])
        seq, qual = raw[so:so + L][::-1][:crop].copy(), raw[qo:qo + L][::-1][:crop]
        if rng.random() < 0.33:
            at = int(rng.integers(20, len(seq)))
            k = min(len(a), len(seq) - at)
            seq[at:at + k] = a[:k]
        parts += [line, seq.tobytes(), b"\n+\n", qual.tobytes(), b"\n"]
    out = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    return out, FR.parse(out)


def compress(tool, d, name, raw, R_mib=1):
    raw.tofile(d / (name + ".fastq"))
    return TF.run_tool(tool, "c", d / (name + ".fastq"), d / (name + ".fqc"), "-t", 3, "-R", R_mib, "-S", 1, "--index", "--checksum")


def record_counts(rep_line, raw, recs, R_mib):
    """the records per chunk of an archive written with -R R_mib: a chunk takes the whole records of its block of the input"""
    ends = recs["qual_off"].astype(np.int64) + recs["len"].astype(np.int64) + 1
    counts, at, done = [], 0, 0
    while done < len(recs):
        k = int(np.searchsorted(ends, at + (R_mib << 20), side="right"))
        counts.append(k - done)
        at, done = int(ends[k - 1]), k
    assert len(counts) == rep_line["blocks"]
    return counts


@pytest.fixture(scope="module")
def farm(F, tool, tmp_path_factory, golden_dir):
    """the planted file of the tail farm as mate 1; mate 2 cropped to 91 bases (its chunks hold other records than mate 1's) and
    mate 2 uncropped (the same records); all compressed with -R 1, the uncropped one with -R 2 as well"""
    d = tmp_path_factory.mktemp("pair_farm")
    raw1, recs1 = GF.planted_file(golden_dir)
    short = mate_of(raw1, recs1, 91)
    full = mate_of(raw1, recs1, 1 << 16)
    assert full[0].size == raw1.size and np.array_equal(full[1], recs1) and short[0].size < raw1.size
    reps = dict(m1=compress(tool, d, "m1", raw1), short=compress(tool, d, "short", short[0]), full=compress(tool, d, "full", full[0]),
                full2=compress(tool, d, "full2", full[0], 2))
    counts = dict(m1=record_counts(reps["m1"], raw1, recs1, 1), short=record_counts(reps["short"], *short, 1),
                  full=record_counts(reps["full"], *full, 1), full2=record_counts(reps["full2"], *full, 2))
    return dict(dir=d, m1=(raw1, recs1), short=short, full=full, reps=reps, counts=counts)


def decodes_of(counts1, counts2):
    """the chunk decodes of archive 2: one per piece of every unit"""
    edges1, edges2 = np.cumsum([0] + counts1), np.cumsum([0] + counts2)
    return sum(int(((edges2[1:] > a) & (edges2[:-1] < b)).sum()) for a, b in zip(edges1[:-1], edges1[1:]))


def holds(rep, want, selection=True):
    out1, out2, rep1, rep2, counters = want
    assert rep["pairs"] == counters and tuple(rep["pairs"]) == PAIR_KEYS
    assert rep["records"] == counters["kept"] and rep["raw_bytes"] == out1.size and rep["raw_bytes2"] == out2.size
    if selection:
        assert rep["mate1"] == {k: int(rep1[w]) for k, w in MATE_WORDS.items()} and rep["mate2"] == {k: int(rep2[w]) for k, w in MATE_WORDS.items()}
        assert list(rep["mate1"]) == list(MATE_WORDS)
    else:
        assert "mate1" not in rep and "mate2" not in rep
    assert "trim" not in rep and "filter" not in rep


@pytest.fixture(scope="module")
def want_short(farm):
    return PR.pair_records(*farm["m1"], *farm["short"], **SELECTION)


def test_archives_whose_chunks_hold_different_records(tool, farm, want_short, tmp_path):
    """both files compressed with -R 1: mate 2's reads are shorter, so its chunks hold more records"""
    d, want = farm["dir"], want_short
    c1, c2 = farm["counts"]["m1"], farm["counts"]["short"]
    assert c1 != c2 and sum(c1) == sum(c2) == len(farm["m1"][1]) and len(c1) >= 3, "the test cannot pass on the aligned path alone"
    assert min(want[4].values()) > 500, "every kind of pair, by the hundred"
    for ext in ("", ".fqx", ".fqs"):
        for name in ("m1", "short"):
            shutil.copy(str(d / (name + ".fqc")) + ext, str(tmp_path / (name + ".fqc")) + ext)
    for with_index in (True, False):
        if not with_index:
            os.remove(tmp_path / "m1.fqc.fqx")
            os.remove(tmp_path / "short.fqc.fqx")
        for t in (1, 4):
            listing = sorted(os.listdir(tmp_path))
            rep = TF.run_tool(tool, "d", tmp_path / "m1.fqc", tmp_path / "o1.fastq", "--mate", tmp_path / "short.fqc", tmp_path / "o2.fastq", "-t", t, *OPTIONS)
            assert (tmp_path / "o1.fastq").read_bytes() == want[0].tobytes() and (tmp_path / "o2.fastq").read_bytes() == want[1].tobytes(), (with_index, t)
            assert sorted(os.listdir(tmp_path)) == sorted(listing + ["o1.fastq", "o2.fastq"]), "the two outputs and nothing else"
            holds(rep, want)
            assert (rep["blocks1"], rep["blocks2"], rep["decodes2"]) == (len(c1), len(c2), decodes_of(c1, c2)) and rep["decodes2"] > len(c2)
            assert rep["index"] == rep["index2"] == ("used" if with_index else "none")
            assert rep["sums"] == rep["sums2"] == "used" and rep["verified"] == len(c1) and rep["verified2"] == rep["decodes2"]
            os.remove(tmp_path / "o1.fastq")
            os.remove(tmp_path / "o2.fastq")
    t1, t2 = FR.parse(want[0]), FR.parse(want[1])
    assert len(t1) == len(t2) == want[4]["kept"] and PR.read_ids(want[0], t1) == PR.read_ids(want[1], t2)


def test_archives_cut_at_the_same_records_and_at_other_block_sizes(tool, farm, tmp_path):
    d = farm["dir"]
    want = PR.pair_records(*farm["m1"], *farm["full"], **SELECTION)
    c1 = farm["counts"]["m1"]
    assert farm["counts"]["full"] == c1, "mate 2 is mate 1 but for its bases: the same chunks"
    rep = TF.run_tool(tool, "d", d / "m1.fqc", tmp_path / "o1.fastq", "--mate", d / "full.fqc", tmp_path / "o2.fastq", "-t", 3, *OPTIONS)
    assert (tmp_path / "o1.fastq").read_bytes() == want[0].tobytes() and (tmp_path / "o2.fastq").read_bytes() == want[1].tobytes()
    holds(rep, want)
    assert rep["decodes2"] == rep["blocks2"] == rep["blocks1"] == len(c1) == rep["verified2"], "every chunk of archive 2 is decoded once"
    # -R 1 against -R 2, either way round
    c2 = farm["counts"]["full2"]
    assert len(c2) < len(c1) and sum(c2) == sum(c1)
    rep = TF.run_tool(tool, "d", d / "m1.fqc", tmp_path / "p1.fastq", "--mate", d / "full2.fqc", tmp_path / "p2.fastq", "-t", 3, *OPTIONS)
    assert (tmp_path / "p1.fastq").read_bytes() == want[0].tobytes() and (tmp_path / "p2.fastq").read_bytes() == want[1].tobytes()
    holds(rep, want)
    assert (rep["blocks1"], rep["blocks2"], rep["decodes2"]) == (len(c1), len(c2), decodes_of(c1, c2))
    swapped = PR.pair_records(*farm["full"], *farm["m1"], a1=SELECTION["a2"], a2=SELECTION["a1"], x=SELECTION["x"], t=SELECTION["t"], f=SELECTION["f"])
    assert swapped[0].tobytes() == want[1].tobytes() and swapped[1].tobytes() == want[0].tobytes()
    options = ["--adapter", ADAPTER2.decode(), "--adapter2", ADAPTER1.decode()] + OPTIONS[4:]
    rep = TF.run_tool(tool, "d", d / "full2.fqc", tmp_path / "q1.fastq", "--mate", d / "m1.fqc", tmp_path / "q2.fastq", "-t", 2, *options)
    assert (tmp_path / "q1.fastq").read_bytes() == want[1].tobytes() and (tmp_path / "q2.fastq").read_bytes() == want[0].tobytes()
    holds(rep, swapped)
    assert (rep["blocks1"], rep["blocks2"], rep["decodes2"]) == (len(c2), len(c1), decodes_of(c2, c1))


def test_without_a_selection_option_both_files_are_restored(tool, farm, tmp_path):
    d = farm["dir"]
    rep = TF.run_tool(tool, "d", d / "m1.fqc", tmp_path / "o1.fastq", "--mate", d / "short.fqc", tmp_path / "o2.fastq", "-t", 3)
    assert (tmp_path / "o1.fastq").read_bytes() == farm["m1"][0].tobytes() and (tmp_path / "o2.fastq").read_bytes() == farm["short"][0].tobytes()
    n = len(farm["m1"][1])
    assert rep["pairs"] == dict(pairs=n, kept=n, dropped_mate1_only=0, dropped_mate2_only=0, dropped_both=0)
    assert rep["records"] == n and rep["raw_bytes"] == farm["m1"][0].size and rep["raw_bytes2"] == farm["short"][0].size
    assert "mate1" not in rep and "mate2" not in rep and "trim" not in rep and "filter" not in rep
    # --adapter alone is mate 2's adapter as well
    want = PR.pair_records(*farm["m1"], *farm["short"], a1=SELECTION["a1"], a2=SELECTION["a1"])
    rep = TF.run_tool(tool, "d", d / "m1.fqc", tmp_path / "a1.fastq", "--mate", d / "short.fqc", tmp_path / "a2.fastq", "-t", 3, "--adapter", ADAPTER1.decode())
    assert (tmp_path / "a1.fastq").read_bytes() == want[0].tobytes() and (tmp_path / "a2.fastq").read_bytes() == want[1].tobytes()
    holds(rep, want)


def nothing_left(tmp_path, before):
    assert sorted(os.listdir(tmp_path)) == before, "neither output nor a .part file"


def test_runs_that_fail_leave_nothing_behind(tool, farm, tmp_path):
    d = farm["dir"]
    raw2, recs2 = farm["short"]
    starts = PR.header_starts(recs2)
    end = lambda r: int(recs2["qual_off"][r]) + int(recs2["len"][r]) + 1  # noqa: E731
    # two records of mate 2 swapped: the first of the two is named, by its number in the archive
    at = 7321
    swapped = np.concatenate((raw2[:starts[at]], raw2[starts[at + 1]:end(at + 1)], raw2[starts[at]:end(at)], raw2[end(at + 1):]))
    assert swapped.size == raw2.size and PR.first_mismatch(*farm["m1"], 0, swapped, FR.parse(swapped), 0, len(recs2)) == at
    compress(tool, tmp_path, "swapped", swapped)
    # mate 2 one record short
    compress(tool, tmp_path, "shorter", raw2[:starts[-1]])
    # one byte of mate 2's archive flipped inside some block's streams
    good = open(d / "short.fqc", "rb").read()
    data = bytearray(good)
    assert len(good) // 2 > (64 << 10)
    data[len(good) // 2] ^= 0x10
    open(tmp_path / "damaged.fqc", "wb").write(data)
    for ext in (".fqx", ".fqs"):
        shutil.copy(str(d / "short.fqc") + ext, str(tmp_path / "damaged.fqc") + ext)
    before = sorted(os.listdir(tmp_path))
    for t in (1, 4):
        for options in (OPTIONS, []):
            r = TF.run_any(tool, "d", d / "m1.fqc", tmp_path / "o1.fastq", "--mate", tmp_path / "swapped.fqc", tmp_path / "o2.fastq", "-t", t, *options)
            assert r.returncode == 1 and r.stdout == "" and ("record %d:" % at) in r.stderr and "read ids" in r.stderr, r.stderr
            nothing_left(tmp_path, before)
        r = TF.run_any(tool, "d", d / "m1.fqc", tmp_path / "o1.fastq", "--mate", tmp_path / "shorter.fqc", tmp_path / "o2.fastq", "-t", t, *OPTIONS)
        n = len(recs2)
        assert r.returncode == 1 and r.stdout == "" and ("%d records" % n) in r.stderr and (" %d:" % (n - 1)) in r.stderr, r.stderr
        nothing_left(tmp_path, before)
        r = TF.run_any(tool, "d", d / "m1.fqc", tmp_path / "o1.fastq", "--mate", tmp_path / "damaged.fqc", tmp_path / "o2.fastq", "-t", t, *OPTIONS)
        assert r.returncode == 1 and r.stdout == "" and r.stderr, r.stdout
        nothing_left(tmp_path, before)
    # the damaged archive as mate 1, and a mate that is not there
    r = TF.run_any(tool, "d", tmp_path / "damaged.fqc", tmp_path / "o1.fastq", "--mate", d / "m1.fqc", tmp_path / "o2.fastq", "-t", 3)
    assert r.returncode == 1 and r.stdout == "" and r.stderr
    nothing_left(tmp_path, before)
    r = TF.run_any(tool, "d", d / "m1.fqc", tmp_path / "o1.fastq", "--mate", tmp_path / "none.fqc", tmp_path / "o2.fastq")
    assert r.returncode == 1 and r.stdout == ""
    nothing_left(tmp_path, before)
