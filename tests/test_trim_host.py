"""The host side of read trimming, no GPU: the reference (tests/trim_ref.py) on a chunk whose windows are worked out by hand,
the three forms of the running-sum walk against each other, fqgpu_trim_check, the device calls' answer without a device, and
the tool's usage errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import filter_ref as FR
import oracle_lib as O
import trim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_NO_DEVICE = -4, -5
FIXTURES = ["SRR065390_sub_1", "without_ns", "SRR065390_sub_2", "SRR065390_1_first5"]


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    F.lib()
    return F


def record(name, seq, phred, plus=b"+"):
    assert len(seq) == len(phred)
    return b"@" + name + b"\n" + seq + b"\n" + plus + b"\n" + bytes(33 + q for q in phred) + b"\n"


# Cutoff 20 at both ends: a walk adds 20 - Phred per base, stops below 0 and cuts behind the first place of its largest sum.
TRIM_Q = dict(q_front=20, q_tail=20)
# ... after one base is cut from either end, and at most three bases of what is left
TRIM_ALL = dict(cut_front=1, cut_tail=1, q_front=20, q_tail=20, crop=3)
# fixed cuts and crop alone: f = min(2, L), t = min(1, L - f), n = min(L - f - t, 3)
TRIM_CUTS = dict(cut_front=2, cut_tail=1, crop=3)
HAND = [  # (name, seq, phred, window under TRIM_Q, under TRIM_ALL, under TRIM_CUTS); (0, 0): emptied
    # both walks stop at their first base (-10)
    (b"untouched", b"ACGTAC", [30, 30, 30, 30, 30, 30], (0, 6), (1, 3), (2, 3)),
    # front: 15, 25 (start 2), 15, 5, -5 stop.  After the cuts, from base 1: 10 (start 2), 0, -10 stop
    (b"front_only", b"ACGTAC", [5, 10, 30, 30, 30, 30], (2, 4), (2, 3), (2, 3)),
    # tail: 18 (stop 5), 28 (stop 4), 18, 8, -2 stop.  After the cuts, from base 4: 10 (stop 4), 0, -10 stop
    (b"tail_only", b"ACGTAC", [30, 30, 30, 30, 10, 2], (0, 4), (1, 3), (2, 3)),
    # front: 18 (start 1), 8, -2 stop; tail: 17 (stop 5), 7, -3 stop
    (b"both_ends", b"ACGTAC", [2, 30, 30, 30, 30, 3], (1, 4), (1, 3), (2, 3)),
    # front: 18, 36, 54, 72 (start 4); tail the same (stop 0).  After the cuts the interval is [1, 3): start 3, stop 1
    (b"emptied", b"ACGT", [2, 2, 2, 2], (0, 0), (0, 0), (2, 1)),
    # the walks are independent and each runs through the good base: front 18, 8, 26 (start 3); tail 18, 8, 26 (stop 0):
    # start >= stop.  After the cuts only the good base is left.  The fixed cuts alone take all three bases
    (b"crossed", b"ACG", [2, 30, 2], (0, 0), (1, 1), (0, 0)),
    # front: 10 (start 1), 0, 10 -- equal to the best, not above it: start stays 1 --, -10 stop
    (b"tie_rule", b"ACGTAC", [10, 30, 10, 40, 40, 40], (1, 5), (1, 3), (2, 3)),
    # Phred values on the cutoff add nothing: front 15 (start 1), 15, 15, -5 stop
    (b"on_the_cutoff", b"ACGTAC", [5, 20, 20, 40, 40, 40], (1, 5), (1, 3), (2, 3)),
    # front: 18 (start 1), -2 stop -- the three low bases behind would have brought it to 52
    (b"dip_and_recover", b"ACGTACGT", [2, 40, 2, 2, 2, 40, 40, 40], (1, 7), (1, 3), (2, 3)),
    # every base on the cutoff: no sum above 0, nothing is cut
    (b"all_on_the_cutoff", b"ACGT", [20, 20, 20, 20], (0, 4), (1, 2), (2, 1)),
]
HAND_TRIMS = [(TRIM_Q, 3), (TRIM_ALL, 4), (TRIM_CUTS, 5)]
HAND_FILTER = dict(min_len=5)   # under TRIM_Q the reads with four bases left are short; an emptied read is "short" whatever min_len


def hand_chunk(plus_repeats=False):
    raw = b"".join(record(n, s, q, b"+" + n if plus_repeats and i % 2 == 0 else b"+") for i, (n, s, q, *_) in enumerate(HAND))
    return np.frombuffer(raw, dtype=np.uint8)


def hand_expected(col, min_len=0):
    """what the windows in column `col` of HAND and a filter min_len say"""
    report = np.zeros(R.REPORT_WORDS, dtype=np.uint64)
    out, keep, win = b"", [], []
    for row in HAND:
        name, seq, phred = row[:3]
        start, n = row[col]
        kept = n > 0 and n >= min_len
        keep.append(kept)
        win.append(start | n << 16)
        report[R.N_RECORDS] += 1
        report[R.BASES_IN] += len(seq)
        report[R.READS_TRIMMED] += n != len(seq)
        report[R.BASES_CUT_FRONT] += start
        report[R.BASES_CUT_TAIL] += len(seq) - start - n
        report[R.READS_EMPTIED] += n == 0
        if kept:
            out += record(name, seq[start:start + n], phred[start:start + n])
            report[R.N_KEPT] += 1
            report[R.BASES_KEPT] += n
        else:
            report[R.DROPPED_SHORT] += 1
    report[R.BYTES_KEPT] = len(out)
    return np.frombuffer(out, dtype=np.uint8), report, np.packbits(keep, bitorder="little"), np.array(win, dtype=np.uint32)


def holds(got, want, what=""):
    assert got[0].tobytes() == want[0].tobytes(), what
    assert got[1].tolist() == want[1].tolist(), what
    assert got[2].tolist() == want[2].tolist(), what
    assert got[3].tolist() == want[3].tolist(), what


@pytest.mark.parametrize("plus_repeats", [False, True])
def test_the_reference_on_a_chunk_trimmed_by_hand(plus_repeats):
    raw = hand_chunk(plus_repeats)
    kinds = {(s > 0, s + n < len(seq), n == 0) for _, seq, _, (s, n), *_ in HAND}
    assert {(False, False, False), (True, False, False), (False, True, False), (True, True, False), (False, True, True)} <= kinds, \
        "an untouched read, one cut at the front, at the tail, at both ends, an emptied one"
    for kw, col in HAND_TRIMS:
        holds(R.trim_chunk(raw, R.trm(**kw)), hand_expected(col), str(kw))
        holds(R.trim_chunk(raw, R.trm(**kw), FR.flt()), hand_expected(col), str(kw))
    want = hand_expected(3, **HAND_FILTER)
    assert 0 < int(want[1][R.N_KEPT]) < len(HAND) - int(want[1][R.READS_EMPTIED])
    holds(R.trim_chunk(raw, R.trm(**TRIM_Q), FR.flt(**HAND_FILTER)), want)


def test_the_filter_judges_what_is_left():
    # the window of "dip_and_recover" under TRIM_Q is (1, 7): Phred 40, 2, 2, 2, 40, 40, 40 -- sum 166, three values below 10
    raw = hand_chunk()
    at = [n for n, *_ in HAND].index(b"dip_and_recover")
    kept = lambda **kw: bool(np.unpackbits(R.trim_chunk(raw, R.trm(**TRIM_Q), FR.flt(**kw))[2], bitorder="little")[at])  # noqa: E731
    assert kept(min_len=7, max_len=7) and not kept(min_len=8) and not kept(max_len=6)
    assert kept(min_mean_q=23) and not kept(min_mean_q=24)                    # 166 >= 23 * 7 = 161, < 24 * 7 = 168
    assert kept(low_q=10, max_low_pct=43) and not kept(low_q=10, max_low_pct=42)  # 100 * 3 = 300 <= 43 * 7 = 301, > 42 * 7
    # the first failing criterion, in the filter's order; an emptied read under "short" whatever min_len is
    r = R.trim_chunk(raw, R.trm(**TRIM_Q), FR.flt(max_len=4, min_mean_q=31))[1]
    assert (int(r[R.DROPPED_SHORT]), int(r[R.DROPPED_LONG]), int(r[R.READS_EMPTIED])) == (2, 4, 2)
    # N is counted over the window only
    with_n = np.frombuffer(record(b"n", b"NACGTN", [2, 30, 30, 30, 30, 2]) + record(b"m", b"ANCGTA", [2, 30, 30, 30, 30, 2]), dtype=np.uint8)
    assert R.trim_chunk(with_n, R.trm(), FR.flt(max_n=0))[1][R.N_KEPT] == 0
    assert np.unpackbits(R.trim_chunk(with_n, R.trm(**TRIM_Q), FR.flt(max_n=0))[2], bitorder="little")[:2].tolist() == [1, 0]


def test_only_the_lines_that_are_read_are_judged_and_those_over_all_their_bytes():
    raw = hand_chunk().copy()
    recs = FR.parse(raw)
    raw[recs["qual_off"][1]] = ord("~")        # the first quality byte of "front_only": cut by TRIM_CUTS and by TRIM_Q
    raw[recs["seq_off"][2] + 5] = ord("X")     # the last base of "tail_only": cut by all three
    for kw, f in ((TRIM_CUTS, FR.flt(min_len=2)), (dict(crop=2), None)):
        assert R.trim_chunk(raw, R.trm(**kw), f)[1][R.N_RECORDS] == len(HAND), "no line is read"
    for kw, f in ((TRIM_Q, None), (TRIM_CUTS, FR.flt(min_mean_q=1)), (TRIM_CUTS, FR.flt(low_q=1, max_low_pct=100)), (TRIM_CUTS, FR.flt(max_n=5))):
        with pytest.raises(R.Refused):
            R.trim_chunk(raw, R.trm(**kw), f)
    for bad in (dict(crop=0), dict(q_tail=65)):
        with pytest.raises(R.Refused):
            R.trim_chunk(hand_chunk(), R.trm(**bad))


def test_the_three_forms_of_the_walk_agree():
    """random lines in the shapes the quality trim meets -- low ends around a plateau, plain noise, lines on the cutoff --
    cut into the pieces a record's lanes hold (a first piece of 1 .. 16 symbols, then sixteen each) and into random pieces"""
    rng = np.random.default_rng(11)
    cut_some = 0
    for i in range(3000):
        L = int(rng.choice([1, 2, 15, 16, 17, 40, 100, 257, 300]))
        kind = i % 3
        if kind == 0:
            phred = np.clip(30 + rng.integers(-6, 7, L), 0, 63)
            a, b = int(rng.choice([0, 0, 3, 10, 40])), int(rng.choice([0, 0, 5, 30, 200]))
            phred[:a] = np.clip(5 + rng.integers(-4, 5, min(a, L)), 0, 63)
            if b:
                phred[-b:] = np.clip(5 + rng.integers(-4, 5, min(b, L)), 0, 63)
        elif kind == 1:
            phred = rng.integers(0, 42, L)
        else:
            phred = 20 + rng.integers(-1, 2, L)
        for inc in (20 - phred, (20 - phred)[::-1]):
            want = R.walk_serial(inc)
            cut_some += want > 0
            assert R.walk(inc) == want
            first = int(rng.integers(1, 17))
            assert R.walk_pieces(inc, sorted({0, L} | set(range(first, L, 16)))) == want
            cuts = sorted(int(x) for x in rng.integers(0, L + 1, int(rng.integers(0, 6))))   # (equal bounds: empty pieces)
            assert R.walk_pieces(inc, [0] + cuts + [L]) == want
    assert cut_some > 1500


@pytest.mark.parametrize("name", FIXTURES)
def test_a_trim_that_cuts_nothing_is_the_filter(golden_dir, name):
    raw, recs = O.load_fastq(os.path.join(golden_dir, name + ".fastq"))
    recs = recs.astype(R.REC_DTYPE)
    for kw in (dict(), dict(max_n=0), dict(min_mean_q=20), dict(min_len=100, low_q=20, max_low_pct=20)):
        want = FR.filter_records(raw, recs, FR.flt(**kw))
        got = R.trim_records(raw, recs, R.trm(), FR.flt(**kw))
        assert got[0].tobytes() == want[0].tobytes() and got[2].tolist() == want[2].tolist(), (name, kw)
        assert got[1][:10].tolist() == want[1][:10].tolist() and not got[1][10:].any(), (name, kw)
        assert got[3].tolist() == (recs["len"].astype(np.uint32) << 16).tolist()
    assert R.trim_records(raw, recs, R.trm())[0].tobytes() == R.trim_records(raw, recs, R.trm(), FR.flt())[0].tobytes()


GOOD_TRIMS = [dict(), dict(cut_front=65535, cut_tail=65535), dict(q_front=64, q_tail=64), dict(crop=1), dict(crop=R.NONE - 1),
              dict(cut_front=3, cut_tail=4, q_front=20, q_tail=30, crop=100)]
BAD_TRIMS = [dict(cut_front=65536), dict(cut_tail=65536), dict(cut_front=R.NONE), dict(q_front=65), dict(q_tail=65), dict(crop=0),
             dict(reserved=(1, 0, 0)), dict(reserved=(0, 1, 0)), dict(reserved=(0, 0, 1))]


def test_trim_check(F):
    for kw in GOOD_TRIMS:
        assert F.binding.trim_check(R.trm(**kw)) == 0 and R.check(R.trm(**kw)), kw
    for kw in BAD_TRIMS:
        assert F.binding.trim_check(R.trm(**kw)) == E_ARG and not R.check(R.trm(**kw)), kw
    assert F.lib().fqgpu_trim_check(None) == E_ARG
    assert F.binding.read_trim(**TRIM_ALL).tolist() == R.trm(**TRIM_ALL).tolist()
    assert F.binding.TRIM_REPORT_WORDS == R.REPORT_WORDS and len(F.binding.TRIM_REPORT_NAMES) == R.READS_EMPTIED + 1


def test_the_device_calls_say_no_device_without_one(F):
    """(with a device in the machine the same calls get as far as their arguments: no handle, FQGPU_E_ARG)"""
    want = E_NO_DEVICE if F.device_count() == 0 else E_ARG
    lib = F.lib()
    t, f = R.trm(**TRIM_Q), FR.flt()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    report = np.full(R.REPORT_WORDS, 7, dtype=np.uint64)
    n = C.c_size_t(7)
    assert lib.fqgpu_chunk_trim(None, p(t), p(f), None, 0, C.byref(n), p(report), None, None) == want
    assert lib.fqgpu_dblock_trim(None, None, p(t), None, None, 0, C.byref(n), p(report), None, None) == want
    assert lib.fqgpu_chunk_trim(None, None, None, None, 0, None, None, None, None) == want, "said before any argument is looked at"
    assert lib.fqgpu_dblock_trim(None, None, None, None, None, 0, None, None, None, None) == want
    if want == E_NO_DEVICE:
        assert n.value == 7 and (report == 7).all(), "nothing is looked at"


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("trim_tool") / "fqc_tool")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tools", "fqc_tool.cpp"),
                    "-L" + os.path.join(ROOT, "fqcomp28_amd"), "-lfqgpu", "-Wl,-rpath," + os.path.join(ROOT, "fqcomp28_amd"),
                    "-lpthread"], check=True)
    return exe


TRIM_OPTIONS = [["--cut-front", "5"], ["--cut-tail", "5"], ["--trim-q5", "20"], ["--trim-q3", "20"], ["--crop", "100"]]


@pytest.mark.parametrize("args", [
    # a trim option on any command but d
    *[["c", "in.fastq", "out.fqc"] + opt for opt in TRIM_OPTIONS],
    *[["x", "in.fqc"] + opt for opt in TRIM_OPTIONS],
    *[["t", "in.fqc"] + opt for opt in TRIM_OPTIONS],
    *[["s", "in.fqc", "report.tsv"] + opt for opt in TRIM_OPTIONS],
    # ... together with --records, --fasta, --index, --index-stride
    *[["d", "in.fqc", "out.fastq"] + opt + other for opt in TRIM_OPTIONS
      for other in (["--records", "0:5"], ["--fasta"], ["--index"], ["--index-stride", "64"])],
    ["d", "in.fqc", "out.fastq", "--records", "0:5", "--crop", "50"],
    ["d", "in.fqc", "out.fastq", "--max-n", "0", "--trim-q3", "20", "--fasta"],
    # values fqgpu_trim_check refuses, alone and beside a filter
    ["d", "in.fqc", "out.fastq", "--cut-front", "65536"],
    ["d", "in.fqc", "out.fastq", "--cut-tail", "65536"],
    ["d", "in.fqc", "out.fastq", "--trim-q5", "65"],
    ["d", "in.fqc", "out.fastq", "--trim-q3", "65"],
    ["d", "in.fqc", "out.fastq", "--crop", "0"],
    ["d", "in.fqc", "out.fastq", "--min-len", "5", "--crop", "0"],
    # a filter the check refuses beside a good trim
    ["d", "in.fqc", "out.fastq", "--trim-q3", "20", "--min-mean-q", "64"],
    # malformed values
    ["d", "in.fqc", "out.fastq", "--cut-front", "-1"],
    ["d", "in.fqc", "out.fastq", "--trim-q3", "x"],
    ["d", "in.fqc", "out.fastq", "--trim-q5", "2.5"],
    ["d", "in.fqc", "out.fastq", "--crop", "1e3"],
    ["d", "in.fqc", "out.fastq", "--crop", "4294967296"],
    ["d", "in.fqc", "out.fastq", "--crop"],
    ["d", "in.fqc", "out.fastq", "--cut-tail"],
])
def test_usage_errors_are_said_before_any_file_or_device_is_touched(tool, tmp_path, args):
    r = subprocess.run([tool] + args, capture_output=True, text=True, cwd=tmp_path, timeout=60)
    assert r.returncode == 2 and r.stdout == "" and r.stderr, (args, r.stderr)
    assert os.listdir(tmp_path) == []
