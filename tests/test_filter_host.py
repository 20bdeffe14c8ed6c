"""The host side of the read filter, no GPU: the reference (tests/filter_ref.py) on a chunk judged by hand, fqgpu_filter_check,
the device calls' answer without a device, and the tool's usage errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import filter_ref as R
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_NO_DEVICE = -4, -5


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    F.lib()
    return F


def record(name, seq, phred, plus=b"+"):
    assert len(seq) == len(phred)
    return b"@" + name + b"\n" + seq + b"\n" + plus + b"\n" + bytes(33 + q for q in phred) + b"\n"


def canonical(name, seq, phred):
    return record(name, seq, phred)


# min_len 4, max_len 8, at most one N, mean Phred at least 20, at most 25 % of the Phred values below 10
HAND_FILTER = dict(min_len=4, max_len=8, max_n=1, min_mean_q=20, low_q=10, max_low_pct=25)
HAND = [  # (name, seq, phred, the report column it is counted in, or None for a kept read)
    (b"plain", b"ACGT", [40, 40, 40, 40], None),
    (b"short", b"ACG", [40, 40, 40], R.DROPPED_SHORT),
    (b"long", b"ACGTACGTA", [40] * 9, R.DROPPED_LONG),
    (b"two_n", b"ANNT", [40, 40, 40, 40], R.DROPPED_N),
    (b"mean_one_less", b"ACGT", [20, 20, 20, 19], R.DROPPED_MEAN_Q),         # sum 79 < 20 * 4
    (b"half_low", b"ACGT", [5, 5, 40, 40], R.DROPPED_LOW_Q),                 # mean 22; 100 * 2 > 25 * 4
    (b"mean_on_the_line", b"ACGT", [20, 20, 20, 20], None),                  # sum 80 == 20 * 4
    (b"one_n", b"ANGT", [40, 40, 40, 40], None),                             # #N == max_n
    (b"low_on_the_line", b"ACGT", [5, 25, 25, 25], None),                    # 100 * 1 == 25 * 4, and sum 80 == 20 * 4
    (b"len_min", b"GGCA", [40, 40, 40, 40], None),
    (b"len_max", b"ACGTACGT", [40] * 8, None),
    (b"short_and_all_n", b"NNN", [0, 0, 0], R.DROPPED_SHORT),                    # counted once, under the first criterion
    (b"two_low_of_eight", b"ACGTACGT", [9, 9, 40, 40, 40, 40, 40, 40], None),  # 100 * 2 == 25 * 8
    (b"three_low_of_eight", b"ACGTACGT", [9, 9, 9, 40, 40, 40, 40, 40], R.DROPPED_LOW_Q),
    (b"mean_low_n", b"NNNN", [1, 1, 1, 1], R.DROPPED_N),                     # fails three: counted under n
]


def hand_chunk(plus_repeats=False):
    raw = b"".join(record(n, s, q, b"+" + n if plus_repeats and i % 2 == 0 else b"+") for i, (n, s, q, _) in enumerate(HAND))
    return np.frombuffer(raw, dtype=np.uint8)


def hand_expected():
    out = b"".join(canonical(n, s, q) for n, s, q, col in HAND if col is None)
    report = np.zeros(R.REPORT_WORDS, dtype=np.uint64)
    report[R.N_RECORDS] = len(HAND)
    report[R.N_KEPT] = sum(col is None for *_, col in HAND)
    report[R.BASES_IN] = sum(len(s) for _, s, _, _ in HAND)
    report[R.BASES_KEPT] = sum(len(s) for _, s, _, col in HAND if col is None)
    report[R.BYTES_KEPT] = len(out)
    for *_, col in HAND:
        if col is not None:
            report[col] += 1
    keep = np.packbits([col is None for *_, col in HAND], bitorder="little")
    return np.frombuffer(out, dtype=np.uint8), report, keep


@pytest.mark.parametrize("plus_repeats", [False, True])
def test_the_reference_on_a_chunk_judged_by_hand(plus_repeats):
    want_out, want_report, want_keep = hand_expected()
    assert all(want_report[c] >= 1 for c in range(R.DROPPED_SHORT, R.DROPPED_LOW_Q + 1)), "one read per report column"
    out, report, keep = R.filter_chunk(hand_chunk(plus_repeats), R.flt(**HAND_FILTER))
    assert out.tobytes() == want_out.tobytes()
    assert report.tolist() == want_report.tolist()
    assert keep.tolist() == want_keep.tolist()


def test_the_reference_one_criterion_at_a_time():
    raw = hand_chunk()
    names = [n for n, *_ in HAND]
    kept = lambda **kw: [names[i].decode() for i in np.flatnonzero(np.unpackbits(R.filter_chunk(raw, R.flt(**kw))[2], bitorder="little")[:len(HAND)])]  # noqa: E731
    assert kept() == [n.decode() for n in names], "the default filter keeps everything"
    assert set(names) - set(n.encode() for n in kept(min_len=4)) == {b"short", b"short_and_all_n"}
    assert set(names) - set(n.encode() for n in kept(max_len=8)) == {b"long"}
    assert set(names) - set(n.encode() for n in kept(max_n=1)) == {b"two_n", b"short_and_all_n", b"mean_low_n"}
    assert set(names) - set(n.encode() for n in kept(max_n=0)) == {b"two_n", b"one_n", b"short_and_all_n", b"mean_low_n"}
    assert set(names) - set(n.encode() for n in kept(min_mean_q=20)) == {b"mean_one_less", b"short_and_all_n", b"mean_low_n"}
    assert set(names) - set(n.encode() for n in kept(low_q=10, max_low_pct=25)) == \
        {b"half_low", b"short_and_all_n", b"three_low_of_eight", b"mean_low_n"}
    assert kept(low_q=64, max_low_pct=99) == [], "every Phred value is below 64"
    assert len(kept(low_q=64, max_low_pct=100)) == len(HAND)
    # only the lines a criterion reads are judged
    bad = raw.copy()
    recs = R.parse(bad)
    bad[recs["qual_off"][0]] = ord("~")
    bad[recs["seq_off"][3]] = ord("X")
    assert R.filter_chunk(bad, R.flt(min_len=4))[1][R.N_KEPT] == len(HAND) - 2
    for kw in (dict(max_n=5), dict(min_mean_q=1), dict(low_q=1, max_low_pct=100)):
        with pytest.raises(R.Refused):
            R.filter_chunk(bad, R.flt(**kw))


GOOD_FILTERS = [dict(), dict(min_len=7, max_len=7), dict(max_len=0), dict(min_mean_q=63), dict(low_q=64, max_low_pct=100), dict(max_n=0),
                dict(min_len=R.NONE, max_len=R.NONE), dict(max_n=R.NONE - 1)]
BAD_FILTERS = [dict(min_len=8, max_len=7), dict(min_mean_q=64), dict(low_q=65), dict(low_q=10, max_low_pct=101), dict(max_low_pct=101),
               dict(reserved=(1, 0)), dict(reserved=(0, 1)), dict(min_len=1, max_len=0)]


def test_filter_check(F):
    lib = F.lib()
    for kw in GOOD_FILTERS:
        assert F.binding.filter_check(R.flt(**kw)) == 0 and R.check(R.flt(**kw)), kw
    for kw in BAD_FILTERS:
        assert F.binding.filter_check(R.flt(**kw)) == E_ARG and not R.check(R.flt(**kw)), kw
    assert lib.fqgpu_filter_check(None) == E_ARG
    assert F.binding.read_filter(**HAND_FILTER).tolist() == R.flt(**HAND_FILTER).tolist()
    assert F.binding.FILTER_NONE == R.NONE and F.binding.FILTER_REPORT_WORDS == R.REPORT_WORDS


def test_the_device_calls_say_no_device_without_one(F):
    """(with a device in the machine the same calls get as far as their arguments: no handle, FQGPU_E_ARG)"""
    want = E_NO_DEVICE if F.device_count() == 0 else E_ARG
    lib = F.lib()
    f = R.flt()
    report = np.full(R.REPORT_WORDS, 7, dtype=np.uint64)
    n = C.c_size_t(7)
    assert lib.fqgpu_chunk_filter(None, f.ctypes.data_as(C.c_void_p), None, 0, C.byref(n), report.ctypes.data_as(C.c_void_p), None) == want
    assert lib.fqgpu_dblock_filter(None, None, f.ctypes.data_as(C.c_void_p), None, 0, C.byref(n), report.ctypes.data_as(C.c_void_p), None) == want
    assert lib.fqgpu_chunk_filter(None, None, None, 0, None, None, None) == want, "said before any argument is looked at"
    assert lib.fqgpu_dblock_filter(None, None, None, None, 0, None, None, None) == want
    if want == E_NO_DEVICE:
        assert n.value == 7 and (report == 7).all(), "nothing is looked at"


@pytest.mark.parametrize("name", ["SRR065390_sub_1", "without_ns", "SRR065390_sub_2", "SRR065390_1_first5"])
def test_the_reference_with_a_pass_all_filter_returns_the_canonical_file(golden_dir, name):
    raw, recs = O.load_fastq(os.path.join(golden_dir, name + ".fastq"))
    assert np.array_equal(R.parse(raw), recs.astype(R.REC_DTYPE)), "the reference parses as fqgpu_parse_fastq does"
    for f in (R.flt(), R.flt(min_len=1, max_n=65535, min_mean_q=0, low_q=64, max_low_pct=100)):
        out, report, keep = R.filter_chunk(raw, f)
        end = int(recs["qual_off"][-1]) + int(recs["len"][-1]) + 1
        assert out.tobytes() == raw[:end].tobytes()
        assert report[:5].tolist() == [len(recs), len(recs), int(recs["len"].sum()), int(recs["len"].sum()), end] and not report[5:].any()
        assert np.unpackbits(keep, bitorder="little")[:len(recs)].all() and not np.unpackbits(keep, bitorder="little")[len(recs):].any()
    # '+' lines that repeat the header: the canonical file is the one with bare '+' lines
    lines = raw.tobytes().split(b"\n")[:-1]
    for r in range(len(recs)):
        lines[4 * r + 2] = b"+" + lines[4 * r][1:]
    fat = np.frombuffer(b"\n".join(lines) + b"\n", dtype=np.uint8)
    assert R.filter_chunk(fat, R.flt())[0].tobytes() == raw[:end].tobytes()


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("filter_tool") / "fqc_tool")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tools", "fqc_tool.cpp"),
                    "-L" + os.path.join(ROOT, "fqcomp28_amd"), "-lfqgpu", "-Wl,-rpath," + os.path.join(ROOT, "fqcomp28_amd"),
                    "-lpthread"], check=True)
    return exe


FILTER_OPTIONS = [["--min-len", "5"], ["--max-len", "100"], ["--max-n", "0"], ["--min-mean-q", "20"], ["--max-low-q", "10:25"]]


@pytest.mark.parametrize("args", [
    # a filter option on any command but d
    *[["c", "in.fastq", "out.fqc"] + opt for opt in FILTER_OPTIONS],
    *[["x", "in.fqc"] + opt for opt in FILTER_OPTIONS],
    *[["t", "in.fqc"] + opt for opt in FILTER_OPTIONS],
    *[["s", "in.fqc", "report.tsv"] + opt for opt in FILTER_OPTIONS],
    # ... together with --records, --fasta, --index, --index-stride
    *[["d", "in.fqc", "out.fastq"] + opt + other for opt in FILTER_OPTIONS
      for other in (["--records", "0:5"], ["--fasta"], ["--index"], ["--index-stride", "64"])],
    ["d", "in.fqc", "out.fastq", "--records", "0:5", "--max-n", "0"],
    # values fqgpu_filter_check refuses
    ["d", "in.fqc", "out.fastq", "--min-len", "9", "--max-len", "8"],
    ["d", "in.fqc", "out.fastq", "--min-mean-q", "64"],
    ["d", "in.fqc", "out.fastq", "--max-low-q", "65:10"],
    ["d", "in.fqc", "out.fastq", "--max-low-q", "10:101"],
    # malformed values
    ["d", "in.fqc", "out.fastq", "--max-low-q", "10"],
    ["d", "in.fqc", "out.fastq", "--max-low-q", "10:"],
    ["d", "in.fqc", "out.fastq", "--max-low-q", ":10"],
    ["d", "in.fqc", "out.fastq", "--max-low-q", "10:2:3"],
    ["d", "in.fqc", "out.fastq", "--max-low-q", "a:b"],
    ["d", "in.fqc", "out.fastq", "--max-low-q"],
    ["d", "in.fqc", "out.fastq", "--min-len", "-1"],
    ["d", "in.fqc", "out.fastq", "--max-n", "x"],
    ["d", "in.fqc", "out.fastq", "--min-mean-q", "2.5"],
    ["d", "in.fqc", "out.fastq", "--max-len"],
])
def test_usage_errors_are_said_before_any_file_or_device_is_touched(tool, tmp_path, args):
    r = subprocess.run([tool] + args, capture_output=True, text=True, cwd=tmp_path, timeout=60)
    assert r.returncode == 2 and r.stdout == "" and r.stderr, (args, r.stderr)
    assert os.listdir(tmp_path) == []
