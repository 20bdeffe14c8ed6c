"""The host side of the mate merge, no GPU: the rule's restatement (tests/merge_ref.py) on hand-made pairs whose answers are
written out by hand -- one for every branch of the rule --, the fixture's counts and the CRC-32 of its merged bytes, the
composition with the correction, fqgpu_merge_check on every bound, the device calls' answer without a device, the report's
text, the word-by-word sum and Selection::check under AddressSanitizer and UBSan (tests/cpp/merge_report_check.cpp, a
stand-alone program), and the tool's usage errors.  Integer arithmetic: there is no tolerance."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

import correct_ref as CR
import merge_ref as MR
import oracle_lib as O
import overlap_ref as OR
import pair_ref as PR
import test_correct_host as TCH
import test_overlap_host as TOH

ROOT = TOH.ROOT
E_ARG, E_NO_DEVICE = -4, -5
LINK = TOH.LINK
rc = OR.revcomp

X = b"ACGTACGTAC"
RX = b"GTACGTACGT"   # rc(X): place p of X stands beside place 9 - p; X[3] = 'T' beside RX[6] = 'A'
Q = b"I" * 10        # Phred 40


def put(s, at, c):
    return s[:at] + c + s[at + 1:]


# (what, s1, q1, s2, q2, I, floor_q, (bases, quals, overlap_bases, places_disagree, places_n)) -- every answer worked out by hand.
# Quality bytes: '!' 0, '#' 2, '$' 3, '+' 10, '5' 20, '6' 21, '8' 23, 'I' 40, '`' 63
HAND = [
    # the fragment AAACCCGG, five bases of either mate: places 0 .. 2 are mate 1's alone, 3 and 4 both mates' -- they agree,
    # and mate 2's Phred 41 and 40 beat 35 and 36 --, 5 .. 7 mate 2's alone, complemented and read backwards
    ("in1 only, agree, in2 only", b"AAACC", b"ABCDE", b"CCGGG", b"567IJ", 8, 2, (b"AAACCCGG", b"ABCJI765", 2, 0, 0)),
    ("agree, mate 1 higher", X, put(Q, 3, b"I"), RX, put(Q, 6, b"5"), 10, 2, (X, Q, 10, 0, 0)),
    ("both N: the lower Phred", put(X, 3, b"N"), put(Q, 3, b"5"), put(RX, 6, b"N"), put(Q, 6, b"+"), 10, 2, (put(X, 3, b"N"), put(Q, 3, b"+"), 10, 0, 1)),
    ("N in mate 1: mate 2's base and Phred", put(X, 3, b"N"), Q, RX, put(Q, 6, b"5"), 10, 2, (X, put(Q, 3, b"5"), 10, 0, 1)),
    ("N in mate 2: mate 1's base and Phred", X, put(Q, 3, b"5"), put(RX, 6, b"N"), Q, 10, 2, (X, put(Q, 3, b"5"), 10, 0, 1)),
    ("differ, mate 1 higher: 40 - 20", put(X, 3, b"G"), Q, RX, put(Q, 6, b"5"), 10, 2, (put(X, 3, b"G"), put(Q, 3, b"5"), 10, 1, 0)),
    ("differ, mate 2 higher: 40 - 20", put(X, 3, b"G"), put(Q, 3, b"5"), RX, Q, 10, 2, (X, put(Q, 3, b"5"), 10, 1, 0)),
    ("a tie: mate 1 wins, the floor bites", put(X, 3, b"G"), put(Q, 3, b"5"), RX, put(Q, 6, b"5"), 10, 2, (put(X, 3, b"G"), put(Q, 3, b"#"), 10, 1, 0)),
    ("a tie at floor 0", put(X, 3, b"G"), put(Q, 3, b"5"), RX, put(Q, 6, b"5"), 10, 0, (put(X, 3, b"G"), put(Q, 3, b"!"), 10, 1, 0)),
    ("21 - 20 below the floor", put(X, 3, b"G"), put(Q, 3, b"6"), RX, put(Q, 6, b"5"), 10, 2, (put(X, 3, b"G"), put(Q, 3, b"#"), 10, 1, 0)),
    ("23 - 20 above the floor", put(X, 3, b"G"), put(Q, 3, b"8"), RX, put(Q, 6, b"5"), 10, 2, (put(X, 3, b"G"), put(Q, 3, b"$"), 10, 1, 0)),
    ("20 - 23: mate 2's base, above the floor", put(X, 3, b"G"), put(Q, 3, b"5"), RX, put(Q, 6, b"8"), 10, 2, (X, put(Q, 3, b"$"), 10, 1, 0)),
    ("the floor at 63", put(X, 3, b"G"), Q, RX, put(Q, 6, b"5"), 10, 63, (put(X, 3, b"G"), put(Q, 3, b"`"), 10, 1, 0)),
    # I = 1: the one place is s1[0] beside s2[0]; I = L1 + L2 - 1: the one place of overlap is s1[9] beside s2[9]
    ("I = 1", X, Q, b"TGGGGGGGGG", put(Q, 0, b"5"), 1, 2, (b"A", b"I", 1, 0, 0)),
    ("I = L1 + L2 - 1", X, Q, b"AAAAAAAAAG", Q, 19, 2, (X + b"TTTTTTTTT", b"I" * 19, 1, 0, 0)),
    # I below both lengths: the bases of either mate at or behind I are adapter, dropped and not looked at
    ("I = 4 of 10 and 10", b"ACGTxxxxxx", b"IIII      ", b"ACGTzzzzzz", b"5555\x7f\x7f\x7f\x7f\x7f\x7f", 4, 2, (b"ACGT", b"IIII", 4, 0, 0)),
]


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    F.lib()
    return F


@pytest.fixture(scope="module")
def golden(golden_dir):
    return [O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_%d.fastq" % m)) for m in (1, 2)]


@pytest.fixture(scope="module")
def golden_overlap(golden):
    (raw1, recs1), (raw2, recs2) = golden
    return OR.overlap_records(raw1, recs1, 0, raw2, recs2, 0, 1000, OR.spec())


def test_the_rule_on_pairs_made_by_hand():
    assert rc(X) == RX and rc(b"AAACCCGG")[:5] == b"CCGGG"
    for what, s1, q1, s2, q2, I, floor_q, want in HAND:
        assert MR.merge_pair(s1, q1, s2, q2, I, floor_q) == want, what
        # ... and as the one record of a pair of chunks: mate 1's header line, the bases, "\n+\n", the qualities, '\n'
        raw1, recs1 = OR.chunk([s1], [q1], [b"pair one/1"])
        raw2, recs2 = OR.chunk([s2], [q2], [b"pair one/2"])
        out, report, merged = MR.merge_records(raw1, recs1, 0, raw2, recs2, 0, 1, [I], None, MR.spec(floor_q))
        assert out.tobytes() == b"@pair one/1\n" + want[0] + b"\n+\n" + want[1] + b"\n", what
        assert report.tolist() == [1, 1, 1, I, 12 + 2 * I + 4, want[2], want[3], want[4], len(s1) - min(len(s1), I), len(s2) - min(len(s2), I), 0, 0, 0, 0, 0, 0], what
        assert merged.tolist() == [1]


def test_eligibility_marks_and_min_len():
    seqs1, seqs2 = [X, put(X, 3, b"G"), X, X], [RX, RX, RX, RX]
    raw1, recs1 = OR.chunk(seqs1)
    raw2, recs2 = OR.chunk(seqs2)
    ins = [10, 10, 0, 14]   # (X has the period 4: at I = 14 places 4 .. 9 have both mates, and they agree)
    out, report, merged = MR.merge_records(raw1, recs1, 0, raw2, recs2, 0, 4, ins, None, MR.spec())
    assert report.tolist() == [4, 3, 3, 34, 3 * 4 + 2 * 34 + 3 * 4, 26, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0] and merged.tolist() == [0b1011]
    assert out.tobytes().count(b"@r") == 3 and out.tobytes().startswith(b"@r0\nACGTACGTAC\n+\nIIIIIIIIII\n@r1\nACGGACGTAC\n+\nIII#IIIIII\n@r3\nAC")
    # the mark: an unmarked pair with an insert is counted and left alone; a pair without an insert is neither
    out, report, merged = MR.merge_records(raw1, recs1, 0, raw2, recs2, 0, 4, ins, [0b0110], MR.spec())
    assert report.tolist() == [4, 3, 1, 10, 4 + 24, 10, 1, 0, 0, 0, 2, 0, 0, 0, 0, 0] and merged.tolist() == [0b0010]
    assert MR.merge_records(raw1, recs1, 0, raw2, recs2, 0, 4, ins, [0], MR.spec())[1].tolist() == [4, 3, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0, 0, 0, 0, 0]
    # min_len at I - 1, I and I + 1
    for min_len, n_merged in ((9, 3), (10, 3), (11, 1), (13, 1), (14, 1), (15, 0)):
        report = MR.merge_records(raw1, recs1, 0, raw2, recs2, 0, 4, ins, None, MR.spec(2, min_len))[1]
        assert (int(report[MR.PAIRS_MERGED]), int(report[MR.PAIRS_TOO_SHORT])) == (n_merged, 3 - n_merged), min_len
    # a sub-range with other firsts: record 1 of mate 1 beside record 0 of mate 2
    out, report, _ = MR.merge_records(raw1, recs1, 1, raw2, recs2, 0, 1, [10], None, MR.spec())
    assert out.tobytes() == b"@r1\nACGGACGTAC\n+\nIII#IIIIII\n"


def test_what_the_reference_refuses():
    long1 = (TOH.FRAG * 13)[:513]
    m = MR.spec()

    def records(s1, q1, s2, q2, I, mark=None, spec=m):
        raw1, recs1 = OR.chunk([X, s1], [Q, q1])     # (the pair in front merges)
        raw2, recs2 = OR.chunk([RX, s2], [Q, q2])
        return MR.merge_records(raw1, recs1, 0, raw2, recs2, 0, 2, [10, I], mark, spec)

    for what, s1, q1, s2, q2, I in [
        ("I == L1 + L2", X, Q, RX, Q, 20), ("I beyond it", X, Q, RX, Q, 600),
        ("513 bases in mate 1", long1, b"I" * 513, RX, Q, 10), ("513 bases in mate 2", X, Q, long1, b"I" * 513, 513),
        ("an x in the read region", put(X, 3, b"x"), Q, RX, Q, 10), ("a lower-case base in mate 2", X, Q, put(RX, 0, b"a"), Q, 10),
        ("a quality byte 32", X, put(Q, 9, b" "), RX, Q, 10), ("a quality byte 97", X, Q, RX, put(Q, 0, b"a"), 10),
    ]:
        with pytest.raises(MR.Refused):
            records(s1, q1, s2, q2, I)
    # an insert that is invalid is refused on an unmarked pair too; a bad byte there is not looked at
    with pytest.raises(MR.Refused):
        records(X, Q, RX, Q, 20, mark=[0b01])
    assert records(put(X, 3, b"x"), Q, RX, put(Q, 0, b"a"), 10, mark=[0b01])[1].tolist()[:4] == [2, 2, 1, 10]
    assert records(put(X, 3, b"x"), Q, RX, put(Q, 0, b"a"), 10, spec=MR.spec(2, 11))[1].tolist()[:4] == [2, 2, 0, 0], "too short: not looked at"
    assert records(put(X, 3, b"x"), Q, RX, put(Q, 0, b"a"), 0)[1].tolist()[:4] == [2, 1, 1, 10]
    # the same bytes behind min(L, I) are not looked at
    assert records(b"ACGTxxxxxx", b"IIII      ", b"ACGTzzzzzz", b"5555aaaaaa", 4)[1].tolist()[:4] == [2, 2, 2, 14]
    raw1, recs1 = OR.chunk([X, X])
    raw2, recs2 = OR.chunk([RX, RX])
    for first_a, first_b, count in ((0, 0, 0), (0, 0, 3), (2, 0, 1), (1, 1, 2)):
        with pytest.raises(MR.Refused):
            MR.merge_records(raw1, recs1, first_a, raw2, recs2, first_b, count, [10, 10], None, m)
    for bad in (None, MR.spec(64, 1), MR.spec(2, 0), MR.spec(2, 1024), MR.spec(reserved=(0, 0, 0, 0, 0, 1))):
        with pytest.raises(MR.Refused):
            MR.merge_records(raw1, recs1, 0, raw2, recs2, 0, 2, [10, 10], None, bad)
    with pytest.raises(MR.Refused):
        MR.merge_records(raw1, recs1, 0, raw2, recs2, 0, 2, None, None, m)
    # one chunk on both sides is allowed: nothing is patched
    assert MR.merge_records(raw1, recs1, 0, raw1, recs1, 1, 1, [19], None, m)[1].tolist()[:4] == [1, 1, 1, 19]
    outside = recs1.copy()
    outside[1]["qual_off"] = len(raw1) - 5
    with pytest.raises(MR.Refused):
        MR.merge_records(raw1, outside, 0, raw2, recs2, 0, 2, [10, 10], None, m)
    assert MR.merge_records(raw1, outside, 0, raw2, recs2, 0, 2, [10, 10], [0b01], m)[1].tolist()[:4] == [2, 2, 1, 10], "unmerged: not looked at"


def test_the_fixture_counts(golden, golden_overlap):
    (raw1, recs1), (raw2, recs2) = golden
    summary, _, _, ins = golden_overlap
    with_insert = ins > 0
    assert int(with_insert.sum()) == 111 and int(ins.sum()) == 12767 and (int(ins[with_insert].min()), int(ins.max())) == (32, 170)
    assert int((ins[with_insert] < recs1["len"][with_insert]).sum()) == 36
    out, report, merged = MR.merge_records(raw1, recs1, 0, raw2, recs2, 0, 1000, ins, None, MR.spec())
    assert report.tolist() == [1000, 111, 111, 12767, 32590, 7011, 159, 10, 1211, 1211, 0, 0, 0, 0, 0, 0]
    assert zlib.crc32(out.tobytes()) == 3403808527 and out.size == 32590
    assert np.array_equal(PR.bits(merged, 1000), with_insert)
    # what the words are made of: the header lines of the merged pairs, the overlap summary's words
    heads = PR.header_lines(raw1, recs1)
    assert int(report[MR.BYTES_OUT]) == sum(len(heads[i]) for i in np.flatnonzero(with_insert)) + 2 * 12767 + 4 * 111
    assert int(report[MR.OVERLAP_BASES]) == int(summary[OR.OVERLAP_BASES]) and int(report[MR.DROPPED_A]) == int(summary[OR.BEHIND_A])
    assert int(report[MR.PLACES_DISAGREE]) + int(report[MR.PLACES_N]) == int(summary[OR.MISMATCHES]), "a mismatch is a disagreement or an N"
    # every merged record is a record: four lines, as many qualities as bases, I of each
    lines = out.tobytes().split(b"\n")
    assert lines[-1] == b"" and len(lines) == 4 * 111 + 1
    assert [len(s) for s in lines[1::4]] == ins[with_insert].tolist() == [len(q) for q in lines[3::4]] and set(lines[2::4]) == {b"+"}
    # two ranges add up to the whole
    lo = MR.merge_records(raw1, recs1, 0, raw2, recs2, 0, 391, ins[:391], None, MR.spec())
    hi = MR.merge_records(raw1, recs1, 391, raw2, recs2, 391, 609, ins[391:], None, MR.spec())
    assert (lo[1] + hi[1]).tolist() == report.tolist() and lo[0].tobytes() + hi[0].tobytes() == out.tobytes()
    # min_len and the mark
    assert MR.merge_records(raw1, recs1, 0, raw2, recs2, 0, 1000, ins, None, MR.spec(2, 100))[1].tolist()[:3] == [1000, 111, int((ins >= 100).sum())]
    every_other = np.packbits(np.arange(1000) % 2 == 0, bitorder="little")
    half = MR.merge_records(raw1, recs1, 0, raw2, recs2, 0, 1000, ins, every_other, MR.spec())[1]
    assert int(half[MR.PAIRS_MERGED]) + int(half[MR.PAIRS_UNMARKED]) == 111 and 0 < int(half[MR.PAIRS_MERGED]) < 111


def test_the_merge_composes_with_the_correction(golden, golden_overlap):
    (raw1, recs1), (raw2, recs2) = golden
    ins = golden_overlap[3]
    a, b, creport, _, _ = CR.correct_records(raw1, recs1, 0, raw2, recs2, 0, 1000, ins, CR.spec())
    left = int(creport[CR.MISMATCHES_SEEN]) - int(creport[CR.FIXED_A]) - int(creport[CR.FIXED_B])
    out, report, _ = MR.merge_records(a, recs1, 0, b, recs2, 0, 1000, ins, None, MR.spec())
    assert int(report[MR.PLACES_DISAGREE]) == left - int(report[MR.PLACES_N]) and report.tolist()[:6] == [1000, 111, 111, 12767, 32590, 7011]
    assert (int(report[MR.PLACES_DISAGREE]), int(report[MR.PLACES_N])) == (101, 6)
    plain = MR.merge_records(raw1, recs1, 0, raw2, recs2, 0, 1000, ins, None, MR.spec())
    assert out.tobytes() != plain[0].tobytes() and out.size == plain[0].size
    # the whole restore: 111 merged, 889 pairs in either mate file, and the pairs add up
    out1, out2, merged_out, rep1, rep2, counters, _, creport2, mreport = MR.pair_records_merged(raw1, recs1, raw2, recs2, OR.spec(), MR.spec(),
                                                                                                 overlap=golden_overlap)
    assert counters == dict(pairs=1000, kept=889, dropped_mate1_only=0, dropped_mate2_only=0, dropped_both=0, merged=111) and creport2 is None
    assert merged_out.tobytes() == plain[0].tobytes() and mreport.tolist() == plain[1].tolist()
    assert out1.tobytes().count(b"\n") == 4 * 889 == out2.tobytes().count(b"\n")
    both = MR.pair_records_merged(raw1, recs1, raw2, recs2, OR.spec(), MR.spec(), c=CR.spec(), overlap=golden_overlap)
    assert both[2].tobytes() == out.tobytes() and both[7].tolist() == creport.tolist()


def test_merge_check_on_every_bound(F):
    B = F.binding
    assert B.MERGE_REPORT_WORDS == MR.REPORT_WORDS == 16 and B.MERGE_REPORT_NAMES[MR.PAIRS_TOO_SHORT] == "pairs_too_short"
    assert {"fqgpu_merge_check", "fqgpu_chunk_pair_merge", "fqgpu_dblock_pair_merge"} <= set(B.EXPORTS)
    assert B.read_merge().tolist() == MR.spec().tolist() == [2, 1, 0, 0, 0, 0, 0, 0]
    for m in ((0, 1), (63, 1), (0, 1023), (63, 1023), (2, 1), (2, 512)):
        assert B.merge_check(B.read_merge(*m)) == 0 and MR.check(MR.spec(*m)), m
    for m in ((64, 1), (2, 0), (2, 1024), (1 << 31, 1), (2, 1 << 31), (64, 0)):
        assert B.merge_check(B.read_merge(*m)) == E_ARG and not MR.check(MR.spec(*m)), m
    for k in range(6):
        reserved = [0] * 6
        reserved[k] = 1
        assert B.merge_check(B.read_merge(reserved=reserved)) == E_ARG and not MR.check(MR.spec(reserved=reserved))
    assert B.merge_check(None) == E_ARG


def test_the_device_calls_say_no_device_without_one(F):
    """(with a device in the machine the same calls get as far as their arguments: no handle, FQGPU_E_ARG)"""
    want = E_NO_DEVICE if F.device_count() == 0 else E_ARG
    lib = F.lib()
    p = lambda v: v.ctypes.data_as(C.c_void_p)  # noqa: E731
    report = np.full(16, 7, dtype=np.uint64)
    ins = np.full(5, 7, dtype=np.uint16)
    out, merged = np.full(64, 7, dtype=np.uint8), np.full(1, 7, dtype=np.uint8)
    n = C.c_size_t(7)
    m = MR.spec()
    assert lib.fqgpu_chunk_pair_merge(None, 0, None, 0, 5, p(ins), None, p(m), p(out), 64, C.byref(n), p(report), p(merged)) == want
    assert lib.fqgpu_dblock_pair_merge(None, None, 0, None, 0, 5, p(ins), None, p(m), p(out), 64, C.byref(n), p(report), p(merged)) == want
    assert lib.fqgpu_chunk_pair_merge(None, 0, None, 0, 0, None, None, None, None, 0, None, None, None) == want, "said before any argument is looked at"
    assert lib.fqgpu_dblock_pair_merge(None, None, 0, None, 0, 0, None, None, None, None, 0, None, None, None) == want
    assert (out == 7).all(), "out is never touched"
    if want == E_NO_DEVICE:
        assert (report == 7).all() and (merged == 7).all() and n.value == 7, "nothing is looked at"


# ---------------------------------------------------------------- the farm's host logic, under the sanitizers
MERGE_LINES = ("min_len", "floor_q", "pairs_merged", "bases_merged", "bytes_merged", "merged_overlap_bases", "places_disagree", "places_n",
               "pairs_too_short")


def report_text(o, words, rows, c=None, cwords=None, m=None, mwords=None):
    """the report's text, restated: the overlap's, the correction's six lines, then -- with a merge -- its nine"""
    text = TCH.report_text(o, words, rows, c, cwords)
    if m is not None:
        text += "".join("%s\t%d\n" % (n, v) for n, v in zip(MERGE_LINES, (m[1], m[0], *mwords[2:8], mwords[11])))
    return text


@pytest.fixture(scope="module")
def report_check(F, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("merge_check") / "merge_report_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "merge_report_check.cpp")] + LINK, check=True)
    return exe


def test_the_report_text_with_and_without_a_merge_under_the_sanitizers(report_check, golden, golden_overlap):
    (raw1, recs1), (raw2, recs2) = golden
    out, _, _, ins = golden_overlap
    creport = CR.correct_records(raw1, recs1, 0, raw2, recs2, 0, 1000, ins, CR.spec())[2].tolist()
    mreport = MR.merge_records(raw1, recs1, 0, raw2, recs2, 0, 1000, ins, None, MR.spec())[1].tolist()
    rows = [(int(r), int(out[OR.HEAD + r])) for r in np.flatnonzero(out[OR.HEAD:])]
    big = [9, 9, 2 ** 64 - 1, 2 ** 63, 3, 4, 5, 6, 9, 9, 9, 7, 9, 9, 9, 9]
    cases = [(out[:8].tolist(), rows, (30, 14), creport, (2, 1), mreport), (out[:8].tolist(), rows, None, [0] * 8, (2, 1), mreport),
             (out[:8].tolist(), rows, (30, 14), creport, None, [0] * 16), (out[:8].tolist(), rows, None, [0] * 8, None, [0] * 16),
             ([0] * 8, [], None, [0] * 8, (0, 1), [0] * 16), ([2 ** 63, 1, 2, 3, 4, 5, 6, 7], [(0, 1), (1023, 2 ** 40)], (63, 62), [1] * 8, (63, 1023), big)]
    for words, rws, c, cwords, m, mwords in cases:
        args = ["text", ",".join(str(w) for w in words), *([str(c[0]), str(c[1])] if c else ["0", "0"]), ",".join(str(w) for w in cwords),
                *([str(m[1]), str(m[0])] if m else ["0", "0"]), ",".join(str(w) for w in mwords)] + ["%d:%d" % rw for rw in rws]
        r = subprocess.run([report_check] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "" and r.stdout == report_text((30, 5, 20), words, rws, c, cwords, m, mwords), r.stderr
    text = report_text((30, 5, 20), out[:8].tolist(), rows, (30, 14), creport, (2, 1), mreport)
    assert text.endswith("n_resolved\t4\nmin_len\t1\nfloor_q\t2\npairs_merged\t111\nbases_merged\t12767\nbytes_merged\t32590\n"
                         "merged_overlap_bases\t7011\nplaces_disagree\t159\nplaces_n\t10\npairs_too_short\t0\n")
    assert text.startswith(TCH.report_text((30, 5, 20), out[:8].tolist(), rows, (30, 14), creport)), "the old lines are the old bytes"


def test_the_sum_of_pieces_and_workers_and_the_selection_check_under_the_sanitizers(report_check):
    for args in (["sum", "1"], ["sum", "2"], ["selection"]):
        r = subprocess.run([report_check] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout == "ok\n" and r.stderr == "", r.stdout + r.stderr


def test_the_older_report_checks_still_build_against_the_new_signature(F, tmp_path):
    for name in ("overlap_report_check", "correct_report_check"):
        exe = str(tmp_path / name)
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", name + ".cpp")] + LINK, check=True)
    r = subprocess.run([str(tmp_path / "overlap_report_check"), "text", "30", "5", "20", "1,1,0,0,0,0,0,30", "30:1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == TOH.report_text((30, 5, 20), [1, 1, 0, 0, 0, 0, 0, 30], [(30, 1)])


# ---------------------------------------------------------------- the tool
@pytest.fixture(scope="module")
def tool(F, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("merge_tool") / "fqc_tool")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tools", "fqc_tool.cpp")] + LINK, check=True)
    return exe


MATE = ["--mate", "in2.fqc", "out2.fastq"]
D = ["d", "in.fqc", "out.fastq"]
MERGE = ["--merge", "merged.fastq"]

USAGE_ERRORS = [
    # --merge without --mate, on any command
    D + MERGE, D + MERGE + ["--merge-min-len", "30"], D + ["--min-len", "30"] + MERGE,
    ["c", "in.fastq", "out.fqc"] + MERGE, ["t", "in.fqc"] + MERGE, ["s", "in.fqc", "report.tsv"] + MERGE, ["c", "in.fastq", "out.fqc"] + MATE + MERGE,
    # --merge-min-len and --merge-floor-q without --merge
    D + MATE + ["--merge-min-len", "30"], D + MATE + ["--merge-floor-q", "2"], D + MATE + ["--overlap-trim", "--merge-floor-q", "2"], D + ["--merge-min-len", "30"],
    # a spec the check refuses, words that are no numbers, a missing value
    D + MATE + MERGE + ["--merge-min-len", "0"], D + MATE + MERGE + ["--merge-min-len", "1024"], D + MATE + MERGE + ["--merge-floor-q", "64"],
    D + MATE + MERGE + ["--merge-min-len", "long"], D + MATE + MERGE + ["--merge-floor-q", "-1"], D + MATE + MERGE + ["--merge-floor-q"], D + MATE + ["--merge"],
    # positional cuts have no meaning on a merged read yet
    D + MATE + MERGE + ["--cut-front", "3"], D + MATE + MERGE + ["--cut-tail", "3"], D + MATE + MERGE + ["--crop", "100"], D + MATE + ["--crop", "100", "--trim-q3", "20"] + MERGE,
    # the overlap spec given with it is still checked, and the other options keep their rules beside it
    D + MATE + MERGE + ["--overlap-min", "0"], D + MATE + MERGE + ["--overlap-err", "51"], D + MATE + MERGE + ["--records", "0:5"],
    D + MATE + MERGE + ["--correct-q", "30:14"],
]


@pytest.mark.parametrize("args", USAGE_ERRORS)
def test_usage_errors_are_said_before_any_file_or_device_is_touched(tool, tmp_path, args):
    r = subprocess.run([tool] + args, capture_output=True, text=True, cwd=tmp_path, timeout=60)
    assert r.returncode == 2 and r.stdout == "" and r.stderr, (args, r.stderr)
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("args", [
    D + MATE + MERGE, D + MATE + MERGE + ["--overlap-min", "20", "--overlap-mism", "2", "--overlap-err", "10"],
    D + MATE + MERGE + ["--merge-min-len", "1023", "--merge-floor-q", "0", "--overlap-correct", "--overlap-trim", "--overlap-report", "r.tsv", "--min-len", "40",
                        "--trim-q3", "20"],
])
def test_the_option_alone_is_an_overlap_option(tool, tmp_path, args):
    """(the command gets past its usage checks: what fails is the archive that is not there, or the device -- exit 1)"""
    r = subprocess.run([tool] + args, capture_output=True, text=True, cwd=tmp_path, timeout=60)
    assert r.returncode == 1 and r.stdout == "", (args, r.stderr)
    assert os.listdir(tmp_path) == []


def test_the_usage_text_names_the_options(tool, tmp_path):
    r = subprocess.run([tool], capture_output=True, text=True, cwd=tmp_path, timeout=60)
    assert r.returncode == 2 and "--merge merged.fastq" in r.stderr and "--merge-min-len N" in r.stderr and "--merge-floor-q Q" in r.stderr
