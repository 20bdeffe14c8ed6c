"""The host side of the overlap correction, no GPU: the rule's restatement (tests/correct_ref.py) on hand-made pairs whose
answers are written out by hand, the fixture's counts, fqgpu_correct_check on every bound, the device calls' answer without a
device, the report's text, the word-by-word sum and Selection::check under AddressSanitizer and UBSan
(tests/cpp/correct_report_check.cpp, a stand-alone program), and the tool's usage errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import correct_ref as CR
import oracle_lib as O
import overlap_ref as OR
import test_overlap_host as TOH

ROOT = TOH.ROOT
E_ARG, E_NO_DEVICE = -4, -5
LINK = TOH.LINK
rc = OR.revcomp

# Phred 40, 30 (good_q), 29, 15, 14 (bad_q), 0 as quality bytes
HI, GOOD, GOOD_1, BAD_1, BAD, ZERO = b"I", b"?", b">", b"0", b"/", b"!"
X = b"ACGTACGTAC"
RX = b"GTACGTACGT"   # rc(X): place i of X stands beside place 9 - i; X[3] = 'T' beside RX[6] = 'A'
Q = HI * 10


def put(s, at, c):
    return s[:at] + c + s[at + 1:]


# (what, s1, q1, s2, q2, I, (s1, q1, s2, q2, fixed_a, fixed_b, n_resolved, mismatches_seen, overlap_bases)) at 30:14 --
# every answer worked out by hand; SAME: one place disagrees and nothing changes
SAME = None
HAND = [
    ("nothing disagrees", X, Q, RX, Q, 10, (X, Q, RX, Q, 0, 0, 0, 0, 10)),
    ("mate 2 wins", put(X, 3, b"G"), put(Q, 3, BAD), RX, Q, 10, (X, Q, RX, Q, 1, 0, 0, 1, 10)),
    ("mate 1 wins", X, Q, put(RX, 6, b"C"), put(Q, 6, BAD), 10, (X, Q, RX, Q, 0, 1, 0, 1, 10)),
    ("both are good: neither wins", put(X, 3, b"G"), Q, RX, Q, 10, SAME),
    ("both are poor: neither wins", put(X, 3, b"G"), put(Q, 3, BAD), RX, put(Q, 6, BAD), 10, SAME),
    # the winner's Phred exactly good_q: the loser takes that quality
    ("p2 == good_q", put(X, 3, b"G"), put(Q, 3, BAD), RX, put(Q, 6, GOOD), 10, (X, put(Q, 3, GOOD), RX, put(Q, 6, GOOD), 1, 0, 0, 1, 10)),
    ("p2 == good_q - 1", put(X, 3, b"G"), put(Q, 3, BAD), RX, put(Q, 6, GOOD_1), 10, SAME),
    ("p1 == good_q", X, put(Q, 3, GOOD), put(RX, 6, b"C"), put(Q, 6, ZERO), 10, (X, put(Q, 3, GOOD), RX, put(Q, 6, GOOD), 0, 1, 0, 1, 10)),
    ("p1 == good_q - 1", X, put(Q, 3, GOOD_1), put(RX, 6, b"C"), put(Q, 6, ZERO), 10, SAME),
    ("the loser's p == bad_q", put(X, 3, b"G"), put(Q, 3, BAD), RX, Q, 10, (X, Q, RX, Q, 1, 0, 0, 1, 10)),
    ("the loser's p == bad_q + 1", put(X, 3, b"G"), put(Q, 3, BAD_1), RX, Q, 10, SAME),
    ("mate 2 loses at bad_q + 1", X, Q, put(RX, 6, b"C"), put(Q, 6, BAD_1), 10, SAME),
    ("an N loser in mate 1 is resolved", put(X, 3, b"N"), put(Q, 3, ZERO), RX, Q, 10, (X, Q, RX, Q, 1, 0, 1, 1, 10)),
    ("an N loser in mate 2 is resolved", X, Q, put(RX, 6, b"N"), put(Q, 6, ZERO), 10, (X, Q, RX, Q, 0, 1, 1, 1, 10)),
    ("an N beside a poor base is not", put(X, 3, b"N"), put(Q, 3, ZERO), RX, put(Q, 6, GOOD_1), 10, SAME),
    ("an N beside an N never is", put(X, 3, b"N"), put(Q, 3, ZERO), put(RX, 6, b"N"), Q, 10, SAME),
    ("a confident N does not win", put(X, 3, b"N"), Q, RX, put(Q, 6, ZERO), 10, SAME),
    # X[0] = 'A' beside RX[9] = 'T'
    ("two places of one pair, one each way", put(X, 3, b"G"), put(Q, 3, BAD), put(RX, 9, b"G"), put(Q, 9, ZERO), 10, (X, Q, RX, Q, 1, 1, 0, 2, 10)),
    # d > 0: s1 = TTTT + ACGTAC, r = ACGTAC + GG, s2 = rc(r) = CCGTACGT: d = 4, I = 12, overlap s1[4, 10), i beside j = 11 - i;
    # s1[5] = 'C' beside s2[6] = 'G'.  The poor T in front of the overlap and the poor C of s2 behind it are not looked at
    ("d > 0", b"TTTTAAGTAC", put(put(Q, 5, BAD), 0, ZERO), b"CCGTACGT", put(HI * 8, 0, ZERO), 12,
     (b"TTTTACGTAC", put(Q, 0, ZERO), b"CCGTACGT", put(HI * 8, 0, ZERO), 1, 0, 0, 1, 6)),
    # d < 0, a read-through: s1 = ACGTAC + GG, s2 = rc(ACGTAC) + TT = GTACGTTT: d = -2, I = 6, overlap s1[0, 6), i beside j = 5 - i
    ("d < 0", b"CCGTACGG", put(HI * 8, 0, BAD), b"GTACGTTT", HI * 8, 6, (b"ACGTACGG", HI * 8, b"GTACGTTT", HI * 8, 1, 0, 0, 1, 6)),
    ("d < 0: the bases behind the fragment disagree and stay", b"ACGTACGG", put(HI * 8, 7, ZERO), b"GTACGTTT", put(HI * 8, 7, ZERO), 6,
     (b"ACGTACGG", put(HI * 8, 7, ZERO), b"GTACGTTT", put(HI * 8, 7, ZERO), 0, 0, 0, 0, 6)),
    # mate 2 inside mate 1: s1 = TT + ACGTAC + GG, s2 = rc(ACGTAC): d = 2, I = 8, overlap s1[2, 8), i beside j = 7 - i
    ("mate 2 contained in mate 1", b"TTACGTACGG", Q, b"GTACGA", put(HI * 6, 5, ZERO), 8, (b"TTACGTACGG", Q, b"GTACGT", HI * 6, 0, 1, 0, 1, 6)),
    # ov == 1: I = 1 puts s1[0] beside s2[0]; I = L1 + L2 - 1 puts s1[L1 - 1] beside s2[L2 - 1].  'A' against comp('G') = 'C'
    ("ov == 1 at I = 1", b"ACGT", HI * 4, b"GGGG", ZERO * 4, 1, (b"ACGT", HI * 4, b"TGGG", HI + ZERO * 3, 0, 1, 0, 1, 1)),
    ("ov == 1 at I = L1 + L2 - 1", b"ACGT", ZERO * 4, b"GGGG", HI * 4, 7, (b"ACGC", ZERO * 3 + HI, b"GGGG", HI * 4, 1, 0, 0, 1, 1)),
]


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    F.lib()
    return F


@pytest.fixture(scope="module")
def golden(golden_dir):
    return [O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_%d.fastq" % m)) for m in (1, 2)]


def test_the_rule_on_pairs_made_by_hand():
    assert rc(X) == RX
    for what, s1, q1, s2, q2, I, want in HAND:
        if want is SAME:
            want = (s1, q1, s2, q2, 0, 0, 0, 1, 10)
        assert CR.correct_pair(s1, q1, s2, q2, I, CR.spec()) == want, what
        # ... and through chunks: the same bytes land in the same lines and nothing else moves
        raw1, recs1 = OR.chunk([s1], [q1])
        raw2, recs2 = OR.chunk([X, s2], [Q, q2])
        a, b, report, fa, fb = CR.correct_records(raw1, recs1, 0, raw2, recs2, 1, 1, [I], CR.spec())
        assert a.tobytes() == OR.chunk([want[0]], [want[1]])[0].tobytes() and b.tobytes() == OR.chunk([X, want[2]], [Q, want[3]])[0].tobytes(), what
        assert report.tolist() == [1, 1, int(want[4] + want[5] > 0), *want[4:]] and (int(fa[0]), int(fb[0])) == want[4:6], what
        # a second pass corrects nothing
        again = CR.correct_records(a, recs1, 0, b, recs2, 1, 1, [I], CR.spec())
        assert again[0].tobytes() == a.tobytes() and again[1].tobytes() == b.tobytes() and again[2][2:6].tolist() == [0, 0, 0, 0], what
        assert int(again[2][CR.MISMATCHES_SEEN]) == want[7] - want[4] - want[5], what
    # another pair of levels moves the bounds: at 20:19 a Phred of 29 wins against one of 15
    assert CR.correct_pair(put(X, 3, b"G"), put(Q, 3, BAD_1), RX, put(Q, 6, GOOD_1), 10, CR.spec(20, 19))[:6] == (X, put(Q, 3, GOOD_1), RX, put(Q, 6, GOOD_1), 1, 0)
    # I == 0: nothing is looked at, not even lines that could not be judged
    raw1, recs1 = OR.chunk([b"xxxx", put(X, 3, b"G")], [b"\x7f" * 4, put(Q, 3, BAD)])
    raw2, recs2 = OR.chunk([b"zzzz", RX], [b" " * 4, Q])
    a, b, report, fa, fb = CR.correct_records(raw1, recs1, 0, raw2, recs2, 0, 2, [0, 10], CR.spec())
    assert report.tolist() == [2, 1, 1, 1, 0, 0, 1, 10] and fa.tolist() == [0, 1] and fb.tolist() == [0, 0] and b.tobytes() == raw2.tobytes()
    assert a.tobytes() == OR.chunk([b"xxxx", X], [b"\x7f" * 4, Q])[0].tobytes()


def test_what_the_reference_refuses():
    long1 = (TOH.FRAG * 13)[:513]
    spec = CR.spec()
    for what, s1, q1, s2, q2, I in [
        ("I == L1 + L2", X, Q, RX, Q, 20), ("I beyond it", X, Q, RX, Q, 600),
        ("513 bases in mate 1", long1, HI * 513, RX, Q, 10), ("513 bases in mate 2", X, Q, long1, HI * 513, 513),
        ("an x inside the overlap", put(X, 3, b"x"), Q, RX, Q, 10), ("a lower-case base in mate 2", X, Q, put(RX, 0, b"a"), Q, 10),
        ("a quality byte 32", X, put(Q, 9, b" "), RX, Q, 10), ("a quality byte 97", X, Q, RX, put(Q, 0, b"a"), 10),
    ]:
        with pytest.raises(CR.Refused):
            CR.correct_pair(s1, q1, s2, q2, I, spec)
        raw1, recs1 = OR.chunk([put(X, 3, b"G"), s1], [put(Q, 3, BAD), q1])   # (the pair in front has something to correct)
        raw2, recs2 = OR.chunk([RX, s2], [Q, q2])
        with pytest.raises(CR.Refused):
            CR.correct_records(raw1, recs1, 0, raw2, recs2, 0, 2, [10, I], spec)
    # the same bytes outside the overlap are not looked at: d = 4 leaves s1[0, 4) and s2[0, 2) out
    got = CR.correct_pair(b"xxxxACGTAC", b" " * 4 + HI * 6, b"xxGTACGT", b"aa" + HI * 6, 12, spec)
    assert got[4:] == (0, 0, 0, 0, 6)
    assert CR.correct_pair((TOH.FRAG * 13)[:512], HI * 512, rc((TOH.FRAG * 13)[:512]), HI * 512, 512, spec)[4:] == (0, 0, 0, 0, 512)
    raw1, recs1 = OR.chunk([put(X, 3, b"G"), X], [put(Q, 3, BAD), Q])
    raw2, recs2 = OR.chunk([RX, RX], [Q, Q])
    ins = [10, 10]
    for first_a, first_b, count in ((0, 0, 0), (0, 0, 3), (2, 0, 1), (1, 1, 2)):
        with pytest.raises(CR.Refused):
            CR.correct_records(raw1, recs1, first_a, raw2, recs2, first_b, count, ins, spec)
    for bad in (None, CR.spec(0, 0), CR.spec(64, 14), CR.spec(30, 30), CR.spec(30, 31), CR.spec(reserved=(0, 0, 0, 0, 0, 1))):
        with pytest.raises(CR.Refused):
            CR.correct_records(raw1, recs1, 0, raw2, recs2, 0, 2, ins, bad)
    with pytest.raises(CR.Refused):
        CR.correct_records(raw1, recs1, 0, raw2, recs2, 0, 2, None, spec)
    with pytest.raises(CR.Refused):
        CR.correct_records(raw1, recs1, 0, raw1, recs1, 1, 1, ins, spec)     # one chunk on both sides
    outside = recs1.copy()
    outside[1]["qual_off"] = len(raw1) - 5
    with pytest.raises(CR.Refused):
        CR.correct_records(raw1, outside, 0, raw2, recs2, 0, 2, ins, spec)
    assert CR.correct_records(raw1, outside, 0, raw2, recs2, 0, 2, [10, 0], spec)[2].tolist() == [2, 1, 1, 1, 0, 0, 1, 10], "without an insert it is not looked at"


def test_the_fixture_counts(golden):
    (raw1, recs1), (raw2, recs2) = golden
    summary, _, _, ins = OR.overlap_records(raw1, recs1, 0, raw2, recs2, 0, 1000, OR.spec())
    a, b, report, fa, fb = CR.correct_records(raw1, recs1, 0, raw2, recs2, 0, 1000, ins, CR.spec())
    assert report.tolist() == [1000, 111, 36, 34, 28, int(report[CR.N_RESOLVED]), 169, 7011]
    assert [int(report[i]) for i in (1, 6, 7)] == [int(summary[i]) for i in (1, 6, 7)], "the overlap summary's words"
    assert int(fa.sum()) == 34 and int(fb.sum()) == 28 and int(((fa > 0) | (fb > 0)).sum()) == 36 and not (fa[ins == 0].any() or fb[ins == 0].any())
    # one base byte and one quality byte per correction, and nothing else
    assert int((a != raw1).sum()) == 2 * 34 and int((b != raw2).sum()) == 2 * 28
    # a second pass corrects nothing and sees what is left
    a2, b2, again, fa2, fb2 = CR.correct_records(a, recs1, 0, b, recs2, 0, 1000, ins, CR.spec())
    assert again.tolist() == [1000, 111, 0, 0, 0, 0, 169 - 62, 7011] and a2.tobytes() == a.tobytes() and b2.tobytes() == b.tobytes()
    assert not fa2.any() and not fb2.any()
    # two ranges add up to the whole, and each patches its own records only
    lo = CR.correct_records(raw1, recs1, 0, raw2, recs2, 0, 391, ins[:391], CR.spec())
    hi = CR.correct_records(lo[0], recs1, 391, lo[1], recs2, 391, 609, ins[391:], CR.spec())
    assert (lo[2] + hi[2]).tolist() == report.tolist() and hi[0].tobytes() == a.tobytes() and hi[1].tobytes() == b.tobytes()
    # stricter levels correct less
    strict = CR.correct_records(raw1, recs1, 0, raw2, recs2, 0, 1000, ins, CR.spec(41, 2))[2]
    assert int(strict[CR.FIXED_A]) + int(strict[CR.FIXED_B]) < 62 and int(strict[CR.MISMATCHES_SEEN]) == 169
    # the whole restore: without a trim the outputs are the patched files
    out1, out2, _, _, counters, summary2, creport = CR.pair_records_corrected(raw1, recs1, raw2, recs2, OR.spec(), CR.spec())
    assert out1.tobytes() == a.tobytes() and out2.tobytes() == b.tobytes() and counters["kept"] == 1000
    assert summary2.tolist() == summary.tolist() and creport.tolist() == report.tolist()


def test_correct_check_on_every_bound(F):
    B = F.binding
    assert B.CORRECT_REPORT_WORDS == CR.REPORT_WORDS == 8 and B.CORRECT_REPORT_NAMES[CR.N_RESOLVED] == "n_resolved"
    assert {"fqgpu_correct_check", "fqgpu_chunk_pair_correct", "fqgpu_dblock_pair_correct"} <= set(B.EXPORTS)
    assert B.read_correct().tolist() == CR.spec().tolist() == [30, 14, 0, 0, 0, 0, 0, 0]
    for c in ((1, 0), (63, 62), (63, 0), (30, 14), (2, 1)):
        assert B.correct_check(B.read_correct(*c)) == 0 and CR.check(CR.spec(*c)), c
    for c in ((0, 0), (64, 14), (64, 63), (30, 30), (30, 31), (1, 1), (63, 63), (1 << 31, 0), (30, 1 << 31)):
        assert B.correct_check(B.read_correct(*c)) == E_ARG and not CR.check(CR.spec(*c)), c
    for k in range(6):
        reserved = [0] * 6
        reserved[k] = 1
        assert B.correct_check(B.read_correct(reserved=reserved)) == E_ARG and not CR.check(CR.spec(reserved=reserved))
    assert B.correct_check(None) == E_ARG


def test_the_device_calls_say_no_device_without_one(F):
    """(with a device in the machine the same calls get as far as their arguments: no handle, FQGPU_E_ARG)"""
    want = E_NO_DEVICE if F.device_count() == 0 else E_ARG
    lib = F.lib()
    p = lambda v: v.ctypes.data_as(C.c_void_p)  # noqa: E731
    report = np.full(8, 7, dtype=np.uint64)
    ins, fa, fb = (np.full(5, 7, dtype=np.uint16) for _ in range(3))
    c = CR.spec()
    assert lib.fqgpu_chunk_pair_correct(None, 0, None, 0, 5, p(ins), p(c), p(report), p(fa), p(fb)) == want
    assert lib.fqgpu_dblock_pair_correct(None, None, 0, None, 0, 5, p(ins), p(c), p(report), p(fa), p(fb)) == want
    assert lib.fqgpu_chunk_pair_correct(None, 0, None, 0, 0, None, None, None, None, None) == want, "said before any argument is looked at"
    assert lib.fqgpu_dblock_pair_correct(None, None, 0, None, 0, 0, None, None, None, None, None) == want
    if want == E_NO_DEVICE:
        assert (report == 7).all() and (fa == 7).all() and (fb == 7).all(), "nothing is looked at"


# ---------------------------------------------------------------- the farm's host logic, under the sanitizers
CORRECT_LINES = ("good_q", "bad_q", "pairs_corrected", "bases_corrected_1", "bases_corrected_2", "n_resolved")


def report_text(o, words, rows, c=None, cwords=None):
    """the report's text, restated: the overlap's, then -- with a correction -- its six lines"""
    text = TOH.report_text(o, words, rows)
    if c is not None:
        text += "".join("%s\t%d\n" % (n, v) for n, v in zip(CORRECT_LINES, (c[0], c[1], *cwords[2:6])))
    return text


@pytest.fixture(scope="module")
def report_check(F, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("correct_check") / "correct_report_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "correct_report_check.cpp")] + LINK, check=True)
    return exe


def test_the_report_text_with_and_without_a_correction_under_the_sanitizers(report_check, golden):
    (raw1, recs1), (raw2, recs2) = golden
    out, _, _, ins = OR.overlap_records(raw1, recs1, 0, raw2, recs2, 0, 1000, OR.spec())
    creport = CR.correct_records(raw1, recs1, 0, raw2, recs2, 0, 1000, ins, CR.spec())[2].tolist()
    rows = [(int(r), int(out[OR.HEAD + r])) for r in np.flatnonzero(out[OR.HEAD:])]
    cases = [(out[:8].tolist(), rows, (30, 14), creport), (out[:8].tolist(), rows, None, [0] * 8), ([0] * 8, [], (1, 0), [0] * 8),
             ([2 ** 63, 1, 2, 3, 4, 5, 6, 7], [(0, 1), (1023, 2 ** 40)], (63, 62), [9, 9, 2 ** 64 - 1, 2 ** 63, 3, 4, 9, 9])]
    for words, rws, c, cwords in cases:
        r = subprocess.run([report_check, "text", ",".join(str(w) for w in words), *([str(c[0]), str(c[1])] if c else ["0", "0"]),
                            ",".join(str(w) for w in cwords)] + ["%d:%d" % rw for rw in rws], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "" and r.stdout == report_text((30, 5, 20), words, rws, c, cwords), r.stderr
    text = report_text((30, 5, 20), out[:8].tolist(), rows, (30, 14), creport)
    assert text.endswith("good_q\t30\nbad_q\t14\npairs_corrected\t36\nbases_corrected_1\t34\nbases_corrected_2\t28\nn_resolved\t%d\n" % creport[5])


def test_the_sum_of_pieces_and_workers_and_the_selection_check_under_the_sanitizers(report_check):
    for args in (["sum", "1"], ["sum", "2"], ["selection"]):
        r = subprocess.run([report_check] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout == "ok\n" and r.stderr == "", r.stdout + r.stderr


def test_the_overlap_report_check_still_builds_against_the_new_signature(F, tmp_path):
    exe = str(tmp_path / "overlap_report_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "overlap_report_check.cpp")] + LINK, check=True)
    r = subprocess.run([exe, "text", "30", "5", "20", "1,1,0,0,0,0,0,30", "30:1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == TOH.report_text((30, 5, 20), [1, 1, 0, 0, 0, 0, 0, 30], [(30, 1)])


# ---------------------------------------------------------------- the tool
@pytest.fixture(scope="module")
def tool(F, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("correct_tool") / "fqc_tool")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tools", "fqc_tool.cpp")] + LINK, check=True)
    return exe


MATE = ["--mate", "in2.fqc", "out2.fastq"]
D = ["d", "in.fqc", "out.fastq"]


@pytest.mark.parametrize("args", [
    # --overlap-correct without --mate, on any command
    D + ["--overlap-correct"], D + ["--overlap-correct", "--correct-q", "30:14"], D + ["--min-len", "30", "--overlap-correct"],
    ["c", "in.fastq", "out.fqc", "--overlap-correct"], ["t", "in.fqc", "--overlap-correct"], ["s", "in.fqc", "report.tsv", "--overlap-correct"],
    ["c", "in.fastq", "out.fqc"] + MATE + ["--overlap-correct"],
    # --correct-q without --overlap-correct
    D + MATE + ["--correct-q", "30:14"], D + MATE + ["--overlap-trim", "--correct-q", "30:14"], D + ["--correct-q", "30:14"],
    # a pair the check refuses, words that are no pair of numbers, a missing value
    D + MATE + ["--overlap-correct", "--correct-q", "0:0"], D + MATE + ["--overlap-correct", "--correct-q", "64:14"],
    D + MATE + ["--overlap-correct", "--correct-q", "30:30"], D + MATE + ["--overlap-correct", "--correct-q", "14:30"],
    D + MATE + ["--overlap-correct", "--correct-q", "30"], D + MATE + ["--overlap-correct", "--correct-q", "30:"],
    D + MATE + ["--overlap-correct", "--correct-q", "good:bad"], D + MATE + ["--overlap-correct", "--correct-q"],
    # the overlap spec given with it is still checked, and the other options keep their rules beside it
    D + MATE + ["--overlap-correct", "--overlap-min", "0"], D + MATE + ["--overlap-correct", "--overlap-err", "51"],
    D + MATE + ["--overlap-correct", "--records", "0:5"], D + MATE + ["--overlap-correct", "--crop", "0"],
])
def test_usage_errors_are_said_before_any_file_or_device_is_touched(tool, tmp_path, args):
    r = subprocess.run([tool] + args, capture_output=True, text=True, cwd=tmp_path, timeout=60)
    assert r.returncode == 2 and r.stdout == "" and r.stderr, (args, r.stderr)
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("args", [
    D + MATE + ["--overlap-correct"], D + MATE + ["--overlap-correct", "--overlap-min", "20", "--overlap-mism", "2", "--overlap-err", "10"],
    D + MATE + ["--overlap-correct", "--correct-q", "63:0", "--overlap-trim", "--overlap-report", "r.tsv", "--min-len", "40"],
])
def test_the_option_alone_is_an_overlap_option(tool, tmp_path, args):
    """(the command gets past its usage checks: what fails is the archive that is not there, or the device -- exit 1)"""
    r = subprocess.run([tool] + args, capture_output=True, text=True, cwd=tmp_path, timeout=60)
    assert r.returncode == 1 and r.stdout == "", (args, r.stderr)
    assert os.listdir(tmp_path) == []


def test_the_usage_text_names_the_options(tool, tmp_path):
    r = subprocess.run([tool], capture_output=True, text=True, cwd=tmp_path, timeout=60)
    assert r.returncode == 2 and "--overlap-correct" in r.stderr and "--correct-q GOOD:BAD" in r.stderr
