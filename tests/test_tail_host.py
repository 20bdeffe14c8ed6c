"""The host side of the tail trims, no GPU: the reference (tests/tail_ref.py) on reads worked out by hand for every clause of
the poly rule and of the window rule, its two forms against each other, fqgpu_tail_check, the device calls' answer without a
device, and the tool's usage errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adapter_ref as AR
import filter_ref as FR
import tail_ref as TR
import test_trim_host as TH
import trim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_NO_DEVICE = -4, -5
TRUSEQ = b"AGATCGGAAGAGC"


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    F.lib()
    return F


def tail_of(*parts):
    """a 3' end from its parts in TAIL order (the read's last base first): the bytes as they stand in the read"""
    return b"".join(parts)[::-1]


FRONT = b"ACGTACGTACCATT"      # its last two bases T, T are two mismatches in a row for every tail of G that reaches them
G = TR.tl("G")                 # the tool's defaults: at least 10, one mismatch per 8, at most 5
G5 = TR.tl("G", poly_min_len=5)

# (what is checked, sequence line, tail, a1): worked out by hand from the definition; a0 is the read's length
POLY_HAND = [
    ("a clean tail of exactly poly_min_len", FRONT + b"G" * 10, G, len(FRONT)),
    ("... and of one less", FRONT + b"G" * 9, G, len(FRONT) + 9),
    ("a mismatch at tail place 7 ends the tail: 1 > 7 / 8", FRONT + tail_of(b"G" * 6, b"A", b"G" * 20), G5, len(FRONT) + 21),
    ("... so that it is too short", FRONT + tail_of(b"G" * 6, b"A", b"G" * 20), G, len(FRONT) + 27),
    ("a mismatch at place 8 is allowed: 1 <= 8 / 8", FRONT + tail_of(b"G" * 7, b"A", b"G" * 4), G, len(FRONT)),
    ("an N is a mismatch: at place 8 allowed", FRONT + tail_of(b"G" * 7, b"N", b"G" * 4), G, len(FRONT)),
    ("... at place 3 not", FRONT + tail_of(b"G" * 2, b"N", b"G" * 20), TR.tl("G", poly_min_len=1), len(FRONT) + 21),
    ("a second mismatch at place 12, before 16: the tail ends in front of it", FRONT + tail_of(b"G" * 7, b"A", b"G" * 3, b"A", b"G" * 9), G, len(FRONT) + 10),
    ("a second mismatch at place 16 is allowed", FRONT + tail_of(b"G" * 7, b"A", b"G" * 7, b"A", b"G" * 4), G, len(FRONT)),
    ("the cap poly_max_mism = 1 refuses it", FRONT + tail_of(b"G" * 7, b"A", b"G" * 7, b"A", b"G" * 4), TR.tl("G", poly_max_mism=1), len(FRONT) + 5),
    ("poly_max_mism = 0: no mismatch anywhere", FRONT + tail_of(b"G" * 11, b"A", b"G" * 4), TR.tl("G", poly_max_mism=0), len(FRONT) + 5),
    ("a tail does not start again behind a violation", FRONT + tail_of(b"G" * 3, b"AA", b"G" * 30), TR.tl("G", poly_min_len=1), len(FRONT) + 32),
    ("... however long the run behind it is", FRONT + tail_of(b"G" * 3, b"AA", b"G" * 30), G, len(FRONT) + 35),
    ("the outermost base is not X: violated at place 1", FRONT + tail_of(b"A", b"G" * 30), TR.tl("G", poly_min_len=1), len(FRONT) + 31),
    ("the cut begins with an X: the allowed mismatches at the inner end stay", b"CC" + tail_of(b"G" * 15, b"A", b"T"), G, 4),
    ("a read that is all tail", b"G" * 40, G, 0),
    ("a tail of another base is not looked for", FRONT + b"A" * 20, G, len(FRONT) + 20),
]


def test_the_poly_rule_clause_by_clause():
    for what, seq, x, a1 in POLY_HAND:
        assert len(seq) - TR.poly_serial(seq, len(seq), x) == a1, what
        raw = np.frombuffer(TH.record(b"r", seq, [30] * len(seq)), dtype=np.uint8)
        out, report, keep, win, places = TR.tail_chunk(raw, None, x)
        assert places.tolist() == [[len(seq), a1, a1, a1]] and win.tolist() == [a1 << 16 if a1 else 0], what
        assert [int(v) for v in report[16:]] == [a1 < len(seq), len(seq) - a1, 0, 0, 0, 0, 0, 0], what
        assert int(report[R.BASES_CUT_TAIL]) == len(seq) - a1 and int(report[R.READS_EMPTIED]) == (a1 == 0), what


def test_poly_x_takes_the_longest_of_four():
    """only the base the read ends with can have a tail (any other has its mismatch at place 1), so the longest of the four IS
    that one's"""
    every = TR.tl("ACGT")
    for c in b"ACGT":
        other = b"A" if c != ord("A") else b"C"
        seq = other * 5 + tail_of(bytes([c]) * 7, other, bytes([c]) * 9)
        want = [TR.poly_serial_base(seq, len(seq), X, 10, 8, 5) for X in b"ACGT"]
        assert sorted(want) == [0, 0, 0, 17] and TR.poly_serial(seq, len(seq), every) == 17
        assert TR.poly_serial(seq, len(seq), TR.tl(chr(c))) == 17
        assert TR.poly_serial(seq, len(seq), TR.tl("ACGT".replace(chr(c), ""))) == 0
    assert TR.poly_serial(b"ACGTNNNNNNNNNNNNNN", 18, every) == 0, "N is no base of the set"


def test_the_poly_tail_stands_behind_the_clip():
    # the adapter at 20; in front of it twelve G: a0 = 20, a1 = 8
    seq = b"ACTACTAC" + b"G" * 12 + TRUSEQ + b"GGGGGGGGGGGG"
    raw = np.frombuffer(TH.record(b"r", seq, [30] * len(seq)) + TH.record(b"e", TRUSEQ + b"GG", [30] * 15), dtype=np.uint8)
    out, report, keep, win, places = TR.tail_chunk(raw, AR.adp(TRUSEQ), G)
    assert places.tolist() == [[20, 8, 8, 8], [0, 0, 0, 0]], "a0 = 0: nothing to walk over"
    assert [int(v) for v in report[14:20]] == [2, len(seq) - 20 + 15, 1, 12, 0, 0] and keep.tolist() == [0b01]
    assert out.tobytes() == TH.record(b"r", seq[:8], [30] * 8)
    # without the adapter the walk starts at the read's end: twelve G, the adapter's last base C (one mismatch in 13), its G
    assert TR.tail_chunk(raw, None, G)[4].tolist() == [[45, 31, 31, 31], [15, 15, 15, 15]]


W4 = TR.tl(window_len=4, window_q=20)


def test_the_window_rule_clause_by_clause():
    S = TR.window_serial
    assert S([2, 2, 2], 0, 3, 4, 20) == 3, "e - f < W: no window, nothing is cut"
    assert S([2, 2, 2, 2], 0, 4, 4, 20) == 0
    p = [30] * 12 + [2, 2] + [30] * 6
    assert S(p, 0, 20, 4, 20) == 12, "the window at 10 fails (30 30 2 2); its two good bases are kept"
    assert S(p, 0, 20, 4, 17) == 12, "64 < 4 * 17: the same window"
    assert S(p, 0, 20, 4, 16) == 20, "64 is not below 4 * 16: no window fails"
    assert S([30, 30, 19, 30, 5], 0, 5, 1, 20) == 2, "W = 1: the first base below Q"
    assert S([30, 30, 20, 30, 20], 0, 5, 1, 20) == 5
    last = [30] * 7 + [2]
    assert S(last, 0, 8, 4, 24) == 7, "only the last window fails, with its last byte: 92 < 96"
    assert S(last, 0, 8, 4, 23) == 8, "92 is not below 92"
    # the fixed cuts come first: a drop inside them is not seen
    p = [2, 2, 2] + [30] * 20 + [2, 2]
    assert S(p, 0, 25, 4, 20) == 0 and S(p, 3, 25, 4, 20) == 23 and S(p, 3, 23, 4, 20) == 23 and S(p, 2, 23, 4, 20) == 23 and S(p, 1, 23, 4, 20) == 1
    raw = np.frombuffer(TH.record(b"r", b"ACGTA" * 5, p), dtype=np.uint8)
    for t, places, win in ((R.trm(), [25, 25, 25, 0], 0), (R.trm(cut_front=3), [25, 25, 25, 23], 3 | 20 << 16),
                           (R.trm(cut_front=3, cut_tail=2), [25, 25, 23, 23], 3 | 20 << 16), (R.trm(cut_front=1, cut_tail=2), [25, 25, 23, 1], 0),
                           (R.trm(cut_front=3, cut_tail=2, crop=7), [25, 25, 23, 23], 3 | 7 << 16)):
        out, report, keep, w, pl = TR.tail_chunk(raw, None, W4, t)
        assert pl.tolist() == [places] and w.tolist() == [win], t
        assert [int(v) for v in report[16:20]] == [0, 0, places[3] < places[2], places[2] - places[3]]
    # the running-sum walks run over [f, e2)
    p = [30] * 10 + [18, 18, 30, 30, 2, 2, 2, 2, 30, 30]
    raw = np.frombuffer(TH.record(b"r", b"ACGTA" * 4, p), dtype=np.uint8)
    assert TR.tail_chunk(raw, None, W4)[4].tolist() == [[20, 20, 20, 14]]
    assert TR.tail_chunk(raw, None, W4, R.trm(q_tail=20))[3].tolist() == [14 << 16], "30 30 at the end of [0, 14) stop the walk at once"
    assert TR.tail_chunk(raw, None, TR.tl(window_len=4, window_q=25), R.trm(q_tail=20))[3].tolist() == [10 << 16], "e2 = 10: the window at 8"
    assert R.trim_chunk(raw, R.trm(q_tail=20))[3].tolist() == [20 << 16], "the running sum alone keeps it all: 30 30 at the end"


def test_both_rules_at_once_and_the_filter():
    # a G tail of 12 with high qualities; in front of it a quality drop
    seq = b"ACTACTACTAACTACTACTACTCA" + b"G" * 12
    p = [30] * 16 + [3] * 8 + [35] * 12
    raw = np.frombuffer(TH.record(b"r", seq, p) + TH.record(b"s", b"ACTGACTGAC", [30] * 10), dtype=np.uint8)
    x = TR.tl("G", window_len=4, window_q=20)
    out, report, keep, win, places = TR.tail_chunk(raw, None, x, None, FR.flt(min_len=12))
    assert places.tolist() == [[36, 24, 24, 16], [10, 10, 10, 10]] and keep.tolist() == [0b01]
    assert [int(v) for v in report[:20]] == [2, 1, 46, 16, len(out), 1, 0, 0, 0, 0, 1, 0, 20, 0, 0, 0, 1, 12, 1, 8]
    assert out.tobytes() == TH.record(b"r", seq[:16], p[:16])
    # a tail with both rules off, or none: the clip's results, eight zero words behind them
    for off in (None, TR.tl()):
        got, want = TR.tail_chunk(raw, AR.adp(TRUSEQ), off, R.trm(q_tail=20)), AR.clip_chunk(raw, AR.adp(TRUSEQ), R.trm(q_tail=20))
        assert all(np.array_equal(g, w) for g, w in zip((got[0], got[1][:16], got[2], got[3]), want[:4])) and not got[1][16:].any()
    with pytest.raises(TR.Refused):
        TR.tail_chunk(raw, None, None)
    # the lines that are read are judged over all their bytes
    spoilt = raw.copy()
    spoilt[FR.parse(raw)["seq_off"][0] + 35] = ord("g")
    assert TR.tail_chunk(spoilt, None, W4)[1][R.N_KEPT] == 2, "the window alone does not read the sequence line"
    with pytest.raises(TR.Refused):
        TR.tail_chunk(spoilt, None, G)
    spoilt = raw.copy()
    spoilt[FR.parse(raw)["qual_off"][0] + 35] = 32
    assert TR.tail_chunk(spoilt, None, G)[1][R.N_KEPT] == 2, "the poly rule alone does not read the quality line"
    with pytest.raises(TR.Refused):
        TR.tail_chunk(spoilt, None, W4)


def test_the_two_forms_of_the_reference_agree_on_random_reads():
    rng = np.random.default_rng(8)
    bases = np.frombuffer(b"ACGTN", dtype=np.uint8)
    tails = cuts = 0
    for trial in range(12):
        seqs, phreds = [], []
        for L in rng.integers(1, 120, 150).tolist():
            s = bases[rng.choice(5, L, p=[0.24, 0.24, 0.24, 0.24, 0.04])].copy()
            k = int(rng.integers(0, 40))
            if k and rng.random() < 0.7:        # a tail of one base with errors in it
                tail = np.full(min(k, L), bases[rng.integers(0, 4)])
                tail[rng.random(tail.size) < 0.08] = bases[rng.integers(0, 5)]
                s[L - tail.size:] = tail
            seqs.append(s.tobytes())
            q = rng.integers(15, 41, L)
            if rng.random() < 0.6:
                at = int(rng.integers(0, L))
                q[at:at + int(rng.integers(1, 12))] = rng.integers(0, 12)
            phreds.append(q)
        raw = np.frombuffer(b"".join(TH.record(b"r%d" % i, s, q) for i, (s, q) in enumerate(zip(seqs, phreds))), dtype=np.uint8)
        recs = FR.parse(raw)
        lens, so, qo = recs["len"].astype(np.int64), recs["seq_off"].astype(np.int64), recs["qual_off"].astype(np.int64)
        x = TR.tl(int(rng.integers(1, 16)), int(rng.integers(1, 15)), int(rng.integers(2, 12)), int(rng.integers(0, 6)))
        a0 = np.maximum(lens - rng.integers(0, 8, lens.size), 0)
        got = TR.poly_all(raw, so, a0, x)
        assert got.tolist() == [TR.poly_serial(s, int(a), x) for s, a in zip(seqs, a0)]
        tails += int((got > 0).sum())
        W, Q = int(rng.choice([1, 2, 4, 7, 16, 32])), int(rng.integers(5, 35))
        f = np.minimum(rng.integers(0, 6, lens.size), lens)
        e = lens - np.minimum(rng.integers(0, 6, lens.size), lens - f)
        got = TR.window_all(raw, qo, f, e, W, Q)
        assert got.tolist() == [TR.window_serial(q, int(a), int(b), W, Q) for q, a, b in zip(phreds, f, e)]
        cuts += int((got < e).sum())
    assert tails > 100 and cuts > 100, (tails, cuts)


P20 = [30] * 12 + [2, 2] + [30] * 6
P25 = [2, 2, 2] + [30] * 20 + [2, 2]
# (Phred values, the trim's fixed cuts, W, Q, e2): the rows above, for the device tests as well; none shorter than three bases
WINDOW_HAND = [([2, 2, 2], {}, 4, 20, 3), ([2, 2, 2, 2], {}, 4, 20, 0), (P20, {}, 4, 20, 12), (P20, {}, 4, 17, 12), (P20, {}, 4, 16, 20),
               ([30, 30, 19, 30, 5], {}, 1, 20, 2), ([30, 30, 20, 30, 20], {}, 1, 20, 5), ([30] * 7 + [2], {}, 4, 24, 7), ([30] * 7 + [2], {}, 4, 23, 8),
               (P25, {}, 4, 20, 0), (P25, dict(cut_front=3), 4, 20, 23), (P25, dict(cut_front=3, cut_tail=2), 4, 20, 23),
               (P25, dict(cut_front=2, cut_tail=2), 4, 20, 23), (P25, dict(cut_front=1, cut_tail=2), 4, 20, 1),
               ([30] * 40 + [10] * 3 + [30] * 10, {}, 32, 29, 40), ([30] * 40 + [10] * 3 + [30] * 10, {}, 32, 28, 53)]


def test_the_window_rows_for_the_device_tests():
    for phred, cuts, W, Q, e2 in WINDOW_HAND:
        raw = np.frombuffer(TH.record(b"r", (b"ACGTA" * 11)[:len(phred)], phred), dtype=np.uint8)
        places = TR.tail_chunk(raw, None, TR.tl(window_len=W, window_q=Q), R.trm(**cuts))[4]
        assert places[0, 3] == e2 and TR.window_serial(phred, int(min(cuts.get("cut_front", 0), len(phred))), int(places[0, 2]), W, Q) == e2, (phred, cuts, W, Q)


GOOD = [dict(), dict(poly="G"), dict(poly="ACGT", poly_min_len=1, poly_every=2, poly_max_mism=0), dict(poly=15, poly_min_len=65535, poly_every=255, poly_max_mism=255),
        dict(window_len=1, window_q=1), dict(window_len=32, window_q=64), dict(poly="T", window_len=4, window_q=20), dict(poly_max_mism=255)]
BAD = [dict(poly=16), dict(poly="G", poly_min_len=0), dict(poly="G", poly_min_len=65536), dict(poly="G", poly_every=1), dict(poly="G", poly_every=0),
       dict(poly="G", poly_every=256), dict(poly="G", poly_max_mism=256), dict(poly_min_len=10), dict(poly_every=8), dict(poly_max_mism=256),
       dict(window_len=33, window_q=20), dict(window_len=4, window_q=0), dict(window_len=4, window_q=65), dict(window_q=20),
       dict(reserved=(1, 0)), dict(poly="G", reserved=(0, 1))]


def test_tail_check(F):
    B = F.binding
    for kw in GOOD:
        assert B.tail_check(TR.tl(**kw)) == 0 and TR.check(TR.tl(**kw)), kw
        assert B.read_tail(**kw).tolist() == TR.tl(**kw).tolist()
    for kw in BAD:
        assert B.tail_check(TR.tl(**kw)) == E_ARG and not TR.check(TR.tl(**kw)), kw
    assert F.lib().fqgpu_tail_check(None) == E_ARG
    assert B.read_tail("G").tolist() == [4, 10, 8, 5, 0, 0, 0, 0], "the defaults: at least 10, one per 8, at most 5"
    assert B.read_tail().nbytes == 32 and not B.read_tail().any()
    assert B.TAIL_REPORT_WORDS == TR.REPORT_WORDS == 24
    assert B.TAIL_REPORT_NAMES[:16] == B.CLIP_REPORT_NAMES
    assert B.TAIL_REPORT_NAMES[16:] == ("reads_with_poly_tail", "bases_cut_poly", "reads_window_cut", "bases_cut_window")
    assert len(B.CLIP_REPORT_NAMES) == 16, "the clip's names are as they were"
    assert {"fqgpu_tail_check", "fqgpu_chunk_tailtrim", "fqgpu_dblock_tailtrim"} <= set(B.EXPORTS)


def test_the_device_calls_say_no_device_without_one(F):
    """(with a device in the machine the same calls get as far as their arguments: no handle, FQGPU_E_ARG)"""
    want = E_NO_DEVICE if F.device_count() == 0 else E_ARG
    lib = F.lib()
    a, x, t, f = AR.adp(TRUSEQ), TR.tl("G", window_len=4, window_q=20), R.trm(q_tail=20), FR.flt()
    p = lambda v: v.ctypes.data_as(C.c_void_p)  # noqa: E731
    report = np.full(TR.REPORT_WORDS, 7, dtype=np.uint64)
    n = C.c_size_t(7)
    assert lib.fqgpu_chunk_tailtrim(None, p(a), p(x), p(t), p(f), None, 0, C.byref(n), p(report), None, None, None) == want
    assert lib.fqgpu_dblock_tailtrim(None, None, p(a), p(x), p(t), None, None, 0, C.byref(n), p(report), None, None, None) == want
    assert lib.fqgpu_chunk_tailtrim(None, None, None, None, None, None, 0, None, None, None, None, None) == want, "said before any argument is looked at"
    assert lib.fqgpu_dblock_tailtrim(None, None, None, None, None, None, None, 0, None, None, None, None, None) == want
    if want == E_NO_DEVICE:
        assert n.value == 7 and (report == 7).all(), "nothing is looked at"


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tail_tool") / "fqc_tool")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tools", "fqc_tool.cpp"),
                    "-L" + os.path.join(ROOT, "fqcomp28_amd"), "-lfqgpu", "-Wl,-rpath," + os.path.join(ROOT, "fqcomp28_amd"),
                    "-lpthread"], check=True)
    return exe


POLY, WINDOW = ["--poly-g"], ["--window", "4:20"]


@pytest.mark.parametrize("args", [
    # a tail option on any command but d
    *[[cmd, "in", "out"] + opt for cmd in ("c", "s") for opt in (POLY, WINDOW, ["--poly-x", "12"])],
    *[[cmd, "in.fqc"] + opt for cmd in ("x", "t") for opt in (POLY, WINDOW)],
    # ... together with --records, --fasta, --index, --index-stride, alone and beside the other options
    *[["d", "in.fqc", "out.fastq"] + opt + other for opt in (POLY, WINDOW)
      for other in (["--records", "0:5"], ["--fasta"], ["--index"], ["--index-stride", "64"])],
    ["d", "in.fqc", "out.fastq", "--records", "0:5", "--trim-q3", "20", "--adapter", "AGATCGGAAGAGC"] + POLY,
    ["d", "in.fqc", "out.fastq", "--fasta", "--poly-every", "4"],
    # values fqgpu_tail_check refuses
    ["d", "in.fqc", "out.fastq", "--poly-g", "0"],
    ["d", "in.fqc", "out.fastq", "--poly-x", "65536"],
    ["d", "in.fqc", "out.fastq"] + POLY + ["--poly-every", "1"],
    ["d", "in.fqc", "out.fastq"] + POLY + ["--poly-every", "256"],
    ["d", "in.fqc", "out.fastq", "--poly-x", "--poly-mism", "256"],
    ["d", "in.fqc", "out.fastq", "--window", "33:20"],
    ["d", "in.fqc", "out.fastq", "--window", "0:20"],
    ["d", "in.fqc", "out.fastq", "--window", "4:0"],
    ["d", "in.fqc", "out.fastq", "--window", "4:65"],
    ["d", "in.fqc", "out.fastq", "--min-len", "20", "--trim-q3", "20"] + POLY + ["--window", "4:65"],
    # an adapter, a trim or a filter its check refuses beside good tail options
    ["d", "in.fqc", "out.fastq"] + POLY + WINDOW + ["--crop", "0"],
    ["d", "in.fqc", "out.fastq"] + POLY + ["--min-mean-q", "64"],
    ["d", "in.fqc", "out.fastq"] + WINDOW + ["--adapter", "agatc"],
    # the other poly options without a set; malformed and missing values
    ["d", "in.fqc", "out.fastq", "--poly-every", "8"],
    ["d", "in.fqc", "out.fastq", "--poly-mism", "2"],
    ["d", "in.fqc", "out.fastq"] + WINDOW + ["--poly-mism", "2"],
    ["d", "in.fqc", "out.fastq", "--poly-g", "x"],
    ["d", "in.fqc", "out.fastq", "--poly-g", "2.5"],
    ["d", "in.fqc", "out.fastq"] + POLY + ["--poly-every", "x"],
    ["d", "in.fqc", "out.fastq"] + POLY + ["--poly-mism", "-1"],
    ["d", "in.fqc", "out.fastq"] + POLY + ["--poly-every"],
    ["d", "in.fqc", "out.fastq", "--window", "4"],
    ["d", "in.fqc", "out.fastq", "--window", "4:"],
    ["d", "in.fqc", "out.fastq", "--window", ":20"],
    ["d", "in.fqc", "out.fastq", "--window", "4:2.0"],
    ["d", "in.fqc", "out.fastq", "--window"],
])
def test_usage_errors_are_said_before_any_file_or_device_is_touched(tool, tmp_path, args):
    r = subprocess.run([tool] + args, capture_output=True, text=True, cwd=tmp_path, timeout=60)
    assert r.returncode == 2 and r.stdout == "" and r.stderr, (args, r.stderr)
    assert os.listdir(tmp_path) == []
