"""The host side of adapter clipping, no GPU: the reference (tests/adapter_ref.py) on reads worked out by hand, the forms
of the search against each other, fqgpu_adapter_check, the device calls' answer without a device, and the tool's usage errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adapter_ref as AR
import filter_ref as FR
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


# (seq, adapter, min_overlap, pct, the clip place): worked out by hand from the definition
HAND = [
    (b"TTTTTTAGATCGGAAGAGCTTTT", TRUSEQ, 5, 10, 6),      # the adapter whole in the middle
    (b"AGATCGGAAGAGCTTTTTT", TRUSEQ, 5, 10, 0),          # at the very front: the read is emptied
    (b"TTTTTTTTAGATC", TRUSEQ, 5, 10, 8),                # its first five bases at the 3' end
    (b"TTTTTTTTTAGAT", TRUSEQ, 5, 10, 13),               # four of them: below min_overlap, no hit
    (b"AGAT", TRUSEQ, 5, 10, 4),                         # a read shorter than min_overlap
    (b"A", b"A", 1, 0, 0),                               # one base, an adapter of one
    (b"C", b"A", 1, 0, 1),
    (b"CCA", b"A", 1, 0, 2),                             # the shortest read a block takes, an adapter of one
    (b"ACC", b"A", 1, 0, 0),
    (b"CCC", b"A", 1, 0, 3),
    (b"AGA", TRUSEQ, 5, 10, 3),                          # ... shorter than min_overlap
    (b"AGA", TRUSEQ, 3, 0, 0),                           # ... and a prefix of the adapter
    (b"AGATCGG", TRUSEQ, 5, 0, 0),                       # the whole read a prefix of the adapter
    (b"TTAGATCGGTAG", TRUSEQ, 5, 10, 2),                 # ov 10, one mismatch: 100 <= 100
    (b"TTTAGATCGGTA", TRUSEQ, 5, 10, 12),                # ov 9, one mismatch: 100 > 90
    (b"TTAGATNGGAAG", TRUSEQ, 5, 10, 2),                 # an N in the occurrence is the one mismatch allowed
    (b"TTAGATNGGAAG", TRUSEQ, 5, 0, 12),
    (b"TAGATCGCAAGAGCTTAGATCGGAAGAGC", TRUSEQ, 5, 10, 1),  # an earlier hit with a mismatch wins over a later perfect one
    (b"GGGGGGGG", b"GGG", 3, 0, 0),
    (b"ACACACAC", b"CA", 2, 0, 1),
    (b"ACGTACGA", b"AT", 1, 0, 7),                       # min_overlap 1: the last base alone
    (b"ACGTACGT", b"AT", 1, 50, 0),                      # ... and with half the bases wrong allowed: A, C against AT
]


def test_the_reference_on_reads_clipped_by_hand():
    for seq, A, mo, pct, want in HAND:
        for form in (AR.find_serial, AR.find_planes, AR.find):
            assert form(np.frombuffer(seq, dtype=np.uint8), A, mo, pct) == want, (seq, A, mo, pct, form.__name__)


def test_the_three_forms_of_the_search_agree():
    """random reads with planted whole and partial adapters, substitutions and N, adapters of 1 .. 64 bases, at every lead"""
    rng = np.random.default_rng(5)
    hit = partial = 0
    for i in range(1500):
        m = int(rng.choice([1, 2, 5, 13, 31, 32, 33, 63, 64]))
        A = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, m)]
        L = int(rng.choice([1, 4, 15, 16, 17, 40, 100, 130, 257]))
        s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, L)].copy()
        kind = i % 4
        if kind == 1 and L > 1:     # planted somewhere, running over the end or not
            p = int(rng.integers(0, L))
            k = min(m, L - p)
            s[p:p + k] = A[:k]
        if kind >= 2:
            s[rng.random(L) < 0.05] = ord("N")
        if kind == 3 and L > 1:
            p = int(rng.integers(0, L))
            k = min(m, L - p)
            s[p:p + k] = A[:k]
            s[p + int(rng.integers(0, k))] = ord("T")
        mo, pct = int(rng.integers(1, m + 1)), int(rng.choice([0, 10, 20, 50]))
        want = AR.find_serial(s, A.tobytes(), mo, pct)
        assert AR.find(s, A.tobytes(), mo, pct) == want
        assert AR.find_planes(s, A.tobytes(), mo, pct, lead=i % 16) == want
        hit += want < L
        partial += want < L and want + m > L
    assert hit > 500 and partial > 100


def record(name, seq, phred):
    return TH.record(name, seq, phred)


def test_the_clip_is_step_0_of_the_trim():
    # adapter at 10 of 30; Phred 30 but for the two bases in front of the adapter and the first base
    seq = b"ACGTTGCATG" + TRUSEQ + b"TTTTTTT"
    phred = [2] + [30] * 7 + [2, 2] + [30] * 20
    raw = np.frombuffer(record(b"r", seq, phred) + record(b"e", TRUSEQ + b"AC", [30] * 15) + record(b"w", b"ACGTACGTAC", [30] * 10), dtype=np.uint8)
    a = AR.adp(TRUSEQ)
    out, report, keep, win, clip = AR.clip_chunk(raw, a)
    assert clip.tolist() == [10, 0, 10] and win.tolist() == [10 << 16, 0, 10 << 16] and keep.tolist() == [0b101]
    assert out.tobytes() == record(b"r", seq[:10], phred[:10]) + record(b"w", b"ACGTACGTAC", [30] * 10)
    assert [int(x) for x in report] == [3, 2, 55, 20, len(out), 1, 0, 0, 0, 0, 2, 0, 35, 1, 2, 35]
    # the walks run over [f, a - t): the tail walk starts at the clip place and takes the two low bases in front of it
    out, report, keep, win, clip = AR.clip_chunk(raw, a, R.trm(q_front=20, q_tail=20))
    assert win.tolist() == [1 | 7 << 16, 0, 10 << 16]
    assert int(report[R.BASES_CUT_TAIL]) == 22 + 15 and int(report[AR.BASES_CUT_ADAPTER]) == 35
    # cut_tail counts from the clip place, crop from the new front; the filter judges what is left
    out, report, keep, win, clip = AR.clip_chunk(raw, a, R.trm(cut_front=2, cut_tail=3, crop=4), FR.flt(min_len=4))
    assert win.tolist() == [2 | 4 << 16, 0, 2 | 4 << 16] and int(report[R.N_KEPT]) == 2
    assert AR.clip_chunk(raw, a, R.trm(cut_tail=7), FR.flt(min_len=4))[2].tolist() == [0]
    # no adapter: exactly the trim
    t = R.trm(q_tail=20)
    got, want = AR.clip_chunk(raw, None, t), R.trim_chunk(raw, t)
    assert all(np.array_equal(g, w) for g, w in zip(got[:4], want)) and got[4].tolist() == [30, 15, 10]
    # the sequence line is read, and judged over all its bytes, whatever the filter says
    spoilt = raw.copy()
    spoilt[FR.parse(raw)["seq_off"][0] + 29] = ord("a")
    assert R.trim_chunk(spoilt, R.trm())[1][R.N_KEPT] == 3
    with pytest.raises(AR.Refused):
        AR.clip_chunk(spoilt, a)


def test_the_search_over_a_whole_chunk_is_the_search_read_by_read():
    rng = np.random.default_rng(6)
    bases = np.frombuffer(b"ACGTN", dtype=np.uint8)
    for m, mo, pct in ((13, 5, 10), (1, 1, 0), (64, 20, 50), (33, 33, 3)):
        A = bases[rng.integers(0, 4, m)].tobytes()
        seqs = []
        for L in rng.integers(1, 200, 300).tolist():
            s = bases[rng.choice(5, L, p=[0.24, 0.24, 0.24, 0.24, 0.04])].copy()
            if rng.random() < 0.5:
                p = int(rng.integers(0, L))
                s[p:p + min(m, L - p)] = np.frombuffer(A[:min(m, L - p)], dtype=np.uint8)
            seqs.append(s.tobytes())
        raw = np.frombuffer(b"".join(record(b"r%d" % i, s, [30] * len(s)) for i, s in enumerate(seqs)), dtype=np.uint8)
        recs = FR.parse(raw)
        got = AR.find_all(raw, recs["seq_off"].astype(np.int64), recs["len"].astype(np.int64), A, mo, pct)
        assert got.tolist() == [AR.find(np.frombuffer(s, dtype=np.uint8), A, mo, pct) for s in seqs]
        assert 50 < (got < recs["len"]).sum() < 300


GOOD = [dict(seq="A", min_overlap=1), dict(seq="ACGT" * 16, min_overlap=64, max_err_pct=50), dict(seq=TRUSEQ), dict(seq=TRUSEQ, min_overlap=13, max_err_pct=0),
        dict(seq=TRUSEQ, min_overlap=1)]
BAD = [dict(seq="", min_overlap=1), dict(seq="", min_overlap=0), dict(seq="ACGT" * 16 + "A"), dict(seq="ACGT" * 16, length=65), dict(seq="acgtacgt"),
       dict(seq="ACGTAcGT"), dict(seq="ACGTNACGT"), dict(seq="ACGTACGT", length=7), dict(seq="ACGTA\0GT"), dict(seq=TRUSEQ, min_overlap=0),
       dict(seq=TRUSEQ, min_overlap=14), dict(seq=TRUSEQ, max_err_pct=51), dict(seq=TRUSEQ, reserved=1), dict(seq="A", min_overlap=2)]


def test_adapter_check(F):
    B = F.binding
    for kw in GOOD:
        assert B.adapter_check(AR.adp(**kw)) == 0 and AR.check(AR.adp(**kw)), kw
        assert B.read_adapter(**kw).tolist() == AR.adp(**kw).tolist()
    for kw in BAD:
        assert B.adapter_check(AR.adp(**kw)) == E_ARG and not AR.check(AR.adp(**kw)), kw
    assert AR.check(AR.adp(TRUSEQ, max_err_pct=50)) and B.adapter_check(AR.adp(TRUSEQ, max_err_pct=50)) == 0
    assert F.lib().fqgpu_adapter_check(None) == E_ARG
    assert B.read_adapter("ACGTAC").tolist() == AR.adp(b"ACGTAC", 5, 10).tolist(), "the defaults: overlap 5, 10 percent"
    assert B.ADAPTER_MAX == AR.ADAPTER_MAX and B.read_adapter("A").nbytes == 80
    assert B.CLIP_REPORT_NAMES[:14] == B.TRIM_REPORT_NAMES and B.CLIP_REPORT_NAMES[14:] == ("reads_with_adapter", "bases_cut_adapter")
    assert len(B.TRIM_REPORT_NAMES) == 14, "the trim's names are as they were"
    assert {"fqgpu_adapter_check", "fqgpu_chunk_clip", "fqgpu_dblock_clip"} <= set(B.EXPORTS)


def test_the_device_calls_say_no_device_without_one(F):
    """(with a device in the machine the same calls get as far as their arguments: no handle, FQGPU_E_ARG)"""
    want = E_NO_DEVICE if F.device_count() == 0 else E_ARG
    lib = F.lib()
    a, t, f = AR.adp(TRUSEQ), R.trm(q_tail=20), FR.flt()
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    report = np.full(R.REPORT_WORDS, 7, dtype=np.uint64)
    n = C.c_size_t(7)
    assert lib.fqgpu_chunk_clip(None, p(a), p(t), p(f), None, 0, C.byref(n), p(report), None, None) == want
    assert lib.fqgpu_dblock_clip(None, None, p(a), p(t), None, None, 0, C.byref(n), p(report), None, None) == want
    assert lib.fqgpu_chunk_clip(None, None, None, None, None, 0, None, None, None, None) == want, "said before any argument is looked at"
    assert lib.fqgpu_dblock_clip(None, None, None, None, None, None, 0, None, None, None, None) == want
    if want == E_NO_DEVICE:
        assert n.value == 7 and (report == 7).all(), "nothing is looked at"


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("adapter_tool") / "fqc_tool")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tools", "fqc_tool.cpp"),
                    "-L" + os.path.join(ROOT, "fqcomp28_amd"), "-lfqgpu", "-Wl,-rpath," + os.path.join(ROOT, "fqcomp28_amd"),
                    "-lpthread"], check=True)
    return exe


ADAPTER = ["--adapter", "AGATCGGAAGAGC"]


@pytest.mark.parametrize("args", [
    # an adapter option on any command but d
    ["c", "in.fastq", "out.fqc"] + ADAPTER,
    ["x", "in.fqc"] + ADAPTER,
    ["t", "in.fqc"] + ADAPTER,
    ["s", "in.fqc", "report.tsv"] + ADAPTER,
    # ... together with --records, --fasta, --index, --index-stride, alone and beside trim and filter options
    *[["d", "in.fqc", "out.fastq"] + ADAPTER + other for other in (["--records", "0:5"], ["--fasta"], ["--index"], ["--index-stride", "64"])],
    ["d", "in.fqc", "out.fastq", "--records", "0:5", "--trim-q3", "20"] + ADAPTER,
    ["d", "in.fqc", "out.fastq", "--min-len", "20"] + ADAPTER + ["--fasta"],
    ["d", "in.fqc", "out.fastq", "--fasta", "--adapter-overlap", "3"],
    # adapters fqgpu_adapter_check refuses
    ["d", "in.fqc", "out.fastq", "--adapter", ""],
    ["d", "in.fqc", "out.fastq", "--adapter", "ACGT" * 16 + "A"],
    ["d", "in.fqc", "out.fastq", "--adapter", "agatcggaagagc"],
    ["d", "in.fqc", "out.fastq", "--adapter", "AGATNGGAAGAGC"],
    ["d", "in.fqc", "out.fastq", "--adapter", "AGAT-GGAAGAGC"],
    ["d", "in.fqc", "out.fastq"] + ADAPTER + ["--adapter-overlap", "0"],
    ["d", "in.fqc", "out.fastq"] + ADAPTER + ["--adapter-err", "51"],
    ["d", "in.fqc", "out.fastq", "--trim-q3", "20", "--min-len", "20"] + ADAPTER + ["--adapter-err", "51"],
    # a trim or a filter its check refuses beside a good adapter
    ["d", "in.fqc", "out.fastq"] + ADAPTER + ["--crop", "0"],
    ["d", "in.fqc", "out.fastq"] + ADAPTER + ["--min-mean-q", "64"],
    # the other adapter options without an adapter; malformed and missing values
    ["d", "in.fqc", "out.fastq", "--adapter-overlap", "5"],
    ["d", "in.fqc", "out.fastq", "--adapter-err", "10"],
    ["d", "in.fqc", "out.fastq"] + ADAPTER + ["--adapter-overlap", "x"],
    ["d", "in.fqc", "out.fastq"] + ADAPTER + ["--adapter-err", "2.5"],
    ["d", "in.fqc", "out.fastq"] + ADAPTER + ["--adapter-err", "-1"],
    ["d", "in.fqc", "out.fastq"] + ADAPTER + ["--adapter-overlap"],
    ["d", "in.fqc", "out.fastq", "--adapter"],
])
def test_usage_errors_are_said_before_any_file_or_device_is_touched(tool, tmp_path, args):
    r = subprocess.run([tool] + args, capture_output=True, text=True, cwd=tmp_path, timeout=60)
    assert r.returncode == 2 and r.stdout == "" and r.stderr, (args, r.stderr)
    assert os.listdir(tmp_path) == []
