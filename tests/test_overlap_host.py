"""The host side of the mate overlap, no GPU: the rule's restatement (tests/overlap_ref.py) on hand-made pairs whose answers
are written out by hand, the fixture's counts, fqgpu_overlap_check, fqgpu_overlap_merge and the fingerprint word, the limit's
restatement against the marked reference, the device calls' answer without a device, the farm's merge and the report's
text under AddressSanitizer and UBSan (tests/cpp/overlap_report_check.cpp, a stand-alone program), and the tool's usage errors."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

import adapter_ref as AR
import filter_ref as FR
import oracle_lib as O
import overlap_ref as OR
import pair_ref as PR
import trim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_NO_DEVICE = -4, -5
LINK = ["-L" + os.path.join(ROOT, "fqcomp28_amd"), "-lfqgpu", "-Wl,-rpath," + os.path.join(ROOT, "fqcomp28_amd"), "-lpthread"]

# forty bases without a repeat worth speaking of, its halves, and twenty more
FRAG = b"ACGGTCATTGCAGGATCCTAAGCTTGACCGTATGCAATCG"
HEAD30, TAIL30 = b"TTGACGCATAGGCTAACGTCCATGGATACC", b"GGCATTCAGTCCAAGTTGCAGATCGTACCA"
MORE20 = b"CTAGGTCAATGCCGATATGC"
rc = OR.revcomp


def sub(s, places):
    """s with the base at each place swapped for another one (A<->C, G<->T)"""
    s = bytearray(s)
    for p in places:
        s[p] = {65: 67, 67: 65, 71: 84, 84: 71}[s[p]]
    return bytes(s)


def put(s, at, c):
    return s[:at] + c + s[at + 1:]


PERIOD = b"ACGGTCAT" * 6
DEFAULTS = (30, 5, 20)
# (what, s1, s2, (min_overlap, max_mism, max_err_pct), the hit (d, mism, ov) or None) -- every answer worked out by hand
HAND = [
    # r = rc(s2) = "CTGCAA" + FRAG: r[6] stands beside s1[0], so d = -6 and I = d + L2 = 40, the fragment's length
    ("an exact read-through", FRAG + b"ACGTAC", rc(FRAG) + b"TTGCAG", DEFAULTS, (-6, 0, 40)),
    ("a hit at d = 0", FRAG, rc(FRAG), DEFAULTS, (0, 0, 40)),
    # r = TAIL30 + MORE20 (L2 = 50), s1 = HEAD30 + TAIL30 (L1 = 60): r[0] beside s1[30], ov = 60 - 30 = 30
    ("d = L1 - min_overlap exactly", HEAD30 + TAIL30, rc(TAIL30 + MORE20), DEFAULTS, (30, 0, 30)),
    ("... and one place beyond it", HEAD30 + b"A" + TAIL30[:29], rc(TAIL30 + MORE20), DEFAULTS, None),
    ("mism == max_mism", sub(FRAG, (1, 9, 17, 25, 33)), rc(FRAG), DEFAULTS, (0, 5, 40)),
    ("... and one more", sub(FRAG, (1, 9, 17, 25, 33, 38)), rc(FRAG), DEFAULTS, None),
    # ov = 40, 10 per cent: 100 * 4 == 10 * 40
    ("100 * mism == pct * ov", sub(FRAG, (1, 9, 17, 25)), rc(FRAG), (30, 5, 10), (0, 4, 40)),
    ("... and one more, within max_mism", sub(FRAG, (1, 9, 17, 25, 33)), rc(FRAG), (30, 5, 10), None),
    ("an N in mate 1", put(FRAG, 3, b"N"), rc(FRAG), DEFAULTS, (0, 1, 40)),
    ("an N in mate 2", FRAG, put(rc(FRAG), 3, b"N"), DEFAULTS, (0, 1, 40)),
    ("an N beside an N", put(FRAG, 3, b"N"), rc(put(FRAG, 3, b"N")), DEFAULTS, (0, 1, 40)),
    ("no N is forgiven at 0 per cent", put(FRAG, 3, b"N"), rc(FRAG), (30, 5, 0), None),
    ("all A against all T: every shift hits, d = 0 wins", b"A" * 100, b"T" * 100, DEFAULTS, (0, 0, 100)),
    # r = PERIOD with place 44 spoilt: d = 0 has one mismatch over 48, d = 8 none over 40 -- the first hit wins
    ("a better match at a later shift loses", PERIOD, rc(sub(PERIOD, (44,))), DEFAULTS, (0, 1, 48)),
    ("... which it would win without mismatches allowed", PERIOD, rc(sub(PERIOD, (44,))), (30, 0, 20), (8, 0, 40)),
    ("L < min_overlap", FRAG[:29], rc(FRAG[:29]), DEFAULTS, None),
    ("L == min_overlap", FRAG[:30], rc(FRAG[:30]), DEFAULTS, (0, 0, 30)),
    # mate 2 alone reaches past the fragment: r = "CTGCAA" + FRAG[:34] against s1 = FRAG[:34]
    ("mate 2 longer than mate 1", FRAG[:34], rc(FRAG[:34]) + b"TTGCAG", DEFAULTS, (-6, 0, 34)),
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
    for what, s1, s2, o, hit in HAND:
        assert OR.pair_overlap(s1, s2, OR.spec(*o)) == hit, what
        L1, L2 = len(s1), len(s2)
        want = (L1, L2, 0) if hit is None else (min(L1, hit[0] + L2), min(L2, hit[0] + L2), hit[0] + L2)
        assert OR.pair_limits(s1, s2, OR.spec(*o)) == want, what
    # the read-through's limits cut both mates at the fragment's end
    assert OR.pair_limits(HAND[0][1], HAND[0][2], OR.spec()) == (40, 40, 40)
    # 513 bases on either side: not analysed, whatever the lines hold
    long1 = (FRAG * 13)[:513]
    assert OR.pair_limits(long1, rc(long1), OR.spec()) == (513, 513, 0) and OR.pair_limits(long1[:512], rc(long1[:512]), OR.spec()) == (512, 512, 512)
    raw1, recs1 = OR.chunk([long1, FRAG, long1[:512]])
    raw2, recs2 = OR.chunk([b"x" * 40, rc(FRAG), rc(long1)])
    out, la, lb, ins = OR.overlap_records(raw1, recs1, 0, raw2, recs2, 0, 3, OR.spec())
    assert out[:8].tolist() == [3, 1, 0, 0, 0, 2, 0, 40] and ins.tolist() == [0, 40, 0] and la.tolist() == [513, 40, 512] and lb.tolist() == [40, 40, 513]
    assert int(out[OR.HEAD + 40]) == 1 == int(out[OR.HEAD:].sum())
    with pytest.raises(OR.Refused):
        OR.overlap_records(raw1, recs1, 1, raw2, recs2, 0, 1, OR.spec())   # the 'x' line is analysed now
    for first_a, first_b, count in ((0, 0, 0), (0, 0, 4), (3, 0, 1), (1, 2, 2)):
        with pytest.raises(OR.Refused):
            OR.overlap_records(raw1, recs1, first_a, raw2, recs2, first_b, count, OR.spec())


def test_the_fixture_counts(golden):
    (raw1, recs1), (raw2, recs2) = golden
    out, la, lb, ins = OR.overlap_records(raw1, recs1, 0, raw2, recs2, 0, 1000, OR.spec())
    assert out[:OR.FINGERPRINT].tolist() == [1000, 111, 36, 1211, 1211, 0, 169, 7011]
    hits = ins > 0
    assert int(hits.sum()) == 111 and int((ins[hits] < 100).sum()) == 36 and int(ins[hits].min()) >= 30 and int(ins.max()) <= 170
    assert np.array_equal(la, np.where(hits, np.minimum(ins, 100), 100)) and np.array_equal(la, lb), "both mates have 100 bases"
    rows = out[OR.HEAD:]
    assert np.array_equal(np.bincount(ins[hits], minlength=OR.ROWS), rows.astype(np.int64))
    # two halves add up to the whole
    lo, hi = OR.overlap_records(raw1, recs1, 0, raw2, recs2, 0, 391, OR.spec()), OR.overlap_records(raw1, recs1, 391, raw2, recs2, 391, 609, OR.spec())
    assert OR.merge(lo[0], hi[0]).tolist() == out.tolist() and np.array_equal(np.concatenate((lo[3], hi[3])), ins)
    # a stricter spec finds fewer, and mates in the wrong order do not look like mates
    strict = OR.overlap_records(raw1, recs1, 0, raw2, recs2, 0, 1000, OR.spec(30, 0, 0))[0]
    assert 0 < int(strict[OR.OVERLAPPED]) < 111 and int(strict[OR.MISMATCHES]) == 0
    assert int(OR.overlap_records(raw1, recs1, 0, raw2, recs2, 1, 999, OR.spec())[0][OR.OVERLAPPED]) < 5


def test_overlap_check_merge_and_the_fingerprint(F):
    B = F.binding
    assert B.OVERLAP_WORDS == OR.WORDS == 1040 and B.OVERLAP_MAX_LEN == OR.MAX_LEN and B.OVERLAP_NAMES[OR.FINGERPRINT] == "fingerprint"
    assert {"fqgpu_overlap_check", "fqgpu_overlap_merge", "fqgpu_chunk_pair_overlap", "fqgpu_dblock_pair_overlap", "fqgpu_chunk_select_limited",
            "fqgpu_dblock_select_limited"} <= set(B.EXPORTS)
    assert B.read_overlap().tolist() == OR.spec().tolist() == [30, 5, 20, 0, 0, 0, 0, 0]
    for o in ((1, 0, 0), (512, 65535, 50), (30, 5, 20)):
        assert B.overlap_check(B.read_overlap(*o)) == 0, o
    for o in ((0, 5, 20), (513, 5, 20), (30, 65536, 20), (30, 5, 51), (1 << 31, 0, 0)):
        assert B.overlap_check(B.read_overlap(*o)) == E_ARG, o
    for k in range(5):
        reserved = [0] * 5
        reserved[k] = 1
        assert B.overlap_check(B.read_overlap(reserved=reserved)) == E_ARG
    assert B.overlap_check(None) == E_ARG
    # the fingerprint is zlib's CRC-32 of the 32 bytes; the merge holds two results against it
    fp = OR.fingerprint(OR.spec())
    assert fp == zlib.crc32(np.array([30, 5, 20, 0, 0, 0, 0, 0], dtype="<u4").tobytes()) != OR.fingerprint(OR.spec(31))
    rng = np.random.default_rng(2)

    def result(o, n):
        w = np.zeros(OR.WORDS, dtype=np.uint64)
        rows = rng.integers(0, 50, OR.ROWS).astype(np.uint64)
        w[OR.HEAD:] = rows
        w[:8] = (n, rows.sum(), 3, 4, 5, 6, 7, 8)
        w[OR.FINGERPRINT] = OR.fingerprint(o)
        return w

    a, b, other = result(OR.spec(), 100000), result(OR.spec(), 70000), result(OR.spec(31), 5)
    dst = np.zeros(OR.WORDS, dtype=np.uint64)
    assert B.overlap_merge(dst, a) == 0 and dst.tolist() == a.tolist(), "an all-zero dst is empty"
    assert B.overlap_merge(dst, b) == 0 and dst.tolist() == OR.merge(a, b).tolist() and int(dst[OR.FINGERPRINT]) == fp
    assert int(dst[0]) == 170000 and int(dst[OR.HEAD:].sum()) == int(dst[1])
    before = dst.copy()
    assert B.overlap_merge(dst, other) == E_ARG and dst.tolist() == before.tolist(), "word 8 must agree"
    empty_src = np.zeros(OR.WORDS, dtype=np.uint64)
    empty_src[OR.FINGERPRINT] = fp
    assert B.overlap_merge(dst, empty_src) == 0 and dst.tolist() == before.tolist()
    empty_dst = empty_src.copy()
    assert B.overlap_merge(empty_dst, other) == E_ARG, "an empty dst that names a spec is held to it"
    assert B.overlap_merge(empty_dst, a) == 0 and empty_dst.tolist() == a.tolist()
    assert B.overlap_merge(dst[:-1].copy(), a) == E_ARG and B.overlap_merge(dst, a[:-1].copy()) == E_ARG
    lib = F.lib()
    assert lib.fqgpu_overlap_merge(None, OR.WORDS, a.ctypes.data_as(C.c_void_p), OR.WORDS) == E_ARG
    assert lib.fqgpu_overlap_merge(dst.ctypes.data_as(C.c_void_p), OR.WORDS, None, OR.WORDS) == E_ARG


def test_the_limit_of_the_reference(golden):
    raw, recs = golden[0]
    recs = recs.astype(FR.REC_DTYPE)
    n = len(recs)
    L = recs["len"].astype(np.int64)
    a, t, f = AR.adp(b"AGATCGGAAGAGC"), R.trm(cut_front=1, q_tail=20), FR.flt(min_len=40)
    mark = np.random.default_rng(4).integers(0, 256, (n + 7) // 8, dtype=np.uint8)
    plain = PR.marked_records(raw, recs, 3, 900, mark[:113], a, None, t, f)
    # no limit, and limits that cut nothing, are the marked call
    for limit in (None, L[3:900], np.full(897, 65535)):
        got = OR.limited_records(raw, recs, 3, 900, mark[:113], limit, a, None, t, f)
        assert all(np.array_equal(g, w) for g, w in zip(got, plain)) and not got[1][21:].any()
    # a limit of 60 everywhere: nobody keeps more than 59 bases behind cut_front, the two new words count what it took
    got = OR.limited_records(raw, recs, 0, n, None, np.full(n, 60), a, None, t, f)
    a_adapter = PR.marked_records(raw, recs, 0, n, None, a, None, t, f)[4][:, 0].astype(np.int64)
    assert int((got[3] >> 16).max()) == 59 and int(got[1][OR.READS_CUT_LIMIT]) == int((a_adapter > 60).sum()) > 900
    assert int(got[1][OR.BASES_CUT_LIMIT]) == int(np.maximum(a_adapter - 60, 0).sum())
    assert int(got[1][14]) == n and int(got[1][15]) == int((L - np.minimum(a_adapter, 60)).sum()), "words 14 / 15 count a0 against L"
    assert int(got[1][R.BASES_IN]) == int(got[1][R.BASES_CUT_FRONT]) + int(got[1][R.BASES_CUT_TAIL]) + int((got[3] >> 16).sum())
    # a limit of 0 empties the read
    zero = np.where(np.arange(n) % 3 == 0, 0, 65535)
    got = OR.limited_records(raw, recs, 0, n, None, zero, None, None, None, None)
    assert int(got[1][R.READS_EMPTIED]) == int(got[1][R.DROPPED_SHORT]) == 334 and int(got[1][R.N_KEPT]) == 666 and not got[3][::3].any()
    assert not PR.bits(got[2], n)[::3].any() and PR.bits(got[2], n)[1::3].all()


def test_the_device_calls_say_no_device_without_one(F):
    """(with a device in the machine the same calls get as far as their arguments: no handle, FQGPU_E_ARG)"""
    want = E_NO_DEVICE if F.device_count() == 0 else E_ARG
    lib = F.lib()
    p = lambda v: v.ctypes.data_as(C.c_void_p)  # noqa: E731
    out = np.full(OR.WORDS, 7, dtype=np.uint64)
    arr = np.full(5, 7, dtype=np.uint16)
    report = np.full(24, 7, dtype=np.uint64)
    n = C.c_size_t(7)
    o = OR.spec()
    assert lib.fqgpu_chunk_pair_overlap(None, 0, None, 0, 5, p(o), p(out), OR.WORDS, p(arr), p(arr), p(arr)) == want
    assert lib.fqgpu_dblock_pair_overlap(None, None, 0, None, 0, 5, p(o), p(out), OR.WORDS, p(arr), p(arr), p(arr)) == want
    assert lib.fqgpu_chunk_pair_overlap(None, 0, None, 0, 0, None, None, 0, None, None, None) == want, "said before any argument is looked at"
    assert lib.fqgpu_dblock_pair_overlap(None, None, 0, None, 0, 0, None, None, 0, None, None, None) == want
    assert lib.fqgpu_chunk_select_limited(None, None, None, None, None, 0, 5, None, p(arr), None, 0, C.byref(n), p(report), None, None, None) == want
    assert lib.fqgpu_dblock_select_limited(None, None, None, None, None, None, 0, 5, None, p(arr), None, 0, C.byref(n), p(report), None, None, None) == want
    if want == E_NO_DEVICE:
        assert n.value == 7 and (report == 7).all() and (out == 7).all() and (arr == 7).all(), "nothing is looked at"


# ---------------------------------------------------------------- the farm's host logic, under the sanitizers
def report_text(o, words, rows):
    """the report's text, restated: the spec, the eight words by name, the non-empty rows"""
    names = ("pairs", "pairs_overlapped", "pairs_read_through", "bases_behind_1", "bases_behind_2", "pairs_not_analysed", "mismatches", "overlap_bases")
    lines = ["#fqgpu-overlap 1", "min_overlap\t%d" % o[0], "max_mism\t%d" % o[1], "max_err_pct\t%d" % o[2]]
    lines += ["%s\t%d" % (n, w) for n, w in zip(names, words)]
    lines += ["insert\t%d\t%d" % (r, c) for r, c in sorted(rows) if c]
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module")
def report_check(F, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("overlap_check") / "overlap_report_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "overlap_report_check.cpp")] + LINK, check=True)
    return exe


def test_the_merge_of_pieces_and_workers_under_the_sanitizers(report_check):
    for seed in (1, 2, 3):
        r = subprocess.run([report_check, "merge", str(seed)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout == "ok\n" and r.stderr == "", r.stdout + r.stderr


def test_the_report_text_under_the_sanitizers(report_check, tmp_path, golden):
    (raw1, recs1), (raw2, recs2) = golden
    out = OR.overlap_records(raw1, recs1, 0, raw2, recs2, 0, 1000, OR.spec())[0]
    rows = [(int(r), int(out[OR.HEAD + r])) for r in np.flatnonzero(out[OR.HEAD:])]
    cases = [((30, 5, 20), out[:8].tolist(), rows), ((1, 0, 0), [0] * 8, []), ((512, 65535, 50), [2 ** 63, 1, 2, 3, 4, 5, 6, 2 ** 64 - 1], [(0, 1), (1023, 2 ** 40)])]
    for o, words, rws in cases:
        r = subprocess.run([report_check, "text"] + [str(v) for v in o] + [",".join(str(w) for w in words)] + ["%d:%d" % rc for rc in rws],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "" and r.stdout == report_text(o, words, rws), r.stderr
    r = subprocess.run([report_check, "text", "30", "5", "20", "1,1,0,0,0,0,0,30", "1024:1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "expected <row>:<count>" in r.stderr
    path = tmp_path / "report.tsv"
    r = subprocess.run([report_check, "file", str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "" and path.read_text() == r.stdout == report_text((30, 5, 20), [10, 3, 2, 7, 8, 1, 4, 160], [(40, 2), (1023, 1)])
    assert os.listdir(tmp_path) == ["report.tsv"], "the .part file is gone"


# ---------------------------------------------------------------- the tool
@pytest.fixture(scope="module")
def tool(F, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("overlap_tool") / "fqc_tool")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tools", "fqc_tool.cpp")] + LINK, check=True)
    return exe


MATE = ["--mate", "in2.fqc", "out2.fastq"]


@pytest.mark.parametrize("args", [
    # any of the five options without --mate
    ["d", "in.fqc", "out.fastq", "--overlap-trim"], ["d", "in.fqc", "out.fastq", "--overlap-report", "r.tsv"],
    ["d", "in.fqc", "out.fastq", "--overlap-min", "20"], ["d", "in.fqc", "out.fastq", "--overlap-mism", "2"],
    ["d", "in.fqc", "out.fastq", "--overlap-err", "10"], ["d", "in.fqc", "out.fastq", "--min-len", "30", "--overlap-trim"],
    ["c", "in.fastq", "out.fqc", "--overlap-trim"], ["s", "in.fqc", "report.tsv", "--overlap-report", "r.tsv"], ["t", "in.fqc", "--overlap-trim"],
    # --mate on another command stays an error with them
    ["c", "in.fastq", "out.fqc"] + MATE + ["--overlap-trim"],
    # the spec's options without anything to use it
    ["d", "in.fqc", "out.fastq"] + MATE + ["--overlap-min", "20"], ["d", "in.fqc", "out.fastq"] + MATE + ["--overlap-err", "10", "--overlap-mism", "1"],
    # a spec the check refuses, words that are no numbers, missing values
    ["d", "in.fqc", "out.fastq"] + MATE + ["--overlap-trim", "--overlap-min", "0"], ["d", "in.fqc", "out.fastq"] + MATE + ["--overlap-trim", "--overlap-min", "513"],
    ["d", "in.fqc", "out.fastq"] + MATE + ["--overlap-trim", "--overlap-mism", "65536"], ["d", "in.fqc", "out.fastq"] + MATE + ["--overlap-trim", "--overlap-err", "51"],
    ["d", "in.fqc", "out.fastq"] + MATE + ["--overlap-report", "r.tsv", "--overlap-err", "ten"], ["d", "in.fqc", "out.fastq"] + MATE + ["--overlap-trim", "--overlap-min"],
    ["d", "in.fqc", "out.fastq"] + MATE + ["--overlap-report"],
    # the other options keep their rules beside them
    ["d", "in.fqc", "out.fastq"] + MATE + ["--overlap-trim", "--records", "0:5"], ["d", "in.fqc", "out.fastq"] + MATE + ["--overlap-trim", "--crop", "0"],
])
def test_usage_errors_are_said_before_any_file_or_device_is_touched(tool, tmp_path, args):
    r = subprocess.run([tool] + args, capture_output=True, text=True, cwd=tmp_path, timeout=60)
    assert r.returncode == 2 and r.stdout == "" and r.stderr, (args, r.stderr)
    assert os.listdir(tmp_path) == []


def test_the_usage_text_names_the_overlap_options(tool, tmp_path):
    r = subprocess.run([tool], capture_output=True, text=True, cwd=tmp_path, timeout=60)
    assert r.returncode == 2 and all(o in r.stderr for o in ("--overlap-trim", "--overlap-report", "--overlap-min", "--overlap-mism", "--overlap-err"))
