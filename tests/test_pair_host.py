"""The host side of the paired restore, no GPU: the read id rule (fqgpu_read_id_len against tests/pair_ref.py), the
reference's range and mark semantics, the golden pair's four numbers, the device calls' answer without a device, the unit plan
and the bit helpers of the farm (tests/cpp/pair_plan_check.cpp), and the tool's usage errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import filter_ref as FR
import oracle_lib as O
import pair_ref as PR
import tail_ref as TR
import trim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_NO_DEVICE = -4, -5
LINK = ["-L" + os.path.join(ROOT, "fqcomp28_amd"), "-lfqgpu", "-Wl,-rpath," + os.path.join(ROOT, "fqcomp28_amd"), "-lpthread"]


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    F.lib()
    return F


@pytest.fixture(scope="module")
def golden(golden_dir):
    return [O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_%d.fastq" % m)) for m in (1, 2)]


# ---------------------------------------------------------------- the id rule
HAND_IDS = [(b"@x/1\n", 1), (b"@x/2\n", 1), (b"@x/3\n", 3), (b"@/1\n", 0), (b"@\n", 0), (b"@", 0), (b"@x/1", 1), (b"@/2", 0),
            (b"@read7\tlane=3\n", 5), (b"@read7/2\tlane=3\n", 5),            # ended by a tab
            (b"@read7\n", 5), (b"@read7", 5), (b"@read7/1\n", 5),            # ended by the line's end
            (b"@a/1b/2c more\n", 7), (b"@a/1b/2 more\n", 4), (b"@a/1/1 x\n", 3),  # a "/1" in the middle stays; only one is taken from the end
            (b"@SRR065390.1 HWUSI-EAS687_61DAJ:8:1:1055:3384 length=100\n", 11), (b"@x /1\n", 1), (b"@ x\n", 0), (b"@1\n", 1), (b"@/\n", 1),
            (b"@x/12\n", 4), (b"@x/0\n", 3), (b"@\xc3\xa9/1 \n", 2)]


def test_the_read_id_rule(F, golden):
    B = F.binding
    for line, want in HAND_IDS:
        assert PR.id_len(line) == want == B.read_id_len(line), line
    assert F.lib().fqgpu_read_id_len(None, 0) == 0 and F.lib().fqgpu_read_id_len(None, 5) == 0 and B.read_id_len(b"") == 0
    for raw, recs in golden:
        lines = PR.header_lines(raw, recs)
        assert len(lines) == 1000 and all(line[:1] == b"@" and line[-1:] == b"\n" for line in lines)
        for r, line in enumerate(lines):
            assert B.read_id_len(line) == PR.id_len(line) == len(b"SRR065390.%d" % (r + 1)), line
            assert B.read_id_len(line[:-1]) == PR.id_len(line), "without its newline"
    assert PR.read_ids(*golden[0]) == PR.read_ids(*golden[1]) == [b"SRR065390.%d" % (r + 1) for r in range(1000)]
    assert {"fqgpu_read_id_len", "fqgpu_chunk_select_marked", "fqgpu_dblock_select_marked", "fqgpu_chunk_pair_names",
            "fqgpu_dblock_pair_names"} <= set(B.EXPORTS)
    assert B.MARKED_REPORT_NAMES[:20] == B.TAIL_REPORT_NAMES and B.MARKED_REPORT_NAMES[B.DROPPED_UNMARKED] == "dropped_unmarked"
    assert B.DROPPED_UNMARKED == PR.DROPPED_UNMARKED == 20 < B.TAIL_REPORT_WORDS == PR.REPORT_WORDS


def test_the_first_mismatch_of_the_reference(golden):
    (raw1, recs1), (raw2, recs2) = golden
    assert PR.first_mismatch(raw1, recs1, 0, raw2, recs2, 0, 1000) is None
    assert PR.first_mismatch(raw1, recs1, 0, raw2, recs2, 1, 999) == 0 and PR.first_mismatch(raw1, recs1, 5, raw2, recs2, 5, 20) is None
    spoilt = raw2.copy()
    spoilt[int(PR.header_starts(recs2)[40]) + 3] ^= 1
    assert PR.first_mismatch(raw1, recs1, 0, spoilt, recs2, 0, 1000) == 40 and PR.first_mismatch(raw1, recs1, 30, spoilt, recs2, 30, 50) == 10
    assert PR.first_mismatch(raw1, recs1, 41, spoilt, recs2, 41, 900) is None


# ---------------------------------------------------------------- a range and a mark
def test_the_golden_pair_under_min_mean_q_20(golden):
    """the four numbers every later test of the pair relies on: all three kinds of dropped pair are there"""
    (raw1, recs1), (raw2, recs2) = golden
    f = FR.flt(min_mean_q=20)
    k1, k2 = (PR.bits(FR.filter_records(raw, recs.astype(FR.REC_DTYPE), f)[2], 1000) for raw, recs in golden)
    assert (int((k1 & k2).sum()), int((~k1 & k2).sum()), int((k1 & ~k2).sum()), int((~k1 & ~k2).sum())) == (619, 80, 84, 217)
    out1, out2, rep1, rep2, counters = PR.pair_records(raw1, recs1, raw2, recs2, f=f)
    assert counters == dict(pairs=1000, kept=619, dropped_mate1_only=80, dropped_mate2_only=84, dropped_both=217)
    t1, t2 = FR.parse(out1), FR.parse(out2)
    assert len(t1) == len(t2) == 619 and PR.read_ids(out1, t1) == PR.read_ids(out2, t2)
    assert int(rep1[R.N_KEPT]) == int(rep2[R.N_KEPT]) == 619 and int(rep1[R.DROPPED_MEAN_Q]) == 80 + 217 and int(rep2[R.DROPPED_MEAN_Q]) == 84 + 217
    with pytest.raises(ValueError):
        PR.pair_records(raw1, recs1, raw2, recs2[:-1], f=f)


def test_range_and_mark_semantics_of_the_reference(golden):
    raw, recs = golden[0]
    recs = recs.astype(FR.REC_DTYPE)
    t, f = R.trm(q_tail=20), FR.flt(min_len=50, min_mean_q=20)
    whole = TR.tail_records(raw, recs, None, None, t, f)
    # the whole range without a mark is the tail call; two ranges add up to it
    got = PR.marked_records(raw, recs, 0, 1000, None, t=t, f=f)
    assert all(np.array_equal(g, w) for g, w in zip(got, whole)) and int(got[1][PR.DROPPED_UNMARKED]) == 0
    lo, hi = PR.marked_records(raw, recs, 0, 333, None, t=t, f=f), PR.marked_records(raw, recs, 333, 1000, None, t=t, f=f)
    assert lo[0].tobytes() + hi[0].tobytes() == whole[0].tobytes() and (lo[1] + hi[1]).tolist() == whole[1].tolist()
    assert np.array_equal(np.concatenate((lo[3], hi[3])), whole[3]) and np.array_equal(np.concatenate((PR.bits(lo[2], 333), PR.bits(hi[2], 667))), PR.bits(whole[2], 1000))
    # a mark drops records that pass, changes no window and none of the records' own counters; padding bits are not looked at
    own = PR.bits(hi[2], 667)
    mark = np.random.default_rng(1).integers(0, 256, 84, dtype=np.uint8)
    marked = PR.marked_records(raw, recs, 333, 1000, mark, t=t, f=f)
    final = PR.bits(marked[2], 667)
    assert np.array_equal(final, own & PR.bits(mark, 667)) and 0 < final.sum() < own.sum()
    assert int(marked[1][PR.DROPPED_UNMARKED]) == int(own.sum() - final.sum()) and marked[1][5:20].tolist() == hi[1][5:20].tolist()
    assert np.array_equal(marked[3], hi[3]) and len(FR.parse(marked[0])) == final.sum() == int(marked[1][1])
    dirty = mark.copy()
    dirty[-1] |= 0xF8       # (667 = 83 * 8 + 3: five bits of padding)
    assert all(np.array_equal(a, b) for a, b in zip(PR.marked_records(raw, recs, 333, 1000, dirty, t=t, f=f), marked))
    for first, end in ((0, 0), (5, 4), (0, 1001)):
        with pytest.raises(PR.Refused):
            PR.marked_records(raw, recs, first, end)


# ---------------------------------------------------------------- without a device
def test_the_device_calls_say_no_device_without_one(F):
    """(with a device in the machine the same calls get as far as their arguments: no handle, FQGPU_E_ARG)"""
    want = E_NO_DEVICE if F.device_count() == 0 else E_ARG
    lib = F.lib()
    report = np.full(TR.REPORT_WORDS, 7, dtype=np.uint64)
    p = lambda v: v.ctypes.data_as(C.c_void_p)  # noqa: E731
    n, m = C.c_size_t(7), C.c_size_t(7)
    assert lib.fqgpu_chunk_select_marked(None, None, None, None, p(FR.flt()), 0, 5, None, None, 0, C.byref(n), p(report), None, None, None) == want
    assert lib.fqgpu_dblock_select_marked(None, None, None, None, None, None, 0, 5, None, None, 0, C.byref(n), p(report), None, None, None) == want
    assert lib.fqgpu_chunk_select_marked(None, None, None, None, None, 5, 0, None, None, 0, None, None, None, None, None) == want, "said before any argument is looked at"
    assert lib.fqgpu_dblock_select_marked(None, None, None, None, None, None, 5, 0, None, None, 0, None, None, None, None, None) == want
    assert lib.fqgpu_chunk_pair_names(None, 0, None, 0, 0, None) == want and lib.fqgpu_dblock_pair_names(None, None, 0, None, 0, 0, None) == want
    if want == E_NO_DEVICE:
        assert n.value == 7 and (report == 7).all(), "nothing is looked at"
        assert lib.fqgpu_chunk_pair_names(None, 0, None, 0, 1, C.byref(m)) == want and lib.fqgpu_dblock_pair_names(None, None, 0, None, 0, 1, C.byref(m)) == want


# ---------------------------------------------------------------- the farm's host arithmetic
@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pair_plan") / "pair_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "pair_plan_check.cpp")] + LINK, check=True)
    return exe


def plan_of(counts1, counts2):
    """per unit of archive 1 the pieces (block, first, end, at) of archive 2 that hold its records' mates, record by record"""
    owner = [(j, i) for j, c in enumerate(counts2) for i in range(c)]
    units, a = [], 0
    for c in counts1:
        pieces = []
        for at in range(c):
            j, i = owner[a + at]
            if pieces and pieces[-1][0] == j:
                pieces[-1][2] = i + 1
            else:
                pieces.append([j, i, i + 1, at])
        units.append((a, a + c, [tuple(pc) for pc in pieces]))
        a += c
    return units


@pytest.mark.parametrize("counts1,counts2,most", [
    ([100, 100, 100, 37], [100, 100, 100, 37], 1),          # aligned
    ([40, 50, 60, 30, 70], [20, 210, 20], 2),               # one chunk of archive 2 spans three units
    ([30, 200, 20], [40, 150, 60], 3),                     # one unit spans three chunks of archive 2
    ([1, 1, 254, 7], [256, 7], 1), ([5], [1, 1, 1, 1, 1], 5), ([3, 3], [6], 1),
], ids=["aligned", "a chunk over three units", "a unit over three chunks", "single records", "many chunks", "one chunk"])
def test_the_unit_plan(plan_check, counts1, counts2, most):
    r = subprocess.run([plan_check, "plan", ",".join(map(str, counts1)), ",".join(map(str, counts2))], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = []
    for line in r.stdout.split("\n"):
        w = line.split()
        if w and w[0] == "unit":
            got.append((int(w[2]), int(w[3]), []))
        elif w:
            got[-1][2].append(tuple(int(v) for v in w[1:]))
    want = plan_of(counts1, counts2)
    assert got == want
    assert max(len(pieces) for _, _, pieces in want) == most
    for a, b, pieces in want:       # the pieces tile the unit in order
        assert [pc[3] for pc in pieces] == list(np.cumsum([0] + [pc[2] - pc[1] for pc in pieces])[:-1]) and sum(pc[2] - pc[1] for pc in pieces) == b - a


def test_the_unit_plan_refuses_records_the_mate_archive_does_not_have(plan_check):
    r = subprocess.run([plan_check, "plan", "10,10", "10,9"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "not a range of the archive's 19 records" in r.stderr


def test_the_bit_helpers(plan_check):
    for seed in (1, 2):
        r = subprocess.run([plan_check, "bits", str(seed)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stdout == "ok\n", r.stdout + r.stderr


# ---------------------------------------------------------------- the tool
@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pair_tool") / "fqc_tool")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tools", "fqc_tool.cpp")] + LINK, check=True)
    return exe


MATE = ["--mate", "in2.fqc", "out2.fastq"]


@pytest.mark.parametrize("args", [
    # --mate on any command but a plain d
    ["c", "in.fastq", "out.fqc"] + MATE, ["s", "in.fqc", "report.tsv"] + MATE, ["x", "in.fqc"] + MATE, ["t", "in.fqc"] + MATE,
    *[["d", "in.fqc", "out.fastq"] + MATE + other for other in (["--records", "0:5"], ["--fasta"], ["--index"], ["--index-stride", "64"])],
    ["d", "in.fqc", "out.fastq", "--min-mean-q", "20", "--records", "3:"] + MATE,
    ["d", "in.fqc", "out.fastq", "--index"] + MATE + ["--adapter", "AGATCGGAAGAGC", "--adapter2", "AGATCGGAAGAGC"],
    # --adapter2 without --mate, alone and beside the other options
    ["d", "in.fqc", "out.fastq", "--adapter2", "AGATCGGAAGAGC"],
    ["d", "in.fqc", "out.fastq", "--adapter", "AGATCGGAAGAGC", "--adapter2", "AGATCGGAAGAGC", "--min-len", "30"],
    ["c", "in.fastq", "out.fqc", "--adapter2", "AGATCGGAAGAGC"],
    # an adapter its check refuses, missing values
    ["d", "in.fqc", "out.fastq"] + MATE + ["--adapter2", "agatc"],
    ["d", "in.fqc", "out.fastq"] + MATE + ["--adapter2", "A" * 65],
    ["d", "in.fqc", "out.fastq"] + MATE + ["--adapter2", "ACGT", "--adapter-err", "51"],
    ["d", "in.fqc", "out.fastq"] + MATE + ["--adapter-overlap", "3"],
    ["d", "in.fqc", "out.fastq"] + MATE + ["--adapter2"],
    ["d", "in.fqc", "out.fastq", "--mate", "in2.fqc"],
    ["d", "in.fqc", "out.fastq", "--mate"],
    # the other options keep their rules beside --mate
    ["d", "in.fqc", "out.fastq"] + MATE + ["--min-mean-q", "64"],
    ["d", "in.fqc", "out.fastq"] + MATE + ["--window", "33:20"],
    ["d", "in.fqc", "out.fastq"] + MATE + ["--crop", "0"],
])
def test_usage_errors_are_said_before_any_file_or_device_is_touched(tool, tmp_path, args):
    r = subprocess.run([tool] + args, capture_output=True, text=True, cwd=tmp_path, timeout=60)
    assert r.returncode == 2 and r.stdout == "" and r.stderr, (args, r.stderr)
    assert os.listdir(tmp_path) == []


def test_the_usage_text_names_the_paired_restore(tool, tmp_path):
    r = subprocess.run([tool], capture_output=True, text=True, cwd=tmp_path, timeout=60)
    assert r.returncode == 2 and "--mate <in2.fqc> <out2.fastq>" in r.stderr and "--adapter2" in r.stderr
