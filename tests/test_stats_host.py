"""The host side of the read summaries, no GPU: fqgpu_stats_words and fqgpu_stats_merge against tests/stats_ref.py, the
report writer of the farm (process.hpp: writeStatsReport, through tests/cpp/stats_tool.cpp under AddressSanitizer and UBSan)
against the renderer written here from the format's description, the tool's usage errors, and the device calls' answer
without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import stats_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_OVERFLOW, E_ARG, E_NO_DEVICE = -1, -4, -5


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    F.lib()
    return F


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_1.fastq"))


def halves(raw, recs, P):
    half = len(recs) // 2
    return R.stats_of(raw, recs[:half], P), R.stats_of(raw, recs[half:], P)


def test_words(F):
    assert [F.stats_words(P) for P in (1, 512, 65535)] == [176 + 70 * 2, 176 + 70 * 513, 176 + 70 * 65536]
    assert [R.words(P) for P in (1, 512, 65535)] == [316, 36086, 4587696]
    assert F.stats_words(0) == 0 and F.stats_words(65536) == 0 and F.stats_words(2 ** 32 - 1) == 0


def test_the_reference_on_a_chunk_counted_by_hand():
    raw = np.frombuffer(b"@a\nACGTN\n+\n!#5I`\n@b\nGGC\n+a\n+++\n", dtype=np.uint8)
    recs = np.array([(3, 11, 5), (20, 27, 3)], dtype=[("seq_off", "<u4"), ("qual_off", "<u4"), ("len", "<u4")])
    v = R.view(R.stats_of(raw, recs, 4))
    assert (v["n_records"], v["n_bases"], v["min_len"], v["max_len"], v["reads_with_n"], v["positions"]) == (2, 8, 3, 5, 1, 4)
    assert v["len_hist"].tolist() == [0, 0, 0, 1, 1]            # 5 -> row 4 (">= 4")
    assert v["base_pos"].tolist() == [[1, 0, 1, 0, 0], [0, 1, 1, 0, 0], [0, 1, 1, 0, 0], [0, 0, 0, 1, 0], [0, 0, 0, 0, 1]]
    # Phred 0 2 20 40 63 -> mean 25; 10 10 10 -> 10.  G + C: 2 of 5 -> 40; 3 of 3 -> 100
    assert np.flatnonzero(v["meanq_hist"]).tolist() == [10, 25] and np.flatnonzero(v["gc_hist"]).tolist() == [40, 100]
    assert [int(np.flatnonzero(v["qual_pos"][r])[0]) for r in (3, 4)] == [40, 63] and v["qual_pos"][0, [0, 10]].tolist() == [1, 1]


def test_merge(F, fixture):
    raw, recs = fixture
    for P in (128, 64, 1):
        a, b = halves(raw, recs, P)
        whole = R.stats_of(raw, recs, P)
        dst = np.zeros(R.words(P), dtype=np.uint64)
        assert F.stats_merge(dst, a) == 0 and np.array_equal(dst, a), "into an empty block: a copy"
        assert F.stats_merge(dst, b) == 0 and np.array_equal(dst, whole), "the halves add up to the whole"
        assert np.array_equal(R.merge(a, b), whole)
        empty = np.zeros(R.words(P), dtype=np.uint64)
        empty[5] = P
        assert F.stats_merge(dst, empty) == 0 and np.array_equal(dst, whole), "an empty summary adds nothing"
        assert F.stats_merge(empty, whole) == 0 and np.array_equal(empty, whole)
        both = np.zeros(R.words(P), dtype=np.uint64)
        both[5] = P
        assert F.stats_merge(both, both.copy()) == 0 and both[5] == P and not both[:5].any(), "empty into empty"


def test_merge_keeps_the_smaller_minimum_and_the_larger_maximum(F):
    def one(lens):
        w = np.zeros(R.words(8), dtype=np.uint64)
        w[0], w[1], w[2], w[3], w[5] = len(lens), sum(lens), min(lens), max(lens), 8
        return w
    for x, y in (([5, 9], [3, 7]), ([3, 7], [5, 9]), ([4], [4]), ([2, 100], [50])):
        dst = one(x)
        assert F.stats_merge(dst, one(y)) == 0
        assert dst[:6].tolist() == [len(x) + len(y), sum(x) + sum(y), min(x + y), max(x + y), 0, 8]


def test_merge_refuses_what_does_not_fit(F, fixture):
    raw, recs = fixture
    a64, a128 = R.stats_of(raw, recs, 64), R.stats_of(raw, recs, 128)
    before = a64.copy()
    assert F.stats_merge(a64, a128) == E_ARG and F.stats_merge(a128, a64) == E_ARG, "another P"
    assert F.stats_merge(a64, a64[:-1].copy()) == E_ARG and F.stats_merge(a64[:-1].copy(), a64) == E_ARG, "a length that is not that of P"
    empty128 = np.zeros(R.words(64), dtype=np.uint64)
    empty128[5] = 128
    assert F.stats_merge(empty128, a64) == E_ARG, "an empty block of another P"
    lib = F.lib()
    assert lib.fqgpu_stats_merge(None, a64.size, a64.ctypes.data_as(C.c_void_p), a64.size) == E_ARG
    assert lib.fqgpu_stats_merge(a64.ctypes.data_as(C.c_void_p), a64.size, None, a64.size) == E_ARG
    assert np.array_equal(a64, before)


def test_view_of_the_binding(F, fixture):
    raw, recs = fixture
    w = R.stats_of(raw, recs, 64)
    v, want = F.stats_view(w), R.view(w)
    assert v["base_pos"].shape == (65, 5) and v["qual_pos"].shape == (65, 64) and v["len_hist"].shape == (65,)
    for key in ("meanq_hist", "gc_hist", "len_hist", "base_pos", "qual_pos"):
        assert np.array_equal(v[key], want[key]) and np.shares_memory(v[key], w), key
    assert [int(v[k][0]) for k in ("n_records", "n_bases", "min_len", "max_len", "reads_with_n", "positions")] == \
           [want[k] for k in ("n_records", "n_bases", "min_len", "max_len", "reads_with_n", "positions")]
    assert int(v["base_pos"].sum()) == want["n_bases"] == int(v["qual_pos"].sum()) and int(v["len_hist"].sum()) == len(recs)


def test_the_renderer_round_trips_through_the_parser(fixture):
    raw, recs = fixture
    for P in (1, 64, 100, 512):
        w = R.stats_of(raw, recs, P)
        text = R.render(w)
        assert np.array_equal(R.parse(text), w), P
        assert text.startswith(b"#fqgpu-stats 1\nrecords\t%d\nbases\t%d\n" % (len(recs), int(recs["len"].sum())))
        assert all(c in b"0123456789\t\n" for c in text.split(b"\n", 1)[1].replace(b"records", b"").replace(b"bases", b"")
                   .replace(b"min_len", b"").replace(b"max_len", b"").replace(b"reads_with_n", b"").replace(b"positions", b"")
                   .replace(b"len", b"").replace(b"mq", b"").replace(b"gc", b"").replace(b"base", b"").replace(b"qual", b""))
    last = max(int(recs["len"].max()) - 1, 0)
    rows = [ln for ln in R.render(R.stats_of(raw, recs, 512)).split(b"\n") if ln.startswith(b"base\t")]
    assert len(rows) == last + 1, "rows 0 .. the last row with any count"


@pytest.fixture(scope="module")
def stats_tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stats_san") / "stats_tool_san")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "stats_tool.cpp"), "-L" + os.path.join(ROOT, "fqcomp28_amd"), "-lfqgpu",
                        "-Wl,-rpath," + os.path.join(ROOT, "fqcomp28_amd"), "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, "the sanitized build of tests/cpp/stats_tool.cpp failed: " + r.stderr[-2000:]
    return exe


ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def run(exe, *args):
    r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, env=ENV, timeout=120)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    return r


def test_the_farms_report_writer_against_the_renderer(stats_tool, fixture, tmp_path):
    raw, recs = fixture
    for P in (1, 64, 100, 512):
        w = R.stats_of(raw, recs, P)
        w.tofile(tmp_path / "w.bin")
        out = tmp_path / "report.tsv"
        r = run(stats_tool, "report", tmp_path / "w.bin", out)
        assert r.returncode == 0, r.stdout + r.stderr
        assert out.read_bytes() == R.render(w), P
        assert not os.path.exists(str(out) + ".part")
        phred_sum = int((R.view(w)["qual_pos"].sum(axis=0) * np.arange(64, dtype=np.uint64)).sum())
        assert r.stdout.strip() == "%.6f" % (phred_sum / int(w[1]))
        os.remove(out)
    # not a summary: refused, no file
    w[:-1].tofile(tmp_path / "short.bin")
    r = run(stats_tool, "report", tmp_path / "short.bin", out)
    assert r.returncode == 1 and r.stdout.startswith("refused: ") and not os.path.exists(out) and not os.path.exists(str(out) + ".part")
    # where the report cannot be written: an error, nothing left behind
    w.tofile(tmp_path / "w.bin")
    r = run(stats_tool, "report", tmp_path / "w.bin", tmp_path / "no_such_dir" / "report.tsv")
    assert r.returncode == 1 and r.stdout.startswith("refused: ")


def test_merging_through_the_shims_headers(stats_tool, fixture, tmp_path):
    raw, recs = fixture
    a, b = halves(raw, recs, 100)
    np.zeros(R.words(100), dtype=np.uint64).tofile(tmp_path / "dst.bin")
    a.tofile(tmp_path / "a.bin")
    b.tofile(tmp_path / "b.bin")
    R.stats_of(raw, recs, 64).tofile(tmp_path / "other.bin")
    r = run(stats_tool, "merge", tmp_path / "dst.bin", tmp_path / "a.bin", tmp_path / "other.bin", tmp_path / "b.bin")
    assert r.stdout.split() == ["0", str(E_ARG), "0"]
    assert np.array_equal(np.fromfile(tmp_path / "dst.bin", dtype=np.uint64), R.stats_of(raw, recs, 100))


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stats_tool") / "fqc_tool")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tools", "fqc_tool.cpp"),
                    "-L" + os.path.join(ROOT, "fqcomp28_amd"), "-lfqgpu", "-Wl,-rpath," + os.path.join(ROOT, "fqcomp28_amd"),
                    "-lpthread"], check=True)
    return exe


@pytest.mark.parametrize("args", [
    ["d", "in.fqc", "out.fastq", "--stats", "report.tsv"],
    ["x", "in.fqc", "--stats", "report.tsv"],
    ["t", "in.fqc", "--stats", "report.tsv"],
    ["t", "in.fqc", "--positions", "64"],
    ["d", "in.fqc", "out.fastq", "--positions", "64"],
    ["c", "in.fastq", "out.fqc", "--positions", "64"],
    ["c", "in.fastq", "out.fqc", "--stats", "report.tsv", "--positions", "0"],
    ["c", "in.fastq", "out.fqc", "--stats", "report.tsv", "--positions", "65536"],
    ["c", "in.fastq", "out.fqc", "--stats"],
    ["s", "in.fqc", "report.tsv", "--positions", "65536"],
    ["s", "in.fqc", "report.tsv", "--positions", "x"],
    ["s", "in.fqc"],
])
def test_usage_errors_are_said_before_any_file_or_device_is_touched(tool, tmp_path, args):
    r = subprocess.run([tool] + args, capture_output=True, text=True, cwd=tmp_path, timeout=60)
    assert r.returncode == 2 and r.stdout == "" and r.stderr, (args, r.stderr)
    assert os.listdir(tmp_path) == []


def test_the_device_calls_say_no_device_without_one(F):
    """(with a device in the machine the same calls get as far as their arguments: no handle, FQGPU_E_ARG)"""
    want = E_NO_DEVICE if F.device_count() == 0 else E_ARG
    out = np.full(R.words(4), 7, dtype=np.uint64)
    lib = F.lib()
    assert lib.fqgpu_chunk_stats(None, 4, out.ctypes.data_as(C.c_void_p), out.size) == want
    assert lib.fqgpu_dblock_stats(None, None, 4, out.ctypes.data_as(C.c_void_p), out.size) == want
    assert lib.fqgpu_chunk_stats(None, 0, None, 0) == want, "said before any argument is looked at"
    assert (out == 7).all()
