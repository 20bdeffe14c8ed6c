"""The host side of the FASTA restore, no GPU: fqgpu_decode_chunk_fasta's answer without a device, the ordered piece
writer and the block read that leaves the quality stream in the file (fqcomp28_amd/csrc/archive.hpp, through
tests/cpp/fasta_tool.cpp under AddressSanitizer + UBSan and once under ThreadSanitizer), and fqc_tool's refusals of
--fasta where it has no meaning."""
import ctypes as C
import os
import platform
import shutil
import subprocess
import sys

import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import fqc_archive as A  # noqa: E402

E_NO_DEVICE, E_ARG = -5, -4
LINK = ["-L" + os.path.join(ROOT, "fqcomp28_amd"), "-lfqgpu", "-Wl,-rpath," + os.path.join(ROOT, "fqcomp28_amd"), "-lpthread"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1",
           TSAN_OPTIONS="halt_on_error=0")
N_PIECES = 40


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    F.lib()
    return F


def test_the_fasta_export_says_no_device_without_one(F):
    """(with a device in the machine the call gets as far as its arguments: no handle, FQGPU_E_ARG)"""
    want = E_NO_DEVICE if F.device_count() == 0 else E_ARG
    out_len, bad = C.c_size_t(7), C.c_size_t(7)
    rc = F.lib().fqgpu_decode_chunk_fasta(None, None, None, 0, None, 0, None, 0, None, 0, None, 0, 0, 0, 0, None, 0,
                                          C.byref(out_len), None, C.byref(bad))
    assert rc == want and out_len.value == 0
    assert F.lib().fqgpu_decode_chunk_fasta(None, None, None, 0, None, 0, None, 0, None, 0, None, 0, 0, 0, 0, None, 0,
                                            None, None, None) == want


# ---------------------------------------------------------------- tests/cpp/fasta_tool.cpp
def compile_tool(exe, *flags):
    return subprocess.run(["g++", "-std=c++17", "-O1", "-g", *flags, "-o", exe, os.path.join(ROOT, "tests", "cpp", "fasta_tool.cpp")] + LINK,
                          capture_output=True, text=True)


@pytest.fixture(scope="module")
def tool_sanitized(F, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fasta_san") / "fasta_tool_san")
    r = compile_tool(exe, "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")
    assert r.returncode == 0, "the sanitized build of tests/cpp/fasta_tool.cpp failed: " + r.stderr[-2000:]
    return exe


@pytest.fixture(scope="module")
def tool_tsan(F, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fasta_tsan") / "fasta_tool_tsan")
    r = compile_tool(exe, "-fsanitize=thread")
    assert r.returncode == 0, "the ThreadSanitizer build of tests/cpp/fasta_tool.cpp failed: " + r.stderr[-2000:]
    return exe


def run(exe, *args, prefix=()):
    r = subprocess.run([*prefix, exe, *[str(a) for a in args]], capture_output=True, text=True, env=ENV, timeout=300)
    for word in ("AddressSanitizer", "runtime error", "ThreadSanitizer"):
        assert word not in r.stderr, r.stderr[-3000:]
    return r


def piece(k, n):
    return bytes((131 * k + 7 * i) & 0xFF for i in range(n))


def check_ordered_file(r, out):
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    sizes = [int(x) for x in lines[0].split()[1:]]
    assert lines[0].startswith("sizes") and len(sizes) == N_PIECES and 0 in sizes and max(sizes) > 100000
    want = b"".join(piece(k, n) for k, n in enumerate(sizes))
    assert lines[1] == "written %d" % len(want)
    assert open(out, "rb").read() == want
    assert not os.path.exists(str(out) + ".part")


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_ordered_writer_places_pieces_that_finish_out_of_order(tool_sanitized, tmp_path, seed):
    out = tmp_path / "o.fasta"
    check_ordered_file(run(tool_sanitized, "writer", out, seed, "ok"), out)


@pytest.mark.parametrize("mode", ["throw", "abort"])
def test_ordered_writer_failure_releases_the_waiters_and_leaves_no_file(tool_sanitized, tmp_path, mode):
    out = tmp_path / "o.fasta"
    r = run(tool_sanitized, "writer", out, 5, mode)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[0].startswith("failed: ")
    if mode == "throw":
        assert "piece 7 could not be decoded" in lines[0]
    # the three other workers sat in the writer with pieces behind the one that never came (abort: the late one too)
    assert int(lines[-1].split()[1]) >= 3, r.stdout
    assert not os.path.exists(out) and not os.path.exists(str(out) + ".part")


def test_ordered_writer_under_thread_sanitizer(tool_tsan, tmp_path):
    # g++ 11's ThreadSanitizer aborts ("unexpected memory mapping") where the kernel randomises mmap with more than 28
    # bits; the runs therefore go without address randomisation, a setting of these processes alone
    no_aslr = ["setarch", platform.machine(), "-R"] if shutil.which("setarch") else []
    out = tmp_path / "o.fasta"
    check_ordered_file(run(tool_tsan, "writer", out, 4, "ok", prefix=no_aslr), out)
    r = run(tool_tsan, "writer", tmp_path / "t.fasta", 4, "throw", prefix=no_aslr)
    assert r.returncode == 0 and not os.path.exists(tmp_path / "t.fasta") and not os.path.exists(str(tmp_path / "t.fasta") + ".part")


def test_block_read_without_the_quality_stream_leaves_it_in_the_file(F, tool_sanitized, tmp_path, golden_dir):
    from test_archive import oracle_archive
    raw, recs = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_1.fastq"))
    arc = str(tmp_path / "o.fqc")
    oracle_archive(F, arc, raw, recs, 5, order=[3, 0, 4, 1, 2])
    _, _, _, blocks, entries = A.read_archive(arc)
    # the blocks' extents, from the index of the Python reading: a block ends where the next one in the file begins
    offs = sorted(off for off, _ in entries)
    ends = dict(zip(offs, offs[1:] + [os.path.getsize(arc) - 16 * len(entries)]))
    extent = {idx: ends[off] - off for off, idx in entries}
    r = run(tool_sanitized, "skipqual", arc)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(blocks) == 5
    for k, (line, b) in enumerate(zip(lines, blocks)):
        assert len(b.qual) > 1000
        assert line == "block %d extent %d qual %d skipped %d same 1" % (k, extent[b.idx], len(b.qual), extent[b.idx] - len(b.qual)), line


# ---------------------------------------------------------------- fqc_tool usage
@pytest.fixture(scope="module")
def fqc_tool(F, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fasta_cli") / "fqc_tool")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-o", exe, os.path.join(ROOT, "tools", "fqc_tool.cpp")] + LINK, check=True)
    return exe


@pytest.mark.parametrize("args", [["c", "in.fastq", "out.fqc", "--fasta"], ["x", "in.fqc", "--fasta"], ["t", "in.fqc", "--fasta"],
                                  ["d", "in.fqc", "out.fasta", "--fasta", "--index"],
                                  ["d", "in.fqc", "out.fasta", "--index-stride", "64", "--fasta"]])
def test_fqc_tool_refuses_fasta_where_it_has_no_meaning(fqc_tool, tmp_path, args):
    """exit 2 with a usage message, decided from the command line alone: the files named do not exist, and a run that got as
    far as opening one (or a device) would end with exit 1 and "fqc_tool:" instead"""
    r = subprocess.run([fqc_tool] + args, capture_output=True, text=True, cwd=tmp_path, timeout=60)
    assert r.returncode == 2, r.stdout + r.stderr
    assert "--fasta" in r.stderr and "fqc_tool:" not in r.stderr and r.stdout == ""
    assert os.listdir(tmp_path) == []
