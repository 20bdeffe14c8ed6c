"""Host side of building a decode index while decoding (CPU only): fqc_tool's `x` command refuses what it cannot do and
leaves no file, and the index file a decode builds -- written to `<archive>.fqx.part`, closed, renamed
(process.hpp: detail::DecodeIndexBuilder) -- reads back, under AddressSanitizer and UBSan.  The GPU side is
tests/test_gpu_build_index.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "fqcomp28_amd")
LINK = ["-L" + LIBDIR, "-lfqgpu", "-Wl,-rpath," + LIBDIR, "-lpthread"]


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    """fqc_tool against the library, as the GPU tests build it (the library loads without a GPU)"""
    if not os.path.exists(os.path.join(LIBDIR, "libfqgpu.so")):
        pytest.fail("libfqgpu.so is not built (run __graft_entry__.build())")
    exe = str(tmp_path_factory.mktemp("tool") / "fqc_tool")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-o", exe, os.path.join(ROOT, "tools", "fqc_tool.cpp")] + LINK, check=True)
    return exe


def run(tool, *args):
    return subprocess.run([tool] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def test_x_with_a_missing_archive_fails_and_leaves_no_file(tool, tmp_path):
    arc = tmp_path / "missing.fqc"
    r = run(tool, "x", arc)
    assert r.returncode != 0 and "fqc_tool:" in r.stderr and "missing.fqc" in r.stderr
    assert r.stdout == "" and os.listdir(tmp_path) == []


def test_x_with_surplus_arguments_fails_and_leaves_no_file(tool, tmp_path):
    arc = tmp_path / "a.fqc"
    arc.write_bytes(b"\0" * 64)  # (never opened: the arguments are judged first)
    for extra in (["out.fastq"], ["-t", "2", "out.fastq"], ["--records", "0:5"], ["--index-stride"]):
        r = run(tool, "x", arc, *extra)
        assert r.returncode != 0 and r.stdout == "", extra
        assert "usage" in r.stderr or "needs a value" in r.stderr, (extra, r.stderr)
        assert sorted(os.listdir(tmp_path)) == ["a.fqc"], extra
    r = run(tool, "x")
    assert r.returncode != 0 and "fqc_tool x <in.fqc>" in r.stderr


def test_x_with_a_file_that_is_no_archive_fails_and_leaves_no_file(tool, tmp_path):
    arc = tmp_path / "a.fqc"
    arc.write_bytes(b"not an archive at all" * 10)
    r = run(tool, "x", arc)
    assert r.returncode != 0 and "fqc_tool:" in r.stderr
    assert sorted(os.listdir(tmp_path)) == ["a.fqc"]


def test_index_file_built_in_a_part_file_reads_back_under_asan_and_ubsan(tmp_path):
    """tests/cpp/index_build_check.cpp with the sanitizers the container's host code is checked with (test_archive.py)"""
    exe = str(tmp_path / "index_build_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "index_build_check.cpp")] + LINK, capture_output=True, text=True)
    if r.returncode != 0 and any(x in r.stderr.lower() for x in ("libasan", "libubsan", "-fsanitize")):
        pytest.skip("no sanitizer runtime for g++ here: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    work = tmp_path / "work"
    work.mkdir()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(work)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout, r.stderr[-3000:])
    assert "index_build_check ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert sorted(os.listdir(work)) == ["a.fqc", "a.fqc.fqx"]
