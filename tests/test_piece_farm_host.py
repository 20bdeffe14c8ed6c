"""The ordered hand-out loop of the restores, no GPU: detail::pieceFarm (fqcomp28_amd/csrc/process.hpp) driven by
tests/cpp/piece_farm_check.cpp with a worker state that holds no workspace, under AddressSanitizer + UBSan and under
ThreadSanitizer -- every item once and in its place, the worker count and the report's shape, a failing item that releases the
waiters, reaches the caller as itself and leaves no file, and the refusal of an empty device list."""
import os
import platform
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINK = ["-L" + os.path.join(ROOT, "fqcomp28_amd"), "-lfqgpu", "-Wl,-rpath," + os.path.join(ROOT, "fqcomp28_amd"), "-lpthread"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1",
           TSAN_OPTIONS="halt_on_error=0")
N_ITEMS, THROWS, WORKERS = 40, 7, 4


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    F.lib()
    return F


def compile_check(exe, *flags):
    return subprocess.run(["g++", "-std=c++17", "-O1", "-g", *flags, "-o", exe, os.path.join(ROOT, "tests", "cpp", "piece_farm_check.cpp")] + LINK,
                          capture_output=True, text=True)


@pytest.fixture(scope="module")
def check_sanitized(F, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("farm_san") / "piece_farm_check_san")
    r = compile_check(exe, "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")
    assert r.returncode == 0, "the sanitized build of tests/cpp/piece_farm_check.cpp failed: " + r.stderr[-2000:]
    return exe


@pytest.fixture(scope="module")
def check_tsan(F, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("farm_tsan") / "piece_farm_check_tsan")
    r = compile_check(exe, "-fsanitize=thread")
    assert r.returncode == 0, "the ThreadSanitizer build of tests/cpp/piece_farm_check.cpp failed: " + r.stderr[-2000:]
    return exe


def run(exe, *args, prefix=()):
    """(a farm that does not end is a failure: subprocess.TimeoutExpired)"""
    r = subprocess.run([*prefix, exe, *[str(a) for a in args]], capture_output=True, text=True, env=ENV, timeout=300)
    for word in ("AddressSanitizer", "runtime error", "ThreadSanitizer"):
        assert word not in r.stderr, r.stderr[-3000:]
    return r


def no_aslr():
    # g++ 11's ThreadSanitizer aborts ("unexpected memory mapping") where the kernel randomises mmap with more than 28
    # bits; the runs therefore go without address randomisation, a setting of these processes alone
    return ["setarch", platform.machine(), "-R"] if shutil.which("setarch") else []


def item(k, n):
    return bytes((131 * k + 7 * i) & 0xFF for i in range(n))


def check_ok(r, out):
    """the program has checked the counts (every item once; 4 entries that sum to 40; 8 entries, at most 3 non-zero, for 3
    items; no body for 0 items); here the file"""
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    sizes = [int(x) for x in lines[0].split()[1:]]
    assert lines[0].startswith("sizes") and len(sizes) == N_ITEMS and 0 in sizes and max(sizes) > 100000
    want = b"".join(item(k, n) for k, n in enumerate(sizes))
    assert lines[1] == "written %d" % len(want)
    assert open(out, "rb").read() == want
    assert not os.path.exists(str(out) + ".part")


def check_throw(r, out):
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == "failed: item 7 could not be decoded"
    # items are handed out in order, and each of the other three workers waits in the writer with at most one item behind
    # the one that never came
    assert lines[1].startswith("started ") and THROWS <= int(lines[1].split()[1]) <= THROWS + (WORKERS - 1), r.stdout
    assert not os.path.exists(out) and not os.path.exists(str(out) + ".part")


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_every_item_runs_once_and_lands_in_its_place(check_sanitized, tmp_path, seed):
    out = tmp_path / "o.bin"
    check_ok(run(check_sanitized, out, seed, "ok"), out)
    assert os.listdir(tmp_path) == ["o.bin"]


def test_a_failing_item_reaches_the_caller_and_leaves_no_file(check_sanitized, tmp_path):
    out = tmp_path / "o.bin"
    check_throw(run(check_sanitized, out, 5, "throw"), out)
    assert os.listdir(tmp_path) == []


def test_no_device_is_refused_before_any_file_is_created(check_sanitized, tmp_path):
    out = tmp_path / "o.bin"
    r = run(check_sanitized, out, 1, "nodevice")
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines() == ["refused: pieceFarmCheck: no device"]
    assert os.listdir(tmp_path) == []


def test_the_farm_under_thread_sanitizer(check_tsan, tmp_path):
    out = tmp_path / "o.bin"
    check_ok(run(check_tsan, out, 4, "ok", prefix=no_aslr()), out)
    check_throw(run(check_tsan, tmp_path / "t.bin", 4, "throw", prefix=no_aslr()), tmp_path / "t.bin")
    r = run(check_tsan, tmp_path / "n.bin", 4, "nodevice", prefix=no_aslr())
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.listdir(tmp_path) == ["o.bin"]
