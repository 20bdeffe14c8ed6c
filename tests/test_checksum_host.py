"""The host side of the chunk checksums, no GPU: fqgpu_crc32_combine against zlib, the device calls' answer without a
device, and the chunk sums file (fqcomp28_amd/csrc/archive.hpp: ChunkSumsFile) through tests/cpp/sums_tool.cpp under
AddressSanitizer and UBSan, against a reading of its layout written here from the class comment."""
import ctypes as C
import os
import random
import struct
import subprocess
import zlib

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NO_DEVICE, E_ARG = -5, -4


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    F.lib()
    return F


def test_combine_agrees_with_zlib_for_random_splits(F):
    rng = random.Random(28)
    for _ in range(300):
        n = rng.choice([0, 1, 2, 3, 7, 64, 1000, rng.randrange(0, 5000)])
        data = rng.randbytes(n)
        cut = rng.choice([0, n, rng.randrange(0, n + 1)])  # empty halves included
        a, b = data[:cut], data[cut:]
        assert F.crc32_combine(zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(data), (n, cut)
    assert F.crc32_combine(0, 0, 0) == 0 and F.crc32_combine(0x12345678, 0, 0) == 0x12345678


def test_combine_for_lengths_around_two_to_the_32(F):
    """B = n zero bytes, which zlib digests piece by piece"""
    block = bytes(1 << 24)
    a = b"the bytes in front"
    below = [0, zlib.crc32(a)]      # digests of (2^32 - 1 zeros) and of (a + as many zeros)
    for k in range(2):
        for _ in range(255):
            below[k] = zlib.crc32(block, below[k])
        below[k] = zlib.crc32(bytes((1 << 24) - 1), below[k])
    for extra in (0, 1, 2):
        n = (1 << 32) - 1 + extra
        zeros, a_zeros = zlib.crc32(bytes(extra), below[0]), zlib.crc32(bytes(extra), below[1])
        assert F.crc32_combine(zlib.crc32(a), zeros, n) == a_zeros, n
        assert F.crc32_combine(zlib.crc32(bytes(5)), zeros, n) == zlib.crc32(bytes(5 + extra), below[0]), n


@pytest.mark.parametrize("pieces", [1, 3, 7])
def test_folding_the_chunks_of_a_fixture_gives_the_files_digest(F, golden_dir, pieces):
    raw, recs = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_1.fastq"))
    ends = [int(recs[i - 1]["qual_off"] + recs[i - 1]["len"] + 1) for i in np.linspace(0, len(recs), pieces + 1).astype(int)[1:]]
    crc, at = 0, 0
    for e in ends:
        part = raw[at:e].tobytes()
        crc = F.crc32_combine(crc, zlib.crc32(part), len(part))
        at = e
    assert at == raw.size and crc == zlib.crc32(raw.tobytes())


def test_the_device_calls_say_no_device_without_one(F):
    """(with a device in the machine the same calls get as far as their arguments: no handle, FQGPU_E_ARG)"""
    want = E_NO_DEVICE if F.device_count() == 0 else E_ARG
    crc, n = C.c_uint32(7), C.c_size_t(7)
    assert F.lib().fqgpu_chunk_crc32(None, C.byref(crc), C.byref(n)) == want and (crc.value, n.value) == (0, 0)
    crc, n = C.c_uint32(7), C.c_size_t(7)
    assert F.lib().fqgpu_dblock_crc32(None, None, C.byref(crc), C.byref(n)) == want and (crc.value, n.value) == (0, 0)


# ---------------------------------------------------------------- the chunk sums file
def fnv1a_words(head):
    """archive.hpp's checksum(head, {}): FNV-1a over 8-byte words, the tail bytewise, each part's size on top"""
    h, mask = 0xcbf29ce484222325, (1 << 64) - 1
    for part in (head, b""):
        i = 0
        while i + 8 <= len(part):
            h = ((h ^ struct.unpack_from("<Q", part, i)[0]) * 0x100000001b3) & mask
            i += 8
        for b in part[i:]:
            h = ((h ^ b) * 0x100000001b3) & mask
        h = ((h ^ len(part)) * 0x100000001b3) & mask
    return h


def read_sums(data):
    """the layout in ChunkSumsFile's class comment -> the lines sums_tool prints"""
    magic, n = struct.unpack_from("<II", data, 0)
    assert magic == struct.unpack("<I", b"FQS1")[0] and len(data) == 44 + 12 * n
    lines = ["n %d" % n]
    for i in range(n):
        lines.append("chunk %d %d %d %d" % ((i,) + struct.unpack_from("<III", data, 8 + 12 * i)))
    at = 8 + 12 * n
    file_crc, file_len, arc_size, arc_hash, own_crc, magic2 = struct.unpack_from("<IQQQII", data, at)
    assert magic2 == magic and own_crc == zlib.crc32(data[:at + 28])
    lines += ["file %d %d" % (file_crc, file_len), "archive %d %d" % (arc_size, arc_hash)]
    return lines


@pytest.fixture(scope="module")
def tool_sanitized(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sums_san") / "sums_tool_san")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "sums_tool.cpp"), "-L" + os.path.join(ROOT, "fqcomp28_amd"), "-lfqgpu",
                        "-Wl,-rpath," + os.path.join(ROOT, "fqcomp28_amd"), "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, "the sanitized build of tests/cpp/sums_tool.cpp failed: " + r.stderr[-2000:]
    return exe


ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def run(exe, *args):
    r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, env=ENV, timeout=120)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    return r


@pytest.mark.parametrize("n", [0, 1, 7, 500])
def test_sums_file_round_trip_and_an_independent_reading(F, tool_sanitized, tmp_path, n):
    arc = tmp_path / "some.fqc"
    arc.write_bytes(random.Random(n).randbytes(100000))
    w = run(tool_sanitized, "write", arc, n, 5 + n)
    assert w.returncode == 0, w.stderr
    side = str(arc) + ".fqs"
    assert os.path.exists(side) and not os.path.exists(side + ".part")
    r = run(tool_sanitized, "read", side)
    assert r.returncode == 0 and r.stdout == w.stdout
    data = open(side, "rb").read()
    lines = read_sums(data)
    assert lines == w.stdout.splitlines()
    # the file's digest is the chunks' digests folded in chunk order; the identity is that of the archive
    crc, total = 0, 0
    for line in lines[1:1 + n]:
        _, _, c, ln, _ = line.split()
        crc, total = F.crc32_combine(crc, int(c), int(ln)), total + int(ln)
    assert lines[1 + n] == "file %d %d" % (crc, total)
    head = arc.read_bytes()[:64 << 10]
    assert lines[2 + n] == "archive %d %d" % (os.path.getsize(arc), fnv1a_words(head))
    assert run(tool_sanitized, "belongs", arc).stdout.split() == ["own", "same-size"]
    with open(arc, "ab") as f:   # grown behind its sums (beyond the hashed head): still its own, the size tells
        f.write(b"more")
    assert run(tool_sanitized, "belongs", arc).stdout.split() == ["own", "other-size"]
    other = tmp_path / "other.fqc"
    other.write_bytes(random.Random(99).randbytes(100000))
    os.replace(side, str(other) + ".fqs")
    assert run(tool_sanitized, "belongs", other).stdout.split()[0] == "foreign"


def test_damaged_sums_files_are_refused_with_a_message(F, tool_sanitized, tmp_path):
    arc = tmp_path / "some.fqc"
    arc.write_bytes(random.Random(3).randbytes(5000))
    assert run(tool_sanitized, "write", arc, 9, 1).returncode == 0
    good = open(str(arc) + ".fqs", "rb").read()
    assert len(good) == 44 + 12 * 9
    bad = tmp_path / "bad.fqs"

    def refused(data, what):
        bad.write_bytes(data)
        r = run(tool_sanitized, "read", bad)
        assert r.returncode == 1 and r.stdout.startswith("refused: chunk sums file: "), (what, r.stdout, r.stderr)

    for cut in (0, 1, 4, 8, 43, 44, len(good) - 20, len(good) - 12, len(good) - 1):
        refused(good[:cut], "cut to %d" % cut)
    refused(good + b"\0", "one byte more")
    refused(good + good[8:20], "one entry more than n says")
    for at in range(len(good)):   # any single byte
        refused(good[:at] + bytes([good[at] ^ (1 << (at % 8))]) + good[at + 1:], "byte %d flipped" % at)
    rng = random.Random(7)
    for n in (1, 43, 44, 45, 152, 4096):
        refused(rng.randbytes(n), "%d random bytes" % n)
        refused(b"FQS1" + rng.randbytes(n) + b"FQS1", "random bytes between the magics")
    # a count that promises more than the file holds: nothing is read past the end
    refused(b"FQS1" + struct.pack("<I", 0xFFFFFFFF) + good[8:], "n = 2^32 - 1")
