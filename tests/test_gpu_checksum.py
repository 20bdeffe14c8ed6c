"""CRC-32 of chunks on the device (fqcomp28_amd/csrc/crc.hip behind fqgpu_chunk_crc32 / fqgpu_dblock_crc32), verified
restores and `fqc_tool t`.  The digest is zlib's CRC-32 of a chunk's canonical bytes, so every expectation here is
zlib.crc32 of bytes the test holds; all comparisons are exact."""
import json
import os
import re
import shutil
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import fqc_archive as A  # noqa: E402
import headers_oracle as HO  # noqa: E402

pytestmark = pytest.mark.gpu

E_CORRUPT, E_ARG = -3, -4
FIXTURES = ["SRR065390_sub_1", "without_ns", "SRR065390_sub_2", "SRR065390_1_first5"]


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    if F.device_count() < 1:
        pytest.fail("no GPU visible: the product path has no CPU fallback")
    return F


def crc_constants():
    """the slice geometry of crc.hip, from its source"""
    src = open(os.path.join(ROOT, "fqcomp28_amd", "csrc", "crc.hip")).read()
    return {k: int(re.search(r"constexpr unsigned %s = (\d+);" % k, src).group(1))
            for k in ("CRC_ROW_BYTES", "CRC_SLICE_BYTES", "CRC_FOLD_THREADS")}


def chunk_of(n_bytes, seed=5):
    """a well-formed FASTQ chunk of exactly n_bytes (>= 64): 64-byte records, the last one's header takes up the rest"""
    assert n_bytes >= 64
    rng = np.random.default_rng(seed)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 20)].tobytes()
    qual = (rng.integers(2, 41, 20) + 33).astype(np.uint8).tobytes()
    rec = b"@" + b"h" * (64 - 46) + b"\n" + seq + b"\n+\n" + qual + b"\n"
    assert len(rec) == 64
    body = (n_bytes - 64) // 64
    last = n_bytes - 64 * body
    out = np.empty(n_bytes, dtype=np.uint8)
    out[: 64 * body] = np.tile(np.frombuffer(rec, dtype=np.uint8), body)
    out[64 * body:] = np.frombuffer(b"@" + b"h" * (last - 46) + b"\n" + seq + b"\n+\n" + qual + b"\n", dtype=np.uint8)
    return out


def fmt_of(first_header):
    types, seps = HO.format_from_header(first_header)
    return ([0 if t == HO.NUMERIC else 1 for t in types], bytes(seps), first_header)


def first_header_of(raw):
    return raw[: int(np.argmax(raw == 10))].tobytes()


def context_for(F, raw, recs=None):
    sft, qft = F.freq_tables(raw, F.parse_fastq(raw) if recs is None else recs)
    return F.Context(sft, qft)


@pytest.fixture(scope="module")
def ctx(F, golden_dir):
    raw, recs = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_1.fastq"))
    c = context_for(F, raw, recs)
    yield c
    c.close()


def dblock_crc(ctx, raw):
    b = ctx.dblock(raw)
    try:
        return b.crc32(want_len=True)
    finally:
        b.close()


# ---------------------------------------------------------------- 1. the digest of a device block
@pytest.mark.parametrize("name", FIXTURES)
def test_dblock_crc_of_the_fixtures(F, ctx, golden_dir, name):
    raw, recs = O.load_fastq(os.path.join(golden_dir, name + ".fastq"))
    assert dblock_crc(ctx, raw) == (zlib.crc32(raw.tobytes()), raw.size)
    b = ctx.dblock(raw, recs)  # with the caller's record table
    assert b.crc32() == zlib.crc32(raw.tobytes())
    b.close()


def test_dblock_crc_of_a_single_record(F, ctx):
    for n in (64, 65, 100, 127):
        raw = chunk_of(n)
        assert len(F.parse_fastq(raw)) == 1
        assert dblock_crc(ctx, raw) == (zlib.crc32(raw.tobytes()), n)


def test_dblock_crc_around_the_row_slice_and_fold_sizes(F, ctx):
    k = crc_constants()
    row, sl, fold = k["CRC_ROW_BYTES"], k["CRC_SLICE_BYTES"], k["CRC_FOLD_THREADS"]
    edges = [row, 4 * row, 5 * row, sl, 2 * sl, 2 * sl + row, 3 * sl + 4 * row, fold * sl]
    for e in edges:
        for n in (e - 1, e, e + 1):
            raw = chunk_of(n, seed=n & 0xFFFF)
            got = dblock_crc(ctx, raw)
            print("len %d: crc %08x" % (n, got[0]))
            assert got == (zlib.crc32(raw.tobytes()), n), n


@pytest.mark.parametrize("mode", [1, 2, 3, 4, 5, 6])
def test_dblock_crc_of_nine_mib_of_every_synth_mode(F, ctx, mode):
    raw, _ = F.synth_fastq(9 << 20, mode, seed=30 + mode)
    assert dblock_crc(ctx, raw) == (zlib.crc32(raw.tobytes()), raw.size)


def test_dblock_crc_of_one_256_mib_block(F, ctx):
    raw, _ = F.synth_fastq(256 << 20, 2, seed=41)
    assert raw.size > 255 << 20
    assert dblock_crc(ctx, raw) == (zlib.crc32(raw.tobytes()), raw.size)


# ---------------------------------------------------------------- 2. every path to a chunk gives the same digest
def chunks_for_paths(F, golden_dir):
    for name in FIXTURES:
        yield name, O.load_fastq(os.path.join(golden_dir, name + ".fastq"))[0]
    yield "mode 4", F.synth_fastq(6 << 20, 4, seed=23)[0]


def test_every_path_to_a_chunk_gives_one_digest(F, golden_dir):
    for name, raw in chunks_for_paths(F, golden_dir):
        recs = F.parse_fastq(raw)
        want = (0, zlib.crc32(raw.tobytes()), raw.size)
        c = context_for(F, raw, recs)
        fmt = fmt_of(first_header_of(raw))
        for flags in (0, F.F_WRITE_BACK_N):
            for table in (recs, None):
                g = c.encode_raw(raw, flags=flags | F.F_DECODE_INDEX, recs=table, header_format=fmt, want_crc=True)
                assert g["rc"] == 0 and g["headers_rc"] == 0 and g["used_len"] == raw.size, name
                assert (0, g["crc32"], g["crc_len"]) == want, (name, flags, table is None)
                assert c.chunk_crc32() == want, "still the chunk's digest behind fqgpu_encode_end"
        args = (fmt, g["header_fields"], g["readlens"], g["seq"], g["qual"], g["n_count"], g["n_pos"], g["used_len"])
        for what, kw in (("indexes", dict(index=g["index"])), ("no indexes", {}), ("indexing", dict(build_index=True))):
            d = c.decode_chunk(*args, **kw)
            assert d["rc"] == 0 and np.array_equal(d["raw"], raw), (name, what)
            assert c.chunk_crc32() == want, (name, what)
        rc, out = c.decode_block(g["seq"], g["qual"], g["n_count"], g["n_pos"], recs, O.blank_skeleton(raw, recs))
        assert rc == 0 and np.array_equal(out, raw)
        assert c.chunk_crc32() == want, (name, "decode_block")
        rc, out = c.decode_block(g["seq"], g["qual"], g["n_count"], g["n_pos"], recs, O.blank_skeleton(raw, recs), index=g["index"])
        assert rc == 0 and c.chunk_crc32() == want, (name, "decode_block_indexed")
        c.close()


# ---------------------------------------------------------------- 3. text behind the '+' is no part of the digest
def test_plus_lines_that_repeat_the_header(F, golden_dir):
    raw, recs = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_2.fastq"))
    lines = raw.tobytes().split(b"\n")[:-1]
    assert len(lines) == 4 * len(recs)
    for r in range(len(recs)):
        lines[4 * r + 2] = b"+" + lines[4 * r][1:]
    fat = np.frombuffer(b"\n".join(lines) + b"\n", dtype=np.uint8)
    fat_recs = F.parse_fastq(fat)
    assert fat.size > raw.size and len(fat_recs) == len(recs)
    want = (0, zlib.crc32(raw.tobytes()), raw.size)   # the canonical chunk IS the fixture
    c = context_for(F, fat, fat_recs)
    fmt = fmt_of(first_header_of(raw))
    for table in (fat_recs, None):
        g = c.encode_raw(fat, recs=table, header_format=fmt, want_crc=True)
        assert g["rc"] == 0 and g["headers_rc"] == 0 and g["used_len"] == fat.size
        assert (0, g["crc32"], g["crc_len"]) == want, table is None
    d = c.decode_chunk(fmt, g["header_fields"], g["readlens"], g["seq"], g["qual"], g["n_count"], g["n_pos"], raw.size)
    assert d["rc"] == 0 and np.array_equal(d["raw"], raw)
    assert c.chunk_crc32() == want
    assert dblock_crc(c, fat) == want[1:]
    c.close()


# ---------------------------------------------------------------- 4. refusals, and the checking mode
def test_refusals_and_the_checking_mode(F, golden_dir):
    raw, recs = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_1.fastq"))
    c = context_for(F, raw, recs)
    assert c.chunk_crc32() == (E_ARG, 0, 0), "a fresh handle holds no chunk"
    fmt = fmt_of(first_header_of(raw))
    g = c.encode_raw(raw, flags=F.F_DECODE_INDEX, header_format=fmt)
    args = (fmt, g["header_fields"], g["readlens"], g["seq"], g["qual"], g["n_count"], g["n_pos"], g["used_len"])
    want = (0, zlib.crc32(raw.tobytes()), raw.size)
    # a damaged quality stream that the decoder refuses (most single bits are; take the first that is)
    for at in range(g["qual"].size // 2, g["qual"].size // 2 + 64):
        q = g["qual"].copy()
        q[at] ^= 0x10
        d = c.decode_chunk(fmt, g["header_fields"], g["readlens"], g["seq"], q, g["n_count"], g["n_pos"], g["used_len"])
        if d["rc"] != 0:
            break
    assert d["rc"] == E_CORRUPT
    assert c.chunk_crc32() == (E_ARG, 0, 0), "nothing to digest after a failed decode"
    assert c.decode_chunk(*args)["rc"] == 0 and c.chunk_crc32() == want
    r = c.decode_chunk_range(*args, 3, 40, index=g["index"])
    assert r["rc"] == 0
    assert c.chunk_crc32() == (E_ARG, 0, 0), "a range is not digested"
    # raw_out == NULL: refused unless the handle only checks
    d = c.decode_chunk(*args, want_raw=False)
    assert d["rc"] == E_ARG and c.chunk_crc32() == (E_ARG, 0, 0)
    c.set_check_only(True)
    for kw in ({}, dict(index=g["index"])):
        d = c.decode_chunk(*args, want_raw=False, **kw)
        assert d["rc"] == 0 and d["raw"] is None and d["laid_out_len"] == raw.size and d["bad_record"] is None
        assert np.array_equal(d["recs"], recs)
        assert c.chunk_crc32() == want
    c.set_check_only(False)
    # a decode that is refused for its arguments ends the digest of the chunk before it as well
    assert c.decode_chunk(*args)["rc"] == 0 and c.chunk_crc32() == want
    assert c.decode_chunk(*args, want_raw=False)["rc"] == E_ARG
    assert c.chunk_crc32() == (E_ARG, 0, 0), "the handle answers for no chunk after a refused decode"
    assert c.decode_chunk(*args)["rc"] == 0 and c.chunk_crc32() == want
    rc, _ = c.decode_block(g["seq"], g["qual"], g["n_count"][:-1], g["n_pos"], recs, O.blank_skeleton(raw, recs))
    assert rc == E_CORRUPT, "an n_count shorter than the record table"
    assert c.chunk_crc32() == (E_ARG, 0, 0)
    c.close()


# ---------------------------------------------------------------- 5. - 7. the farm and the tool
@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sums") / "fqc_tool")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-o", exe, os.path.join(ROOT, "tools", "fqc_tool.cpp"),
                    "-L" + os.path.join(ROOT, "fqcomp28_amd"), "-lfqgpu", "-Wl,-rpath," + os.path.join(ROOT, "fqcomp28_amd"),
                    "-lpthread"], check=True)
    return exe


def run_any(tool, *args):
    return subprocess.run([tool] + [str(a) for a in args], capture_output=True, text=True, timeout=600)


def run_tool(tool, *args):
    r = run_any(tool, *args)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1]), r.stderr


def read_sums(path):
    """the layout in ChunkSumsFile's class comment (fqcomp28_amd/csrc/archive.hpp)
    -> ([(crc32, canonical length, n_records)], file crc32, file length, archive size)"""
    data = open(path, "rb").read()
    magic, n = struct.unpack_from("<II", data, 0)
    assert magic == struct.unpack("<I", b"FQS1")[0] and len(data) == 44 + 12 * n
    sums = [struct.unpack_from("<III", data, 8 + 12 * i) for i in range(n)]
    at = 8 + 12 * n
    file_crc, file_len, arc_size, _, own_crc, magic2 = struct.unpack_from("<IQQQII", data, at)
    assert magic2 == magic and own_crc == zlib.crc32(data[:at + 28])
    return sums, file_crc, file_len, arc_size


def same_blocks(a, b):
    assert a[:3] == b[:3] and len(a[3]) == len(b[3])
    for x, y in zip(a[3], b[3]):   # blocks sorted by chunk: the same fields, byte for byte
        assert (x.idx, x.total, x.n_records, x.seq, x.qual, x.readlens, x.n_count, x.n_pos, x.fields) == \
               (y.idx, y.total, y.n_records, y.seq, y.qual, y.readlens, y.n_count, y.n_pos, y.fields)


@pytest.fixture(scope="module")
def farm(F, tool, tmp_path_factory):
    """44 MiB of mode 4 compressed with -R 8: plain, --checksum, --checksum --index"""
    d = tmp_path_factory.mktemp("sums_farm")
    raw, _ = F.synth_fastq(44 << 20, 4, seed=29)
    src = d / "in.fastq"
    raw.tofile(src)
    reps = {}
    for name, opts in (("plain", []), ("sums", ["--checksum"]), ("both", ["--checksum", "--index"])):
        reps[name], _ = run_tool(tool, "c", src, d / (name + ".fqc"), "-t", 3, "-R", 8, "-S", 4, *opts)
    return dict(dir=d, raw=raw, src=src, reps=reps)


def test_farm_writes_the_sums_and_verifies_every_restore(F, tool, farm):
    d, raw, reps = farm["dir"], farm["raw"], farm["reps"]
    plain = A.read_archive(str(d / "plain.fqc"))
    assert not os.path.exists(str(d / "plain.fqc") + ".fqs") and "sums" not in reps["plain"]
    want_file = zlib.crc32(raw.tobytes())
    for name in ("sums", "both"):
        arc = d / (name + ".fqc")
        rep = reps[name]
        blocks = rep["blocks"]
        assert blocks >= 5 and rep["sums"] == "written" and rep["crc32"] == "%08x" % want_file
        same_blocks(plain, A.read_archive(str(arc)))
        assert os.path.exists(str(arc) + ".fqx") == (name == "both")
        sums, file_crc, file_len, arc_size = read_sums(str(arc) + ".fqs")
        assert len(sums) == blocks and arc_size == os.path.getsize(arc) and not os.path.exists(str(arc) + ".fqs.part")
        at = 0
        for b, (crc, length, n_records) in zip(plain[3], sums):
            assert (crc, length, n_records) == (zlib.crc32(raw[at: at + b.total].tobytes()), b.total, b.n_records), b.idx
            at += b.total
        assert at == raw.size and (file_crc, file_len) == (want_file, raw.size)
        back = d / "back.fastq"
        rep_d, _ = run_tool(tool, "d", arc, back, "-t", 3)
        assert rep_d["verified"] == blocks and rep_d["sums"] == "used" and rep_d["crc32"] == "%08x" % want_file
        assert np.array_equal(np.fromfile(back, dtype=np.uint8), raw)
        os.remove(back)
        before = sorted(os.listdir(d))
        rep_t, _ = run_tool(tool, "t", arc, "-t", 3)
        assert rep_t["verified"] == blocks and rep_t["crc32"] == "%08x" % want_file
        assert rep_t["index"] == ("used" if name == "both" else "none")
        assert sorted(os.listdir(d)) == before, "t writes no file"
        # a range is never verified
        rep_r, _ = run_tool(tool, "d", arc, back, "-t", 2, "--records", "5:4000")
        assert rep_r["verified"] == 0
        os.remove(back)
    # without a sums file: d as ever, t decodes everything and says that nothing was compared
    rep_d, _ = run_tool(tool, "d", d / "plain.fqc", d / "back.fastq", "-t", 3)
    assert rep_d["verified"] == 0 and rep_d["sums"] == "none"
    os.remove(d / "back.fastq")
    rep_t, err = run_tool(tool, "t", d / "plain.fqc", "-t", 3)
    assert rep_t["sums"] == "none" and rep_t["verified"] == 0 and "no chunk sums file" in err


def write_variant(F, path, arc, change):
    """the archive with one block changed by change(block, recs table helpers) -> the block's chunk number"""
    first_header, sft, qft, blocks, _ = arc
    k = change(blocks)
    A.write_archive(str(path), first_header, sft, qft, blocks)
    return k


def recode(F, part, fn, dtype):
    orig, c = part
    v = np.frombuffer(F.memdecompress(np.frombuffer(c, dtype=np.uint8), orig).tobytes(), dtype=dtype).copy()
    fn(v)
    out = v.tobytes()
    return (len(out), F.memcompress(np.frombuffer(out, dtype=np.uint8)).tobytes())


def test_damage_the_format_lets_through_is_found_by_the_sums(F, tool, farm):
    """Two well-formed archives that differ from the original in one VALIDLY recoded side stream: nothing in the format
    notices (the restore succeeds, with other bytes); the chunk sums do."""
    d, raw = farm["dir"], farm["raw"]
    good = d / "sums.fqc"
    types, _ = HO.format_from_header(A.read_archive(str(good))[0])
    id_field = [i for i, t in enumerate(types) if t == HO.NUMERIC][0]
    K = 2

    def one_read_id(blocks):
        def bump(deltas):
            ids = np.cumsum(deltas.astype(np.int64))   # (the dataset's first header holds id 0)
            r = next(r for r in range(1, len(ids) - 1) if len(str(int(ids[r]))) == len(str(int(ids[r]) + 1)))
            deltas[r] += 1
            deltas[r + 1] -= 1
        blocks[K].fields[id_field][0] = recode(F, blocks[K].fields[id_field][0], bump, "<u4")
        return K

    def one_n_moved(blocks):
        b = blocks[K]
        counts = np.frombuffer(F.memdecompress(np.frombuffer(b.n_count[1], dtype=np.uint8), b.n_count[0]).tobytes(), dtype="<u2")
        lens = np.frombuffer(F.memdecompress(np.frombuffer(b.readlens[1], dtype=np.uint8), b.readlens[0]).tobytes(), dtype="<u2")
        first = np.concatenate(([0], np.cumsum(counts.astype(np.int64))))

        def move(pos):
            r = next(r for r in range(len(counts)) if counts[r] == 1 and int(pos[first[r]]) + 1 < int(lens[r]))
            pos[first[r]] += 1
        b.n_pos = recode(F, b.n_pos, move, "<u2")
        return K

    for what, change in (("one read id", one_read_id), ("one N moved", one_n_moved)):
        bad = d / "variant.fqc"
        k = write_variant(F, bad, A.read_archive(str(good)), change)
        back = d / "variant.fastq"
        side = str(bad) + ".fqs"
        if os.path.exists(side):
            os.remove(side)
        rep, _ = run_tool(tool, "d", bad, back, "-t", 3)          # no sums: nothing notices
        got = np.fromfile(back, dtype=np.uint8)
        assert rep["verified"] == 0 and got.size == raw.size and not np.array_equal(got, raw), what
        os.remove(back)
        shutil.copy(str(good) + ".fqs", side)                       # the head is unchanged: the sums still belong
        r = run_any(tool, "d", bad, back, "-t", 3)
        assert r.returncode == 1 and "checksum of chunk %d does not hold" % k in r.stderr, (what, r.stdout, r.stderr)
        assert not os.path.exists(back) and not os.path.exists(str(back) + ".part")
        r = run_any(tool, "t", bad, "-t", 3)
        assert r.returncode == 1 and "checksum of chunk %d does not hold" % k in r.stderr, (what, r.stdout, r.stderr)
        os.remove(side)
        os.remove(bad)


def test_the_sums_file_is_optional_for_d_but_not_for_t(F, tool, farm, tmp_path):
    d, raw, blocks = farm["dir"], farm["raw"], farm["reps"]["sums"]["blocks"]
    arc = tmp_path / "a.fqc"
    shutil.copy(d / "sums.fqc", arc)
    side = str(arc) + ".fqs"
    good = open(str(d / "sums.fqc") + ".fqs", "rb").read()
    raw2, _ = F.synth_fastq(12 << 20, 2, seed=31)
    src2 = tmp_path / "in2.fastq"
    raw2.tofile(src2)
    run_tool(tool, "c", src2, tmp_path / "other.fqc", "-t", 2, "-R", 8, "-S", 4, "--checksum")
    foreign = open(str(tmp_path / "other.fqc") + ".fqs", "rb").read()
    back = tmp_path / "back.fastq"
    for what, data in (("cut", good[:-20]), ("a byte flipped", good[:21] + bytes([good[21] ^ 0x40]) + good[22:]), ("foreign", foreign)):
        open(side, "wb").write(data)
        rep, err = run_tool(tool, "d", arc, back, "-t", 3)
        assert rep["verified"] == 0 and rep["sums"] == "unusable" and "not used" in err and ".fqs" in err, (what, err)
        assert np.array_equal(np.fromfile(back, dtype=np.uint8), raw), what
        os.remove(back)
        r = run_any(tool, "t", arc, "-t", 3)
        assert r.returncode == 1 and ".fqs" in r.stderr, (what, r.stdout, r.stderr)
    # the good one again: verified
    open(side, "wb").write(good)
    rep, _ = run_tool(tool, "t", arc, "-t", 3)
    assert rep["verified"] == blocks
    # a plain compression onto the same name removes the sums file
    run_tool(tool, "c", src2, arc, "-t", 2, "-R", 8, "-S", 4)
    assert not os.path.exists(side)
