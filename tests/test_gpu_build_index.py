"""A decode that leaves the decode index behind (the indexing walk, k_resolve_states and k_dindex_meta of
fqcomp28_amd/csrc/decode.hip; fqgpu_decode_chunk_indexing, fqgpu_decode_index, fqgpu_dblocks_decode_indexing; fqc_tool x and
d --index).  The reference throughout is the ENCODER's index of the same block (enc_index.h: sorted tiles and segment entry
states), code that shares nothing with the walk: the two must agree byte for byte."""
import json
import os
import shutil
import struct
import sys

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import fqc_archive as A  # noqa: E402
import headers_oracle as HO  # noqa: E402
from test_gpu_decode_chunk import FIXTURES, fmt_of, tool  # noqa: E402,F401
from test_gpu_decode_range import STRIDE, IX_HEAD, aligned, check, expect, farm_ranges, restore_ranges, run  # noqa: E402

pytestmark = pytest.mark.gpu

E_CORRUPT = -3
B = (256, 8192)  # contexts of the sequence / quality stream


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    assert F.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return F


def snap_bytes(stream):
    return 16 + 2 * B[stream]


def index_fields(ix, stream):
    """-> (stride, n_snap, n_sym, [(bitpos, prev bytes, states)])"""
    ix = bytes(ix)
    magic, s, stride, n_snap, n_sym, _ = struct.unpack_from("<IIIIQQ", ix, 0)
    assert magic == 0x58495146 and s == stream and len(ix) == IX_HEAD + n_snap * snap_bytes(stream)
    snaps = []
    for k in range(n_snap):
        at = IX_HEAD + k * snap_bytes(stream)
        snaps.append((struct.unpack_from("<Q", ix, at)[0], ix[at + 8: at + 12], np.frombuffer(ix, "<u2", B[stream], at + 16)))
    return stride, n_snap, n_sym, snaps


def same_index(got, want, what):
    """equality, and on failure where the two differ"""
    for s in (0, 1):
        g, w = bytes(got[s]), bytes(want[s])
        if g == w:
            continue
        assert len(g) == len(w), (what, s, len(g), len(w))
        at = next(i for i in range(len(g)) if g[i] != w[i])
        k, off = divmod(at - IX_HEAD, snap_bytes(s)) if at >= IX_HEAD else (-1, at)
        field = "header" if k < 0 else "bitpos" if off < 8 else "prev" if off < 12 else "word3" if off < 16 else "state of context %d" % ((off - 16) // 2)
        raise AssertionError("%s: stream %d differs at byte %d: snapshot %d, %s (got %d, want %d)" % (what, s, at, k + 1, field, g[at], w[at]))


def build(F, raw, first, sft=None, qft=None, stride=STRIDE):
    """encode with F_DECODE_INDEX on one context; decode the streams with build_index on a FRESH one.
    -> (encode result, decode result)"""
    if sft is None:
        sft, qft = F.freq_tables(raw, F.parse_fastq(raw))
    enc, dec = F.Context(sft, qft), F.Context(sft, qft)
    try:
        enc.set_index_stride(stride)
        dec.set_index_stride(stride)
        g = enc.encode_raw(raw, flags=F.F_DECODE_INDEX, header_format=fmt_of(first))
        assert g["rc"] == 0 and g["headers_rc"] == 0
        d = dec.decode_chunk(fmt_of(first), g["header_fields"], g["readlens"], g["seq"], g["qual"], g["n_count"], g["n_pos"],
                             g["used_len"], build_index=True)
        assert d["rc"] == 0 and d["bad_record"] is None, (d["rc"], d["bad_record"])
        assert np.array_equal(d["raw"], raw), int(np.argmax(d["raw"] != raw))
        # index only: nothing of the chunk comes back, the same indexes do
        d2 = dec.decode_chunk(fmt_of(first), g["header_fields"], g["readlens"], g["seq"], g["qual"], g["n_count"], g["n_pos"],
                              g["used_len"], build_index=True, want_raw=False)
        assert d2["rc"] == 0 and d2["raw"] is None and d2["laid_out_len"] == raw.size
        same_index(d2["index"], d["index"], "index-only call")
        return g, d
    finally:
        enc.close()
        dec.close()


# ---------------------------------------------------------------- 1. byte identity with the encoder's index
@pytest.mark.parametrize("name", FIXTURES)
def test_golden_fixtures_index_equals_the_encoders(F, golden_dir, name):
    raw, recs = O.load_fastq(os.path.join(golden_dir, name + ".fastq"))
    _, _, sft, qft = O.freq_tables(raw, recs)
    g, d = build(F, raw, A.headers_of(raw, recs[:1])[0], sft, qft)
    same_index(d["index"], g["index"], name)
    assert index_fields(d["index"][0], 0)[1] == (int(recs["len"].sum()) - 1) // STRIDE


@pytest.mark.parametrize("mode", [2, 3, 4, 5, 6])
def test_synth_index_equals_the_encoders(F, mode):
    raw, _ = F.synth_fastq(12 << 20, mode, seed=60 + mode)
    recs = F.parse_fastq(raw)
    g, d = build(F, raw, A.headers_of(raw, recs[:1])[0])
    stride, n_snap, n_sym, snaps = index_fields(g["index"][0], 0)
    assert stride == STRIDE and n_snap > 24 and n_sym == int(recs["len"].sum())  # dozens of strides
    same_index(d["index"], g["index"], "mode %d" % mode)
    if mode == 4:  # the host-pointer encode keeps the chunk's own Ns in `prev`: the corner the restored chunk is read for
        assert any(b"N" in prev for _, prev, _ in snaps)
        assert any(b"N" in prev for _, prev, _ in index_fields(d["index"][0], 0)[3])


# ---------------------------------------------------------------- 2. boundaries
@pytest.mark.parametrize("mode", [2, 4])
def test_records_that_start_at_and_beside_a_boundary(F, mode):
    targets = [5 * STRIDE, 11 * STRIDE - 1, 17 * STRIDE + 1, 23 * STRIDE]
    raw, recs, hit = aligned(F, mode, 12 << 20, targets, seed=60 + mode)
    assert len(hit) >= 3
    rs = np.concatenate([[0], np.cumsum(recs["len"].astype(np.int64))])
    assert all(rs[r] in targets for r in hit)
    g, d = build(F, raw, A.headers_of(raw, recs[:1])[0])
    same_index(d["index"], g["index"], "aligned mode %d" % mode)


@pytest.mark.parametrize("length", [3, 4, 5])
@pytest.mark.parametrize("shift", [0, 1, 2, 3, 4])
def test_short_reads_next_to_a_boundary(F, length, shift):
    """a read of 3, 4 or 5 bases that ends `shift` symbols behind the first boundary: the boundary falls on its first, a middle
    or its last position, or between it and its neighbour"""
    raw, _ = F.synth_fastq(1 << 20, 2, seed=3 + length)
    recs = F.parse_fastq(raw)
    b = raw.tobytes()
    source = [(b[int(r["seq_off"]):][:int(r["len"])], b[int(r["qual_off"]):][:int(r["len"])]) for r in recs]
    front = STRIDE + shift - length  # symbols in front of the short read
    reads, total, i = [], 0, 0
    while total + len(source[i][0]) <= front:
        reads.append(source[i])
        total += len(source[i][0])
        i += 1
    room = front - total
    if 0 < room < 3:  # no read is shorter than 3: the read in front gives the rest
        s, q = reads[-1]
        reads[-1] = (s[: room - 3], q[: room - 3])
        room = 3
    if room:
        reads.append((source[i][0][:room], source[i][1][:room]))
    reads.append((source[i + 1][0][:length], source[i + 1][1][:length]))
    total = STRIDE + shift
    for s, q in source[i + 2:]:
        if total >= 2 * STRIDE + 1000:
            break
        reads.append((s, q))
        total += len(s)
    out = np.frombuffer(b"".join(b"@r.%d\n" % k + s + b"\n+\n" + q + b"\n" for k, (s, q) in enumerate(reads)), dtype=np.uint8)
    orecs = F.parse_fastq(out)
    ends = np.cumsum(orecs["len"].astype(np.int64))
    assert STRIDE + shift in ends and int(orecs[int(np.searchsorted(ends, STRIDE + shift))]["len"]) == length
    g, d = build(F, out, b"@r.0")
    assert index_fields(g["index"][0], 0)[1] == 2
    same_index(d["index"], g["index"], "length %d shift %d" % (length, shift))


# ---------------------------------------------------------------- 3. oracle-written streams
def oracle_case(F, raw, recs, sft, qft, ranges):
    e = O.OracleCtx(sft, qft).encode(raw, recs)
    assert e["rc"] == 0
    first = A.headers_of(raw, recs[:1])[0]
    _, _, streams = HO.encode_headers(A.headers_of(raw, recs), first)
    fields = [(bytes(s.flags), bytes(s.content), bytes(s.lengths)) for s in streams]
    readlens = recs["len"].astype(np.uint16)
    ctx = F.Context(sft, qft)
    try:
        ctx.set_index_stride(STRIDE)
        g = ctx.encode_raw(raw, flags=F.F_DECODE_INDEX)
        assert g["rc"] == 0 and np.array_equal(g["seq"], e["seq"]) and np.array_equal(g["qual"], e["qual"])
        d = ctx.decode_chunk(fmt_of(first), fields, readlens, e["seq"], e["qual"], e["n_count"], e["n_pos"], raw.size, build_index=True)
        assert d["rc"] == 0 and np.array_equal(d["raw"], raw)
        same_index(d["index"], g["index"], "oracle-written streams")
        for a, b in ranges:
            r = ctx.decode_chunk_range(fmt_of(first), fields, readlens, e["seq"], e["qual"], e["n_count"], e["n_pos"], raw.size,
                                       int(a), int(b), index=d["index"])
            check(r, raw, recs, int(a), int(b))
    finally:
        ctx.close()


def test_oracle_written_fixture(F, golden_dir):
    name = "SRR065390_sub_1"
    raw, recs = O.load_fastq(os.path.join(golden_dir, name + ".fastq"))
    _, _, sft, qft = O.freq_tables(raw, recs)
    n = len(recs)
    rng = np.random.default_rng(len(name) + 7)  # the ranges test_golden_ranges draws with the index
    ranges = [(0, 1), (n - 1, n), (0, n)] + [tuple(sorted(rng.choice(n + 1, 2, replace=False))) for _ in range(6)]
    oracle_case(F, raw, recs, sft, qft, ranges)


def test_oracle_written_synthetic_block(F):
    raw, _ = F.synth_fastq(3 << 20, 4, seed=21)
    recs = O.parse_fastq(raw)
    _, _, sft, qft = O.freq_tables(raw, recs)
    n = len(recs)
    oracle_case(F, raw, recs, sft, qft, [(0, 1), (n - 1, n), (0, n), (n // 3, n // 3 + 9), (n // 2, n // 2 + 1)])


# ---------------------------------------------------------------- 4. use
def test_resident_blocks_get_their_indexes_and_decode_from_them(F):
    raw, _ = F.synth_fastq(6 << 20, 4, seed=33)
    recs = F.parse_fastq(raw)
    small = raw[: int(recs[99]["qual_off"]) + int(recs[99]["len"]) + 1]  # 100 reads: fewer symbols than a stride
    sft, qft = F.freq_tables(raw, recs)
    ctx = F.Context(sft, qft)
    try:
        ctx.set_index_stride(STRIDE)
        ref = ctx.dblock(raw, recs)
        ref.encode(F.F_DECODE_INDEX)
        ctx.sync()
        want = (ref.fetch_index(0), ref.fetch_index(1))
        n_snap = (int(recs["len"].sum()) - 1) // STRIDE
        assert n_snap > 10 and [len(x) for x in want] == [32 + n_snap * (16 + 2 * B[s]) for s in (0, 1)]

        b, sb = ctx.dblock(raw, recs), ctx.dblock(small, recs[:100])
        for x in (b, sb):
            x.encode(0)
        ctx.sync()
        assert len(b.fetch_index(0)) == 0 and len(b.fetch_index(1)) == 0
        # an index already on the block is ignored and replaced: a wrong one is loaded first
        bad = [np.array(x, copy=True) for x in want]
        bad[1][IX_HEAD] ^= 1  # the first snapshot's bit position
        for s in (0, 1):
            assert b.load_index(s, bad[s]) == 0
        for x in (b, sb):
            x.wipe()
        ctx.decode_dblocks_indexing([b, sb])
        for x, r in ((b, raw), (sb, small)):
            assert x.status()[0] == 0
            assert np.array_equal(x.fetch_raw()[: r.size], r)
        same_index((b.fetch_index(0), b.fetch_index(1)), want, "resident block")
        assert [len(sb.fetch_index(s)) for s in (0, 1)] == [32, 32]
        assert index_fields(sb.fetch_index(1), 1)[1] == 0

        # the following decode runs from the indexes the block now holds
        b.wipe()
        ctx.decode_dblocks([b])
        assert b.status()[0] == 0 and np.array_equal(b.fetch_raw()[: raw.size], raw)
        # ... which a decode of the same block with the wrong bit position shows: only the indexed walk reads it
        for s in (0, 1):
            assert b.load_index(s, bad[s]) == 0
        b.wipe()
        ctx.decode_dblocks([b])
        assert b.status()[0] == E_CORRUPT
        for x in (ref, b, sb):
            x.close()
    finally:
        ctx.close()


# ---------------------------------------------------------------- 5. damage
def test_damaged_streams_report_what_the_plain_decode_reports_and_leave_no_index(F, golden_dir):
    raw, _ = F.synth_fastq(2 << 20, 4, seed=12)
    recs = F.parse_fastq(raw)
    first = A.headers_of(raw, recs[:1])[0]
    sft, qft = F.freq_tables(raw, recs)
    ctx = F.Context(sft, qft)
    try:
        ctx.set_index_stride(STRIDE)
        g = ctx.encode_raw(raw, header_format=fmt_of(first))
        assert g["rc"] == 0
        skeleton = O.blank_skeleton(raw, recs)
        n_corrupt = 0
        for stream, frac in [("seq", 0.1), ("seq", 0.5), ("seq", 0.93), ("qual", 0.07), ("qual", 0.5), ("qual", 0.77), ("qual", 0.99)]:
            s = {k: np.array(g[k], copy=True) for k in ("seq", "qual")}
            s[stream][int(frac * s[stream].size)] ^= 0x5A
            plain, _ = ctx.decode_block(s["seq"], s["qual"], g["n_count"], g["n_pos"], recs, skeleton)  # the judge
            n_corrupt += plain == E_CORRUPT
            d = ctx.decode_chunk(fmt_of(first), g["header_fields"], g["readlens"], s["seq"], s["qual"], g["n_count"], g["n_pos"],
                                 g["used_len"], build_index=True)
            assert d["rc"] == plain, (stream, frac, d["rc"], plain)
            if plain != 0:
                assert d["bad_record"] is None and [len(x) for x in d["index"]] == [0, 0], (stream, frac)
            # the handle goes on: the undamaged streams right afterwards
            ok = ctx.decode_chunk(fmt_of(first), g["header_fields"], g["readlens"], g["seq"], g["qual"], g["n_count"], g["n_pos"],
                                  g["used_len"], build_index=True)
            assert ok["rc"] == 0 and np.array_equal(ok["raw"], raw) and len(ok["index"][1]) > IX_HEAD
        assert n_corrupt >= 5, n_corrupt  # the flips were chosen to be seen: the test does not pass by finding nothing

        # a resident block with a damaged quality stream: CORRUPT in its status, no index; its neighbour keeps its own
        good, hurt = ctx.dblock(raw, recs), ctx.dblock(raw, recs)
        q = np.array(g["qual"], copy=True)
        q[q.size // 2] ^= 0x5A
        good.load_streams(g["seq"], g["qual"], g["n_count"], g["n_pos"])
        hurt.load_streams(g["seq"], q, g["n_count"], g["n_pos"])
        ctx.decode_dblocks([hurt])
        plain = hurt.status()[0]
        assert plain == E_CORRUPT
        ctx.decode_dblocks_indexing([good, hurt])
        assert good.status()[0] == 0 and hurt.status()[0] == plain
        assert [len(hurt.fetch_index(s)) for s in (0, 1)] == [0, 0]
        assert len(good.fetch_index(0)) > IX_HEAD and len(good.fetch_index(1)) > IX_HEAD
        good.close()
        hurt.close()
    finally:
        ctx.close()


# ---------------------------------------------------------------- 6. the property the resolve rests on
def degenerate_contexts(ctx):
    """[(stream, context)] whose DTable holds one word twice"""
    found = []
    for stream in (0, 1):
        for c in range(B[stream]):
            _, dt = ctx.dump_tables(stream, c)
            words = dt[1:]
            assert words.size == 1 << int(dt[0] & 0xFFFF)
            if np.unique(words).size != words.size:
                found.append((stream, c))
    return found


@pytest.mark.parametrize("source", ["SRR065390_sub_1", "mode 2"])
def test_the_words_of_a_dtable_are_pairwise_distinct(F, golden_dir, source):
    if source.startswith("mode"):
        raw, _ = F.synth_fastq(4 << 20, 2, seed=62)
        recs = F.parse_fastq(raw)
        sft, qft = F.freq_tables(raw, recs)
    else:
        raw, recs = O.load_fastq(os.path.join(golden_dir, source + ".fastq"))
        _, _, sft, qft = O.freq_tables(raw, recs)
    ctx = F.Context(sft, qft)
    try:
        ctx.set_index_stride(STRIDE)
        found = degenerate_contexts(ctx)
        if not found:
            return
        # a degenerate table: the resolve takes the LOWEST state with the entry; the encoder's index must name that one
        g = ctx.encode_raw(raw, flags=F.F_DECODE_INDEX)
        assert g["rc"] == 0
        for stream, c in found:
            words = ctx.dump_tables(stream, c)[1][1:]
            for k, (_, _, states) in enumerate(index_fields(g["index"][stream], stream)[3]):
                x = int(states[c])
                lowest = int(np.argmax(words == words[x]))
                assert x == lowest, "stream %d context %d: degenerate DTable, snapshot %d holds state %d, the lowest with its entry is %d" % (
                    stream, c, k + 1, x, lowest)
    finally:
        ctx.close()


# ---------------------------------------------------------------- 7. the farm: fqc_tool x and d --index
def read_fqx(path):
    """`<archive>.fqx` by the layout archive.hpp documents (DecodeIndexFile) -> ({chunk_idx: (seq index, qual index)},
    (archive size, archive hash)); every entry's checksum is verified"""
    d = open(path, "rb").read()
    assert d[:4] == b"FQX1" and d[-4:] == b"FQX1", "not a closed decode index file"
    n, size, ahash = struct.unpack_from("<QQQ", d, len(d) - 28)
    out = {}
    for off in struct.unpack_from("<%dQ" % n, d, len(d) - 28 - 8 * n):
        idx, zero, ns, nq, want = struct.unpack_from("<IIQQQ", d, off)
        a, b = d[off + 32: off + 32 + ns], d[off + 32 + ns: off + 32 + ns + nq]
        h = 0xcbf29ce484222325  # FNV-1a over 8-byte words, then the tail's bytes, then the length; both indexes in turn
        for v in (a, b):
            whole = len(v) // 8
            for w in struct.unpack_from("<%dQ" % whole, v, 0):
                h = ((h ^ w) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
            for x in v[8 * whole:]:
                h = ((h ^ x) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
            h = ((h ^ len(v)) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
        assert zero == 0 and h == want and idx not in out, "entry of chunk %d" % idx
        out[idx] = (a, b)
    return out, (size, ahash)


def report(r):
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def no_leftovers(arc):
    assert not os.path.exists(str(arc) + ".fqx.part")


@pytest.fixture(scope="module")
def farm(F, tool, tmp_path_factory):
    """a 40 MiB mode-4 input, archived without (a.fqc) and with (b.fqc + b.fqc.fqx) the encoder's decode indexes"""
    d = tmp_path_factory.mktemp("build_index_farm")
    raw, _ = F.synth_fastq(40 << 20, 4, seed=9)
    fq = d / "in.fastq"
    raw.tofile(fq)
    a, b = d / "a.fqc", d / "b.fqc"
    assert run(tool, "c", fq, a, "-t", 4, "-R", 4, "-S", 4).returncode == 0
    assert run(tool, "c", fq, b, "-t", 4, "-R", 4, "-S", 4, "--index", "--index-stride", 64).returncode == 0
    assert not os.path.exists(str(a) + ".fqx")
    return d, fq, raw, F.parse_fastq(raw), a, b


def test_x_builds_the_file_the_encoder_writes(F, tool, farm, tmp_path):
    d, fq, raw, recs, a, b = farm
    n_blocks = len(A.read_archive(str(a))[3])
    rep = report(run(tool, "x", a, "-t", 3, "--index-stride", 64))
    no_leftovers(a)
    built, ident = read_fqx(str(a) + ".fqx")
    encoded, _ = read_fqx(str(b) + ".fqx")
    assert ident[0] == os.path.getsize(a)
    assert sorted(built) == sorted(encoded) == list(range(n_blocks))
    for k in range(n_blocks):
        same_index(built[k], encoded[k], "chunk %d" % k)
    # 4 MiB blocks hold dozens of strides each (the input's tail, a block of a few reads, holds none: the header alone)
    assert sum(len(q) > IX_HEAD + 10 * snap_bytes(1) for _, q in built.values()) >= n_blocks - 1
    assert rep["index"] == "built" and rep["indexed_blocks"] == n_blocks
    assert rep["index_bytes"] == sum(len(s) + len(q) for s, q in built.values())
    # the built file serves a restore and the record ranges
    back = tmp_path / "back.fastq"
    rep = report(run(tool, "d", a, back, "-t", 3))
    assert rep["index"] == "used" and rep["indexed_blocks"] == n_blocks
    assert open(back, "rb").read() == raw.tobytes()
    counts = [blk.n_records for blk in A.read_archive(str(a))[3]]
    restore_ranges(tool, tmp_path, a, raw, recs, counts, farm_ranges(counts, len(recs)))


def test_d_with_index_restores_and_leaves_the_file(F, tool, farm, tmp_path):
    d, fq, raw, recs, a, b = farm
    c = tmp_path / "c.fqc"
    shutil.copy(a, c)
    back = tmp_path / "back.fastq"
    rep = report(run(tool, "d", c, back, "-t", 3, "--index", "--index-stride", 64))
    assert open(back, "rb").read() == raw.tobytes()
    no_leftovers(c)
    built, _ = read_fqx(str(c) + ".fqx")
    encoded, _ = read_fqx(str(b) + ".fqx")
    assert sorted(built) == sorted(encoded)
    for k in built:
        same_index(built[k], encoded[k], "chunk %d" % k)
    assert rep["index"] == "built" and rep["indexed_blocks"] == len(built)
    # a usable file beside the archive: used, nothing built, and the report says so
    before = open(str(c) + ".fqx", "rb").read()
    rep = report(run(tool, "d", c, back, "-t", 3, "--index", "--index-stride", 64))
    assert rep["index"] == "used" and rep["indexed_blocks"] == len(built)
    assert open(str(c) + ".fqx", "rb").read() == before and open(back, "rb").read() == raw.tobytes()
    # --records never builds
    os.remove(str(c) + ".fqx")
    rep = report(run(tool, "d", c, back, "-t", 2, "--records", "5:9", "--index"))
    assert rep["index"] == "none" and rep["indexed_blocks"] == 0 and not os.path.exists(str(c) + ".fqx")
    assert open(back, "rb").read() == expect(raw, recs, 5, 9)


def test_x_takes_an_oracle_written_archive(F, tool, tmp_path):
    from test_archive import oracle_archive
    raw, _ = F.synth_fastq(9 << 20, 4, seed=5)
    recs = F.parse_fastq(raw)
    arc = tmp_path / "o.fqc"
    oracle_archive(F, str(arc), raw, recs, 7, order=[4, 1, 6, 0, 3, 5, 2])
    rep = report(run(tool, "x", arc, "-t", 2, "--index-stride", 64))
    assert rep["index"] == "built" and rep["indexed_blocks"] == 7
    built, _ = read_fqx(str(arc) + ".fqx")
    assert sorted(built) == list(range(7)) and all(len(q) > IX_HEAD for _, q in built.values())
    back = tmp_path / "back.fastq"
    rep = report(run(tool, "d", arc, back, "-t", 2))
    assert rep["index"] == "used" and rep["indexed_blocks"] == 7 and open(back, "rb").read() == raw.tobytes()


# ---------------------------------------------------------------- 8. replacement and failure
def test_x_replaces_a_truncated_a_foreign_and_a_tiny_file(F, tool, farm, tmp_path):
    d, fq, raw, recs, a, b = farm
    arc = tmp_path / "r.fqc"
    shutil.copy(a, arc)
    side = str(arc) + ".fqx"
    n_blocks = len(A.read_archive(str(arc))[3])
    other, _ = F.synth_fastq(6 << 20, 2, seed=4)
    other.tofile(tmp_path / "other.fastq")
    assert run(tool, "c", tmp_path / "other.fastq", tmp_path / "other.fqc", "-t", 2, "-R", 2, "-S", 2, "--index", "--index-stride", 64).returncode == 0
    good = open(str(b) + ".fqx", "rb").read()
    for what, content in (("truncated", good[: len(good) // 2]), ("foreign", open(str(tmp_path / "other.fqc") + ".fqx", "rb").read()),
                          ("three bytes", b"FQX")):
        open(side, "wb").write(content)
        rep = report(run(tool, "x", arc, "-t", 3, "--index-stride", 64))
        assert rep["index"] == "built" and rep["indexed_blocks"] == n_blocks, what
        no_leftovers(arc)
        assert sorted(read_fqx(side)[0]) == list(range(n_blocks)), what
        back = tmp_path / "back.fastq"
        rep = report(run(tool, "d", arc, back, "-t", 3))
        assert rep["index"] == "used" and rep["indexed_blocks"] == n_blocks, what  # the new file is the one in use
        assert open(back, "rb").read() == raw.tobytes(), what
        os.remove(back)


def test_x_on_a_damaged_archive_leaves_nothing_and_touches_nothing(F, tool, farm, tmp_path):
    d, fq, raw, recs, a, b = farm
    data = bytearray(open(a, "rb").read())
    _, _, _, blocks, entries = A.read_archive(str(a))
    off = sorted(e[0] for e in entries)[2]  # the third block in the file, a bit inside its streams
    data[off + 40 + len(blocks[0].seq) // 2] ^= 0x10
    bad = tmp_path / "bad.fqc"
    open(bad, "wb").write(data)
    out = tmp_path / "bad.fastq"
    r = run(tool, "d", bad, out, "-t", 3)  # the judge: the restore of today refuses this archive
    assert r.returncode == 1 and "fqc_tool:" in r.stderr
    side = str(bad) + ".fqx"
    r = run(tool, "x", bad, "-t", 3, "--index-stride", 64)
    assert r.returncode != 0 and "fqc_tool:" in r.stderr
    assert not os.path.exists(side) and not os.path.exists(side + ".part")
    r = run(tool, "d", bad, out, "-t", 3, "--index", "--index-stride", 64)
    assert r.returncode != 0
    assert not os.path.exists(side) and not os.path.exists(side + ".part") and not os.path.exists(out)
    # a file that was there stays as it was
    valid = open(str(b) + ".fqx", "rb").read()
    open(side, "wb").write(valid)
    r = run(tool, "x", bad, "-t", 3, "--index-stride", 64)
    assert r.returncode != 0
    assert open(side, "rb").read() == valid and not os.path.exists(side + ".part")
