"""Read summaries on the device (fqcomp28_amd/csrc/stats.hip behind fqgpu_chunk_stats / fqgpu_dblock_stats) against the
numpy restatement in stats_ref.py.  Everything is integer counting: all comparisons are exact."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import oracle_lib as O
import stats_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import headers_oracle as HO  # noqa: E402

pytestmark = pytest.mark.gpu

E_OVERFLOW, E_CORRUPT, E_ARG = -1, -3, -4
FIXTURES = ["SRR065390_sub_1", "without_ns", "SRR065390_sub_2", "SRR065390_1_first5"]


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    if F.device_count() < 1:
        pytest.fail("no GPU visible: the product path has no CPU fallback")
    return F


def stats_constants():
    """the tiling of stats.hip, from its source"""
    src = open(os.path.join(ROOT, "fqcomp28_amd", "csrc", "stats.hip")).read()
    return {k: int(re.search(r"constexpr unsigned %s = (\d+);" % k, src).group(1))
            for k in ("STATS_THREADS", "STATS_WINDOW_ROWS", "STATS_UNROLL", "STATS_REDUCE_SLABS", "STATS_SPAN_RECORDS", "STATS_STAGES")}


def chunk_from(lens, seed=1, n_rate=0.02, phred=(0, 64), seq=None, qual=None):
    """a FASTQ chunk whose records have these lengths -> (raw, recs): bases ACGT with N at n_rate, Phred uniform over
    phred[0] .. phred[1] - 1; seq / qual: one byte for every symbol instead"""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.int64)
    n = len(lens)
    heads = [b"@r%d" % i for i in range(n)]
    hl = np.array([len(h) for h in heads], dtype=np.int64)
    size = hl + 1 + lens + 3 + lens + 1
    start = np.concatenate(([0], np.cumsum(size)))
    raw = np.full(int(start[-1]), 10, dtype=np.uint8)
    recs = np.zeros(n, dtype=[("seq_off", "<u4"), ("qual_off", "<u4"), ("len", "<u4")])
    recs["seq_off"] = start[:-1] + hl + 1
    recs["qual_off"] = recs["seq_off"] + lens + 3
    recs["len"] = lens
    total = int(lens.sum())
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, total)]
    bases[rng.random(total) < n_rate] = ord("N")
    quals = (rng.integers(phred[0], phred[1], total) + 33).astype(np.uint8)
    if seq is not None:
        bases[:] = seq
    if qual is not None:
        quals[:] = qual
    rec_of = np.repeat(np.arange(n), lens)
    pos = np.arange(total) - np.concatenate(([0], np.cumsum(lens)))[:-1][rec_of]
    raw[recs["seq_off"].astype(np.int64)[rec_of] + pos] = bases
    raw[recs["qual_off"].astype(np.int64)[rec_of] + pos] = quals
    for i, h in enumerate(heads):
        raw[start[i]:start[i] + hl[i]] = np.frombuffer(h, dtype=np.uint8)
    raw[recs["seq_off"].astype(np.int64) + lens + 1] = ord("+")
    return raw, recs


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


def dblock_stats(ctx, raw, recs, P):
    b = ctx.dblock(raw, recs)
    try:
        return b.stats(P)
    finally:
        b.close()


def same(got, want, what=""):
    if not np.array_equal(got, want):
        diff = np.flatnonzero(got != want)
        raise AssertionError("%s: %d words differ, first at %d: got %d, want %d" % (what, diff.size, diff[0], got[diff[0]], want[diff[0]]))


# ---------------------------------------------------------------- 1. the summary of a device block
@pytest.mark.parametrize("name", FIXTURES)
def test_dblock_stats_of_the_fixtures(F, ctx, golden_dir, name):
    raw, recs = O.load_fastq(os.path.join(golden_dir, name + ".fastq"))
    for P in (128, 64, 1):
        want = R.stats_of(raw, recs, P)
        same(dblock_stats(ctx, raw, recs, P), want, "%s P %d" % (name, P))
        if P == 64 and int(recs["len"].max()) > 64:
            assert R.view(want)["base_pos"][64].sum() > 0, "row P is in use"
    b = ctx.dblock(raw)  # with the device parser's record table
    same(b.stats(128), R.stats_of(raw, recs, 128), name)
    v = F.binding.stats_view(b.stats(128))
    assert v["base_pos"].shape == (129, 5) and v["qual_pos"].shape == (129, 64) and int(v["n_records"][0]) == len(recs)
    b.close()


def test_one_record_of_length_three(F, ctx):
    raw, recs = chunk_from([3], seed=3)
    for P in (1, 2, 3, 4, 512):
        same(dblock_stats(ctx, raw, recs, P), R.stats_of(raw, recs, P), "P %d" % P)


@pytest.mark.parametrize("P", [65535, 100])
def test_one_record_of_length_65535(F, ctx, P):
    raw, recs = chunk_from([65535], seed=4)
    same(dblock_stats(ctx, raw, recs, P), R.stats_of(raw, recs, P))


@pytest.fixture(scope="module")
def mixed():
    """5,000 records of 3 .. 300 symbols, half of them shorter than 64; N among the bases, every Phred 0 .. 63"""
    rng = np.random.default_rng(11)
    lens = np.where(rng.random(5000) < 0.5, rng.integers(3, 64, 5000), rng.integers(64, 301, 5000))
    raw, recs = chunk_from(lens, seed=12)
    assert (lens < 64).sum() > 2000 and (raw == ord("N")).sum() > 1000
    assert np.count_nonzero(R.view(R.stats_of(raw, recs, 1))["qual_pos"].sum(axis=0)) == 64
    return raw, recs


@pytest.mark.parametrize("P", [512, 37])
def test_mixed_lengths(F, ctx, mixed, P):
    raw, recs = mixed
    same(dblock_stats(ctx, raw, recs, P), R.stats_of(raw, recs, P))


def test_constant_data(F, ctx):
    raw, _ = F.synth_fastq(4 << 20, 5, seed=7)
    recs = F.parse_fastq(raw)
    got = dblock_stats(ctx, raw, recs, 512)
    same(got, R.stats_of(raw, recs, 512))
    v = R.view(got)
    assert v["base_pos"][:, 1:].sum() == 0 and np.count_nonzero(v["qual_pos"].sum(axis=0)) == 1, "every symbol in one column"


def test_around_the_tiling_constants(F, ctx):
    k = stats_constants()
    span, stages = k["STATS_SPAN_RECORDS"], k["STATS_STAGES"]   # consecutive records of a wave; of them, loaded together
    wg_records = k["STATS_THREADS"] // 64 * span                 # records a workgroup takes in one round
    window, step = k["STATS_WINDOW_ROWS"], 64 * k["STATS_UNROLL"]
    # numbers of records at and around one batch, one span, one round of a workgroup, the slabs a reduce thread adds, and
    # one round of 256 workgroups
    for edge in (stages, span, wg_records, k["STATS_REDUCE_SLABS"] * wg_records, 256 * wg_records):
        for n in (edge - 1, edge, edge + 1):
            rng = np.random.default_rng(n)
            lens = rng.integers(3, 12, n)
            lens[rng.integers(0, n, 3)] = (window + 1, 63, step + 1)   # a read longer than the window in every chunk
            raw, recs = chunk_from(lens, seed=n)
            same(dblock_stats(ctx, raw, recs, 512), R.stats_of(raw, recs, 512), "%d records" % n)
    # read lengths at and around a wave's step, the steps in flight together, and the window; P inside, at and beyond it
    lens = [e + d for e in (64, step, 2 * step, window, window + 64) for d in (-1, 0, 1)] * 3
    raw, recs = chunk_from(lens, seed=99)
    for P in (window - 1, window, window + 1, window + 63, 2 * window, 63, 64, 65):
        same(dblock_stats(ctx, raw, recs, P), R.stats_of(raw, recs, P), "P %d" % P)


@pytest.mark.parametrize("mode,mib", [(2, 32), (4, 8)])
def test_synth_blocks(F, ctx, mode, mib):
    raw, _ = F.synth_fastq(mib << 20, mode, seed=40 + mode)
    recs = F.parse_fastq(raw)
    same(dblock_stats(ctx, raw, recs, 512), R.stats_of(raw, recs, 512))


def test_merge_of_two_blocks_is_the_summary_of_both(F, ctx, mixed):
    raw, recs = mixed
    half = len(recs) // 2
    cut = int(recs["seq_off"][half]) - len(b"@r%d" % half) - 1
    a = dblock_stats(ctx, raw[:cut], recs[:half], 100)
    tail = recs[half:].copy()
    tail["seq_off"] -= cut
    tail["qual_off"] -= cut
    b = dblock_stats(ctx, raw[cut:], tail, 100)
    assert F.binding.stats_merge(a, b) == 0
    same(a, dblock_stats(ctx, raw, recs, 100))
    same(a, R.stats_of(raw, recs, 100))


@pytest.mark.parametrize("what", ["quality a", "quality space", "base X"])
def test_bytes_that_cannot_be_counted(F, ctx, what):
    raw, recs = chunk_from([40, 150, 90, 7] * 30, seed=21)
    r = recs[77]
    if what == "base X":
        raw[r["seq_off"] + 5] = ord("X")
    else:
        raw[r["qual_off"] + 5] = ord("a") if what == "quality a" else ord(" ")
    b = ctx.dblock(raw, recs)
    out = np.full(R.words(64), 7, dtype=np.uint64)
    rc = F.binding.lib().fqgpu_dblock_stats(ctx.h, b.h, 64, out.ctypes.data_as(C.c_void_p), out.size)
    b.close()
    assert rc == E_ARG and not out.any()


def test_a_buffer_one_word_short(F, ctx):
    raw, recs = chunk_from([50] * 20, seed=22)
    b = ctx.dblock(raw, recs)
    out = np.full(R.words(64), 7, dtype=np.uint64)
    L = F.binding.lib()
    assert L.fqgpu_dblock_stats(ctx.h, b.h, 64, out.ctypes.data_as(C.c_void_p), out.size - 1) == E_OVERFLOW
    assert (out == 7).all(), "nothing is written"
    assert L.fqgpu_dblock_stats(ctx.h, b.h, 0, out.ctypes.data_as(C.c_void_p), out.size) == E_ARG
    assert L.fqgpu_dblock_stats(ctx.h, b.h, 65536, out.ctypes.data_as(C.c_void_p), out.size) == E_ARG
    assert L.fqgpu_dblock_stats(ctx.h, b.h, 64, None, out.size) == E_ARG
    assert L.fqgpu_dblock_stats(ctx.h, None, 64, out.ctypes.data_as(C.c_void_p), out.size) == E_ARG
    assert L.fqgpu_dblock_stats(ctx.h, b.h, 64, out.ctypes.data_as(C.c_void_p), out.size) == 0
    same(out, R.stats_of(raw, recs, 64))
    b.close()


def test_the_launch_is_timed_as_stats(F, golden_dir):
    raw, recs = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_1.fastq"))
    c = context_for(F, raw, recs)
    b = c.dblock(raw, recs)
    c.enable_timing(True)
    b.stats(128)
    _, groups = c.last_timing()
    assert [(name, calls) for name, _, calls in groups if name == "stats"] == [("stats", 1)], groups
    b.close()
    # P beyond the window and a read that reaches there: still one timed call (the rows behind the window are counted by
    # the same launch)
    window = stats_constants()["STATS_WINDOW_ROWS"]
    long_raw, long_recs = chunk_from([100, 3 * window + 5, 60], seed=31)
    b = c.dblock(long_raw, long_recs)
    same(b.stats(4 * window), R.stats_of(long_raw, long_recs, 4 * window))
    _, groups = c.last_timing()
    assert [calls for name, _, calls in groups if name == "stats"] == [2], groups
    b.close()
    c.close()


# ---------------------------------------------------------------- 2. the chunk on the handle's staging block
def test_every_path_to_a_chunk_gives_one_summary(F, golden_dir):
    P = 128
    for name in ("SRR065390_sub_1", "without_ns"):
        raw, recs = O.load_fastq(os.path.join(golden_dir, name + ".fastq"))
        want = R.stats_of(raw, recs, P)
        assert name == "without_ns" or want[4] > 0, "the fixture holds N"
        c = context_for(F, raw, recs)
        fmt = fmt_of(first_header_of(raw))
        for flags in (0, F.F_WRITE_BACK_N):   # (the device copy is never patched: N is counted as N)
            for table in (recs, None):
                g = c.encode_raw(raw, flags=flags | F.F_DECODE_INDEX, recs=table, header_format=fmt, want_stats=P)
                assert g["rc"] == 0 and g["headers_rc"] == 0
                same(g["stats"], want, "%s in flight, flags %d, %s table" % (name, flags, "the caller's" if table is not None else "the parser's"))
                rc, again = c.chunk_stats(P)
                assert rc == 0
                same(again, want, "behind fqgpu_encode_end")
        args = (fmt, g["header_fields"], g["readlens"], g["seq"], g["qual"], g["n_count"], g["n_pos"], g["used_len"])
        for what, kw in (("indexes", dict(index=g["index"])), ("no indexes", {}), ("indexing", dict(build_index=True))):
            d = c.decode_chunk(*args, want_stats=P, **kw)
            assert d["rc"] == 0 and d["stats_rc"] == 0 and np.array_equal(d["raw"], raw), (name, what)
            same(d["stats"], want, name + " decoded, " + what)
        c.set_check_only(True)
        d = c.decode_chunk(*args, want_raw=False, want_stats=P)
        assert d["rc"] == 0 and d["raw"] is None and d["stats_rc"] == 0
        same(d["stats"], want, name + " check-only")
        c.set_check_only(False)
        for index in (None, g["index"]):
            rc, out = c.decode_block(g["seq"], g["qual"], g["n_count"], g["n_pos"], recs, O.blank_skeleton(raw, recs), index=index)
            assert rc == 0 and np.array_equal(out, raw)
            rc, got = c.chunk_stats(P)
            assert rc == 0
            same(got, want, name + " decode_block")
        c.close()


def test_plus_lines_that_repeat_the_header(F, golden_dir):
    raw, recs = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_2.fastq"))
    lines = raw.tobytes().split(b"\n")[:-1]
    for r in range(len(recs)):
        lines[4 * r + 2] = b"+" + lines[4 * r][1:]
    fat = np.frombuffer(b"\n".join(lines) + b"\n", dtype=np.uint8)
    want = R.stats_of(raw, recs, 128)
    c = context_for(F, raw, recs)
    for table in (F.parse_fastq(fat), None):
        g = c.encode_raw(fat, recs=table, want_stats=128)
        assert g["rc"] == 0
        same(g["stats"], want, "the parser's table" if table is None else "the caller's table")
    c.close()


def test_beside_the_digest_in_both_orders(F, golden_dir):
    import zlib
    raw, recs = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_1.fastq"))
    want, crc = R.stats_of(raw, recs, 64), (0, zlib.crc32(raw.tobytes()), raw.size)
    c = context_for(F, raw, recs)
    L = F.binding.lib()
    for stats_first in (True, False):
        n, nb, used = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        buf = raw.copy()
        assert L.fqgpu_encode_begin(c.h, buf.ctypes.data_as(C.c_void_p), buf.size, None, 0, 0, C.byref(n), C.byref(nb), C.byref(used)) == 0
        if stats_first:
            rc, got = c.chunk_stats(64)
            assert c.chunk_crc32() == crc
        else:
            assert c.chunk_crc32() == crc
            rc, got = c.chunk_stats(64)
        assert rc == 0
        same(got, want)
        assert c.chunk_crc32() == crc
        rc, got = c.chunk_stats(64)
        assert rc == 0
        same(got, want)
        assert L.fqgpu_encode_cancel(c.h) == 0
    c.close()


def test_states_without_a_chunk_to_summarise(F, golden_dir):
    raw, recs = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_1.fastq"))
    c = context_for(F, raw, recs)
    L = F.binding.lib()
    want = R.stats_of(raw, recs, 64)

    def refused(what):
        out = np.full(R.words(64), 7, dtype=np.uint64)
        rc = L.fqgpu_chunk_stats(c.h, 64, out.ctypes.data_as(C.c_void_p), out.size)
        assert rc == E_ARG and not out.any(), what

    def holds(what):
        rc, got = c.chunk_stats(64)
        assert rc == 0, what
        same(got, want, what)

    refused("a fresh handle")
    fmt = fmt_of(first_header_of(raw))
    g = c.encode_raw(raw, flags=F.F_DECODE_INDEX, header_format=fmt)
    holds("behind an encode")
    args = (fmt, g["header_fields"], g["readlens"], g["seq"], g["qual"], g["n_count"], g["n_pos"], g["used_len"])
    r = c.decode_chunk_range(*args, 3, 40, index=g["index"])
    assert r["rc"] == 0
    refused("after a range")
    assert c.decode_chunk(*args)["rc"] == 0
    holds("after a decode")
    r = c.decode_chunk_fasta(fmt, g["header_fields"], g["readlens"], g["seq"], g["n_count"], g["n_pos"], g["used_len"], 0, len(recs),
                             seq_index=g["index"][0])
    assert r["rc"] == 0
    refused("after a FASTA restore")
    for at in range(g["qual"].size // 2, g["qual"].size // 2 + 64):
        q = g["qual"].copy()
        q[at] ^= 0x10
        d = c.decode_chunk(fmt, g["header_fields"], g["readlens"], g["seq"], q, g["n_count"], g["n_pos"], g["used_len"])
        if d["rc"] != 0:
            break
    assert d["rc"] == E_CORRUPT
    refused("after a damaged stream")
    n, nb, used = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    buf = raw.copy()
    assert L.fqgpu_encode_begin(c.h, buf.ctypes.data_as(C.c_void_p), buf.size, None, 0, 0, C.byref(n), C.byref(nb), C.byref(used)) == 0
    holds("a chunk in flight")
    assert L.fqgpu_encode_cancel(c.h) == 0
    refused("after fqgpu_encode_cancel")
    out = np.full(R.words(64), 7, dtype=np.uint64)
    assert L.fqgpu_chunk_stats(c.h, 64, out.ctypes.data_as(C.c_void_p), out.size - 1) == E_OVERFLOW and (out == 7).all()
    c.close()
