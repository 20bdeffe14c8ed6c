"""The read filter on the device (fqcomp28_amd/csrc/select.hip behind fqgpu_chunk_filter / fqgpu_dblock_filter) against the
numpy restatement in filter_ref.py: the kept bytes, the report and the keep bits.  Integer arithmetic: every comparison is exact."""
import ctypes as C
import os
import re
import zlib

import numpy as np
import pytest

import filter_ref as R
import oracle_lib as O
import stats_ref as SR
import test_filter_host as TH
import test_gpu_stats as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

E_OVERFLOW, E_CORRUPT, E_ARG = -1, -3, -4
FIXTURES = ["SRR065390_sub_1", "without_ns", "SRR065390_sub_2", "SRR065390_1_first5"]


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    if F.device_count() < 1:
        pytest.fail("no GPU visible: the product path has no CPU fallback")
    return F


@pytest.fixture(scope="module")
def ctx(F, golden_dir):
    raw, recs = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_1.fastq"))
    c = TS.context_for(F, raw, recs)
    yield c
    c.close()


def filter_constants():
    """the tiling of select.hip, from its source: its SEL_* constants under the names the tests here use"""
    src = open(os.path.join(ROOT, "fqcomp28_amd", "csrc", "select.hip")).read()
    return {"FILT_" + k: int(re.search(r"constexpr unsigned SEL_%s = (\d+);" % k, src).group(1))
            for k in ("THREADS", "WAVE_RECORDS", "GROUP_LANES", "UNROLL", "GATHER_THREADS", "GATHER_WORDS")}


def build(entries, seed=1):
    """a FASTQ chunk from (header length with its '@', read length, quality level, number of N) per record -> (raw, recs): the
    header line is '@' and filler, the Phred values the level +- 6 clipped to 0 .. 63, N at random places"""
    rng = np.random.default_rng(seed)
    e = np.asarray(entries, dtype=np.int64).reshape(-1, 4)
    n = len(e)
    hl, lens, level, n_n = e[:, 0] + 1, e[:, 1], e[:, 2], np.minimum(e[:, 3], e[:, 1])   # hl: with the '\n'
    size = hl + 2 * lens + 4
    start = np.concatenate(([0], np.cumsum(size)))
    raw = np.full(int(start[-1]), ord("h"), dtype=np.uint8)
    recs = np.zeros(n, dtype=R.REC_DTYPE)
    recs["seq_off"] = start[:-1] + hl
    recs["qual_off"] = recs["seq_off"] + lens + 3
    recs["len"] = lens
    so, qo = recs["seq_off"].astype(np.int64), recs["qual_off"].astype(np.int64)
    raw[start[:-1]] = ord("@")
    raw[so - 1] = 10
    raw[so + lens] = 10
    raw[so + lens + 1] = ord("+")
    raw[so + lens + 2] = 10
    raw[qo + lens] = 10
    total = int(lens.sum())
    rec_of = np.repeat(np.arange(n), lens)
    pos = np.arange(total, dtype=np.int64) - np.concatenate(([0], np.cumsum(lens)))[:-1][rec_of]
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, total)]
    # the first n_n places of a random order of the read's positions hold N
    order = np.argsort(rng.random(total) + rec_of)          # a shuffle inside every read (reads stay in order)
    rank = np.empty(total, dtype=np.int64)
    rank[order] = pos
    bases[rank < n_n[rec_of]] = ord("N")
    phred = np.clip(level[rec_of] + rng.integers(-6, 7, total), 0, 63)
    raw[so[rec_of] + pos] = bases
    raw[qo[rec_of] + pos] = (phred + 33).astype(np.uint8)
    return raw, recs


def drawn(lens, seed):
    """reads of these lengths with per-read quality levels 4 .. 40 and 0, 0, 1, 2 or 5 N, drawn"""
    rng = np.random.default_rng(seed)
    n = len(lens)
    entries = np.stack([rng.integers(2, 9, n), np.asarray(lens), rng.integers(4, 41, n), rng.choice([0, 0, 1, 2, 5], n)], axis=1)
    return build(entries, seed + 1)


def same(ctx, raw, recs, f, what="", share=None, **kw):
    """the device's answer for the block (raw, recs) against the reference's; share: the reference must keep a share of the
    reads inside these bounds"""
    want_out, want_report, want_keep = R.filter_records(raw, recs, f)
    if share is not None:
        kept = int(want_report[R.N_KEPT]) / len(recs)
        assert share[0] <= kept <= share[1], "%s: the reference keeps %.1f %% of the reads: a vacuous input" % (what, 100 * kept)
    b = ctx.dblock(raw, recs)
    try:
        g = b.filter(f, **kw)
    finally:
        b.close()
    assert g["rc"] == 0, (what, g["rc"])
    assert g["report"].tolist() == want_report.tolist(), what
    assert g["keep"].tolist() == want_keep.tolist(), what
    assert g["out_len"] == want_out.size, what
    if not np.array_equal(g["out"], want_out):
        at = int(np.flatnonzero(g["out"] != want_out)[0])
        raise AssertionError("%s: the kept bytes differ, first at %d of %d" % (what, at, want_out.size))
    return g


# ---------------------------------------------------------------- 1. a device block against the reference
FILTERS = [dict(), dict(max_n=0), dict(min_mean_q=20), dict(min_mean_q=30), dict(low_q=20, max_low_pct=20), dict(min_len=100), dict(max_len=99),
           dict(max_n=2, min_mean_q=15, low_q=10, max_low_pct=40)]


@pytest.mark.parametrize("name", FIXTURES)
def test_the_fixtures_under_several_filters(F, ctx, golden_dir, name):
    raw, recs = O.load_fastq(os.path.join(golden_dir, name + ".fastq"))
    for kw in FILTERS:
        same(ctx, raw, recs, R.flt(**kw), "%s %s" % (name, kw))
    b = ctx.dblock(raw)   # with the device parser's record table
    g = b.filter(R.flt(min_mean_q=20))
    b.close()
    want = R.filter_chunk(raw, R.flt(min_mean_q=20))
    assert g["rc"] == 0 and np.array_equal(g["out"], want[0]) and g["report"].tolist() == want[1].tolist()


def criteria(lo_len, hi_len):
    return [("min_len", dict(min_len=lo_len)), ("max_len", dict(max_len=hi_len)), ("max_n", dict(max_n=0)), ("mean_q", dict(min_mean_q=22)),
            ("low_q", dict(low_q=15, max_low_pct=30)),
            ("all", dict(min_len=lo_len, max_len=hi_len, max_n=1, min_mean_q=14, low_q=10, max_low_pct=50))]


@pytest.mark.parametrize("length", [3, 63, 64, 65, 255, 256, 257, 1023, 65535])
def test_reads_of_one_length_and_its_neighbours(F, ctx, length):
    """a quarter of the reads one shorter (or, at the ends of the range, placed so that three lengths fit), a quarter one
    longer: every criterion alone drops a real share, the length criteria too"""
    mid = min(max(length, 4), 65534)
    n = min(max(300000 // length, 40), 800)
    rng = np.random.default_rng(length)
    lens = mid + rng.choice([-1, 0, 0, 1], n)
    assert (lens == length).sum() >= 3
    raw, recs = drawn(lens, 100 + length)
    for what, kw in criteria(mid, mid):
        same(ctx, raw, recs, R.flt(**kw), "length %d, %s" % (length, what), share=(0.10, 0.90))


def test_a_mix_of_lengths(F, ctx):
    rng = np.random.default_rng(5)
    lens = np.concatenate((rng.choice([3, 63, 64, 65, 255, 256, 257, 1023], 3000), rng.integers(3, 301, 3000), [65535, 65535]))
    rng.shuffle(lens)
    raw, recs = drawn(lens, 6)
    for what, kw in criteria(64, 256):
        same(ctx, raw, recs, R.flt(**kw), "mix, " + what, share=(0.10, 0.90))


@pytest.mark.parametrize("plus_repeats", [False, True])
def test_the_boundary_reads_of_the_host_test(F, ctx, plus_repeats):
    raw = TH.hand_chunk(plus_repeats)
    want_out, want_report, want_keep = TH.hand_expected()
    for table in (R.parse(raw), None):
        b = ctx.dblock(raw, table)
        g = b.filter(R.flt(**TH.HAND_FILTER))
        b.close()
        assert g["rc"] == 0 and g["out"].tobytes() == want_out.tobytes()
        assert g["report"].tolist() == want_report.tolist() and g["keep"].tolist() == want_keep.tolist()


# ---------------------------------------------------------------- 2. keep patterns: the gather
KEEP = dict(min_mean_q=20)   # a read of level 40 is kept, one of level 2 dropped


def pattern(keeps, hl=4, length=50, seed=3):
    """records kept / dropped by their quality level -> (raw, recs)"""
    keeps = np.asarray(keeps, dtype=bool)
    n = len(keeps)
    hl = np.broadcast_to(hl, n)
    length = np.broadcast_to(length, n)
    return build(np.stack([hl, length, np.where(keeps, 40, 2), np.zeros(n, dtype=np.int64)], axis=1), seed)


def test_all_kept_is_the_canonical_chunk(F, ctx):
    for n in (1, 700, 20000):
        raw, recs = pattern(np.ones(n, bool), hl=np.random.default_rng(n).integers(2, 12, n), length=np.random.default_rng(n + 1).integers(3, 200, n))
        g = same(ctx, raw, recs, R.flt(**KEEP), "%d records" % n)
        assert g["out"].tobytes() == raw.tobytes()
        b = ctx.dblock(raw, recs)
        assert zlib.crc32(g["out"].tobytes()) == b.crc32()
        for kw in (dict(), dict(min_len=3)):   # filters that read no line at all
            assert b.filter(R.flt(**kw))["out"].tobytes() == raw.tobytes()
        b.close()


def test_none_kept(F, ctx):
    raw, recs = pattern(np.zeros(500, bool))
    g = same(ctx, raw, recs, R.flt(**KEEP))
    assert g["rc"] == 0 and g["out_len"] == 0 and g["out"].size == 0 and int(g["report"][R.DROPPED_MEAN_Q]) == 500 and not g["keep"].any()
    g = same(ctx, raw, recs, R.flt(**KEEP), out_cap=64)
    assert g["rc"] == 0 and g["out_len"] == 0


@pytest.mark.parametrize("which", ["first", "last", "alternating", "pairs", "long runs", "random"])
def test_keep_patterns(F, ctx, which):
    n = 3001
    rng = np.random.default_rng(17)
    keeps = np.zeros(n, bool)
    if which == "first":
        keeps[0] = True
    elif which == "last":
        keeps[-1] = True
    elif which == "alternating":
        keeps[::2] = True
    elif which == "pairs":
        keeps[(np.arange(n) // 2) % 2 == 0] = True
    elif which == "long runs":
        keeps[(np.arange(n) // 700) % 2 == 1] = True
    else:
        keeps = rng.random(n) < 0.5
    raw, recs = pattern(keeps, hl=rng.integers(2, 12, n), length=rng.integers(3, 200, n))
    g = same(ctx, raw, recs, R.flt(**KEEP), which)
    assert int(g["report"][R.N_KEPT]) == int(keeps.sum())
    assert np.unpackbits(g["keep"], bitorder="little")[:n].astype(bool).tolist() == keeps.tolist()


def test_around_the_tiling_constants(F, ctx):
    k = filter_constants()
    round_records = k["FILT_WAVE_RECORDS"] // k["FILT_GROUP_LANES"]        # records a wave reads at a time
    wg_records = k["FILT_THREADS"] // 64 * k["FILT_WAVE_RECORDS"]          # records of a judge workgroup
    step = k["FILT_GROUP_LANES"] * 16 * k["FILT_UNROLL"]                   # bytes of a line a record's lanes ask for in one go
    sweep = k["FILT_GATHER_THREADS"] * 16                                  # output bytes of one sweep of a gather workgroup
    tile = sweep * k["FILT_GATHER_WORDS"]                                  # ... of the workgroup
    # record counts and run lengths (in records) at and around a round, a wave, a workgroup
    for edge in (round_records, k["FILT_WAVE_RECORDS"], wg_records):
        for n in (edge - 1, edge, edge + 1):
            rng = np.random.default_rng(n)
            for keeps in (rng.random(n) < 0.5, np.ones(n, bool), (np.arange(n) // max(n // 3, 1)) % 2 == 0):
                raw, recs = pattern(keeps, hl=rng.integers(2, 12, n), length=rng.integers(3, 90, n), seed=n)
                same(ctx, raw, recs, R.flt(**KEEP), "%d records" % n)
            run = (np.arange(4 * n + 5) // n) % 2 == 0                       # runs of n kept, n dropped
            raw, recs = pattern(run, hl=rng.integers(2, 12, run.size), length=rng.integers(3, 90, run.size), seed=n + 1)
            same(ctx, raw, recs, R.flt(**KEEP), "runs of %d records" % n)
    # read lengths at and around a 16-byte word, one request of a record's lanes, two of them
    lens = [e + d for e in (16, step, 2 * step, 3 * step) for d in (-17, -16, -15, -1, 0, 1, 15, 16, 17) if e + d >= 3]
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        entries = np.stack([rng.integers(2, 20, len(lens)), rng.permutation(lens), rng.integers(4, 41, len(lens)), rng.choice([0, 1, 3], len(lens))], axis=1)
        raw, recs = build(entries, seed)
        for what, kw in criteria(16, 2 * step):
            same(ctx, raw, recs, R.flt(**kw), "line lengths, " + what)
    # runs whose BYTES end one below, at and one above a word, a sweep and a tile of the gather: a record of 2 len + 4 + hl bytes
    for edge in (16, sweep, tile, 2 * tile):
        for d in (-1, 0, 1):
            size = edge + d
            hl = 3 if size % 2 == 0 else 4         # (with the '\n': 4 or 5)
            length = (size - 4 - (hl + 1)) // 2
            assert (hl + 1) + 2 * length + 4 == size
            for lead in (0, 1, 7):                 # kept bytes in front, so that the run also STARTS off a word
                keeps = [True] * (1 if lead else 0) + [False, True, False, True, True, False]
                hls = [2] * (1 if lead else 0) + [5, hl, 5, hl, 9, 5]
                lengths = [(lead + 1) // 2 + 3] * (1 if lead else 0) + [40, length, 33, length, 21, 40]
                raw, recs = pattern(keeps, hl=hls, length=lengths, seed=size)
                same(ctx, raw, recs, R.flt(**KEEP), "a run of %d bytes behind %d" % (size, lead))


# ---------------------------------------------------------------- 3. synthetic blocks, and the summary of the same block
@pytest.mark.parametrize("mode,kw", [(4, dict(max_n=0)), (2, dict(min_mean_q=34))])
def test_synth_blocks(F, ctx, mode, kw):
    """Kept shares, derived from the generator and not from a run: mode 4 draws N at a rate of 1 % over lengths 50 .. 300, so
    a read of length L has none with probability 0.99^L -- averaged over the lengths about 22 %; mode 2 draws the Phred values
    of 150 bases as round(N(34, 5)) clipped at 41, whose mean reaches 34 for about a third of the reads."""
    raw, _ = F.synth_fastq(8 << 20, mode, seed=50 + mode)
    recs = F.parse_fastq(raw)
    g = same(ctx, raw, recs, R.flt(**kw), "mode %d" % mode, share=(0.05, 0.95))
    b = ctx.dblock(raw, recs)
    v = SR.view(b.stats(64))
    for q in (1, 20, 34, 41, 63):
        assert int(b.filter(R.flt(min_mean_q=q), query=True, want_keep=False)["report"][R.N_KEPT]) == int(v["meanq_hist"][q:].sum()), q
    r = b.filter(R.flt(max_n=0), query=True, want_keep=False)["report"]
    assert int(r[R.N_RECORDS] - r[R.N_KEPT]) == v["reads_with_n"] == int(r[R.DROPPED_N])
    b.close()
    assert g["rc"] == 0


# ---------------------------------------------------------------- 4. the chunk on the handle's staging block
def begin(F, c, raw, recs=None):
    """fqgpu_encode_begin -> (the buffer the call reads from: to be kept until the cancel, number of records)"""
    n, nb, used = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    buf = raw.copy()
    table = None if recs is None else np.ascontiguousarray(recs, dtype=F.REC_DTYPE)
    rc = F.binding.lib().fqgpu_encode_begin(c.h, buf.ctypes.data_as(C.c_void_p), buf.size, None if table is None else table.ctypes.data_as(C.c_void_p),
                                            0 if table is None else len(table), 0, C.byref(n), C.byref(nb), C.byref(used))
    assert rc == 0
    return (buf, table), n.value


def test_plus_lines_that_repeat_the_header(F, golden_dir):
    raw, recs = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_2.fastq"))
    lines = raw.tobytes().split(b"\n")[:-1]
    for r in range(len(recs)):
        lines[4 * r + 2] = b"+" + lines[4 * r][1:]
    fat = np.frombuffer(b"\n".join(lines) + b"\n", dtype=np.uint8)
    c = TS.context_for(F, raw, recs)
    for kw in (dict(), dict(min_mean_q=20), dict(max_n=0, low_q=15, max_low_pct=20)):
        want = R.filter_records(raw, recs, R.flt(**kw))    # of the file with bare '+' lines: the canonical output
        assert kw == {} or 0 < want[1][R.N_KEPT] < len(recs)
        for table in (F.parse_fastq(fat), None):
            alive, n = begin(F, c, fat, table)
            g = c.chunk_filter(R.flt(**kw), n)
            assert F.binding.lib().fqgpu_encode_cancel(c.h) == 0
            assert g["rc"] == 0 and n == len(recs)
            assert g["out"].tobytes() == want[0].tobytes() and g["report"].tolist() == want[1].tolist() and g["keep"].tolist() == want[2].tolist()
    c.close()


def test_every_path_to_a_chunk_gives_one_output(F, golden_dir):
    for name in ("SRR065390_sub_1", "without_ns"):
        raw, recs = O.load_fastq(os.path.join(golden_dir, name + ".fastq"))
        f = R.flt(max_n=0, min_mean_q=18) if name == "SRR065390_sub_1" else R.flt(min_mean_q=22, low_q=10, max_low_pct=20)
        want = R.filter_records(raw, recs, f)
        assert 0 < want[1][R.N_KEPT] < len(recs)

        def holds(g, what):
            assert g["rc"] == 0, what
            assert g["out"].tobytes() == want[0].tobytes() and g["report"].tolist() == want[1].tolist() and g["keep"].tolist() == want[2].tolist(), what

        c = TS.context_for(F, raw, recs)
        fmt = TS.fmt_of(TS.first_header_of(raw))
        for table in (recs, None):
            alive, n = begin(F, c, raw, table)
            holds(c.chunk_filter(f, n), name + " in flight")
            assert F.binding.lib().fqgpu_encode_cancel(c.h) == 0
        g = c.encode_raw(raw, flags=F.F_DECODE_INDEX, header_format=fmt)
        assert g["rc"] == 0 and g["headers_rc"] == 0
        holds(c.chunk_filter(f, len(recs)), name + " behind fqgpu_encode_end")
        args = (fmt, g["header_fields"], g["readlens"], g["seq"], g["qual"], g["n_count"], g["n_pos"], g["used_len"])
        for what, kw in (("indexes", dict(index=g["index"])), ("no indexes", {}), ("indexing", dict(build_index=True))):
            d = c.decode_chunk(*args, **kw)
            assert d["rc"] == 0 and np.array_equal(d["raw"], raw)
            holds(c.chunk_filter(f, len(recs)), name + " decoded, " + what)
        c.set_check_only(True)
        d = c.decode_chunk(*args, want_raw=False, index=g["index"])
        assert d["rc"] == 0 and d["raw"] is None
        holds(c.chunk_filter(f, len(recs)), name + " check-only")
        c.set_check_only(False)
        for index in (None, g["index"]):
            rc, out = c.decode_block(g["seq"], g["qual"], g["n_count"], g["n_pos"], recs, O.blank_skeleton(raw, recs), index=index)
            assert rc == 0 and np.array_equal(out, raw)
            holds(c.chunk_filter(f, len(recs)), name + " decode_block")
        b = c.dblock(raw, recs)
        holds(b.filter(f), name + " dblock")
        b.close()
        c.close()


def test_digest_and_summary_are_the_same_before_and_after(F, golden_dir):
    raw, recs = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_1.fastq"))
    f = R.flt(max_n=0, min_mean_q=18)
    want = R.filter_records(raw, recs, f)
    crc, stats = (0, zlib.crc32(raw.tobytes()), raw.size), SR.stats_of(raw, recs, 64)
    c = TS.context_for(F, raw, recs)
    for order in ("filter first", "filter last", "filter between"):
        alive, n = begin(F, c, raw)
        steps = {"filter first": "fcs", "filter last": "csf", "filter between": "cfs"}[order] + "fcs"
        for s in steps:
            if s == "f":
                g = c.chunk_filter(f, n)
                assert g["rc"] == 0 and g["out"].tobytes() == want[0].tobytes() and g["report"].tolist() == want[1].tolist(), order
            elif s == "c":
                assert c.chunk_crc32() == crc, order
            else:
                rc, got = c.chunk_stats(64)
                assert rc == 0 and np.array_equal(got, stats), order
        assert F.binding.lib().fqgpu_encode_cancel(c.h) == 0
    b = c.dblock(raw, recs)
    before = (b.crc32(), b.stats(64))
    assert b.filter(f)["rc"] == 0
    assert b.crc32() == before[0] and np.array_equal(b.stats(64), before[1]) and np.array_equal(b.fetch_raw(), raw)
    b.close()
    c.close()


# ---------------------------------------------------------------- 5. arguments
def raw_call(F, ctx, b, f, out, cap, keep=None):
    n = C.c_size_t(77)
    report = np.full(R.REPORT_WORDS, 7, dtype=np.uint64)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = F.binding.lib().fqgpu_dblock_filter(ctx.h, b.h if b is not None else None, p(f), p(out), cap, C.byref(n), p(report), p(keep))
    return rc, n.value, report


def test_size_query_and_a_buffer_one_byte_short(F, ctx):
    raw, recs = drawn(np.random.default_rng(8).integers(3, 200, 900), 9)
    f = R.flt(min_mean_q=22)
    want = R.filter_records(raw, recs, f)
    assert 0 < want[0].size < raw.size
    b = ctx.dblock(raw, recs)
    keep = np.full((len(recs) + 7) // 8, 0xAA, dtype=np.uint8)
    rc, n, report = raw_call(F, ctx, b, f, None, 0, keep)
    assert rc == 0 and n == want[0].size and report.tolist() == want[1].tolist() and keep.tolist() == want[2].tolist(), "the size query"
    rc, n, report = raw_call(F, ctx, b, f, None, 1 << 40)
    assert rc == 0 and n == want[0].size, "out == NULL is a size query whatever out_cap says"
    out = np.full(want[0].size + 32, 0x5A, dtype=np.uint8)
    rc, n, report = raw_call(F, ctx, b, f, out, want[0].size - 1)
    assert rc == E_OVERFLOW and n == want[0].size and report.tolist() == want[1].tolist()
    assert (out == 0x5A).all(), "nothing is written"
    rc, n, report = raw_call(F, ctx, b, f, out, want[0].size)
    assert rc == 0 and n == want[0].size and out[:n].tobytes() == want[0].tobytes() and (out[n:] == 0x5A).all(), "exactly *out_len bytes"
    # a NULL where data is expected, a filter the check refuses
    for bad in TH.BAD_FILTERS:
        rc, n, report = raw_call(F, ctx, b, R.flt(**bad), out, out.size)
        assert rc == E_ARG and n == 0 and not report.any(), bad
    rc, n, report = raw_call(F, ctx, b, None, out, out.size)
    assert rc == E_ARG and n == 0 and not report.any()
    rc, n, report = raw_call(F, ctx, None, f, out, out.size)
    assert rc == E_ARG and n == 0 and not report.any()
    L = F.binding.lib()
    assert L.fqgpu_dblock_filter(ctx.h, b.h, f.ctypes.data_as(C.c_void_p), None, 0, None, report.ctypes.data_as(C.c_void_p), None) == E_ARG
    nn = C.c_size_t(5)
    assert L.fqgpu_dblock_filter(ctx.h, b.h, f.ctypes.data_as(C.c_void_p), None, 0, C.byref(nn), None, None) == E_ARG and nn.value == 0
    b.close()


@pytest.mark.parametrize("what", ["quality a", "quality space", "quality 200", "base X", "base 0xC1", "base n"])
def test_bytes_that_cannot_be_judged(F, ctx, what):
    raw, recs = drawn([40, 150, 90, 7, 300] * 30, 21)
    r = recs[77]
    in_seq = what.startswith("base")
    byte = {"quality a": ord("a"), "quality space": ord(" "), "quality 200": 200, "base X": ord("X"), "base 0xC1": 0xC1, "base n": ord("n")}[what]
    raw[(r["seq_off"] if in_seq else r["qual_off"]) + r["len"] - 1] = byte
    reads_it = [dict(max_n=3)] if in_seq else [dict(min_mean_q=1), dict(low_q=1, max_low_pct=100)]
    reads_it_not = [dict(), dict(min_len=50)] + ([dict(min_mean_q=20), dict(low_q=10, max_low_pct=20)] if in_seq else [dict(max_n=0)])
    b = ctx.dblock(raw, recs)
    for kw in reads_it:
        out = np.full(raw.size, 0x5A, dtype=np.uint8)
        keep = np.full((len(recs) + 7) // 8, 0xAA, dtype=np.uint8)
        for o in (None, out):
            rc, n, report = raw_call(F, ctx, b, R.flt(**kw), o, out.size, keep)
            assert rc == E_ARG and n == 0 and not report.any(), (what, kw)
        assert (out == 0x5A).all()
        with pytest.raises(R.Refused):
            R.filter_records(raw, recs, R.flt(**kw))
    b.close()
    for kw in reads_it_not:   # the criterion that would read that line is off: the byte is not looked at
        same(ctx, raw, recs, R.flt(**kw), "%s under %s" % (what, kw))


def test_states_without_a_chunk(F, golden_dir):
    raw, recs = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_1.fastq"))
    c = TS.context_for(F, raw, recs)
    L = F.binding.lib()
    f = R.flt(min_mean_q=18)
    want = R.filter_records(raw, recs, f)

    def refused(what):
        out = np.full(raw.size, 0x5A, dtype=np.uint8)
        n = C.c_size_t(77)
        report = np.full(R.REPORT_WORDS, 7, dtype=np.uint64)
        rc = L.fqgpu_chunk_filter(c.h, f.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), out.size, C.byref(n),
                                  report.ctypes.data_as(C.c_void_p), None)
        assert rc == E_ARG and n.value == 0 and not report.any() and (out == 0x5A).all(), what

    def holds(what):
        g = c.chunk_filter(f, len(recs))
        assert g["rc"] == 0 and g["out"].tobytes() == want[0].tobytes() and g["report"].tolist() == want[1].tolist(), what

    refused("a fresh handle")
    fmt = TS.fmt_of(TS.first_header_of(raw))
    g = c.encode_raw(raw, flags=F.F_DECODE_INDEX, header_format=fmt)
    holds("behind an encode")
    args = (fmt, g["header_fields"], g["readlens"], g["seq"], g["qual"], g["n_count"], g["n_pos"], g["used_len"])
    assert c.decode_chunk_range(*args, 3, 40, index=g["index"])["rc"] == 0
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
    alive, n = begin(F, c, raw)
    holds("a chunk in flight")
    assert L.fqgpu_encode_cancel(c.h) == 0
    refused("after fqgpu_encode_cancel")
    c.close()


def test_the_launches_are_timed_as_filter(F, golden_dir):
    raw, recs = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_1.fastq"))
    c = TS.context_for(F, raw, recs)
    b = c.dblock(raw, recs)
    c.enable_timing(True)
    f = R.flt(min_mean_q=18)
    size = b.filter(f, query=True)["out_len"]      # a size query: the judge
    _, groups = c.last_timing()
    assert [(name, calls) for name, _, calls in groups if name == "filter"] == [("filter", 1)], groups
    assert size > 0 and b.filter(f, out_cap=size)["rc"] == 0      # with a buffer: the judge and the scan, then the gather
    _, groups = c.last_timing()
    assert [calls for name, _, calls in groups if name == "filter"] == [3], groups
    assert all(ms >= 0 for name, ms, _ in groups if name == "filter")
    b.close()
    c.close()
