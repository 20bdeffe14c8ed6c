"""The device FASTQ parser (fqcomp28_amd/csrc/parse.hip: k_nl_count, the scan, k_nl_write, k_records, k_count_n) against
the line-by-line reference of parse_ref.py, through both of its entry points -- fqgpu_dblock_create_from_raw and
fqgpu_encode_begin(recs == NULL), the one the product's `fqc_tool c` takes for every chunk -- on the families of inputs
parse_ref.cases() builds (tests/test_parse_host.py holds that reference and the inputs against the host parser and the
reference's compiled parser first):

  boundary  a newline of each line kind on the last byte of a lane word, wave and workgroup and on the first of the next
  ends      blocks that end on such a boundary or one byte past it
  dense     five newlines a lane word, more than 256 records a workgroup; newlines at every residue mod 16
  sparse    a read of 65535 bases: some thirty workgroups without a newline; 65536 bases are refused
  cuts      a block cut at every byte of its last two records; one to three whole lines behind the last record
  pin       '+' lines that repeat the header, qualities that begin with '@' or '+'
  defect    one malformed record at thread 0, 63, 64, 255, 256 of k_records and in the last record; exact error codes
  crlf      the table is the reference's (the length counts the carriage return); the encode refuses the reads
  many      60500 records in 2243 chunks: the scan leaves its first chunk of 2048 items, k_count_n strides over its grid

Every comparison is an equality: of tables, of counts, of error codes, of streams with the CPU oracle's."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as O
import parse_ref as P

pytestmark = pytest.mark.gpu

STREAMS = ("seq", "qual", "readlens", "n_count", "n_pos")
SMALL = "ends:block-of-2720-bytes"   # the well-formed block a handle parses after each refusal
FAMILIES = list(P.FAMILIES)


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    assert F.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return F


@pytest.fixture(scope="module")
def ctx(F, golden_dir):
    """the parser-only checks' handle: the tables of a fixture, which code any read of valid symbols"""
    raw, recs = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_1.fastq"))
    _, _, sft, qft = O.freq_tables(raw, recs)
    ctx = F.Context(sft, qft)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def many():
    """the many-records block, its reference parse, its own tables and the oracle's encoding under them, computed once"""
    raw = np.frombuffer(P.shared_cases()[P.MANY], dtype=np.uint8)
    verdict, recs, used, n_bases, n_n = P.reference(P.MANY)
    assert verdict == "ok" and used == raw.size
    _, _, sft, qft = O.freq_tables(raw, recs)
    octx = O.OracleCtx(sft, qft)
    want = octx.encode(raw, recs)
    octx.close()
    assert want["rc"] == 0 and len(want["n_pos"]) == n_n
    for a in want.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return dict(raw=raw, recs=recs, n_bases=n_bases, n_n=n_n, tables=(sft, qft), want=want)


def array_of(name):
    return np.frombuffer(P.shared_cases()[name], dtype=np.uint8)


def through_dblock(F, ctx, raw):
    """fqgpu_dblock_create_from_raw -> (code, table, raw_len)"""
    try:
        b = ctx.dblock(raw)
    except F.FqgpuError as e:
        return e.code, None, None
    try:
        assert b.n_recs > 0
        return 0, b.records(), b.raw_len
    finally:
        b.close()


def through_begin(F, ctx, raw):
    """fqgpu_encode_begin without a record table, fqgpu_encode_records, fqgpu_encode_cancel
    -> (code, table, *n_recs_out, *n_bases_out, *used_len)"""
    raw = np.array(raw)
    n, nb, used = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    lib = F.lib()
    rc = lib.fqgpu_encode_begin(ctx.h, raw.ctypes.data, raw.size, None, 0, 0, C.byref(n), C.byref(nb), C.byref(used))
    if rc:
        return rc, None, None, None, None
    table = np.zeros(n.value, dtype=F.REC_DTYPE)
    rc_records = lib.fqgpu_encode_records(ctx.h, table.ctypes.data, len(table))
    assert lib.fqgpu_encode_cancel(ctx.h) == 0
    assert rc_records == 0
    return 0, table, n.value, nb.value, used.value


def check_dblock(F, ctx, name):
    verdict, recs, used, _, _ = P.reference(name)
    code, table, raw_len = through_dblock(F, ctx, array_of(name))
    assert code == P.CODE[verdict], (name, verdict, code)
    if verdict == "ok":
        assert table.dtype == recs.dtype and np.array_equal(table, recs), name
        assert raw_len == used, (name, raw_len, used)
    return code


def check_begin(F, ctx, name):
    verdict, recs, used, n_bases, _ = P.reference(name)
    code, table, got_recs, got_bases, got_used = through_begin(F, ctx, array_of(name))
    assert code == P.CODE[verdict], (name, verdict, code)
    if verdict == "ok":
        assert (got_recs, got_bases, got_used) == (len(recs), n_bases, used), (name, got_recs, got_bases, got_used)
        assert table.dtype == recs.dtype and np.array_equal(table, recs), name
    return code


@pytest.mark.parametrize("family", FAMILIES)
def test_both_entry_points_against_the_reference(F, ctx, family):
    """every case: the table, the record and base counts and the bytes used, or the exact refusal; after every refusal the
    same handle parses a small well-formed block"""
    names = P.names_of(family)
    assert names
    for name in names:
        if check_dblock(F, ctx, name):
            assert check_dblock(F, ctx, SMALL) == 0, name
        if name in P.PARSE_ONLY:
            continue
        if check_begin(F, ctx, name):
            assert check_begin(F, ctx, SMALL) == 0, name


def test_reads_no_table_codes_are_parsed_and_then_refused_by_the_encode(F, ctx):
    """carriage returns: the parser's table is the reference's, and the encoder refuses the reads under the bad-symbol
    rule of include/fqgpu.h (a sequence byte that is neither a base nor N); the handle goes on"""
    for name, code in P.PARSE_ONLY.items():
        assert P.reference(name)[0] == "ok"
        assert ctx.encode_raw(array_of(name))["rc"] == code, name
        assert check_begin(F, ctx, SMALL) == 0


def same_streams(got, want, what):
    assert got["rc"] == 0, (what, got["rc"])
    for k in STREAMS:
        assert np.array_equal(np.asarray(got[k]), want[k]), (what, k)


def test_stale_newlines_behind_the_chunk_and_in_the_scratch(F, many):
    """one host-pointer handle: the many-records block sizes the staging block and the parser's scratch, every byte of them
    is then set to a newline, and the blocks that end on a boundary and the block cut at every byte are parsed in what is
    left: every byte behind a chunk, and every scratch word nobody wrote, reads as a newline"""
    ctx = F.Context(*many["tables"])
    try:
        same_streams(ctx.encode_raw(many["raw"]), many["want"], "before the fill")
        buffers, n_bytes = ctx.fill_scratch(0x0A)
        assert buffers > 0 and n_bytes > many["raw"].size
        for family in ("ends", "cuts"):
            for name in P.names_of(family):
                assert check_begin(F, ctx, name) == 0, name
    finally:
        ctx.close()


def test_n_counts_and_the_whole_path_on_many_records(F, many):
    """the unparsed chunk through the encoder: the parser's N count sizes the n_pos buffer of the host-pointer path, its
    base count the streams; the five streams are the oracle's byte for byte, again directly behind a fill with 0xFF; the
    device-resident block, whose n_pos buffer the same count sizes, likewise"""
    ctx = F.Context(*many["tables"])
    try:
        for what in ("fresh handle", "behind fill_scratch(0xFF)"):
            got = ctx.encode_raw(many["raw"])
            same_streams(got, many["want"], what)
            assert np.array_equal(got["recs"], many["recs"]), what
            assert (got["n_bases"], got["used_len"], len(got["n_pos"])) == (many["n_bases"], many["raw"].size, many["n_n"]), what
            assert ctx.fill_scratch(0xFF)[0] > 0
        b = ctx.dblock(many["raw"])
        try:
            b.encode()
            ctx.sync()
            rc, st = b.status()
            assert rc == 0 and (st["n_bases"], st["n_pos_len"]) == (many["n_bases"], many["n_n"])
            same_streams(dict(b.fetch(), rc=0), many["want"], "device-resident block")
        finally:
            b.close()
    finally:
        ctx.close()
