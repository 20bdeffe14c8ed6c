"""Pins the CPU oracle to the reference's compiled code.

Every parity test trusts oracle/fqc_oracle.c and oracle/headers_oracle.py, which are this project's reading of the
reference's src/fse_sequence.cpp, src/fse_quality.cpp, src/workspace.cpp, src/headers.cpp and src/fastq_io.cpp.  Here
the reading meets the thing read: oracle/_ref/ref_tool_asan is those sources, unmodified, compiled with asserts on and
under AddressSanitizer against the shim of oracle/ref/ (zstd's names over oracle/fse_oracle.c; the project's misc coder
for libbsc), driven by oracle/ref/ref_tool.cpp.  Every comparison is an equality of bytes or an agreed refusal (the
reference aborts on an assert or throws exactly where the oracle returns an error or raises).

The reference is only given inputs the oracle codes (rc 0): on overflow it has undefined behaviour.
What stays unpinned: the arithmetic of the zstd fork behind the shim (fse_oracle.c, pinned to libzstd 1.4.8 in
test_oracle_zstd.py) and libbsc's bytes.
"""
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
import ref_pin as R

sys.path.insert(0, os.path.join(R.ROOT, "oracle"))
import headers_oracle as HO  # noqa: E402

TOOL = R.REF_TOOL_ASAN

if not os.path.exists(TOOL) and not R.reference_tree_present():
    pytestmark = pytest.mark.skip(reason="neither oracle/_ref/ref_tool_asan nor the reference tree it is built from is here")

FIXTURES = ["SRR065390_sub_1", "without_ns", "SRR065390_sub_2", "SRR065390_1_first5"]
SYNTH_MODES = [1, 2, 3, 4, 5, 6]
INPUTS = FIXTURES + ["synth%d" % m for m in SYNTH_MODES] + ["edge"]

E_SHORT_READ = -2


@pytest.fixture(scope="module", autouse=True)
def tool():
    assert os.path.exists(TOOL), "oracle/_ref/ref_tool_asan is missing: run build() (make -C oracle) where the reference tree is"
    return TOOL


_cache = {}


def chunk(name, seed=28):
    """-> (raw, recs, headers) of a named input, made once"""
    key = (name, seed)
    if key not in _cache:
        if name in FIXTURES:
            raw = np.fromfile(os.path.join(R.ROOT, "tests", "golden", name + ".fastq"), dtype=np.uint8)
        elif name.startswith("synth"):
            import fqcomp28_amd as F  # (the generator is host code of the library: no GPU involved)
            raw, _ = F.synth_fastq(1 << 20, int(name[5:]), seed=seed)
        else:
            raw = R.edge_chunk(3)
        recs = O.parse_fastq(raw)
        _cache[key] = (raw, recs, R.headers_of(raw, recs))
    return _cache[key]


def oracle_tables(name, seed=28):
    key = ("ft", name, seed)
    if key not in _cache:
        raw, recs, _ = chunk(name, seed)
        _cache[key] = O.freq_tables(raw, recs)[2:]
    return _cache[key]


def sample_for(name):
    """another sample for an input: another fixture, or the same synthetic mode from another seed (tables of another
    kind of data would push a stream past the capacity rule, where the reference may not be called)"""
    if name.startswith("synth"):
        return name, 5
    return ("SRR065390_sub_2" if name != "SRR065390_sub_2" else "SRR065390_sub_1"), 28


def assert_streams(e, o):
    assert o["rc"] == 0, "the reference may only be given what the oracle codes"
    for k in R.STREAMS:
        assert e[k].tobytes() == o[k].tobytes(), "stream %s: the reference and the oracle differ" % k
    assert e["raw_after"].tobytes() == o["raw_after"].tobytes(), "the chunk after N replacement differs"


def assert_fields(e, headers, first_header=None):
    types, seps, fields = R.oracle_fields(headers, first_header)
    assert e["types"] == types and e["seps"] == list(seps)
    assert len(e["fields"]) == len(fields)
    for i, (got, want) in enumerate(zip(e["fields"], fields)):
        for part, g, w in zip(("flags", "content", "lengths"), got, want):
            assert g.tobytes() == w, "header field %d, %s: the reference and the oracle differ" % (i, part)


# ------------------------------------------------------------------------------------------------------------ tables
@pytest.mark.parametrize("name", INPUTS)
def test_tables_and_format(name, tmp_path):
    """`analyze` (DatasetMeta(chunk): both calculateFreqTable, HeaderFormatSpeciciation::fromHeader) against
    O.freq_tables and HO.format_from_header: whole structs, first header, field types and separators"""
    raw, recs, hdrs = chunk(name)
    a = R.analyze(TOOL, raw, tmp_path)
    sft, qft = oracle_tables(name)
    assert a["seq_ft"].tobytes() == sft.tobytes(), "sequence FreqTable struct differs"
    assert a["qual_ft"].tobytes() == qft.tobytes(), "quality FreqTable struct differs"
    types, seps = HO.format_from_header(hdrs[0])
    assert a["first_header"] == hdrs[0] and a["types"] == types and a["seps"] == list(seps)


# ----------------------------------------------------------------------------------------------------------- streams
@pytest.mark.parametrize("tables", ["own", "other_sample"])
@pytest.mark.parametrize("name", INPUTS)
def test_streams_and_header_fields(name, tables, tmp_path):
    """`encode` (CompressionWorkspace::encodeChunk) against OracleCtx.encode and headers_oracle.encode_headers: the five
    streams, the chunk after N replacement, every header field's three buffers; then each side decodes the other's"""
    raw, recs, hdrs = chunk(name)
    if tables == "own":
        sft, qft = oracle_tables(name)
        e = R.encode(TOOL, raw, tmp_path)
    else:
        sname, seed = sample_for(name)
        sft, qft = oracle_tables(sname, seed)
        e = R.encode(TOOL, raw, tmp_path, sample=chunk(sname, seed)[0])
    assert e["seq_ft"].tobytes() == sft.tobytes() and e["qual_ft"].tobytes() == qft.tobytes()
    octx = O.OracleCtx(sft, qft)
    o = octx.encode(raw, recs)
    assert_streams(e, o)
    assert_fields(e, hdrs)
    assert (e["raw_len"], e["n_records"]) == (raw.size, len(recs))

    # the oracle's decoders restore the reference's streams
    rc, back = octx.decode(e["seq"], e["qual"], e["n_count"], e["n_pos"], recs, O.blank_skeleton(raw, recs))
    assert rc == 0 and back.tobytes() == raw.tobytes()
    assert HO.decode_headers(len(hdrs), hdrs[0], [_streams_of(f) for f in e["fields"]]) == hdrs
    # DecompressionWorkspace::decodeChunk restores the oracle's
    _, _, fields = R.oracle_fields(hdrs)
    d = R.write_encoded(R.fresh_dir(tmp_path, "from_oracle"), hdrs[0], sft, qft, o, fields, raw.size, len(recs))
    assert R.decode(TOOL, d).tobytes() == raw.tobytes()
    octx.close()


def test_committed_golden_vectors_are_what_the_reference_writes(tmp_path):
    """tests/golden/SRR065390_1_first5.*.bin (make_golden.py writes them from the oracle)"""
    golden = os.path.join(R.ROOT, "tests", "golden")
    e = R.encode(TOOL, chunk("SRR065390_1_first5")[0], tmp_path)
    for k, data in (("seq", e["seq"]), ("qual", e["qual"]), ("n_pos", e["n_pos"]), ("seq_ft", e["seq_ft"])):
        with open(os.path.join(golden, "SRR065390_1_first5.%s.bin" % k), "rb") as f:
            assert f.read() == data.tobytes(), k


def _streams_of(parts):
    s = HO.FieldStreams()
    s.flags, s.content, s.lengths = (bytearray(p.tobytes()) for p in parts)
    return s


def test_streams_with_foreign_log12_tables(tmp_path):
    """tables the reference never builds but its format allows (every context at log 12), given as struct files.  (The
    log-5 tables of test_foreign_table_logs are left out: both coders refuse them under the capacity rule, and past it
    the reference has undefined behaviour.)"""
    raw, recs, hdrs = chunk("synth2")
    sft, qft = oracle_tables("synth2")
    sft12, qft12 = R.rescale_tables(sft, 12), R.rescale_tables(qft, 12)
    octx = O.OracleCtx(sft12, qft12)
    o = octx.encode(raw, recs)
    e = R.encode(TOOL, raw, tmp_path, tables=(sft12, qft12))
    assert e["seq_ft"].tobytes() == sft12.tobytes() and e["qual_ft"].tobytes() == qft12.tobytes()
    assert_streams(e, o)
    _, _, fields = R.oracle_fields(hdrs)
    d = R.write_encoded(R.fresh_dir(tmp_path, "from_oracle"), hdrs[0], sft12, qft12, o, fields, raw.size, len(recs))
    assert R.decode(TOOL, d).tobytes() == raw.tobytes()
    octx.close()


# ----------------------------------------------------------------------------------------------------- the edge chunk
def test_edge_chunk_holds_what_it_says():
    recs = R.edge_records(1)
    lens = {len(s) for _, s, _ in recs}
    assert set(R.EDGE_LENGTHS) <= lens
    for n in R.EDGE_LENGTHS:
        mine = [(s, q) for _, s, q in recs if len(s) == n]
        assert any(s[:1] == b"N" for s, _ in mine) and any(s[-1:] == b"N" for s, _ in mine), n
        assert any(q[0] == R.PHRED0 for _, q in mine) and any(q[-1] == R.PHRED63 for _, q in mine), n
        if n < 65535:
            assert any(s == b"N" * n for s, _ in mine), n
        if n >= 3:
            assert any(b"NN" in s and s != b"N" * n for s, _ in mine), n
        # the quality context of symbol i looks at the pair (q[i-2], q[i-3]), a missing one counting as 0, and at whether
        # the two are equal: both kinds at the third symbol (the pair is (q[0], nothing)) and at every later one
        if 3 <= n < 65535:   # (there is one read of 65535 bases: its third symbol sees one kind, its later ones both)
            assert {q[0] == R.PHRED0 for _, q in mine} == {True, False}, n
        if n >= 4:
            assert {q[i - 2] == q[i - 3] for _, q in mine for i in range(3, min(n, 200))} == {True, False}, n
    hl = {len(h) for h, _, _ in recs}
    assert 2 in hl and 254 in hl
    assert len(R.edge_chunk(3)) < 200 << 10


def _short_read_chunk(quality):
    """one short read with this quality line in front of four ordinary reads of the edge chunk"""
    n = len(quality)
    return R.fastq_of_records([(b"@a", b"ACGT"[:n], quality)] + R.edge_records(3)[:4])


def _oracle_refuses_as_short(raw):
    sft, qft = oracle_tables("edge")
    octx = O.OracleCtx(sft, qft)
    try:
        return octx.encode(raw, O.parse_fastq(raw))["rc"] == E_SHORT_READ
    finally:
        octx.close()


# QualityEncoder::encodeRecord (src/fse_quality.cpp:5-53) starts from the last quality and takes the three symbols before it
# from the bytes in front of it, whatever they are.  For a read of one or two bases those bytes are the newline and the
# '+' of the separator line, and the asserts of lines 44 and 50 compare what was taken with the read's own qualities:
#   two bases, unequal qualities   line 44 fails: the symbol taken for the first quality is not the second
#   two bases, equal qualities     line 44 holds; line 50 fails: the byte in front of the line is the newline, never a quality
#   one base, any quality but '+'  line 50 fails: the byte two in front of the line is the '+' of the separator line
#   one base, quality '+'          line 50 HOLDS: that '+' happens to be the read's quality (next test)
@pytest.mark.parametrize("quality,line", [(b"I", 50), (b"!", 50), (b"I5", 44), (b"II", 50), (b"++", 50)])
def test_reads_the_oracle_refuses_the_reference_refuses(quality, line, tmp_path):
    """Of the edge chunk's lengths 1, 2, 3, 4, 5, 6, 7 and 65535 the oracle takes 3 and more (test_streams_...[edge]) and
    refuses 1 and 2 with FQO_E_SHORT_READ.  The reference aborts on them, at the assert the table above names -- with the
    one exception of the next test."""
    raw = _short_read_chunk(quality)
    assert _oracle_refuses_as_short(raw)
    sft, qft = oracle_tables("edge")
    with pytest.raises(R.Refused) as x:
        R.encode(TOOL, raw, tmp_path, tables=(sft, qft))
    assert x.value.how == "assert" and "fse_quality.cpp:%d" % line in x.value.stderr


def test_the_one_short_read_the_reference_codes_and_the_oracle_refuses(tmp_path):
    """A DIFFERENCE, kept on purpose: a read of one base whose quality is '+' (Phred 10) passes the
    reference's asserts by coincidence -- the byte its coder takes for the quality is the '+' of the separator line -- and
    the reference codes it, correctly: its own decoder restores the chunk.  Were the separator line to repeat the header
    (`+name`), the same read would abort.  The oracle and the library refuse every read shorter than three bases
    (FQO_E_SHORT_READ / FQGPU_E_SHORT_READ) instead of depending on what lies in front of the quality line."""
    raw = _short_read_chunk(b"+")
    assert raw.tobytes().startswith(b"@a\nA\n+\n+\n")
    assert _oracle_refuses_as_short(raw)
    e = R.encode(TOOL, raw, tmp_path)
    recs = O.parse_fastq(raw)
    assert e["n_records"] == len(recs) == 5 and e["raw_len"] == raw.size
    assert e["readlens"].tolist() == recs["len"].tolist() and e["readlens"][0] == 1
    assert e["raw_after"].tobytes() == raw.tobytes()   # (no N in this chunk)
    assert R.decode(TOOL, e["dir"]).tobytes() == raw.tobytes()
    # the oracle's decoder has no length rule: it restores what the reference wrote
    octx = O.OracleCtx(np.frombuffer(e["seq_ft"].tobytes(), dtype=O.SEQ_FT_DTYPE).copy(),
                       np.frombuffer(e["qual_ft"].tobytes(), dtype=O.QUAL_FT_DTYPE).copy())
    rc, back = octx.decode(e["seq"], e["qual"], e["n_count"], e["n_pos"], recs, O.blank_skeleton(raw, recs))
    octx.close()
    assert rc == 0 and back.tobytes() == raw.tobytes()
    # with the separator line repeating the header the coincidence is gone
    named = np.frombuffer(raw.tobytes().replace(b"@a\nA\n+\n+\n", b"@a\nA\n+a\n+\n", 1), dtype=np.uint8)
    with pytest.raises(R.Refused) as x:
        R.encode(TOOL, named, tmp_path, "named")
    assert x.value.how == "assert" and "fse_quality.cpp:50" in x.value.stderr


# ----------------------------------------------------------------------------------------------------- header fields
@pytest.mark.parametrize("first", ["a_header_from_the_middle_of_another_chunk", "the_one_of_test_gpu_headers"])
def test_first_header_of_the_dataset_is_not_the_chunks_first(first, tmp_path):
    """Workspace::startNewChunk: a chunk's first header is coded against the dataset's"""
    raw, recs, hdrs = chunk("SRR065390_sub_2")
    first = {"a_header_from_the_middle_of_another_chunk": chunk("SRR065390_sub_1")[2][500],
             "the_one_of_test_gpu_headers": b"@SRR065390.1 HWUSI-EAS687_61DAJ:1:1:1055:3384 length=100"}[first]
    assert first != hdrs[0] and HO.format_from_header(first) == HO.format_from_header(hdrs[0])
    e = R.encode(TOOL, raw, tmp_path, first_header=first)
    assert e["first_header"] == first
    assert_fields(e, hdrs, first)
    own = R.oracle_fields(hdrs)[2]
    assert any(g.tobytes() != w for got, want in zip(e["fields"], own) for g, w in zip(got, want)), \
        "the fields differ from those coded against the chunk's own first header"


@pytest.mark.parametrize("which", ["changing_wrapping_cut", "single_field", "64_fields", "254_bytes", "300_bytes_never_changing"])
def test_awkward_headers(which, tmp_path):
    """the lists tests/test_gpu_headers.py gives the device coder: values that repeat, wrap or are cut, `12ab`, `007`, `-0`, one field, 64
    fields, a field of 254 bytes that changes and one of 300 that never does"""
    hdrs = {"changing_wrapping_cut": R.headers_changing_wrapping_cut, "single_field": R.headers_single_field,
            "64_fields": R.headers_64_fields,
            "254_bytes": lambda: [b"@r.%d %s" % (i + 1, b"z" * 254) for i in range(300)],
            "300_bytes_never_changing": lambda: [b"@r.%d %s" % (i + 1, b"z" * 300) for i in range(300)]}[which]()
    if which == "changing_wrapping_cut":
        assert any(b" 12ab " in h for h in hdrs) and any(b" 007 " in h for h in hdrs) and any(b" -0 " in h for h in hdrs)
    if which == "64_fields":
        assert len(HO.format_from_header(hdrs[0])[0]) == 64
    raw = R.fastq_of_headers(hdrs)
    sft, qft = oracle_tables("SRR065390_sub_1")
    e = R.encode(TOOL, raw, tmp_path, tables=(sft, qft))
    assert_fields(e, hdrs)
    # what the reference's own decoder makes of its fields is what the oracle's makes of them
    # (a number written `007`, `-0` or `12ab` comes back as 7, 0, 12: the restored chunk is then shorter than its buffer)
    import fqcomp28_amd as F
    back = R.decode(TOOL, e["dir"])
    want = HO.decode_headers(len(hdrs), hdrs[0], [_streams_of(f) for f in e["fields"]])
    assert R.headers_of(back, F.parse_fastq(back)) == want
    assert (want == hdrs) == (which != "changing_wrapping_cut")


@pytest.mark.parametrize("at,bad", R.UNCODABLE + (R.UNCODABLE_LATER,))
def test_headers_that_cannot_be_coded_are_refused_at_the_same_record(at, bad, tmp_path):
    """the reference asserts (src/headers.cpp: from_chars, FIELDLEN_MAX) exactly where the oracle raises: the headers up
    to the bad one are coded by both, with the bad one as the last both refuse"""
    good = R.UNCODABLE_GOOD
    hdrs = list(good[:at]) + [bad]
    sft, qft = oracle_tables("SRR065390_sub_1")
    if at:
        assert_fields(R.encode(TOOL, R.fastq_of_headers(hdrs[:at]), tmp_path, "before", tables=(sft, qft), first_header=good[0]),
                      hdrs[:at], good[0])
    with pytest.raises(ValueError):
        HO.encode_headers(hdrs, good[0])
    with pytest.raises(R.Refused) as x:
        R.encode(TOOL, R.fastq_of_headers(hdrs), tmp_path, "with", tables=(sft, qft), first_header=good[0])
    assert x.value.how == "assert" and "headers.cpp" in x.value.stderr


@pytest.mark.parametrize("header", [b"@a.", b"@SRR1 x ", b"@r:1:"])
def test_a_first_header_that_ends_in_a_separator_is_refused(header, tmp_path):
    with pytest.raises(ValueError):
        HO.format_from_header(header)
    raw = R.fastq_of_headers([header, header])
    with pytest.raises(R.Refused) as x:
        R.analyze(TOOL, raw, tmp_path)
    assert x.value.how == "exception" and "alnum" in x.value.stderr


# --------------------------------------------------------------------------------------------------------- container
def test_container(tmp_path):
    """`write-archive` (FastqReader::readNextChunk, encodeChunk and Archive::writeBlock in the loop of src/process.cpp)
    against oracle/fqc_archive.py and the oracle, block by block; `read-archive` restores it, and restores the same
    blocks written by fqc_archive.write_archive.  The loop keeps one CompressedBuffersDst, whose clear() leaves n_count
    and n_pos alone: a block's two N buffers begin with those of the blocks before it."""
    import fqcomp28_amd as F
    import fqc_archive as A
    raw, _ = F.synth_fastq(1 << 20, 4, seed=5)
    src, arc = R.put(os.path.join(tmp_path, "in.fastq"), raw), os.path.join(tmp_path, "r.fqc")
    R.run(TOOL, "write-archive", src, arc, 200 << 10, 300 << 10)
    first, sft_b, qft_b, blocks, entries = A.read_archive(arc)
    assert len(blocks) >= 5 and [b.idx for b in blocks] == list(range(len(blocks)))

    # the dataset's tables are those of the whole records in the first 300 KiB
    recs = O.parse_fastq(raw)
    ends = recs["qual_off"].astype(np.int64) + recs["len"] + 1
    sample = raw[: int(ends[ends <= 300 << 10][-1])]
    sft, qft = O.freq_tables(sample, O.parse_fastq(sample))[2:]
    assert first == R.headers_of(raw, recs[:1])[0] and sft_b == sft.tobytes() and qft_b == qft.tobytes()

    octx = O.OracleCtx(sft, qft)
    unpack = lambda part: F.memdecompress(np.frombuffer(part[1], dtype=np.uint8), part[0]).tobytes()  # noqa: E731
    at, n_count, n_pos, rebuilt = 0, b"", b"", []
    for b in blocks:
        # a chunk is the whole records of the reader's next 200 KiB, the cut-off record carried over
        assert at + b.total <= raw.size and b.total <= 200 << 10 and (at + b.total == raw.size or b.total > (200 << 10) - 700)
        part = raw[at: at + b.total]
        at += b.total
        precs = O.parse_fastq(part)
        o = octx.encode(part, precs)
        assert o["rc"] == 0 and b.n_records == len(precs)
        assert b.seq == o["seq"].tobytes() and b.qual == o["qual"].tobytes()
        assert unpack(b.readlens) == o["readlens"].tobytes()
        n_count += o["n_count"].tobytes()
        n_pos += o["n_pos"].tobytes()
        assert unpack(b.n_count) == n_count and unpack(b.n_pos) == n_pos
        types, _, fields = R.oracle_fields(R.headers_of(part, precs), first)
        for t, got, want in zip(types, b.fields, fields):
            want = want if t == HO.STRING else want[1:2]
            assert [unpack(g) for g in got] == list(want)
        rebuilt.append(A.block_from_streams(b.idx, part, precs, o, first, compress=lambda d: F.memcompress(np.frombuffer(d, dtype=np.uint8)).tobytes(),
                                            n_count_prefix=n_count[: len(n_count) - o["n_count"].nbytes],
                                            n_pos_prefix=n_pos[: len(n_pos) - o["n_pos"].nbytes]))
    assert at == raw.size
    octx.close()

    back = os.path.join(tmp_path, "back.fastq")
    R.run(TOOL, "read-archive", arc, back)
    assert open(back, "rb").read() == raw.tobytes()
    # the second reading of the container writes the very file, and the reference reads what it writes
    again = os.path.join(tmp_path, "again.fqc")
    A.write_archive(again, first, sft_b, qft_b, rebuilt)
    assert open(again, "rb").read() == open(arc, "rb").read()
    A.write_archive(again, first, sft_b, qft_b, rebuilt[::-1])   # (blocks in another order: the index says which is which)
    R.run(TOOL, "read-archive", again, back)
    assert open(back, "rb").read() == raw.tobytes()


# ------------------------------------------------------------------------------------------------------------ bounds
QUAL_FLOOR = 8192 * 1024
BOUND_SIZES = ([0, 1, 1023, 1024, 1025] + [QUAL_FLOOR * 8 // 7 + d for d in (-2, -1, 0, 1, 2)]
               + [(QUAL_FLOOR - 1024) * 8 // 7 + d for d in (-1, 0, 1, 2)]   # where the quality bound leaves its floor
               + [1 << 28])


def test_bounds():
    """Workspace::compressBoundSequence / compressBoundQuality against the oracle's and the library's"""
    import fqcomp28_amd as F
    lines = R.run(TOOL, "bounds", *[str(n) for n in BOUND_SIZES]).split("\n")
    got = [tuple(int(v) for v in ln.split()) for ln in lines if ln]
    assert [g[0] for g in got] == BOUND_SIZES
    L = O.lib()
    for n, seq, qual in got:
        assert (L.fqo_bound_seq(n), L.fqo_bound_qual(n)) == (seq, qual), n
        assert (F.bound_seq(n), F.bound_qual(n)) == (seq, qual), n
    quals = [q for _, _, q in got]
    assert min(quals) == QUAL_FLOOR and quals[10] == QUAL_FLOOR and quals[13] == QUAL_FLOOR + 1


# ------------------------------------------------------------------------------------------------------------ parser
CUTS = ["cut-in-line", "cut-at-start-of-line", "cut-before-newline-of-line"]
PARSER_CASES = ([name + "-whole" for name in FIXTURES]
                + ["%s-%s-%d" % (name, cut, k) for name in FIXTURES for k in range(4) for cut in CUTS]
                + ["plus-lines-repeat-the-header-qualities-start-with-at-or-plus", "same-cut-in-a-quality-that-starts-with-at",
                   "one-header-line-only"])


def _parser_cases():
    """-> {case: chunk}, made once: the fixtures whole and cut inside each of the four lines of the last record, at the
    start of each and just before each one's newline; '+' lines that repeat the header; qualities that begin with @ or +"""
    if "parser" not in _cache:
        cases = {}
        for name in FIXTURES:
            raw = chunk(name)[0]
            b = raw.tobytes()
            cases[name + "-whole"] = raw
            lines = b.split(b"\n")[-5:-1]
            ends, pos = [], len(b)
            for ln in reversed(lines):
                ends.insert(0, pos)
                pos -= len(ln) + 1
            starts = [pos] + ends[:-1]
            assert b[starts[0]:starts[0] + 1] == b"@" and b[starts[2]:starts[2] + 1] == b"+"
            for k in range(4):
                cases["%s-cut-in-line-%d" % (name, k)] = raw[: (starts[k] + ends[k]) // 2]
                cases["%s-cut-at-start-of-line-%d" % (name, k)] = raw[: starts[k]]
                cases["%s-cut-before-newline-of-line-%d" % (name, k)] = raw[: ends[k] - 1]
        plus = b"".join(b"@r%d x\nACGTN\n+r%d x\n%s\n" % (i, i, q)
                        for i, q in enumerate([b"IIIII", b"@IIII", b"+IIII", b"@@@@@", b"+++++", b"I@+@I"]))
        cases["plus-lines-repeat-the-header-qualities-start-with-at-or-plus"] = np.frombuffer(plus, dtype=np.uint8)
        cases["same-cut-in-a-quality-that-starts-with-at"] = np.frombuffer(plus[:-4], dtype=np.uint8)
        cases["one-header-line-only"] = np.frombuffer(b"@r0 x", dtype=np.uint8)
        assert sorted(cases) == sorted(PARSER_CASES)
        _cache["parser"] = cases
    return _cache["parser"]


@pytest.mark.parametrize("case", PARSER_CASES)
def test_parser(case, tmp_path):
    """FastqReader::parseRecords against fqgpu_parse_fastq (host): the record table and where the cut-off record starts"""
    import fqcomp28_amd as F
    raw = np.ascontiguousarray(_parser_cases()[case])
    table, used = R.parse(TOOL, raw, tmp_path)
    recs = F.parse_fastq(raw)
    assert len(table) == len(recs)
    for k in ("seq_off", "qual_off", "len"):
        assert np.array_equal(table[k], recs[k]), k
    ends = recs["qual_off"].astype(np.int64) + recs["len"] + 1
    assert used == (int(ends[-1]) if len(recs) else 0)
    hdr_off = np.concatenate(([0], ends[:-1])) if len(recs) else ends
    assert np.array_equal(table["hdr_off"], hdr_off) and np.array_equal(table["hdr_len"], recs["seq_off"] - 1 - hdr_off)


# -------------------------------------------------------------------------------------------------------------- shim
def _shim_sizes(log, max_sv):
    got = R.run(TOOL, "shim-sizes", str(log), str(max_sv)).split()
    return {got[i]: int(got[i + 1]) for i in range(0, len(got), 2)}


def test_shim_size_macros_against_libzstd():
    """the shim's table sizes are the oracle's layouts, and libzstd's FSE_buildCTable_wksp / FSE_buildDTable_wksp accept
    the workspaces the reference sizes with the shim's macros: one of (MAX_SYMBOL + 1, max_log) for every CTable and one
    of (max_log, MAX_SYMBOL) for every DTable (src/fse_common.hpp), for every max_log a dataset can have -- 5 and more
    with four symbols, 7 and more with 64 (FSE_optimalTableLog) -- and every table log up to it.  (The macros are zstd
    1.5's; below log 7 with 64 symbols libzstd 1.4.8 asks for more than they give, which no table of the reference meets.)"""
    import test_oracle_zstd as TZ
    if TZ.Z is None:
        pytest.skip("libzstd.so.1 with FSE exports not found")
    L = O.lib()
    for max_sv, min_log in ((3, 5), (63, 7)):
        assert L.fo_optimal_table_log(0, max_sv + 1, max_sv) >= min_log
        for max_log in range(min_log, 13):
            c_wksp = _shim_sizes(max_log, max_sv + 1)["ctable_wksp_bytes"]
            d = _shim_sizes(max_log, max_sv)
            d_wksp = d["dtable_wksp_bytes"]
            assert d["dtable_wksp_u32"] * 4 >= d_wksp
            assert d["ctable_u32"] == L.fo_ctable_words(max_log, max_sv) and d["dtable_u32"] == L.fo_dtable_words(max_log)
            wk = np.zeros(max(c_wksp, d_wksp) + 8, dtype=np.uint8)
            for log in range(min_log, max_log + 1):
                norm = np.full(max_sv + 1, (1 << log) // (max_sv + 1), dtype=np.int16)
                ct = np.zeros(L.fo_ctable_words(log, max_sv), dtype=np.uint32)
                dt = np.zeros(L.fo_dtable_words(log), dtype=np.uint32)
                assert TZ.Z.FSE_buildCTable_wksp(O.ptr(ct), O.ptr(norm), max_sv, log, O.ptr(wk), c_wksp) == 0, (max_sv, max_log, log)
                assert TZ.Z.FSE_buildDTable_wksp(O.ptr(dt), O.ptr(norm), max_sv, log, O.ptr(wk), d_wksp) == 0, (max_sv, max_log, log)
                ours_c, ours_d = np.zeros_like(ct), np.zeros_like(dt)
                assert L.fo_build_ctable(O.ptr(ours_c), O.ptr(norm), max_sv, log) == 0 and np.array_equal(ours_c, ct)
                assert L.fo_build_dtable(O.ptr(ours_d), O.ptr(norm), max_sv, log) == 0 and np.array_equal(ours_d, dt)
