"""The HIP path against the reference's compiled code, directly.

tests/test_reference_pin.py pins the CPU oracle to oracle/_ref/ref_tool (the reference's own coder, header coder,
workspace, parser and container sources, compiled: oracle/ref/); the rest of the GPU suite compares the library with the
oracle.  Here the middleman is left out: dataset analysis, the encode of an unparsed chunk with its header fields, the
decode of a chunk and whole archives cross between the library and ref_tool.  ref_tool is a CPU program run as a child
process; it needs no reference tree once built.  Every comparison is an equality of bytes.
"""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import ref_pin as R

pytestmark = pytest.mark.gpu

TOOL = R.REF_TOOL
FIXTURES = ["SRR065390_sub_1", "without_ns", "SRR065390_sub_2", "SRR065390_1_first5"]
SORT_FROM = 1 << 20   # bases from which fq_build_freq_tables takes the quality counts through the encoder's sort (tables.hip)
CUT_OFF_TAIL = b"@cut.off 1\nACGTAC"   # a record the chunk ends in the middle of: both sides leave it out


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    assert F.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return F


@pytest.fixture(scope="module", autouse=True)
def tool():
    assert os.path.exists(TOOL), ("oracle/_ref/ref_tool is missing: run build() (python __graft_entry__.py) on a machine that has the "
                                  "reference tree; the binary then travels with the working tree")
    return TOOL


_cache = {}


def synth_at_sort_threshold(F, mode):
    """the shortest run of whole synthetic records with at least SORT_FROM bases"""
    raw, _ = F.synth_fastq(4 << 20, mode, seed=31)
    recs = F.parse_fastq(raw)
    total = np.cumsum(recs["len"].astype(np.int64))
    last = int(np.searchsorted(total, SORT_FROM))
    raw = raw[: int(recs[last]["qual_off"]) + int(recs[last]["len"]) + 1]
    assert SORT_FROM <= int(total[last]) < SORT_FROM + int(recs[last]["len"]) and raw.size < 4 << 20
    return raw


def chunk(F, name):
    """-> (raw, recs) of a named input, made once"""
    if name not in _cache:
        if name in FIXTURES:
            raw = np.fromfile(os.path.join(R.ROOT, "tests", "golden", name + ".fastq"), dtype=np.uint8)
        elif name == "edge":
            raw = R.edge_chunk(3)   # (the library, like the oracle, takes reads of 3 bases and more: test_gpu_parity.test_errors)
        elif name.endswith("-sorted"):
            raw = synth_at_sort_threshold(F, int(name[5]))
        else:
            raw, _ = F.synth_fastq(1 << 20, int(name[5]), seed=31)
        raw = np.ascontiguousarray(raw)
        _cache[name] = (raw, O.parse_fastq(raw))
    return _cache[name]


def struct_of(data, dtype):
    return np.frombuffer(data.tobytes(), dtype=dtype).copy()


def format_of(e):
    return ([0 if t == "N" else 1 for t in e["types"]], bytes(e["seps"]), e["first_header"])


# ------------------------------------------------------------------------------------------------------------ tables
@pytest.mark.parametrize("name", FIXTURES + ["synth2-small", "synth4-small", "synth2-sorted", "synth4-sorted"])
def test_dataset_analysis(F, name, tmp_path):
    """F.freq_tables against `ref_tool analyze` (FSE_Sequence / FSE_Quality::calculateFreqTable): the whole structs.
    The fixtures and the small samples take the scattered-atomics histogram, the -sorted ones the encoder's sort."""
    raw, recs = chunk(F, name)
    bases = int(recs["len"].sum())
    assert (bases >= SORT_FROM) == name.endswith("-sorted")
    a = R.analyze(TOOL, raw, tmp_path)
    sft, qft = F.freq_tables(raw, recs)
    assert sft.tobytes() == a["seq_ft"].tobytes(), "sequence FreqTable struct differs from the reference's"
    assert qft.tobytes() == a["qual_ft"].tobytes(), "quality FreqTable struct differs from the reference's"


# ----------------------------------------------------------------------------------------------------------- streams
@pytest.mark.parametrize("table", ["device_parser", "callers_table"])
@pytest.mark.parametrize("name", FIXTURES + ["edge", "synth2-sorted", "synth4-sorted", "synth6-sorted"])
def test_encode_and_decode(F, name, table, tmp_path):
    """ctx.encode_raw with the header coder against `ref_tool encode` (CompressionWorkspace::encodeChunk): the five
    streams, every header field's flags, content and lengths, and where the cut-off record starts; then decode_chunk
    restores the reference's streams and `ref_tool decode` (DecompressionWorkspace::decodeChunk) restores the GPU's"""
    whole, recs = chunk(F, name)
    cut_off = np.concatenate([whole, np.frombuffer(CUT_OFF_TAIL, dtype=np.uint8)])
    e = R.encode(TOOL, cut_off, tmp_path)
    # the device parser finds where the cut-off record starts; a caller with a table has parsed the chunk and cut it there
    # already, as FastqReader::readNextChunk does before encodeChunk sees it (src/fastq_io.cpp:52-60)
    raw = cut_off if table == "device_parser" else whole
    assert e["raw_len"] == whole.size and e["n_records"] == len(recs)
    sft, qft = struct_of(e["seq_ft"], O.SEQ_FT_DTYPE), struct_of(e["qual_ft"], O.QUAL_FT_DTYPE)
    fmt = format_of(e)
    ctx = F.Context(sft, qft)
    try:
        # (F_WRITE_BACK_N: N -> A inside the caller's chunk, as the reference leaves it)
        g = ctx.encode_raw(raw, flags=F.F_WRITE_BACK_N, recs=recs if table == "callers_table" else None, header_format=fmt)
        assert g["rc"] == 0 and g["headers_rc"] == 0, (g["rc"], g.get("headers_rc"), g.get("bad_record"))
        assert g["used_len"] == e["raw_len"]
        assert np.array_equal(g["recs"], recs)
        for k in R.STREAMS:
            assert g[k].tobytes() == e[k].tobytes(), "stream %s differs from the reference's" % k
        assert g["raw_after"][: whole.size].tobytes() == e["raw_after"].tobytes(), "the chunk after N replacement differs"
        assert g["raw_after"][whole.size:].tobytes() == raw[whole.size:].tobytes()
        assert len(g["header_fields"]) == len(e["fields"])
        for i, (got, want) in enumerate(zip(g["header_fields"], e["fields"])):
            for part, a, b in zip(("flags", "content", "lengths"), got, want):
                assert a.tobytes() == b.tobytes(), "header field %d, %s differs from the reference's" % (i, part)
        if table == "device_parser":
            d = ctx.decode_chunk(fmt, e["fields"], e["readlens"], e["seq"], e["qual"], e["n_count"], e["n_pos"], e["raw_len"])
            assert d["rc"] == 0 and d["laid_out_len"] == whole.size
            assert d["raw"].tobytes() == whole.tobytes(), "decode_chunk does not restore the reference's streams"
            dd = R.write_encoded(R.fresh_dir(tmp_path, "from_gpu"), e["first_header"], sft, qft, g, g["header_fields"],
                                 whole.size, len(recs))
            assert R.decode(TOOL, dd).tobytes() == whole.tobytes(), "the reference does not restore the GPU's streams"
    finally:
        ctx.close()


E_SHORT_READ = -2


@pytest.mark.parametrize("table", ["device_parser", "callers_table"])
@pytest.mark.parametrize("quality", [b"I", b"+", b"I5", b"II"])
def test_edge_lengths_the_library_refuses(F, quality, table, tmp_path):
    """Of the edge chunk's lengths 1, 2, 3, 4, 5, 6, 7 and 65535 the library takes 3 and more (test_encode_and_decode[edge])
    and refuses 1 and 2 with FQGPU_E_SHORT_READ.  The reference aborts on its asserts for all of these but one: the read
    of one base with quality '+', which it codes by coincidence (tests/test_reference_pin.py has the cases and the cause,
    DESIGN.md section 2 the decision); the library refuses that one too, on purpose."""
    n = len(quality)
    ordinary = R.edge_records(3)
    raw = R.fastq_of_records(ordinary[:4] + [(b"@a", b"ACGT"[:n], quality)] + ordinary[4:8])
    recs = O.parse_fastq(raw)
    e = R.encode(TOOL, R.edge_chunk(3), tmp_path)
    ctx = F.Context(struct_of(e["seq_ft"], O.SEQ_FT_DTYPE), struct_of(e["qual_ft"], O.QUAL_FT_DTYPE))
    try:
        g = ctx.encode_raw(raw, recs=recs if table == "callers_table" else None)
        assert g["rc"] == E_SHORT_READ
        assert ctx.encode_raw(R.edge_chunk(3))["rc"] == 0, "the handle works afterwards"
    finally:
        ctx.close()


def test_the_short_read_the_reference_codes_is_refused_in_both_directions(F, tmp_path):
    """the read of one base with quality '+': `ref_tool encode` codes the chunk (tests/test_reference_pin.py says why);
    the library's decode applies the length rule of its encode and refuses the reference's streams with
    FQGPU_E_SHORT_READ -- the deliberate, stricter refusal of DESIGN.md section 2, pinned here so that it cannot change
    unnoticed"""
    raw = R.fastq_of_records([(b"@a", b"A", b"+")] + R.edge_records(3)[:4])
    e = R.encode(TOOL, raw, tmp_path)
    assert e["n_records"] == 5 and e["readlens"][0] == 1 and R.decode(TOOL, e["dir"]).tobytes() == raw.tobytes()
    ctx = F.Context(struct_of(e["seq_ft"], O.SEQ_FT_DTYPE), struct_of(e["qual_ft"], O.QUAL_FT_DTYPE))
    try:
        d = ctx.decode_chunk(format_of(e), e["fields"], e["readlens"], e["seq"], e["qual"], e["n_count"], e["n_pos"], e["raw_len"])
        assert d["rc"] == E_SHORT_READ
        assert ctx.encode_raw(raw)["rc"] == E_SHORT_READ
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------- archives
@pytest.fixture(scope="module")
def fqc_tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pin_tool") / "fqc_tool")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-o", exe, os.path.join(R.ROOT, "tools", "fqc_tool.cpp"),
                    "-L" + os.path.join(R.ROOT, "fqcomp28_amd"), "-lfqgpu", "-Wl,-rpath," + os.path.join(R.ROOT, "fqcomp28_amd"),
                    "-lpthread"], check=True)
    return exe


@pytest.fixture(scope="module")
def archive_input(F, tmp_path_factory):
    raw, _ = F.synth_fastq(3 << 20, 4, seed=5)
    path = str(tmp_path_factory.mktemp("pin_archives") / "in.fastq")
    raw.tofile(path)
    return path, raw


def n_blocks(path):
    return int(np.fromfile(path, dtype="<u4", count=1)[0])   # (the container begins with its number of blocks)


def test_the_reference_restores_an_archive_of_fqc_tool(fqc_tool, archive_input, tmp_path):
    src, raw = archive_input
    arc, back = str(tmp_path / "g.fqc"), str(tmp_path / "back.fastq")
    r = subprocess.run([fqc_tool, "c", src, arc, "-t", "2", "-R", "1", "-S", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert n_blocks(arc) >= 3
    R.run(TOOL, "read-archive", arc, back)
    assert open(back, "rb").read() == raw.tobytes()


@pytest.mark.parametrize("index", [False, True])
def test_fqc_tool_restores_an_archive_of_the_reference(fqc_tool, archive_input, index, tmp_path):
    """(the reference's loop keeps one CompressedBuffersDst for all its chunks, so the N buffers of a block hold those of
    the blocks before it: the restore reads them from the end)"""
    src, raw = archive_input
    arc, back = str(tmp_path / "r.fqc"), str(tmp_path / "back.fastq")
    R.run(TOOL, "write-archive", src, arc, 1 << 20, 1 << 20)
    assert n_blocks(arc) >= 3
    r = subprocess.run([fqc_tool, "d", arc, back, "-t", "2"] + (["--index"] if index else []), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    assert open(back, "rb").read() == raw.tobytes()
