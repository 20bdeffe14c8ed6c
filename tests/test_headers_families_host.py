"""The header families of tests/headers_ref.py held to account on the CPU: the generator's own property asserts, the
reference (`restate` over oracle/headers_oracle.py) against the host coder (fqcomp28_amd/csrc/headers.hpp through
tests/cpp/headers_tool.cpp, under AddressSanitizer and UBSan where g++ has them) and, where it is built, against the
reference's compiled code (oracle/_ref/ref_tool_asan).  tests/test_gpu_headers_families.py gives the same cases to the
device."""
import os
import subprocess
import sys

import numpy as np
import pytest

import headers_ref as H
import oracle_lib as O
import ref_pin as R
from test_headers import tool  # noqa: F401  (the fixture that builds headers_tool)

sys.path.insert(0, os.path.join(R.ROOT, "oracle"))
import headers_oracle as HO  # noqa: E402

REF = R.REF_TOOL_ASAN
needs_ref = pytest.mark.skipif(not os.path.exists(REF) and not R.reference_tree_present(),
                               reason="neither oracle/_ref/ref_tool_asan nor the reference tree it is built from is here")

CODED = H.by_kind("ok", "windows", "refusals")
UNCODABLE = H.by_kind("uncodable")


def ids(cases):
    return [H.case_id(c) for c in cases]


def test_every_family_is_there_and_asserts_its_property():
    """families() runs every generator, and every generator asserts the property its cases are named for"""
    cases = H.families()
    assert [f.__name__ for f in H.FAMILIES] == ["_edge_new", "_carried_value", "_group_of_256", "_encode_rounds", "_decode_rounds",
                                                "_stage_threshold", "_numeric_text", "_uncodable", "_separator_first", "_windows", "_refusals"]
    assert {c.family for c in cases} == {"edge-new", "carried-value", "group-of-256", "encode-rounds", "decode-rounds",
                                         "stage-threshold", "numeric-text", "uncodable", "separator-first", "windows", "refusals"}
    assert sorted(len(c.headers) for c in cases if c.family == "encode-rounds") == [16383, 16384, 16385, 32769]
    assert sorted(len(c.headers) for c in cases if c.family == "decode-rounds") == [65536, 65537]
    assert sum(len(c.headers) for c in cases) <= 400000, "the Python reference is the long pole"
    assert len(CODED) + len(UNCODABLE) == len(cases)
    for c in cases:  # two to four fields
        assert 2 <= len(HO.format_from_header(c.first)[0]) <= 4


def write_fastq(path, headers):
    with open(path, "wb") as f:
        f.write(b"".join(h + b"\nA\n+\nI\n" for h in headers))
    return str(path)


def hex_line(b):
    return bytes(b).hex() if len(b) else "-"


def host_decode(tool, path, first, n, fields):  # noqa: F811
    """-> [headers] or the record headers.hpp's decodeHeader throws at"""
    with open(path, "w") as f:
        f.write(first.decode("latin-1") + "\n%d\n" % n)
        for parts in fields:
            for p in parts:
                f.write(hex_line(p) + "\n")
    r = subprocess.run([tool, "decode", str(path)], capture_output=True)
    if r.returncode == 3:
        return int(r.stdout.split()[2].rstrip(b":"))
    assert r.returncode == 0, r.stdout[-400:] + r.stderr[-2000:]
    lines = r.stdout.split(b"\n")
    assert lines[-2] == b"decoded ok %d" % n
    return lines[:-2]


@pytest.mark.parametrize("case", CODED, ids=ids(CODED))
def test_host_coder_gives_the_oracles_streams_and_decodes_them(tool, tmp_path, case):  # noqa: F811
    fields = H.oracle_fields(case)
    types = HO.format_from_header(case.first)[0]
    r = subprocess.run([tool, "code", write_fastq(tmp_path / "in.fastq", case.headers), case.first.decode("latin-1")], capture_output=True, text=True)
    lossless = case.extra.get("lossless", True)
    # (the tool compares what it decodes with its input: a text that does not come back ends it with 1 behind the streams)
    assert r.returncode == (0 if lossless else 1), r.stdout[-400:] + r.stderr[-2000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("field ")]
    assert [p[2] for p in lines] == types
    for p, want in zip(lines, fields):
        got = tuple(b"" if x == "-" else bytes.fromhex(x) for x in p[3:6])
        assert got == want
    if lossless:
        assert r.stdout.splitlines()[-1] == "roundtrip ok %d" % len(case.headers)
    # the reference layout's headers are what the host decoder makes of the streams
    rds = H.reads(len(case.headers))
    total = H.chunk_table(HO.decode_headers(len(case.headers), case.first, [_streams(f) for f in fields]), rds)[1]
    L = H.restate(case.first, fields, rds, total)
    assert L.starts[-1] == total and (L.headers == case.headers) == lossless
    assert host_decode(tool, tmp_path / "streams.txt", case.first, len(case.headers), fields) == L.headers
    if lossless:
        assert L.raw == R.fastq_of_headers(case.headers).tobytes()
        assert L.recs == H.chunk_table(case.headers, rds)[0]
        assert L.window(0, len(rds)) == (L.raw, L.recs)
        fa, fa_recs = L.fasta(0, len(rds))
        assert fa == b"".join(b">" + h[1:] + b"\n" + s + b"\n" for h, (s, _) in zip(case.headers, rds))
        assert all(fa[o: o + n] == s for (o, q, n), (s, _) in zip(fa_recs, rds)) and all(q == 0 for _, q, _ in fa_recs)


def _streams(parts):
    s = HO.FieldStreams()
    s.flags, s.content, s.lengths = (bytearray(p) for p in parts)
    return s


@pytest.mark.parametrize("case", UNCODABLE, ids=ids(UNCODABLE))
def test_host_coder_refuses_at_the_same_record(tool, tmp_path, case):  # noqa: F811
    with pytest.raises(ValueError):
        HO.encode_headers(case.headers, case.first)
    assert H.first_uncodable(case.headers, case.first) == case.extra["bad"]
    r = subprocess.run([tool, "code", write_fastq(tmp_path / "in.fastq", case.headers), case.first.decode("latin-1")], capture_output=True, text=True)
    assert r.returncode == 3, r.stdout[-400:] + r.stderr[-2000:]
    assert r.stdout.startswith("refused at %d: " % case.extra["bad"]), r.stdout


def test_windows_of_the_reference_are_slices_of_its_chunk():
    for case in H.by_kind("windows"):
        n = len(case.headers)
        rds = H.reads(n)
        L = H.restate(case.first, H.oracle_fields(case), rds, H.chunk_table(case.headers, rds)[1])
        bounds = [b for b in case.extra["bounds"] if b <= n]
        for a in bounds:
            for b in bounds:
                if a >= b:
                    continue
                w, recs = L.window(a, b)
                assert w == L.raw[L.starts[a]: L.starts[b]]
                assert recs == [(s - L.starts[a], q - L.starts[a], ln) for s, q, ln in L.recs[a:b]]
                fa, fa_recs = L.fasta(a, b)
                assert len(fa) == sum(len(h) + 2 + len(s) for h, (s, _) in zip(L.headers[a:b], rds[a:b]))


def test_damaged_streams_are_refused_by_the_host_coder_at_the_reference_record(tool, tmp_path):  # noqa: F811
    (case,) = H.by_kind("refusals")
    n = len(case.headers)
    rds = H.reads(n)
    fields = H.oracle_fields(case)
    total = H.chunk_table(case.headers, rds)[1]
    good = H.restate(case.first, fields, rds, total)
    seen = set()
    for name, damage, want in case.extra["damage"]:
        bad_fields, delta = damage(fields)
        assert (bad_fields != fields) != (delta != 0) or name.startswith("two-defects"), name
        try:
            L = H.restate(case.first, bad_fields, rds, total + delta)
            got = None
            assert L.raw[:total] == good.raw and not any(L.raw[total:]), name  # what is too long is ignored
        except H.Refused as e:
            got = e.record
        assert got == want, "%s: the case is named for the record the reference refuses" % name
        seen.add(want)
        if delta == 0:  # (the chunk's size is not the header coder's business)
            h = host_decode(tool, tmp_path / "streams.txt", case.first, n, bad_fields)
            assert h == (want if want is not None else good.headers), name
    assert seen == {None, 0, 255, 256, 300, 511, 768, 1023}


# ------------------------------------------------------------------------------------------- the reference's compiled code
@pytest.fixture(scope="module")
def ref_tables():
    raw, recs = O.load_fastq(os.path.join(R.ROOT, "tests", "golden", "SRR065390_sub_1.fastq"))
    return O.freq_tables(raw, recs)[2:]


@needs_ref
@pytest.mark.parametrize("case", CODED, ids=ids(CODED))
def test_reference_gives_the_oracles_streams_and_the_reference_layout(tmp_path, ref_tables, case):
    assert os.path.exists(REF), "oracle/_ref/ref_tool_asan is missing: run build() (make -C oracle) where the reference tree is"
    raw = R.fastq_of_headers(case.headers)
    e = R.encode(REF, raw, tmp_path, tables=ref_tables, first_header=case.first)
    fields = H.oracle_fields(case)
    assert e["first_header"] == case.first and len(e["fields"]) == len(fields)
    for i, (got, want) in enumerate(zip(e["fields"], fields)):
        for part, g, w in zip(("flags", "content", "lengths"), got, want):
            assert g.tobytes() == w, "header field %d, %s: the reference and the oracle differ" % (i, part)
    rds = H.reads(len(case.headers))
    decoded = HO.decode_headers(len(case.headers), case.first, [_streams(f) for f in fields])
    total = H.chunk_table(decoded, rds)[1]
    d = R.write_encoded(R.fresh_dir(tmp_path, "oracle_fields"), case.first, e["seq_ft"], e["qual_ft"], e,
                        [tuple(np.frombuffer(p, dtype=np.uint8) for p in f) for f in fields], total, len(case.headers))
    assert R.decode(REF, d).tobytes() == H.restate(case.first, fields, rds, total).raw


@needs_ref
def test_reference_refuses_the_uncodable_at_the_same_record(tmp_path, ref_tables):
    """the reference asserts without a record number: it codes the headers in front of the bad one and refuses as soon
    as the bad one is the last"""
    assert os.path.exists(REF), "oracle/_ref/ref_tool_asan is missing: run build() (make -C oracle) where the reference tree is"
    for case in UNCODABLE:
        at = case.extra["bad"]
        if at and "first-header" not in case.name:
            e = R.encode(REF, R.fastq_of_headers(case.headers[:at]), tmp_path, "before", tables=ref_tables, first_header=case.first)
            want = R.oracle_fields(case.headers[:at], case.first)[2]
            assert [tuple(p.tobytes() for p in f) for f in e["fields"]] == want, case.name
        with pytest.raises(R.Refused):
            R.encode(REF, R.fastq_of_headers(case.headers[: at + 1]), tmp_path, "with", tables=ref_tables, first_header=case.first)
