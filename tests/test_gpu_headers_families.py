"""The device header coder (fqcomp28_amd/csrc/headers.hip: k_hdr_count, k_hdr_layout, k_hdr_write) and the device header
decode and chunk layout (decode_headers.hip: k_chunk_agg, k_chunk_scan, k_chunk_measure, k_chunk_write, k_chunk_pick) at
the edges of their prefix sums: every case of tests/headers_ref.py's families goes through both directions and is
compared, byte for byte, with oracle/headers_oracle.py's streams and with `restate`'s layout.
tests/test_headers_families_host.py holds the same cases, the reference and the generator to the host coder and to the
reference's compiled code."""
import os

import numpy as np
import pytest

import headers_ref as H
import oracle_lib as O
import ref_pin as R

pytestmark = pytest.mark.gpu

E_CORRUPT, E_ARG, E_HEADER = -3, -4, -8
STREAMS = ("seq", "qual", "readlens", "n_count", "n_pos")

CODED = H.by_kind("ok", "windows", "refusals")
UNCODABLE = H.by_kind("uncodable")


def ids(cases):
    return [H.case_id(c) for c in cases]


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    assert F.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return F


@pytest.fixture(scope="module")
def ctx(F, golden_dir):
    raw, recs = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_1.fastq"))
    _, _, sft, qft = O.freq_tables(raw, recs)
    c = F.Context(sft, qft)
    yield c
    c.close()


def table(F, recs):
    from fqcomp28_amd.binding import REC_DTYPE
    t = np.zeros(len(recs), dtype=REC_DTYPE)
    a = np.array(recs, dtype=np.int64).reshape(len(recs), 3)
    t["seq_off"], t["qual_off"], t["len"] = a[:, 0], a[:, 1], a[:, 2]
    return t


def same_table(got, want):
    return all(np.array_equal(got[k], want[k]) for k in ("seq_off", "qual_off", "len"))


def assert_streams(g, fields):
    assert g["rc"] == 0 and g["headers_rc"] == 0, (g["rc"], g.get("headers_rc"), g.get("bad_record"))
    assert len(g["header_fields"]) == len(fields)
    for i, (got, want) in enumerate(zip(g["header_fields"], fields)):
        for part, x, w in zip(("flags", "content", "lengths"), got, want):
            assert x.size == len(w), (i, part, "size", x.size, len(w))
            assert x.tobytes() == w, (i, part, int(np.argmax(x != np.frombuffer(w, dtype=np.uint8))))


def coded(F, ctx, case, cache={}):
    """one case through the encoder, made once: the chunk, the reference layout, the device's streams"""
    key = H.case_id(case)
    if key not in cache:
        cache.clear()  # (one case at a time: the large ones are 14 MB)
        n = len(case.headers)
        rds = H.reads(n)
        raw = R.fastq_of_headers(case.headers)
        fields = H.oracle_fields(case)
        g = ctx.encode_raw(raw, header_format=H.fmt_of(case.first))
        total = H.chunk_table(H.HO.decode_headers(n, case.first, [_streams(f) for f in fields]), rds)[1]
        cache[key] = dict(raw=raw, reads=rds, fields=fields, g=g, L=H.restate(case.first, fields, rds, total), total=total)
    return cache[key]


def _streams(parts):
    s = H.HO.FieldStreams()
    s.flags, s.content, s.lengths = (bytearray(p) for p in parts)
    return s


def decode(ctx, case, g, fields, raw_len):
    return ctx.decode_chunk(H.fmt_of(case.first), fields, g["readlens"], g["seq"], g["qual"], g["n_count"], g["n_pos"], raw_len)


@pytest.mark.parametrize("case", CODED, ids=ids(CODED))
def test_encode_gives_the_oracles_streams(F, ctx, case):
    c = coded(F, ctx, case)
    assert_streams(c["g"], c["fields"])
    want_recs, used = H.chunk_table(case.headers, c["reads"])
    assert c["g"]["used_len"] == used == c["raw"].size and same_table(c["g"]["recs"], table(F, want_recs))
    # the caller's record table instead of the device parser's
    assert_streams(ctx.encode_raw(c["raw"], recs=table(F, want_recs), header_format=H.fmt_of(case.first)), c["fields"])
    plain = ctx.encode_raw(c["raw"])  # the block's own streams are what they are without the header coder
    assert plain["rc"] == 0
    for k in STREAMS:
        assert np.array_equal(c["g"][k], plain[k]), k


@pytest.mark.parametrize("case", CODED, ids=ids(CODED))
def test_decode_gives_the_reference_layout(F, ctx, case):
    c = coded(F, ctx, case)
    L, g = c["L"], c["g"]
    assert g["rc"] == 0 and g["headers_rc"] == 0
    want_recs = table(F, L.recs)
    for whose, fields in (("oracle", c["fields"]), ("device", g["header_fields"])):
        d = decode(ctx, case, g, fields, c["total"])
        assert d["rc"] == 0 and d["bad_record"] is None, (whose, d["rc"], d["bad_record"])
        assert d["laid_out_len"] == c["total"] == L.starts[-1], whose
        got = d["raw"].tobytes()
        assert got == L.raw, (whose, next(i for i in range(len(got)) if got[i] != L.raw[i]))
        assert same_table(d["recs"], want_recs), whose
    if case.extra.get("lossless", True):
        assert L.raw == c["raw"].tobytes()


@pytest.mark.parametrize("case", UNCODABLE, ids=ids(UNCODABLE))
def test_uncodable_headers_are_refused_with_their_record(F, ctx, case):
    with pytest.raises(ValueError):
        H.HO.encode_headers(case.headers, case.first)
    raw = R.fastq_of_headers(case.headers)
    for recs in (None, table(F, H.chunk_table(case.headers, H.reads(len(case.headers)))[0])):
        g = ctx.encode_raw(raw, recs=recs, header_format=H.fmt_of(case.first))
        assert g["rc"] == 0 and (g["headers_rc"], g.get("bad_record")) == (E_HEADER, case.extra["bad"]), (g["rc"], g.get("headers_rc"), g.get("bad_record"))


WINDOWS = H.by_kind("windows")


@pytest.mark.parametrize("case", WINDOWS, ids=ids(WINDOWS))
def test_windows_are_the_references_and_slices_of_the_whole_decode(F, ctx, case):
    n = len(case.headers)
    rds = H.reads(n)
    raw = R.fastq_of_headers(case.headers)
    fmt = H.fmt_of(case.first)
    fields = H.oracle_fields(case)
    g = ctx.encode_raw(raw, flags=F.F_DECODE_INDEX, header_format=fmt)
    assert_streams(g, fields)
    L = H.restate(case.first, fields, rds, raw.size)
    whole = decode(ctx, case, g, fields, raw.size)
    assert whole["rc"] == 0 and whole["raw"].tobytes() == L.raw == raw.tobytes()
    bounds = case.extra["bounds"]
    taken = refused = 0
    for a in bounds:
        for b in bounds:
            calls = [("range", lambda: ctx.decode_chunk_range(fmt, fields, g["readlens"], g["seq"], g["qual"], g["n_count"], g["n_pos"], raw.size, a, b)),
                     ("range+index", lambda: ctx.decode_chunk_range(fmt, fields, g["readlens"], g["seq"], g["qual"], g["n_count"], g["n_pos"], raw.size, a, b,
                                                                    index=g["index"])),
                     ("fasta", lambda: ctx.decode_chunk_fasta(fmt, fields, g["readlens"], g["seq"], g["n_count"], g["n_pos"], raw.size, a, b)),
                     ("fasta+index", lambda: ctx.decode_chunk_fasta(fmt, fields, g["readlens"], g["seq"], g["n_count"], g["n_pos"], raw.size, a, b,
                                                                    seq_index=g["index"][0]))]
            for what, call in calls:
                d = call()
                if a >= b or b > n:  # the documented refusal: first >= end, end > n_recs
                    assert d["rc"] == E_ARG and d["raw"] is None, (what, a, b, d["rc"])
                    refused += 1
                    continue
                want, want_recs = L.fasta(a, b) if what.startswith("fasta") else L.window(a, b)
                assert d["rc"] == 0 and d["bad_record"] is None and d["out_len"] == len(want), (what, a, b, d["rc"], d["out_len"], len(want))
                assert d["raw"].tobytes() == want, (what, a, b)
                assert same_table(d["recs"], table(F, want_recs)), (what, a, b)
                if what.startswith("range"):  # the same slice of decode_chunk's output
                    assert d["raw"].tobytes() == whole["raw"][L.starts[a]: L.starts[b]].tobytes(), (what, a, b)
                    off = L.starts[a]
                    assert np.array_equal(d["recs"]["seq_off"] + off, whole["recs"]["seq_off"][a:b])
                    assert np.array_equal(d["recs"]["qual_off"] + off, whole["recs"]["qual_off"][a:b])
                taken += 1
    ok = sum(1 for a in bounds for b in bounds if a < b <= n)
    assert taken == 4 * ok and refused == 4 * (len(bounds) ** 2 - ok) and ok >= 6


def test_damaged_streams_are_refused_at_the_references_record(F, ctx):
    (case,) = H.by_kind("refusals")
    c = coded(F, ctx, case)
    g, fields, total, rds = c["g"], c["fields"], c["total"], c["reads"]
    assert_streams(g, fields)
    fmt = H.fmt_of(case.first)
    for name, damage, _ in case.extra["damage"]:
        bad_fields, delta = damage(fields)
        try:
            want = H.restate(case.first, bad_fields, rds, total + delta)
        except H.Refused as e:
            want = e
        d = decode(ctx, case, g, bad_fields, total + delta)
        if isinstance(want, H.Refused):
            assert (d["rc"], d["bad_record"]) == (E_CORRUPT, want.record), (name, d["rc"], d["bad_record"])
            assert not d["raw"].any() and not d["recs"]["seq_off"].any(), name  # nothing written on a refusal
            for fa in (False, True):  # the range calls judge the whole chunk: same verdict
                if fa:
                    r = ctx.decode_chunk_fasta(fmt, bad_fields, g["readlens"], g["seq"], g["n_count"], g["n_pos"], total + delta, 1, 3)
                else:
                    r = ctx.decode_chunk_range(fmt, bad_fields, g["readlens"], g["seq"], g["qual"], g["n_count"], g["n_pos"], total + delta, 1, 3)
                assert (r["rc"], r["bad_record"]) == (E_CORRUPT, want.record), (name, fa, r["rc"], r["bad_record"])
        else:
            assert d["rc"] == 0 and d["bad_record"] is None and d["laid_out_len"] == total, (name, d["rc"], d["bad_record"])
            assert d["raw"].tobytes() == want.raw, name
        # the same handle restores a good chunk right afterwards
        d = decode(ctx, case, g, g["header_fields"], total)
        assert d["rc"] == 0 and d["raw"].tobytes() == c["L"].raw, name
