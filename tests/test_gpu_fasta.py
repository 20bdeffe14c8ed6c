"""Sequences alone, as FASTA (fqgpu_decode_chunk_fasta: the FastaForm instances of the layout kernels in
fqcomp28_amd/csrc/decode_headers.hip, the sequence-only launch of decode.hip), through the C ABI and the binding.
The expected FASTA is always made here from the input FASTQ -- b">" + header[1:] + b"\\n" + seq + b"\\n" per record --
never from the code under test; where the verdict matters it is compared with fqgpu_decode_chunk's for the same inputs."""
import os
import sys

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import fqc_archive as A  # noqa: E402
from test_gpu_decode_chunk import FIXTURES, damaged_cases, fmt_of  # noqa: E402
from test_gpu_decode_range import aligned, strides  # noqa: E402

pytestmark = pytest.mark.gpu

E_OVERFLOW, E_CORRUPT, E_ARG = -1, -3, -4
STRIDE = 64 << 10
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    assert F.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return F


def fasta_records(raw, recs):
    """the expected FASTA of a parsed FASTQ chunk, record by record"""
    b = raw.tobytes()
    return [b">" + h[1:] + b"\n" + b[int(r["seq_off"]): int(r["seq_off"]) + int(r["len"])] + b"\n"
            for h, r in zip(A.headers_of(raw, recs), recs)]


def parse_fasta(data):
    """[(seq_off, len)] of two-line FASTA records"""
    out, at = [], 0
    while at < len(data):
        assert data[at] == ord(">"), at
        s = data.index(b"\n", at) + 1
        e = data.index(b"\n", s)
        out.append((s, e - s))
        at = e + 1
    return out


def encode(F, ctx, raw, first, index):
    g = ctx.encode_raw(raw, flags=F.F_DECODE_INDEX if index else 0, header_format=fmt_of(first))
    assert g["rc"] == 0 and g["headers_rc"] == 0
    return g


def fasta(ctx, g, first, a, b, index=True, fields=None, seq=None, raw_len=None, n_count=None, seq_index=None, **kw):
    if seq_index is None and index and "index" in g:
        seq_index = g["index"][0]
    return ctx.decode_chunk_fasta(fmt_of(first), g["header_fields"] if fields is None else fields, g["readlens"],
                                  g["seq"] if seq is None else seq, g["n_count"] if n_count is None else n_count, g["n_pos"],
                                  g["used_len"] if raw_len is None else raw_len, a, b, seq_index=seq_index, **kw)


def fastq(ctx, g, first, index=True, fields=None, seq=None, raw_len=None, n_count=None):
    return ctx.decode_chunk(fmt_of(first), g["header_fields"] if fields is None else fields, g["readlens"],
                            g["seq"] if seq is None else seq, g["qual"], g["n_count"] if n_count is None else n_count, g["n_pos"],
                            g["used_len"] if raw_len is None else raw_len, index=g.get("index") if index else None)


def check(d, want_recs, a, b):
    want = b"".join(want_recs[a:b])
    assert d["rc"] == 0 and d["bad_record"] is None, (a, b, d["rc"], d["bad_record"])
    got = d["raw"].tobytes()
    assert d["out_len"] == len(want) and got == want, (a, b, d["out_len"], len(want))
    table = parse_fasta(got)
    assert [(int(r["seq_off"]), int(r["len"])) for r in d["recs"]] == table, (a, b)
    assert not d["recs"]["qual_off"].any()


def whole_chunk(F, ctx, raw, recs, first, index):
    """item 1: the whole chunk, the size query, the record table, and the FASTA of decode_chunk's own output"""
    g = encode(F, ctx, raw, first, index)
    want = fasta_records(raw, recs)
    n = len(recs)
    q = fasta(ctx, g, first, 0, n, index, out_cap=0)
    assert q["rc"] == 0 and q["raw"] is None and q["out_len"] == sum(len(x) for x in want)
    d = fasta(ctx, g, first, 0, n, index)
    check(d, want, 0, n)
    assert d["out_len"] == q["out_len"]
    w = fastq(ctx, g, first, index)
    assert w["rc"] == 0
    assert d["raw"].tobytes() == b"".join(fasta_records(w["raw"][:w["laid_out_len"]], w["recs"]))
    return g, want


# ---------------------------------------------------------------- 1. whole chunks
@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("index", [False, True])
def test_whole_chunk_golden_fixtures(F, golden_dir, name, index):
    raw, recs = O.load_fastq(os.path.join(golden_dir, name + ".fastq"))
    _, _, sft, qft = O.freq_tables(raw, recs)
    ctx = F.Context(sft, qft)
    try:
        ctx.set_index_stride(STRIDE)
        whole_chunk(F, ctx, raw, recs, A.headers_of(raw, recs[:1])[0], index)
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", [1, 2, 3, 4, 5, 6])
def test_whole_chunk_synth_32mib(F, mode):
    raw, _ = F.synth_fastq(32 << 20, mode, seed=140 + mode)
    recs = F.parse_fastq(raw)
    sft, qft = F.freq_tables(raw, recs)
    ctx = F.Context(sft, qft)
    try:
        ctx.set_index_stride(STRIDE)
        whole_chunk(F, ctx, raw, recs, A.headers_of(raw, recs[:1])[0], True)
    finally:
        ctx.close()


# ---------------------------------------------------------------- 2. ranges
@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("index", [False, True])
def test_ranges_golden_fixtures(F, golden_dir, name, index):
    raw, recs = O.load_fastq(os.path.join(golden_dir, name + ".fastq"))
    _, _, sft, qft = O.freq_tables(raw, recs)
    ctx = F.Context(sft, qft)
    try:
        ctx.set_index_stride(STRIDE)
        first = A.headers_of(raw, recs[:1])[0]
        g = encode(F, ctx, raw, first, index)
        want = fasta_records(raw, recs)
        n = len(recs)
        rng = np.random.default_rng(len(name) + 11 * index)
        ranges = [(0, 1), (n - 1, n), (0, n)] + [tuple(sorted(rng.choice(n + 1, 2, replace=False))) for _ in range(6)]
        for a, b in ranges:
            check(fasta(ctx, g, first, int(a), int(b), index), want, int(a), int(b))
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", [2, 4])
def test_ranges_on_stride_boundaries(F, mode):
    targets = [5 * STRIDE, 11 * STRIDE - 1, 17 * STRIDE + 1, 23 * STRIDE]
    raw, recs, hit = aligned(F, mode, 12 << 20, targets, seed=160 + mode)
    assert len(hit) >= 3
    sft, qft = F.freq_tables(raw, recs)
    ctx = F.Context(sft, qft)
    try:
        ctx.set_index_stride(STRIDE)
        first = A.headers_of(raw, recs[:1])[0]
        g = encode(F, ctx, raw, first, True)
        want = fasta_records(raw, recs)
        rs = np.concatenate([[0], np.cumsum(recs["len"].astype(np.int64))])
        n = len(recs)
        ranges = []
        for r in hit:
            assert rs[r] in targets  # the boundaries are really there
            ranges += [(r, r + 3), (r - 3, r), (r - 1, r + 1), (r, r + 1), (r - 1, r)]
        k = 30  # inside one stride
        lo = int(np.searchsorted(rs, k * STRIDE + 1000))
        assert rs[lo + 3] < (k + 1) * STRIDE
        ranges += [(lo, lo + 3), (lo + 1, lo + 2), (0, 1), (n - 1, n), (0, n), (n // 3, 2 * n // 3)]
        rng = np.random.default_rng(mode)
        ranges += [tuple(int(x) for x in sorted(rng.choice(n + 1, 2, replace=False))) for _ in range(6)]
        for a, b in ranges:
            check(fasta(ctx, g, first, a, b), want, a, b)
    finally:
        ctx.close()


# ---------------------------------------------------------------- 3. .. 5. on one block of many strides
@pytest.fixture(scope="module")
def block(F):
    raw, _ = F.synth_fastq(8 << 20, 4, seed=177)
    recs = F.parse_fastq(raw)
    sft, qft = F.freq_tables(raw, recs)
    ctx = F.Context(sft, qft)
    ctx.set_index_stride(STRIDE)
    first = A.headers_of(raw, recs[:1])[0]
    g = encode(F, ctx, raw, first, True)
    yield ctx, g, raw, recs, first, fasta_records(raw, recs)
    ctx.close()


def mid_stride_range(g, recs):
    """four records wholly inside the middle sequence stride"""
    stride, spans = strides(bytes(g["index"][0]), len(g["seq"]))
    k = len(spans) // 2
    rs = np.concatenate([[0], np.cumsum(recs["len"].astype(np.int64))])
    a = int(np.searchsorted(rs, k * stride + 1))
    assert rs[a + 4] < (k + 1) * stride
    return spans, k, a, a + 4


def garbage(seq, span, seed):
    """the stream with the inside of one stride's bit span overwritten"""
    lo, hi = (span[0] + 7) // 8 + 8, span[1] // 8 - 8
    assert hi - lo > 1000
    out = np.array(seq, dtype=np.uint8, copy=True)
    out[lo:hi] = np.random.default_rng(seed).integers(0, 256, hi - lo, dtype=np.uint8)
    return out


def test_only_the_strides_of_the_range_are_decoded(F, block):
    """with the sequence index and nothing else"""
    ctx, g, raw, recs, first, want = block
    spans, k, a, b = mid_stride_range(g, recs)
    assert k > 1 and k + 2 < len(spans)
    for other in (0, k - 1, k + 1, len(spans) - 1):  # strides wholly outside the range, the neighbours among them
        check(fasta(ctx, g, first, a, b, seq=garbage(g["seq"], spans[other], other)), want, a, b)
    bad = garbage(g["seq"], spans[k], k)
    d = fasta(ctx, g, first, a, b, seq=bad)
    assert d["rc"] == E_CORRUPT and d["bad_record"] is None
    check(fasta(ctx, g, first, a, b), want, a, b)  # the handle is still usable
    # without the index the whole stream is walked and the damage anywhere is seen
    assert fasta(ctx, g, first, a, b, index=False, seq=garbage(g["seq"], spans[0], 0))["rc"] != 0
    check(fasta(ctx, g, first, a, b, index=False), want, a, b)


def cut(data, where):
    """one byte less: the first, the middle one, the last"""
    data = bytes(data)
    at = {"start": 0, "middle": len(data) // 2, "end": len(data) - 1}[where]
    return data[:at] + data[at + 1:]


def layout_damage(fields, types):
    s = next(i for i, t in enumerate(types) if t == 1)
    n = next(i for i, t in enumerate(types) if t == 0)

    def with_field(i, k, val):
        out = [list(f) for f in fields]
        out[i][k] = val
        return [tuple(f) for f in out]

    for k, what in enumerate(("flags", "content", "lengths")):
        for where in ("start", "middle", "end"):
            yield "%s cut at the %s" % (what, where), with_field(s, k, cut(fields[s][k], where))
    yield "numeric content short", with_field(n, 1, fields[n][1][:-4])
    yield "numeric content one byte short", with_field(n, 1, fields[n][1][:-1])
    yield from damaged_cases(fields, types)


def test_same_verdict_as_the_fastq_decode(F, block):
    ctx, g, raw, recs, first, want = block
    types = fmt_of(first)[0]
    fields = [tuple(x.tobytes() for x in f) for f in g["header_fields"]]
    n = len(recs)
    total = sum(len(x) for x in want)
    cases = [(what, dict(fields=f)) for what, f in layout_damage(fields, types)]
    cases += [("raw_len one byte too small", dict(raw_len=g["used_len"] - 1)), ("raw_len far too small", dict(raw_len=10)),
              ("n_count short", dict(n_count=g["n_count"][: n - 1]))]
    refused = 0
    for what, kw in cases:
        w = fastq(ctx, g, first, **kw)
        for a, b in ((0, n), (n // 2, n // 2 + 9)):
            out = np.full(total + 64, SENTINEL, dtype=np.uint8)
            d = fasta(ctx, g, first, a, b, out=out, **kw)
            assert (d["rc"], d["bad_record"]) == (w["rc"], w["bad_record"]), (what, a, b, d["rc"], d["bad_record"], w["rc"], w["bad_record"])
            q = fasta(ctx, g, first, a, b, out_cap=0, **kw)  # the size query judges alike
            assert (q["rc"], q["bad_record"]) == (w["rc"], w["bad_record"]), what
            if w["rc"] != 0:
                assert (out == SENTINEL).all(), what
                refused += 1
            else:  # a layout the host decoder takes too: the same headers and reads as the FASTQ decode laid out
                assert out[:d["out_len"]].tobytes() == b"".join(fasta_records(w["raw"][:w["laid_out_len"]], w["recs"])[a:b]), what
                assert (out[d["out_len"]:] == SENTINEL).all()
    assert refused >= 2 * 8
    check(fasta(ctx, g, first, 0, n), want, 0, n)


def test_damaged_sequence_stream_is_judged_as_by_the_fastq_decode(F, block):
    ctx, g, raw, recs, first, want = block
    n = len(recs)
    rng = np.random.default_rng(64)
    seen = set()
    for i in range(64):
        seq = np.array(g["seq"], dtype=np.uint8, copy=True)
        seq[int(rng.integers(seq.size))] ^= int(rng.integers(1, 256))
        index = i % 2 == 0
        w = fastq(ctx, g, first, index, seq=seq)  # (its quality stream is good)
        d = fasta(ctx, g, first, 0, n, index, seq=seq)
        assert d["rc"] == w["rc"], (i, d["rc"], w["rc"])
        assert d["bad_record"] is None
        seen.add(d["rc"])
        if d["rc"] == 0:
            assert d["raw"].tobytes() == b"".join(fasta_records(w["raw"][:w["laid_out_len"]], w["recs"])), i
    assert seen - {0}, "no damage was seen at all"
    check(fasta(ctx, g, first, 0, n), want, 0, n)


def test_overflow_digest_and_refused_arguments(F, block):
    ctx, g, raw, recs, first, want = block
    n = len(recs)
    for a, b in [(10, 20), (0, 1), (n - 7, n), (0, n)]:
        size = sum(len(x) for x in want[a:b])
        out = np.full(size - 1, SENTINEL, dtype=np.uint8)
        d = fasta(ctx, g, first, a, b, out=out)
        assert d["rc"] == E_OVERFLOW and d["out_len"] == size and (out == SENTINEL).all()
        check(fasta(ctx, g, first, a, b, out_cap=size), want, a, b)
    # a FASTA piece is never digested -- not even the whole chunk, and not what a FASTQ decode left before it
    w = fastq(ctx, g, first)
    assert w["rc"] == 0 and ctx.chunk_crc32()[0] == 0
    for a, b in [(0, n), (3, 9)]:
        check(fasta(ctx, g, first, a, b), want, a, b)
        assert ctx.chunk_crc32() == (E_ARG, 0, 0)
    # the refusals of fqgpu_decode_chunk_range
    rng_of = lambda a, b: ctx.decode_chunk_range(fmt_of(first), g["header_fields"], g["readlens"], g["seq"], g["qual"], g["n_count"],  # noqa: E731
                                                 g["n_pos"], g["used_len"], a, b, index=g["index"])
    for a, b in [(5, 5), (6, 5), (0, n + 1), (n, n + 1)]:
        d = fasta(ctx, g, first, a, b)
        assert d["rc"] == E_ARG == rng_of(a, b)["rc"] and d["out_len"] == 0 and d["bad_record"] is None
    assert fasta(ctx, g, first, 0, n, seq=np.zeros(0, np.uint8))["rc"] == E_ARG
    many = b"@" + b":".join(b"%d" % k for k in range(65))
    d = ctx.decode_chunk_fasta(fmt_of(many), [(b"", b"\0" * 4 * n, b"")] * 65, g["readlens"], g["seq"], g["n_count"], g["n_pos"],
                               g["used_len"], 0, n)
    assert d["rc"] == E_ARG
    # a damaged sequence index: behind the layout's verdict, as in _range
    six = np.array(g["index"][0], dtype=np.uint8, copy=True)
    six[0] ^= 0xFF
    d = fasta(ctx, g, first, 0, 10, seq_index=six)
    r = ctx.decode_chunk_range(fmt_of(first), g["header_fields"], g["readlens"], g["seq"], g["qual"], g["n_count"], g["n_pos"],
                               g["used_len"], 0, 10, index=(six, g["index"][1]))
    assert d["rc"] == r["rc"] != 0
    check(fasta(ctx, g, first, 0, n), want, 0, n)
