"""Records [first, end) of a chunk (fqgpu_decode_chunk_range, the windowed N pass of fqcomp28_amd/csrc/decode.hip and the
WINDOW pass of decode_headers.hip) and of an archive (fqc_tool d --records A:B): byte-equal to the input's records and to the matching
slice of decode_chunk, with only the strides that hold the range decoded when both decode indexes are there."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import fqc_archive as A  # noqa: E402
import headers_oracle as HO  # noqa: E402
from test_gpu_decode_chunk import FIXTURES, fmt_of  # noqa: E402

pytestmark = pytest.mark.gpu

E_OVERFLOW, E_CORRUPT, E_ARG = -1, -3, -4
STRIDE = 64 << 10
IX_HEAD = 32


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    assert F.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return F


def starts(recs, used):
    """byte offset of every record's header line, and the end of the last record"""
    s = np.zeros(len(recs) + 1, dtype=np.int64)
    s[1:] = recs["qual_off"].astype(np.int64) + recs["len"] + 1
    s[-1] = used
    return s


def expect(raw, recs, a, b):
    s = starts(recs, int(recs[-1]["qual_off"]) + int(recs[-1]["len"]) + 1)
    return raw[s[a]: s[b]].tobytes()


def encode(F, ctx, raw, first, index):
    g = ctx.encode_raw(raw, flags=F.F_DECODE_INDEX if index else 0, header_format=fmt_of(first))
    assert g["rc"] == 0 and g["headers_rc"] == 0
    return g


def rng_decode(ctx, g, first, a, b, index=True, fields=None, seq=None, qual=None, out_cap=None):
    return ctx.decode_chunk_range(fmt_of(first), g["header_fields"] if fields is None else fields, g["readlens"],
                                  g["seq"] if seq is None else seq, g["qual"] if qual is None else qual, g["n_count"], g["n_pos"],
                                  g["used_len"], a, b, index=g.get("index") if index else None, out_cap=out_cap)


def check(d, raw, recs, a, b, whole=None):
    assert d["rc"] == 0, (a, b, d["rc"], d["bad_record"])
    want = expect(raw, recs, a, b)
    got = d["raw"].tobytes()
    assert d["out_len"] == len(want) and got == want, (a, b, d["out_len"], len(want))
    if whole is not None:  # the same slice of decode_chunk's output
        assert got == whole[len(expect(raw, recs, 0, a)):][:len(got)]
    assert np.array_equal(d["recs"], O.parse_fastq(np.frombuffer(got, dtype=np.uint8))), (a, b)


def strides(index, stream_len):
    """bit spans [lo, hi) of every stride of a decode index"""
    stride, n_snap = struct.unpack_from("<II", index, 8)
    sb = (len(index) - IX_HEAD) // n_snap
    pos = [0] + [struct.unpack_from("<Q", index, IX_HEAD + j * sb)[0] for j in range(n_snap)] + [8 * stream_len]
    return stride, list(zip(pos[:-1], pos[1:]))


# ---------------------------------------------------------------- golden fixtures
@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("index", [False, True])
def test_golden_ranges(F, golden_dir, name, index):
    raw, recs = O.load_fastq(os.path.join(golden_dir, name + ".fastq"))
    _, _, sft, qft = O.freq_tables(raw, recs)
    ctx = F.Context(sft, qft)
    try:
        ctx.set_index_stride(STRIDE)
        first = A.headers_of(raw, recs[:1])[0]
        g = encode(F, ctx, raw, first, index)
        n = len(recs)
        rng = np.random.default_rng(len(name) + 7 * index)
        ranges = [(0, 1), (n - 1, n), (0, n)] + [tuple(sorted(rng.choice(n + 1, 2, replace=False))) for _ in range(6)]
        for a, b in ranges:
            check(rng_decode(ctx, g, first, int(a), int(b), index), raw, recs, int(a), int(b))
    finally:
        ctx.close()


# ---------------------------------------------------------------- many strides
def records(raw, recs):
    s = starts(recs, raw.size)
    b = raw.tobytes()
    return [(b[s[i]: int(r["seq_off"]) - 1], b[int(r["seq_off"]): int(r["seq_off"]) + int(r["len"])],
             b[int(r["qual_off"]): int(r["qual_off"]) + int(r["len"])]) for i, r in enumerate(recs)]


def aligned(F, mode, size, targets, seed):
    """synthetic reads, one read cut short in front of every target symbol so that a record starts exactly there"""
    raw, _ = F.synth_fastq(size, mode, seed=seed)
    reads = records(raw, F.parse_fastq(raw))
    hit = []
    for p in targets:
        at = 0
        for i, (_, s, _) in enumerate(reads):
            if at + len(s) > p:
                break
            at += len(s)
        if p - at >= 3:
            h, s, q = reads[i]
            reads[i] = (h, s[: p - at], q[: p - at])
            hit.append(i + 1)
        elif p == at:
            hit.append(i)
    out = np.frombuffer(b"".join(h + b"\n" + s + b"\n+\n" + q + b"\n" for h, s, q in reads), dtype=np.uint8)
    return out, F.parse_fastq(out), hit


@pytest.mark.parametrize("mode", [2, 4])
def test_many_strides_boundaries(F, mode):
    targets = [5 * STRIDE, 11 * STRIDE - 1, 17 * STRIDE + 1, 23 * STRIDE]
    raw, recs, hit = aligned(F, mode, 12 << 20, targets, seed=60 + mode)
    assert len(hit) >= 3
    sft, qft = F.freq_tables(raw, recs)
    ctx = F.Context(sft, qft)
    try:
        ctx.set_index_stride(STRIDE)
        first = A.headers_of(raw, recs[:1])[0]
        g = encode(F, ctx, raw, first, True)
        si, qi = g["index"]
        assert struct.unpack_from("<II", bytes(si), 8)[1] > 24  # dozens of strides
        whole = ctx.decode_chunk(fmt_of(first), g["header_fields"], g["readlens"], g["seq"], g["qual"], g["n_count"],
                                 g["n_pos"], g["used_len"], index=g["index"])
        assert whole["rc"] == 0
        whole = whole["raw"].tobytes()
        rs = np.concatenate([[0], np.cumsum(recs["len"].astype(np.int64))])
        n = len(recs)
        ranges = []
        for r in hit:
            ranges += [(r, r + 3), (r - 3, r), (r - 1, r + 1), (r, r + 1), (r - 1, r)]
        k = 30  # inside one stride
        lo = int(np.searchsorted(rs, k * STRIDE + 1000))
        assert rs[lo + 3] < (k + 1) * STRIDE
        ranges += [(lo, lo + 3), (lo + 1, lo + 2)]
        ranges += [(0, 1), (n - 1, n), (0, n), (n // 3, 2 * n // 3)]
        for a, b in ranges:
            check(rng_decode(ctx, g, first, a, b), raw, recs, a, b, whole)
        for r in hit:  # the boundaries are really there
            assert rs[r] in targets
    finally:
        ctx.close()


# ---------------------------------------------------------------- oracle-written streams
def test_oracle_written_streams(F, golden_dir):
    raw, recs = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_1.fastq"))
    _, _, sft, qft = O.freq_tables(raw, recs)
    e = O.OracleCtx(sft, qft).encode(raw, recs)
    first = A.headers_of(raw, recs[:1])[0]
    _, _, streams = HO.encode_headers(A.headers_of(raw, recs), first)
    fields = [(bytes(s.flags), bytes(s.content), bytes(s.lengths)) for s in streams]
    ctx = F.Context(sft, qft)
    try:
        n = len(recs)
        for a, b in [(0, 1), (n - 1, n), (0, n), (123, 456)]:
            d = ctx.decode_chunk_range(fmt_of(first), fields, recs["len"].astype(np.uint16), e["seq"], e["qual"], e["n_count"],
                                       e["n_pos"], raw.size, a, b)
            check(d, raw, recs, a, b)
    finally:
        ctx.close()


# ---------------------------------------------------------------- locality, size query, refusals
@pytest.fixture(scope="module")
def block(F):
    raw, _ = F.synth_fastq(8 << 20, 4, seed=77)
    recs = F.parse_fastq(raw)
    sft, qft = F.freq_tables(raw, recs)
    ctx = F.Context(sft, qft)
    ctx.set_index_stride(STRIDE)
    first = A.headers_of(raw, recs[:1])[0]
    g = encode(F, ctx, raw, first, True)
    yield ctx, g, raw, recs, first
    ctx.close()


def mid_stride_range(g, recs):
    """four records wholly inside the middle stride"""
    stride, spans = strides(bytes(g["index"][1]), len(g["qual"]))
    k = len(spans) // 2
    rs = np.concatenate([[0], np.cumsum(recs["len"].astype(np.int64))])
    a = int(np.searchsorted(rs, k * stride + 1))
    assert rs[a + 4] < (k + 1) * stride
    return spans, k, a, a + 4


def test_locality_damage_outside_the_range_goes_unseen(F, block):
    ctx, g, raw, recs, first = block
    spans, k, a, b = mid_stride_range(g, recs)
    assert k > 1
    lo, hi = spans[0]  # quality stride 0: far in front of the range
    qual = np.array(g["qual"], dtype=np.uint8, copy=True)
    qual[(lo + hi) // 16] ^= 0x5A
    check(rng_decode(ctx, g, first, a, b, qual=qual), raw, recs, a, b)
    d = ctx.decode_chunk(fmt_of(first), g["header_fields"], g["readlens"], g["seq"], qual, g["n_count"], g["n_pos"],
                         g["used_len"], index=g["index"])
    assert d["rc"] == E_CORRUPT or d["raw"].tobytes()[:raw.size] != raw.tobytes()


def test_damage_inside_a_decoded_stride_is_corrupt(F, block):
    ctx, g, raw, recs, first = block
    spans, k, a, b = mid_stride_range(g, recs)
    lo, hi = spans[k]
    qual = np.array(g["qual"], dtype=np.uint8, copy=True)
    qual[(lo + hi) // 16] ^= 0x5A
    assert rng_decode(ctx, g, first, a, b, qual=qual)["rc"] == E_CORRUPT
    check(rng_decode(ctx, g, first, a, b), raw, recs, a, b)  # the handle is still usable


def test_size_query_and_capacity(F, block):
    ctx, g, raw, recs, first = block
    for a, b in [(10, 20), (0, 1), (len(recs) - 7, len(recs))]:
        q = rng_decode(ctx, g, first, a, b, out_cap=0)
        assert q["rc"] == 0 and q["raw"] is None and q["out_len"] == len(expect(raw, recs, a, b))
        short = rng_decode(ctx, g, first, a, b, out_cap=q["out_len"] - 1)
        assert short["rc"] == E_OVERFLOW and short["out_len"] == q["out_len"]
        assert not short["raw"].any()  # no byte written
        check(rng_decode(ctx, g, first, a, b, out_cap=q["out_len"]), raw, recs, a, b)


def test_refusals(F, block):
    ctx, g, raw, recs, first = block
    n = len(recs)
    assert rng_decode(ctx, g, first, 5, 5)["rc"] == E_ARG
    assert rng_decode(ctx, g, first, 6, 5)["rc"] == E_ARG
    assert rng_decode(ctx, g, first, 0, n + 1)["rc"] == E_ARG
    # a header stream cut short behind the range: the layout is judged over the whole chunk
    types = fmt_of(first)[0]
    s = next(i for i, t in enumerate(types) if t == 1)
    fields = [tuple(bytes(x) for x in f) for f in g["header_fields"]]
    fields[s] = (fields[s][0][: n - 100],) + fields[s][1:]
    whole = ctx.decode_chunk(fmt_of(first), fields, g["readlens"], g["seq"], g["qual"], g["n_count"], g["n_pos"],
                             g["used_len"], index=g["index"])
    assert whole["rc"] == E_CORRUPT and whole["bad_record"] == n - 100
    for out_cap in (None, 0):
        d = rng_decode(ctx, g, first, 0, 10, fields=fields, out_cap=out_cap)
        assert (d["rc"], d["bad_record"]) == (whole["rc"], whole["bad_record"])
    check(rng_decode(ctx, g, first, 0, 10), raw, recs, 0, 10)


# ---------------------------------------------------------------- fqc_tool d --records
@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("range") / "fqc_tool")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-o", exe, os.path.join(ROOT, "tools", "fqc_tool.cpp"),
                    "-L" + os.path.join(ROOT, "fqcomp28_amd"), "-lfqgpu", "-Wl,-rpath," + os.path.join(ROOT, "fqcomp28_amd"),
                    "-lpthread"], check=True)
    return exe


def run(tool, *args):
    return subprocess.run([tool] + [str(x) for x in args], capture_output=True, text=True, timeout=600)


def restore_ranges(tool, tmp_path, arc, raw, recs, counts, ranges):
    import json
    edges = np.concatenate([[0], np.cumsum(counts)])
    for a, b in ranges:
        out = tmp_path / "r.fastq"
        r = run(tool, "d", arc, out, "-t", 3, "--records", "%d:%s" % (a, "" if b is None else b))
        assert r.returncode == 0, r.stderr
        b = len(recs) if b is None else b
        rep = json.loads(r.stdout.strip().splitlines()[-1])
        got = open(out, "rb").read()
        assert got == expect(raw, recs, a, b), (a, b)
        assert rep["records"] == b - a and rep["raw_bytes"] == len(got)
        overlap = sum(1 for k in range(len(counts)) if edges[k] < b and edges[k + 1] > a)
        assert sum(rep["blocks_per_worker"]) == overlap, (a, b)
        os.remove(out)


def farm_ranges(counts, n):
    e = np.concatenate([[0], np.cumsum(counts)]).astype(int)
    assert len(counts) >= 5
    return [(0, 1), (n - 1, n), (e[2] + 10, e[2] + 50), (e[1] + 7, e[4] - 9), (e[3], e[4]), (0, None)]


@pytest.fixture(scope="module")
def farm_input(F, tmp_path_factory):
    d = tmp_path_factory.mktemp("range_farm")
    raw, _ = F.synth_fastq(40 << 20, 4, seed=9)
    fq = d / "in.fastq"
    raw.tofile(fq)
    return d, fq, raw, F.parse_fastq(raw)


@pytest.mark.parametrize("extra", [[], ["--accumulate-n"]])
def test_farm_records(F, tool, farm_input, tmp_path, extra):
    _, fq, raw, recs = farm_input
    arc = tmp_path / "a.fqc"
    r = run(tool, "c", fq, arc, "-t", 4, "-R", 4, "-S", 4, "--index", "--index-stride", 64, *extra)
    assert r.returncode == 0, r.stderr
    counts = [b.n_records for b in A.read_archive(str(arc))[3]]
    ranges = farm_ranges(counts, len(recs))
    restore_ranges(tool, tmp_path, arc, raw, recs, counts, ranges)
    full = tmp_path / "full.fastq"
    assert run(tool, "d", arc, full, "-t", 3).returncode == 0
    assert open(full, "rb").read() == raw.tobytes()
    if not extra:  # without the sidecar: whole streams
        os.remove(str(arc) + ".fqx")
        restore_ranges(tool, tmp_path, arc, raw, recs, counts, ranges)


def test_farm_records_oracle_written_archive(F, tool, tmp_path):
    from test_archive import oracle_archive
    raw, _ = F.synth_fastq(9 << 20, 4, seed=5)
    recs = F.parse_fastq(raw)
    arc = tmp_path / "o.fqc"
    parts, _, _, _ = oracle_archive(F, str(arc), raw, recs, 7, order=[4, 1, 6, 0, 3, 5, 2])
    counts = [len(p[1]) for p in parts]
    restore_ranges(tool, tmp_path, arc, raw, recs, counts, farm_ranges(counts, len(recs)))


def test_farm_bad_ranges(F, tool, farm_input, tmp_path):
    d, fq, raw, recs = farm_input
    arc = tmp_path / "b.fqc"
    assert run(tool, "c", fq, arc, "-t", 2, "-R", 8, "-S", 4).returncode == 0
    for spec in ["5:3", "4:4", "0:%d" % (len(recs) + 1), "%d:" % len(recs), "x:y", "7", "-1:5"]:
        out = tmp_path / "bad.fastq"
        r = run(tool, "d", arc, out, "--records", spec)
        assert r.returncode != 0, spec
        assert "records" in r.stderr, (spec, r.stderr)
        assert not os.path.exists(out) and not os.path.exists(str(out) + ".part"), spec
