"""Adapter clipping on the device (k_adapter_find and the judge's CLIP flag in fqcomp28_amd/csrc/select.hip, behind
fqgpu_chunk_clip / fqgpu_dblock_clip) against the numpy restatement in adapter_ref.py: the kept bytes, the report, the keep
bits and the windows, byte for byte.  Integer arithmetic: every comparison is exact.  With no trim and no filter a record's
window is (0, clip place), so the windows ARE the search's results."""
import ctypes as C
import os

import numpy as np
import pytest

import adapter_ref as AR
import filter_ref as FR
import oracle_lib as O
import test_adapter_host as AH
import test_gpu_stats as TS
import test_gpu_trim as TT
import trim_ref as R

pytestmark = pytest.mark.gpu

E_OVERFLOW, E_SHORT_READ, E_ARG = -1, -2, -4
TRUSEQ = AH.TRUSEQ
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
Q20 = TT.Q20


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


def chunk_with(hls, seqs, phreds=None, **kw):
    """test_gpu_trim.chunk_of with the sequence lines given: (raw, recs)"""
    phreds = [np.full(len(s), 30) for s in seqs] if phreds is None else phreds
    raw, recs = TT.chunk_of(hls, phreds, **kw)
    raw = raw.copy()
    for r, s in zip(recs, seqs):
        raw[int(r["seq_off"]):int(r["seq_off"]) + int(r["len"])] = np.frombuffer(bytes(s), dtype=np.uint8)
    return raw, recs


def same(ctx, raw, recs, a, t=None, f=None, what="", **kw):
    """the device's answer for the block (raw, recs) against the reference's -> (the device's, the reference's)"""
    want = AR.clip_records(raw, recs, a, t, f)
    b = ctx.dblock(raw, recs)
    try:
        g = b.clip(a, t, f, **kw)
    finally:
        b.close()
    TT.holds(g, want[:4], what)
    return g, want


# ---------------------------------------------------------------- 1. reads built by hand
def long_adapter_reads():
    """an adapter of 64 bases: whole in the middle of a read, its first 40 bases at a read's end, one substitution in six of
    sixty (10 percent: a hit), in seven of sixty (no hit)"""
    rng = np.random.default_rng(64)
    A = BASES[rng.integers(0, 4, 64)].tobytes()
    other = lambda c: b"A" if c != ord("A") else b"C"  # noqa: E731
    spoil = lambda s, k: b"".join(other(c) if i % 9 == 0 and i // 9 < k else bytes([c]) for i, c in enumerate(s))  # noqa: E731
    back = lambda n: BASES[rng.integers(0, 4, n)].tobytes()  # noqa: E731
    return A, [(back(70) + A + back(30), 70), (back(90) + A[:40], 90), (back(33) + spoil(A[:60], 6), 33), (back(33) + spoil(A[:60], 7), None)]


def test_reads_built_by_hand(F, ctx):
    """A read of fewer than three bases never reaches the device: every way to a block (fqgpu_dblock_create, the parser, the
    decode) refuses it with FQGPU_E_SHORT_READ, as the reference coder leaves it undefined.  The rows of one base are therefore
    checked to be refused there (the reference's answer for them is checked on the host, test_adapter_host.py), and rows of
    three bases, the shortest a block takes, stand beside them."""
    assert sum(len(row[0]) < 3 for row in AH.HAND) == 2 and sum(len(row[0]) == 3 for row in AH.HAND) >= 5
    for seq, A, mo, pct, clip in AH.HAND:     # a chunk of one read each
        for hl in (2, 9):
            raw, recs = chunk_with([hl], [seq])
            if len(seq) < 3:
                with pytest.raises(F.binding.FqgpuError) as refused:
                    ctx.dblock(raw, recs)
                assert refused.value.code == E_SHORT_READ
                continue
            g, want = same(ctx, raw, recs, AR.adp(A, mo, pct), what="%s %s %d %d" % (seq, A, mo, pct))
            assert want[4].tolist() == [clip] and g["win"].tolist() == [clip << 16 if clip else 0]
            assert int(g["report"][AR.READS_WITH_ADAPTER]) == (clip < len(seq)) and int(g["report"][AR.BASES_CUT_ADAPTER]) == len(seq) - clip
            assert int(g["report"][R.READS_EMPTIED]) == (clip == 0) == int(g["report"][R.DROPPED_SHORT])
    # ... and those with the TruSeq prefix in one chunk
    rows = [row for row in AH.HAND if row[1:4] == (TRUSEQ, 5, 10)]
    raw, recs = chunk_with(2 + np.arange(len(rows)) * 5 % 16, [row[0] for row in rows])
    g, want = same(ctx, raw, recs, AR.adp(TRUSEQ), what="the TruSeq rows")
    assert want[4].tolist() == [row[4] for row in rows]
    A, reads = long_adapter_reads()
    raw, recs = chunk_with([7, 3, 12, 5], [s for s, _ in reads])
    g, want = same(ctx, raw, recs, AR.adp(A, 20, 10), what="64 bases")
    assert want[4].tolist() == [len(s) if p is None else p for s, p in reads]
    g, want = same(ctx, raw, recs, AR.adp(A, 64, 0), what="64 bases, all of them, exactly")
    assert want[4].tolist() == [70] + [len(s) for s, _ in reads[1:]]
    for m in (1, 31, 32, 33, 63):     # around the adapter length at which the search takes its second register
        g, want = same(ctx, raw, recs, AR.adp(A[:m], min(m, 12), 10), what="%d bases" % m)
        assert want[4][0] <= 70 and want[4][1] <= 90


# ---------------------------------------------------------------- 2. the occurrence at every byte of a word, across words and requests
def placed_reads(L, seed):
    """reads of L random bases with ONE occurrence of the TruSeq prefix each, whole or running over the read's end, put so that
    in the line's 16-byte words -- `rel` counts bytes from the aligned word that holds the line's first byte -- it starts at
    every byte of the first two words, around the boundary between a lane's two words (rel 128), around the request boundary
    (rel 256, 512) and in the last words of the line; header lines of 2 .. 17 bytes (with the '\\n': 3 .. 18) put the line's first
    byte at every byte of a word -> (raw, recs, [(lead, rel)])"""
    rng = np.random.default_rng(seed)
    rels = sorted(set(range(0, 34)) | set(range(112, 132)) | set(range(240, 262)) | {500, 511, 512, 513} | set(range(L - 20, L + 15)))
    seqs, hls, plan, at = [], [], [], 0
    for rel in rels:
        for i in range(4):
            lead = (5 * i) % (rel + 1) if rel < 16 else (7 * rel + 5 * i) % 16     # (in front of byte `rel`, every lead in turn)
            p = rel - lead
            if 0 <= p <= L - 5:
                s = BASES[rng.integers(0, 4, L)].copy()
                k = min(len(TRUSEQ), L - p)
                s[p:p + k] = np.frombuffer(TRUSEQ[:k], dtype=np.uint8)
                seqs.append(s.tobytes())
                hls.append(TT.aligned_header(at, L, lead))
                plan.append((lead, rel))
                at += hls[-1] + 2 * L + 5
    raw, recs = chunk_with(hls, seqs)
    assert [(int(r["seq_off"]) & 15) for r in recs] == [lead for lead, _ in plan] and set(hls) <= set(range(2, 18))
    return raw, recs, plan


@pytest.mark.parametrize("L", [255, 256, 257, 600])
def test_an_occurrence_at_every_alignment(F, ctx, L):
    raw, recs, plan = placed_reads(L, L)
    g, want = same(ctx, raw, recs, AR.adp(TRUSEQ), what="placed in %d" % L)
    clip = want[4]
    found = np.array([lead + int(c) == rel for (lead, rel), c in zip(plan, clip)])
    assert found.mean() > 0.9, "the occurrence that was put there is the one found (a chance hit in front of it is rare)"
    met = {(lead, rel) for (lead, rel), ok in zip(plan, found) if ok}
    assert {lead for lead, _ in met} == set(range(16)), "the line starts at every byte of a word"
    assert {rel % 16 for _, rel in met} == set(range(16)) and {rel for _, rel in met if rel < 32} == set(range(32))
    for edge in (128, 256) + ((512,) if L > 512 else ()):      # a start just in front of the boundary straddles it
        assert {edge - 12, edge - 1, edge, edge + 1} <= {rel for _, rel in met}, edge
    partial = [(lead, rel) for lead, rel in met if rel - lead + len(TRUSEQ) > L]
    assert len(partial) >= 8, "occurrences that run over the read's end"
    same(ctx, raw, recs, AR.adp(TRUSEQ, 13, 0), R.trm(**Q20), FR.flt(max_n=0, min_len=30), what="placed in %d, whole ones only" % L)


def test_the_longest_read(F, ctx):
    L = 65535
    rng = np.random.default_rng(4)     # (a draw without a chance hit in front of the planted ones)
    seqs = []
    for p in (65500, 0, 65530, None, 65279, 256 * 100 - 7):
        s = BASES[rng.integers(0, 4, L)].copy()
        if p is not None:
            k = min(len(TRUSEQ), L - p)
            s[p:p + k] = np.frombuffer(TRUSEQ[:k], dtype=np.uint8)
        seqs.append(s.tobytes())
    seqs.insert(2, BASES[rng.integers(0, 4, 100)].tobytes())     # short reads among them, in the same rounds
    raw, recs = chunk_with([5, 2, 9, 16, 3, 11, 7], seqs)
    g, want = same(ctx, raw, recs, AR.adp(TRUSEQ), what="65535")
    assert want[4].tolist() == [65500, 0, 100, 65530, 65535, 65279, 25593]
    same(ctx, raw, recs, AR.adp(TRUSEQ), R.trm(cut_front=3, cut_tail=2, crop=65000), FR.flt(min_len=200), what="65535, cut")


# ---------------------------------------------------------------- 3. drawn reads with planted adapters
def planted(n, seed, lo=30, hi=300, plus_repeats=False, kinds=None):
    """n reads of lo .. hi bases with drawn qualities: a quarter with the whole adapter at a random place, a quarter with its
    first 5 .. 20 bases at the 3' end, one substitution in half of the planted ones, N at rate 0.01 -> (raw, recs, adapter)"""
    rng = np.random.default_rng(seed)
    A = BASES[np.random.default_rng(1000).integers(0, 4, 33)].tobytes()     # (one adapter for all chunks)
    lens = rng.integers(lo, hi + 1, n)
    seqs = []
    for r, L in enumerate(lens.tolist()):
        s = BASES[rng.integers(0, 4, L)].copy()
        kind = int(rng.integers(0, 4)) if kinds is None else kinds[r]
        if kind == 0:
            p = int(rng.integers(0, L))
            k = min(len(A), L - p)
        elif kind == 1:
            k = min(int(rng.integers(5, 21)), L)
            p = L - k
        if kind <= 1:
            s[p:p + k] = np.frombuffer(A[:k], dtype=np.uint8)
            if rng.random() < 0.5:
                at = p + int(rng.integers(0, k))
                s[at] = BASES[(int(np.flatnonzero(BASES == s[at])[0]) + 1 + int(rng.integers(0, 3))) % 4]
        s[rng.random(L) < 0.01] = ord("N")
        seqs.append(s.tobytes())
    raw, recs = chunk_with(rng.integers(2, 18, n), seqs, [TT.plateau(rng, int(L)) for L in lens], plus_repeats=plus_repeats)
    return raw, recs, AR.adp(A, 5, 10)


def clip_shares(want, recs, a):
    """of a reference result: the shares of reads clipped, clipped by an occurrence that runs over the read's end, left whole"""
    m = AR.fields(a)[1]
    L, clip = recs["len"].astype(np.int64), want[4]
    return (clip < L).mean() + 0.0, ((clip < L) & (clip + m > L)).mean() + 0.0, (clip == L).mean() + 0.0


@pytest.mark.parametrize("n", [63, 64, 65, 257, 1000])
def test_record_counts(F, ctx, n):
    raw, recs, a = planted(n, 100 + n)
    g, want = same(ctx, raw, recs, a, what="%d records" % n)
    clipped, partial, whole = clip_shares(want, recs, a)
    print("%d records: %.0f %% clipped, %.0f %% by a partial overlap, %.0f %% whole" % (n, 100 * clipped, 100 * partial, 100 * whole))
    assert clipped >= 0.20 and partial >= 0.05 and whole >= 0.20, "a degenerate draw"
    same(ctx, raw, recs, a, R.trm(**Q20), FR.flt(max_n=0), what="%d records, trimmed and filtered" % n)


def test_one_record(F, ctx):
    """a chunk of one read cannot hold the three kinds at once: one chunk for each"""
    seen = []
    for kind in (0, 1, 2):
        raw, recs, a = planted(1, 203 + kind, kinds=[kind])
        g, want = same(ctx, raw, recs, a, what="one record, kind %d" % kind)
        seen.append(clip_shares(want, recs, a))
        same(ctx, raw, recs, a, R.trm(**Q20), FR.flt(max_n=0), what="one record, kind %d, trimmed" % kind)
    assert seen == [(1.0, 0.0, 0.0), (1.0, 1.0, 0.0), (0.0, 0.0, 1.0)]


@pytest.fixture(scope="module")
def thousand():
    return planted(1000, 1100)


COMPOSITIONS = [(dict(cut_front=3), None), (dict(cut_tail=4), None), (dict(cut_front=2, cut_tail=60), dict(min_len=1)), (Q20, None),
                (dict(q_front=20), dict(min_mean_q=25)), (dict(q_tail=20, crop=70), dict(max_n=0)), (dict(crop=40), dict(min_len=40)),
                (dict(cut_front=1, cut_tail=2, q_front=20, q_tail=20, crop=120), dict(max_n=1, min_len=25, min_mean_q=22)),
                (dict(), dict(max_n=0, min_len=50, max_len=250, low_q=15, max_low_pct=20))]


def test_the_clip_in_front_of_every_step_of_the_trim_and_the_filter(F, ctx, thousand):
    raw, recs, a = thousand
    b = ctx.dblock(raw, recs)
    for t, f in COMPOSITIONS:
        t, f = R.trm(**t), None if f is None else FR.flt(**f)
        want = AR.clip_records(raw, recs, a, t, f)
        TT.holds(b.clip(a, t, f), want[:4], "%s %s" % (t, f))
        assert 0 < int(want[1][R.N_KEPT]) < len(recs) or f is None
        assert int(want[1][AR.READS_WITH_ADAPTER]) == int((want[4] < recs["len"]).sum()) > 200
    b.close()


# ---------------------------------------------------------------- 4. equivalences
def test_without_an_adapter_it_is_the_trim(F, ctx, thousand):
    raw, recs, _ = thousand
    b = ctx.dblock(raw, recs)
    for t, f in COMPOSITIONS:
        t, f = R.trm(**t), None if f is None else FR.flt(**f)
        g, want = b.clip(None, t, f), b.trim(t, f)
        assert g["rc"] == 0 == want["rc"] and g["out_len"] == want["out_len"] and g["out"].tobytes() == want["out"].tobytes()
        assert all(np.array_equal(g[k], want[k]) for k in ("report", "keep", "win")) and not g["report"][14:].any()
    assert b.clip(None, None, None)["rc"] == E_ARG, "as fqgpu_dblock_trim without a trim"
    b.close()


def test_an_adapter_that_cannot_hit_gives_the_trim(F, ctx):
    rng = np.random.default_rng(9)
    lens = rng.integers(3, 300, 300)
    raw, recs = chunk_with(rng.integers(2, 18, 300), [b"A" * int(L) for L in lens], [TT.plateau(rng, int(L)) for L in lens])
    a = AR.adp(b"CCCCC", 5, 0)
    b = ctx.dblock(raw, recs)
    for t, f in ((dict(), None), (Q20, None), (dict(cut_front=2, q_tail=25, crop=100), dict(min_len=20, max_n=0, min_mean_q=20))):
        t, f = R.trm(**t), None if f is None else FR.flt(**f)
        g, want = b.clip(a, t, f), b.trim(t, f)
        assert g["rc"] == 0 == want["rc"] and g["out"].tobytes() == want["out"].tobytes()
        assert all(np.array_equal(g[k], want[k]) for k in ("report", "keep", "win")) and not g["report"][14:].any()
        TT.holds(g, AR.clip_records(raw, recs, a, t, f)[:4])
    b.close()


def test_a_null_trim_and_a_null_filter(F, ctx, thousand):
    raw, recs, a = thousand
    b = ctx.dblock(raw, recs)
    none, every = R.trm(), FR.flt()
    first = b.clip(a, None, None)
    TT.holds(first, AR.clip_records(raw, recs, a)[:4], "NULL, NULL")
    for t, f in ((none, None), (None, every), (none, every)):
        g = b.clip(a, t, f)
        assert g["rc"] == 0 and g["out"].tobytes() == first["out"].tobytes() and all(np.array_equal(g[k], first[k]) for k in ("report", "keep", "win"))
    f = FR.flt(min_len=60, max_n=0)
    TT.holds(b.clip(a, None, f), AR.clip_records(raw, recs, a, None, f)[:4], "NULL trim, a filter")
    b.close()


# ---------------------------------------------------------------- 5. arguments
def raw_call(F, ctx, b, a, t, f, out, cap, keep=None, win=None):
    n = C.c_size_t(77)
    report = np.full(R.REPORT_WORDS, 7, dtype=np.uint64)
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = F.binding.lib().fqgpu_dblock_clip(ctx.h, b.h if b is not None else None, p(a), p(t), p(f), p(out), cap, C.byref(n), p(report), p(keep), p(win))
    return rc, n.value, report


def test_size_query_and_a_buffer_one_byte_short(F, ctx, thousand):
    raw, recs, a = thousand
    t, f = R.trm(q_tail=20), FR.flt(min_len=20)
    want = AR.clip_records(raw, recs, a, t, f)
    assert 0 < want[0].size < raw.size
    b = ctx.dblock(raw, recs)
    before = b.crc32()
    keep = np.full((len(recs) + 7) // 8, 0xAA, dtype=np.uint8)
    win = np.full(len(recs), 0xAAAAAAAA, dtype=np.uint32)
    rc, n, report = raw_call(F, ctx, b, a, t, f, None, 0, keep, win)
    assert rc == 0 and n == want[0].size and report.tolist() == want[1].tolist(), "the size query"
    assert keep.tolist() == want[2].tolist() and win.tolist() == want[3].tolist()
    out = np.full(want[0].size + 32, 0x5A, dtype=np.uint8)
    rc, n, report = raw_call(F, ctx, b, a, t, f, out, want[0].size - 1)
    assert rc == E_OVERFLOW and n == want[0].size and report.tolist() == want[1].tolist() and (out == 0x5A).all(), "nothing is written"
    rc, n, report = raw_call(F, ctx, b, a, t, f, out, want[0].size)
    assert rc == 0 and n == want[0].size and out[:n].tobytes() == want[0].tobytes() and (out[n:] == 0x5A).all(), "exactly *out_len bytes"
    for bad in AH.BAD:      # an adapter, a trim, a filter its check refuses; a NULL where data is expected
        rc, n, report = raw_call(F, ctx, b, AR.adp(**bad), t, f, out, out.size)
        assert rc == E_ARG and n == 0 and not report.any(), bad
    for bt, bf in ((R.trm(crop=0), f), (t, FR.flt(min_mean_q=64))):
        rc, n, report = raw_call(F, ctx, b, a, bt, bf, out, out.size)
        assert rc == E_ARG and n == 0 and not report.any()
    rc, n, report = raw_call(F, ctx, None, a, t, f, out, out.size)
    assert rc == E_ARG and n == 0 and not report.any()
    assert (out[want[0].size:] == 0x5A).all()
    assert b.crc32() == before and np.array_equal(b.fetch_raw(), raw), "the chunk is left as it is"
    TT.holds(b.trim(t, f), R.trim_records(raw, recs, t, f), "a trim call behind the clip calls")
    TT.holds(b.clip(a, t, f), want[:4], "and a clip call behind that")
    b.close()


@pytest.mark.parametrize("byte", [ord("a"), ord("X"), 0xC1, 0])
@pytest.mark.parametrize("where", ["clipped", "kept"])
def test_a_byte_that_is_no_base_refuses_the_chunk(F, ctx, thousand, byte, where):
    """the sequence line is read because an adapter is given, and judged over all its bytes, the clipped ones too"""
    raw, recs, a = thousand
    clip = AR.clip_records(raw, recs, a)[4]
    r = int(np.flatnonzero((clip < recs["len"] - 2) & (clip > 2))[7])
    raw = raw.copy()
    raw[int(recs["seq_off"][r]) + (int(recs["len"][r]) - 1 if where == "clipped" else 1)] = byte
    b = ctx.dblock(raw, recs)
    out = np.full(raw.size, 0x5A, dtype=np.uint8)
    keep = np.full((len(recs) + 7) // 8, 0xAA, dtype=np.uint8)
    win = np.full(len(recs), 0xAAAAAAAA, dtype=np.uint32)
    for o in (None, out):
        rc, n, report = raw_call(F, ctx, b, a, None, None, o, out.size, keep, win)
        assert rc == E_ARG and n == 0 and not report.any() and not keep.any() and not win.any()
    assert (out == 0x5A).all()
    with pytest.raises(AR.Refused):
        AR.clip_records(raw, recs, a)
    TT.holds(b.trim(R.trm(crop=50)), R.trim_records(raw, recs, R.trm(crop=50)), "without an adapter the line is not read")
    b.close()


def test_text_behind_the_plus(F, ctx):
    raw, recs, a = planted(500, 77, plus_repeats=True)
    for t, f in ((None, None), (R.trm(**Q20), FR.flt(min_len=30, max_n=0))):
        g, want = same(ctx, raw, recs, a, t, f, what="'+' lines that repeat the header")
        assert 0 < int(want[1][AR.READS_WITH_ADAPTER]) < len(recs)
    b = ctx.dblock(raw)   # with the device parser's record table
    TT.holds(b.clip(a, R.trm(**Q20)), AR.clip_chunk(raw, a, R.trm(**Q20))[:4], "parsed on the device")
    b.close()


def test_the_chunk_on_the_staging_block_after_a_decode(F, golden_dir):
    raw, recs = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_1.fastq"))
    a, t, f = AR.adp(TRUSEQ), R.trm(q_tail=20), FR.flt(min_len=25)
    table = recs.astype(R.REC_DTYPE)
    want = AR.clip_records(raw, table, a, t, f)
    print("SRR065390_sub_1, the TruSeq prefix: found in %d of %d reads, %d bases" % (int(want[1][14]), len(recs), int(want[1][15])))
    c = TS.context_for(F, raw, recs)
    fmt = TS.fmt_of(TS.first_header_of(raw))
    g = c.encode_raw(raw, flags=F.F_DECODE_INDEX, header_format=fmt)
    assert g["rc"] == 0 and g["headers_rc"] == 0
    TT.holds(c.chunk_clip(a, len(recs), t, f), want[:4], "behind fqgpu_encode_end")
    args = (fmt, g["header_fields"], g["readlens"], g["seq"], g["qual"], g["n_count"], g["n_pos"], g["used_len"])
    d = c.decode_chunk(*args, index=g["index"])
    assert d["rc"] == 0 and np.array_equal(d["raw"], raw)
    crc = c.chunk_crc32()
    TT.holds(c.chunk_clip(a, len(recs), t, f), want[:4], "decoded")
    TT.holds(c.chunk_clip(a, len(recs)), AR.clip_records(raw, table, a)[:4], "decoded, the clip alone")
    TT.holds(c.chunk_clip(None, len(recs), t, f), R.trim_records(raw, table, t, f), "decoded, no adapter")
    assert c.chunk_crc32() == crc
    c.set_check_only(True)
    d = c.decode_chunk(*args, want_raw=False, index=g["index"])
    assert d["rc"] == 0 and d["raw"] is None
    TT.holds(c.chunk_clip(a, len(recs), t, f), want[:4], "check-only")
    c.set_check_only(False)
    assert c.decode_chunk_range(*args, 3, 40, index=g["index"])["rc"] == 0
    assert c.chunk_clip(a, len(recs), t, f)["rc"] == E_ARG and c.chunk_trim(t, len(recs), f)["rc"] == E_ARG, "refused where the trim is"
    c.enable_timing(True)
    b = c.dblock(raw, recs)
    assert b.clip(a, t, f, query=True)["rc"] == 0
    _, groups = c.last_timing()
    assert [(name, calls) for name, _, calls in groups if name in ("clip", "trim", "filter")] == [("clip", 1)], groups
    b.close()
    c.close()
