"""The tail trims on the device (k_tail_find and the judge's SEL_TAIL mode in fqcomp28_amd/csrc/select.hip, behind
fqgpu_chunk_tailtrim / fqgpu_dblock_tailtrim) against the numpy restatement in tail_ref.py: the kept bytes, all 24 report
words, the keep bits, the windows and the places a0, a1, e, e2, for equality.  Integer arithmetic: there is no tolerance."""
import ctypes as C
import os

import numpy as np
import pytest

import adapter_ref as AR
import filter_ref as FR
import oracle_lib as O
import tail_ref as TR
import test_gpu_adapter as TA
import test_gpu_stats as TS
import test_gpu_trim as TT
import test_tail_host as HT
import trim_ref as R

pytestmark = pytest.mark.gpu

E_OVERFLOW, E_ARG = -1, -4
TRUSEQ = HT.TRUSEQ
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
NOT_G = np.frombuffer(b"ACT", dtype=np.uint8)
G, W4 = HT.G, HT.W4
BOTH = TR.tl("G", window_len=4, window_q=20)


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


def holds(g, want, what=""):
    TT.holds(g, want[:4], what)
    if not np.array_equal(g["places"], want[4]):
        at = int(np.flatnonzero((g["places"] != want[4]).any(axis=1))[0])
        raise AssertionError("%s: the places differ, first at record %d: %s, expected %s" % (what, at, g["places"][at].tolist(), want[4][at].tolist()))


def same(ctx, raw, recs, a, x, t=None, f=None, what="", **kw):
    """the device's answer for the block (raw, recs) against the reference's -> (the device's, the reference's)"""
    want = TR.tail_records(raw, recs, a, x, t, f)
    b = ctx.dblock(raw, recs)
    try:
        g = b.tailtrim(a, x, t, f, **kw)
    finally:
        b.close()
    holds(g, want, what)
    return g, want


# ---------------------------------------------------------------- 1. reads built by hand
def test_the_poly_reads_built_by_hand(F, ctx):
    for what, seq, x, a1 in HT.POLY_HAND:       # a chunk of one read each
        for hl in (2, 9):
            raw, recs = TA.chunk_with([hl], [seq])
            g, want = same(ctx, raw, recs, None, x, what=what)
            assert g["places"].tolist() == [[len(seq), a1, a1, a1]], what
            assert [int(v) for v in g["report"][16:]] == [a1 < len(seq), len(seq) - a1, 0, 0, 0, 0, 0, 0], what
    rows = [row for row in HT.POLY_HAND if row[2] is G]     # ... and those of one tail in one chunk
    raw, recs = TA.chunk_with(2 + np.arange(len(rows)) * 5 % 16, [row[1] for row in rows])
    g, want = same(ctx, raw, recs, None, G, what="the rows with the defaults")
    assert g["places"][:, 1].tolist() == [row[3] for row in rows]
    for c in b"ACGT":                           # poly-X: the longest of four
        other = b"A" if c != ord("A") else b"C"
        seq = other * 5 + HT.tail_of(bytes([c]) * 7, other, bytes([c]) * 9)
        raw, recs = TA.chunk_with([5], [seq])
        assert same(ctx, raw, recs, None, TR.tl("ACGT"))[0]["places"].tolist() == [[22, 5, 5, 5]]
        assert same(ctx, raw, recs, None, TR.tl("ACGT".replace(chr(c), "")))[0]["places"].tolist() == [[22, 22, 22, 22]]
    # a0 = 0: the read starts with the adapter; and a tail in front of an adapter
    seq = b"ACTACTAC" + b"G" * 12 + TRUSEQ + b"GGGGGGGGGGGG"
    raw, recs = TA.chunk_with([4, 7], [seq, TRUSEQ + b"GG"])
    g, want = same(ctx, raw, recs, AR.adp(TRUSEQ), G, what="behind the clip")
    assert g["places"].tolist() == [[20, 8, 8, 8], [0, 0, 0, 0]] and [int(v) for v in g["report"][14:20]] == [2, 40, 1, 12, 0, 0]


def test_the_window_reads_built_by_hand(F, ctx):
    for phred, cuts, W, Q, e2 in HT.WINDOW_HAND:
        for hl in (2, 9):
            raw, recs = TT.chunk_of([hl], [np.array(phred)])
            g, want = same(ctx, raw, recs, None, TR.tl(window_len=W, window_q=Q), R.trm(**cuts), what="%s %s %d:%d" % (phred, cuts, W, Q))
            assert g["places"][0, 3] == e2 and int(g["report"][TR.BASES_CUT_WINDOW]) == int(g["places"][0, 2]) - e2
    raw, recs = TT.chunk_of(2 + np.arange(len(HT.WINDOW_HAND)) * 7 % 16, [np.array(row[0]) for row in HT.WINDOW_HAND])
    same(ctx, raw, recs, None, W4, R.trm(cut_front=1, cut_tail=1, q_front=20, q_tail=20), what="the rows in one chunk")


# ---------------------------------------------------------------- 2. a tail end and a window hit at every alignment
def placed_reads(L, seed):
    """reads of L bases without G but for a tail of G at the 3' end whose inner end -- and a quality drop whose first byte --
    falls on bytes around the word, lane and request boundaries of the line; header lines that put the sequence line's first
    byte at every byte of a 16-byte word (the quality line's then as well) -> (raw, recs, leads)"""
    rng = np.random.default_rng(seed)
    ends = [e for e in sorted(set(range(0, 20)) | set(range(124, 133)) | set(range(250, 260)) | {511, 512, 513, L - 17, L - 16, L - 10}) if 0 <= e <= L - 10]
    seqs, phreds, hls, leads, at = [], [], [], [], 0
    for n, end in enumerate(ends):
        for i in range(16):
            lead = (5 * i + n) % 16                               # (every end at every lead)
            s = NOT_G[rng.integers(0, 3, L)].copy()
            s[end:] = ord("G")                                   # a1 = end
            errs = end + 9 + 9 * np.arange((L - end) // 9)      # mismatches the rule allows: one per nine bases, five at the most
            s[errs[(errs < L - 8)][-5:]] = ord("A") if i % 2 else ord("N")
            q = 30 + rng.integers(0, 8, L)
            drop = (end * 7 + 3 * i) % max(end, 1)               # the drop: in front of the tail, two low bytes, good ones around
            q[drop:drop + 2] = 2
            seqs.append(s.tobytes())
            phreds.append(q)
            hls.append(TT.aligned_header(at, L, lead))
            leads.append(lead)
            at += hls[-1] + 2 * L + 5
    raw, recs = TA.chunk_with(hls, seqs, phreds)
    assert [(int(r["seq_off"]) & 15) for r in recs] == leads
    return raw, recs, np.array(leads)


@pytest.mark.parametrize("L", [255, 256, 257, 600])
def test_a_tail_end_and_a_window_hit_at_every_alignment(F, ctx, L):
    raw, recs, leads = placed_reads(L, L)
    g, want = same(ctx, raw, recs, None, G, what="poly alone, %d" % L)
    a1 = want[4][:, 1].astype(np.int64)
    assert (a1 < L).mean() > 0.9 and set(leads[a1 < L].tolist()) == set(range(16))
    assert {int(v) % 16 for v in leads + a1} == set(range(16)), "the tail's inner end at every byte of a word"
    assert {127, 128, 129, 255, 256, 257} <= {int(v) for v in leads + a1}, "around the boundary of a lane's two words and of two requests"
    g, want = same(ctx, raw, recs, None, W4, what="window alone, %d" % L)
    e2 = want[4][:, 3].astype(np.int64)
    assert (e2 < L).mean() > 0.8 and set(leads[e2 < L].tolist()) == set(range(16))
    qlead = recs["qual_off"].astype(np.int64) & 15
    assert {int(v) % 16 for v in qlead + e2} == set(range(16)) and set(qlead.tolist()) == set(range(16))
    same(ctx, raw, recs, AR.adp(TRUSEQ), BOTH, R.trm(cut_front=2, q_tail=25), FR.flt(min_len=20, max_n=0), what="both, %d" % L)
    same(ctx, raw, recs, None, TR.tl("ACGT", 8, 9, 3, 17, 30), what="poly-X and 17:30, %d" % L)


def test_the_longest_read(F, ctx):
    L = 65535
    rng = np.random.default_rng(11)
    seqs, phreds = [], []
    for tail, errs, drop in ((0, 0, 65400), (30000, 4, 20000), (L, 0, None), (2000, 5, 300), (40, 1, 65300), (12, 0, None)):
        s = NOT_G[rng.integers(0, 3, L)].copy()
        s[L - tail:] = ord("G")
        if errs:
            s[L - 1 - 8 * (1 + np.arange(errs)) * max(tail // 64, 1)] = ord("T")
        q = 30 + rng.integers(0, 8, L)
        if drop is not None:
            q[drop:drop + 3] = 3
        seqs.append(s.tobytes())
        phreds.append(q)
    seqs.insert(2, NOT_G[rng.integers(0, 3, 90)].tobytes() + b"G" * 10)     # short reads among them, in the same rounds
    phreds.insert(2, np.full(100, 30))
    raw, recs = TA.chunk_with([5, 2, 9, 16, 3, 11, 7], seqs, phreds)
    g, want = same(ctx, raw, recs, None, TR.tl("G", 10, 8, 255, 4, 20), what="65535")
    assert want[4][:, 1].tolist() == [L, L - 30000, 90, 0, L - 2000, L - 40, L - 12]
    assert want[4][:, 3].tolist() == [65400, 20000, 90, 0, 300, 65300, L - 12]
    same(ctx, raw, recs, None, TR.tl("ACGT", 10, 8, 255, 32, 29), R.trm(cut_front=3, cut_tail=2, q_tail=20, crop=65000), FR.flt(min_len=200), what="65535, cut")


# ---------------------------------------------------------------- 3. drawn reads with planted tails, drops and adapters
ADAPTER = BASES[np.random.default_rng(1000).integers(0, 4, 33)].tobytes()


def planted(n, seed, lo=30, hi=300, plus_repeats=False):
    """n reads of lo .. hi bases (one in forty up to 700): a third end in a G tail of 5 .. 60 bases with one base in twenty
    wrong, a quarter carry the adapter (whole somewhere, or its first bases at the end), a quarter of those a G tail in front of
    it; N at rate 0.01; qualities a plateau with low ends, half of the reads with a drop of 1 .. 8 low bases inside, the G
    tails with high qualities -> (raw, recs)"""
    rng = np.random.default_rng(seed)
    lens = np.where(rng.random(n) < 0.025, rng.integers(300, 701, n), rng.integers(lo, hi + 1, n))
    seqs, phreds = [], []
    for L in lens.tolist():
        s = BASES[rng.integers(0, 4, L)].copy()
        q = TT.plateau(rng, L)
        end = L
        if rng.random() < 0.25:
            end = int(rng.integers(0, L))
            k = min(len(ADAPTER), L - end) if rng.random() < 0.5 else min(int(rng.integers(5, 21)), L - end)
            end = L - k if k < len(ADAPTER) else end
            s[end:end + k] = np.frombuffer(ADAPTER[:k], dtype=np.uint8)
        if rng.random() < (0.25 if end < L else 0.33):
            k = min(int(rng.integers(5, 61)), end)
            tail = np.full(k, ord("G"), dtype=np.uint8)
            wrong = rng.random(k) < 0.05
            tail[wrong] = BASES[rng.integers(0, 4, int(wrong.sum()))]
            s[end - k:end] = tail
            q[end - k:end] = 36
        if rng.random() < 0.5:
            at = int(rng.integers(0, L))
            q[at:at + int(rng.integers(1, 9))] = rng.integers(0, 10)
        s[rng.random(L) < 0.01] = ord("N")
        seqs.append(s.tobytes())
        phreds.append(q)
    return TA.chunk_with(rng.integers(2, 18, n), seqs, phreds, plus_repeats=plus_repeats)


def shares(want):
    """of a reference result: the shares of reads with a poly tail, with a window cut"""
    p = want[4].astype(np.int64)
    return (p[:, 1] < p[:, 0]).mean() + 0.0, (p[:, 3] < p[:, 2]).mean() + 0.0


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_record_counts(F, ctx, n):
    raw, recs = planted(n, 300 + n)
    a = AR.adp(ADAPTER, 5, 10)
    g, want = same(ctx, raw, recs, None, BOTH, what="%d records" % n)
    if n >= 63:
        poly, window = shares(want)
        print("%d records: %.0f %% with a poly tail, %.0f %% cut by the window" % (n, 100 * poly, 100 * window))
        assert poly >= 0.08 and window >= 0.2, "a degenerate draw"
    same(ctx, raw, recs, a, BOTH, R.trm(**TT.Q20), FR.flt(max_n=0), what="%d records, clipped, trimmed and filtered" % n)


@pytest.fixture(scope="module")
def thousand():
    return planted(1000, 1300)


@pytest.mark.parametrize("W", [1, 4, 16, 17, 32])
def test_window_lengths(F, ctx, thousand, W):
    """the bytes of a window come from one, two and three words"""
    raw, recs = thousand
    b = ctx.dblock(raw, recs)
    for Q in (15, 25):
        for t in (None, R.trm(cut_front=4, cut_tail=3)):
            x = TR.tl(window_len=W, window_q=Q)
            want = TR.tail_records(raw, recs, None, x, t)
            holds(b.tailtrim(None, x, t), want, "%d:%d %s" % (W, Q, t))
            assert 50 < int(want[1][TR.READS_WINDOW_CUT]) < len(recs)
    b.close()


COMPOSITIONS = [(dict(), None), (dict(cut_front=3), None), (dict(cut_tail=4), None), (dict(cut_front=2, cut_tail=60), dict(min_len=1)), (TT.Q20, None),
                (dict(q_front=20), dict(min_mean_q=25)), (dict(q_tail=20, crop=70), dict(max_n=0)), (dict(crop=40), dict(min_len=40)),
                (dict(cut_front=1, cut_tail=2, q_front=20, q_tail=20, crop=120), dict(max_n=1, min_len=25, max_len=200, min_mean_q=22, low_q=15, max_low_pct=20))]


def test_everything_at_once(F, ctx, thousand):
    """adapter + poly + window + both running-sum walks + crop + every filter criterion"""
    raw, recs = thousand
    a = AR.adp(ADAPTER, 5, 10)
    b = ctx.dblock(raw, recs)
    for x in (BOTH, TR.tl("ACGT", 6, 4, 9, 7, 18)):
        for adapter in (a, None):
            for t, f in COMPOSITIONS:
                t, f = R.trm(**t), None if f is None else FR.flt(**f)
                want = TR.tail_records(raw, recs, adapter, x, t, f)
                holds(b.tailtrim(adapter, x, t, f), want, "%s %s %s %s" % (x, adapter is not None, t, f))
                assert 0 < int(want[1][R.N_KEPT]) < len(recs) or f is None
                assert int(want[1][TR.READS_WITH_POLY]) > 100 and int(want[1][TR.READS_WINDOW_CUT]) > 100
                assert (int(want[1][AR.READS_WITH_ADAPTER]) > 100) == (adapter is not None)
    b.close()


# ---------------------------------------------------------------- 4. equivalences
def test_without_a_tail_it_is_the_clip(F, ctx, thousand):
    raw, recs = thousand
    a = AR.adp(ADAPTER, 5, 10)
    b = ctx.dblock(raw, recs)
    for x in (None, TR.tl(), TR.tl(poly_max_mism=7)):
        for adapter in (a, None):
            for t, f in COMPOSITIONS[3:]:
                t, f = R.trm(**t), None if f is None else FR.flt(**f)
                want = b.clip(adapter, t, f)
                for places in (True, False):
                    g = b.tailtrim(adapter, x, t, f, want_places=places)
                    assert g["rc"] == 0 == want["rc"] and g["out_len"] == want["out_len"] and g["out"].tobytes() == want["out"].tobytes()
                    assert g["report"][:16].tolist() == want["report"].tolist() and not g["report"][16:].any()
                    assert np.array_equal(g["keep"], want["keep"]) and np.array_equal(g["win"], want["win"])
                holds(b.tailtrim(adapter, x, t, f), TR.tail_records(raw, recs, adapter, x, t, f), "off")
        g, want = b.tailtrim(a, x, None, None), b.clip(a, None, None)
        assert g["rc"] == 0 and g["out"].tobytes() == want["out"].tobytes() and g["report"][:16].tolist() == want["report"].tolist()
        assert b.tailtrim(None, x, None, None)["rc"] == E_ARG == b.clip(None, None, None)["rc"], "a NULL adapter follows the clip's rules"
    g = b.tailtrim(None, BOTH, None, None)
    holds(g, TR.tail_records(raw, recs, None, BOTH), "a tail alone: NULL adapter, trim and filter")
    b.close()


# ---------------------------------------------------------------- 5. arguments
def raw_call(F, ctx, b, a, x, t, f, out, cap, keep=None, win=None, places=None):
    n = C.c_size_t(77)
    report = np.full(TR.REPORT_WORDS, 7, dtype=np.uint64)
    p = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = F.binding.lib().fqgpu_dblock_tailtrim(ctx.h, b.h if b is not None else None, p(a), p(x), p(t), p(f), p(out), cap, C.byref(n), p(report),
                                               p(keep), p(win), p(places))
    return rc, n.value, report


def test_size_query_and_a_buffer_one_byte_short(F, ctx, thousand):
    raw, recs = thousand
    a, t, f = AR.adp(ADAPTER, 5, 10), R.trm(q_tail=20), FR.flt(min_len=20)
    want = TR.tail_records(raw, recs, a, BOTH, t, f)
    assert 0 < want[0].size < raw.size
    b = ctx.dblock(raw, recs)
    before = b.crc32()
    keep = np.full((len(recs) + 7) // 8, 0xAA, dtype=np.uint8)
    win = np.full(len(recs), 0xAAAAAAAA, dtype=np.uint32)
    places = np.full((len(recs), 4), 0xAAAA, dtype=np.uint16)
    rc, n, report = raw_call(F, ctx, b, a, BOTH, t, f, None, 0, keep, win, places)
    assert rc == 0 and n == want[0].size and report.tolist() == want[1].tolist(), "the size query"
    assert keep.tolist() == want[2].tolist() and win.tolist() == want[3].tolist() and places.tolist() == want[4].tolist()
    out = np.full(want[0].size + 32, 0x5A, dtype=np.uint8)
    rc, n, report = raw_call(F, ctx, b, a, BOTH, t, f, out, want[0].size - 1)
    assert rc == E_OVERFLOW and n == want[0].size and report.tolist() == want[1].tolist() and (out == 0x5A).all(), "nothing is written"
    rc, n, report = raw_call(F, ctx, b, a, BOTH, t, f, out, want[0].size)
    assert rc == 0 and n == want[0].size and out[:n].tobytes() == want[0].tobytes() and (out[n:] == 0x5A).all(), "exactly *out_len bytes"
    for bad in HT.BAD:      # a tail, an adapter, a trim, a filter its check refuses; a NULL where data is expected
        rc, n, report = raw_call(F, ctx, b, a, TR.tl(**bad), t, f, out, out.size)
        assert rc == E_ARG and n == 0 and not report.any(), bad
    for ba, bt, bf in ((AR.adp(b"ACGT", 5), t, f), (a, R.trm(crop=0), f), (a, t, FR.flt(min_mean_q=64))):
        rc, n, report = raw_call(F, ctx, b, ba, BOTH, bt, bf, out, out.size)
        assert rc == E_ARG and n == 0 and not report.any()
    rc, n, report = raw_call(F, ctx, None, a, BOTH, t, f, out, out.size)
    assert rc == E_ARG and n == 0 and not report.any()
    assert (out[want[0].size:] == 0x5A).all()
    assert b.crc32() == before and np.array_equal(b.fetch_raw(), raw), "the chunk is left as it is"
    TT.holds(b.clip(a, t, f), AR.clip_records(raw, recs, a, t, f)[:4], "a clip call behind the tail calls")
    holds(b.tailtrim(a, BOTH, t, f), want, "and a tail call behind that")
    b.close()


@pytest.mark.parametrize("byte", [ord("a"), ord("X"), 0xC1, 0])
@pytest.mark.parametrize("where", ["cut", "kept"])
def test_a_byte_that_is_no_base_refuses_the_chunk_when_only_poly_reads_the_line(F, ctx, thousand, byte, where):
    raw, recs = thousand
    a1 = TR.tail_records(raw, recs, None, G)[4][:, 1].astype(np.int64)
    r = int(np.flatnonzero((a1 < recs["len"] - 2) & (a1 > 2))[7])
    raw = raw.copy()
    raw[int(recs["seq_off"][r]) + (int(recs["len"][r]) - 1 if where == "cut" else 1)] = byte
    b = ctx.dblock(raw, recs)
    out = np.full(raw.size, 0x5A, dtype=np.uint8)
    keep = np.full((len(recs) + 7) // 8, 0xAA, dtype=np.uint8)
    win = np.full(len(recs), 0xAAAAAAAA, dtype=np.uint32)
    places = np.full((len(recs), 4), 0xAAAA, dtype=np.uint16)
    for o in (None, out):
        rc, n, report = raw_call(F, ctx, b, None, G, None, None, o, out.size, keep, win, places)
        assert rc == E_ARG and n == 0 and not report.any() and not keep.any() and not win.any() and not places.any()
    assert (out == 0x5A).all()
    with pytest.raises(TR.Refused):
        TR.tail_records(raw, recs, None, G)
    holds(b.tailtrim(None, W4, R.trm(crop=50)), TR.tail_records(raw, recs, None, W4, R.trm(crop=50)), "the window alone does not read the line")
    b.close()


@pytest.mark.parametrize("byte", [32, 97, 0xC1])
def test_a_quality_byte_outside_refuses_the_chunk_when_only_the_window_reads_the_line(F, ctx, thousand, byte):
    raw, recs = thousand
    e2 = TR.tail_records(raw, recs, None, W4)[4][:, 3].astype(np.int64)
    r = int(np.flatnonzero((e2 < recs["len"] - 2) & (e2 > 2))[5])
    for at in (1, int(recs["len"][r]) - 1):      # a kept byte, a cut one
        spoilt = raw.copy()
        spoilt[int(recs["qual_off"][r]) + at] = byte
        b = ctx.dblock(spoilt, recs)
        places = np.full((len(recs), 4), 0xAAAA, dtype=np.uint16)
        rc, n, report = raw_call(F, ctx, b, None, W4, None, None, None, 0, None, None, places)
        assert rc == E_ARG and n == 0 and not report.any() and not places.any()
        with pytest.raises(TR.Refused):
            TR.tail_records(spoilt, recs, None, W4)
        holds(b.tailtrim(None, G, R.trm(crop=50)), TR.tail_records(spoilt, recs, None, G, R.trm(crop=50)), "the poly rule alone does not read the line")
        b.close()


def test_text_behind_the_plus(F, ctx):
    raw, recs = planted(500, 77, plus_repeats=True)
    a = AR.adp(ADAPTER, 5, 10)
    for adapter, t, f in ((None, None, None), (a, R.trm(**TT.Q20), FR.flt(min_len=30, max_n=0))):
        g, want = same(ctx, raw, recs, adapter, BOTH, t, f, what="'+' lines that repeat the header")
        assert 0 < int(want[1][TR.READS_WITH_POLY]) < len(recs) and 0 < int(want[1][TR.READS_WINDOW_CUT]) < len(recs)
    b = ctx.dblock(raw)   # with the device parser's record table
    holds(b.tailtrim(a, BOTH, R.trm(**TT.Q20)), TR.tail_chunk(raw, a, BOTH, R.trm(**TT.Q20)), "parsed on the device")
    b.close()


def test_the_chunk_on_the_staging_block_after_a_decode(F, golden_dir):
    raw, recs = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_1.fastq"))
    a, x, t, f = AR.adp(TRUSEQ), TR.tl("ACGT", 8, 8, 5, 4, 15), R.trm(q_tail=20), FR.flt(min_len=25)
    table = recs.astype(R.REC_DTYPE)
    want = TR.tail_records(raw, table, a, x, t, f)
    print("SRR065390_sub_1: %d of %d reads with a poly-X tail, %d cut by the window 4:15" % (int(want[1][16]), len(recs), int(want[1][18])))
    c = TS.context_for(F, raw, recs)
    fmt = TS.fmt_of(TS.first_header_of(raw))
    g = c.encode_raw(raw, flags=F.F_DECODE_INDEX, header_format=fmt)
    assert g["rc"] == 0 and g["headers_rc"] == 0
    holds(c.chunk_tailtrim(len(recs), a, x, t, f), want, "behind fqgpu_encode_end")
    args = (fmt, g["header_fields"], g["readlens"], g["seq"], g["qual"], g["n_count"], g["n_pos"], g["used_len"])
    d = c.decode_chunk(*args, index=g["index"])
    assert d["rc"] == 0 and np.array_equal(d["raw"], raw)
    crc = c.chunk_crc32()
    holds(c.chunk_tailtrim(len(recs), a, x, t, f), want, "decoded")
    holds(c.chunk_tailtrim(len(recs), None, x), TR.tail_records(raw, table, None, x), "decoded, the tail alone")
    g2 = c.chunk_tailtrim(len(recs), a, None, t, f)
    TT.holds(dict(g2, report=g2["report"][:16]), AR.clip_records(raw, table, a, t, f)[:4], "decoded, no tail")
    assert c.chunk_crc32() == crc
    c.set_check_only(True)
    d = c.decode_chunk(*args, want_raw=False, index=g["index"])
    assert d["rc"] == 0 and d["raw"] is None
    holds(c.chunk_tailtrim(len(recs), a, x, t, f), want, "check-only")
    c.set_check_only(False)
    assert c.decode_chunk_range(*args, 3, 40, index=g["index"])["rc"] == 0
    assert c.chunk_tailtrim(len(recs), a, x, t, f)["rc"] == E_ARG and c.chunk_clip(a, len(recs), t, f)["rc"] == E_ARG, "refused where the clip is"
    c.enable_timing(True)
    b = c.dblock(raw, recs)
    assert b.tailtrim(a, x, t, f, query=True)["rc"] == 0
    _, groups = c.last_timing()
    assert [(name, calls) for name, _, calls in groups if name in ("tailtrim", "clip", "trim", "filter")] == [("tailtrim", 1)], groups
    b.close()
    c.close()
