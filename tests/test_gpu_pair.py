"""The paired calls on the device (k_select_mark and the judge's range in fqcomp28_amd/csrc/select.hip, k_pair_names in pair.hip, behind
fqgpu_*_select_marked and fqgpu_*_pair_names) against the numpy restatement in pair_ref.py: the kept bytes, all 24 report
words, the final keep bits, the windows and the places of a record range under a mark, and the first pair whose read ids
differ, for equality.  Integer arithmetic: there is no tolerance."""
import ctypes as C
import os

import numpy as np
import pytest

import adapter_ref as AR
import filter_ref as FR
import oracle_lib as O
import pair_ref as PR
import tail_ref as TR
import test_gpu_stats as TS
import test_gpu_tail as TG
import test_tail_host as HT
import trim_ref as R

pytestmark = pytest.mark.gpu

E_ARG = -4
TRUSEQ = HT.TRUSEQ
Q20 = FR.flt(min_mean_q=20)
# an adapter, poly-G, a window, a trim and a filter together
FULL = dict(a=AR.adp(TRUSEQ), x=TR.tl("G", window_len=4, window_q=20), t=R.trm(cut_front=1, q_tail=20), f=FR.flt(min_len=30, max_n=1, min_mean_q=18))


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    if F.device_count() < 1:
        pytest.fail("no GPU visible: the product path has no CPU fallback")
    return F


@pytest.fixture(scope="module")
def golden(golden_dir):
    return [O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_%d.fastq" % m)) for m in (1, 2)]


@pytest.fixture(scope="module")
def ctx(F, golden):
    c = TS.context_for(F, *golden[0])
    yield c
    c.close()


@pytest.fixture(scope="module")
def mode4(F):
    """about 300 records of 50 .. 300 bases, N at one base in a hundred"""
    raw, n = F.synth_fastq(116000, 4, seed=41)
    raw = raw[:].copy()
    recs = F.parse_fastq(raw)
    assert 280 <= len(recs) == n <= 330 and len(set(recs["len"].tolist())) > 100
    return raw, recs


def with_plus_text(raw, recs):
    """the same records with the header line's text behind every '+' -> (raw, recs)"""
    raw = np.asarray(raw, dtype=np.uint8)
    lines, seq, qual = PR.header_lines(raw, recs), recs["seq_off"].astype(np.int64), recs["qual_off"].astype(np.int64)
    parts, table, at = [], np.zeros(len(recs), dtype=R.REC_DTYPE), 0
    for r, head in enumerate(lines):
        L = int(recs["len"][r])
        plus = b"+" + head[1:]
        table[r] = (at + len(head), at + len(head) + L + 1 + len(plus), L)
        parts += [head, raw[seq[r]:seq[r] + L].tobytes(), b"\n", plus, raw[qual[r]:qual[r] + L].tobytes(), b"\n"]
        at += len(head) + 2 * L + 2 + len(plus)
    return np.frombuffer(b"".join(parts), dtype=np.uint8), table


def opts(o):
    return dict(adapter=o.get("a"), tail=o.get("x"), trim=o.get("t"), flt=o.get("f"))


def counted(report):
    assert int(report[0]) == int(report[1]) + int(report[5:10].sum()) + int(report[PR.DROPPED_UNMARKED]), "n_records = n_kept + the drops + dropped_unmarked"
    assert not report[21:].any()


def same(b, raw, recs, first, end, mark=None, what="", **o):
    """the device's answer for the range against the reference's -> (the device's, the reference's)"""
    want = PR.marked_records(raw, recs, first, end, mark, o.get("a"), o.get("x"), o.get("t"), o.get("f"))
    g = b.select_marked(first, end, mark, **opts(o))
    TG.holds(g, want, "%s [%d, %d)" % (what, first, end))
    counted(g["report"])
    return g, want


# ---------------------------------------------------------------- 1. the whole range without a mark is the tail call
@pytest.mark.parametrize("o", [FULL, dict(f=Q20)], ids=["everything", "a filter alone"])
def test_the_whole_range_without_a_mark_is_the_tail_call(F, ctx, golden, o):
    raw, recs = golden[0]
    b = ctx.dblock(raw, recs)
    g = b.select_marked(0, len(recs), None, **opts(o))
    # (the tail call refuses four NULLs: a trim that cuts nothing stands for "no trim" there)
    w = b.tailtrim(o.get("a"), o.get("x"), o.get("t", R.trm()), o.get("f"))
    assert g["rc"] == 0 == w["rc"] and 0 < g["out_len"] == w["out_len"] < raw.size and g["out"].tobytes() == w["out"].tobytes()
    assert g["report"][:20].tolist() == w["report"][:20].tolist() and not g["report"][20:].any()
    assert np.array_equal(g["keep"], w["keep"]) and np.array_equal(g["win"], w["win"]) and np.array_equal(g["places"], w["places"])
    q = b.select_marked(0, len(recs), None, query=True, **opts(o))
    assert q["rc"] == 0 and q["out_len"] == g["out_len"] and q["report"].tolist() == g["report"].tolist() and np.array_equal(q["keep"], g["keep"])
    if "a" not in o:
        assert g["out"].tobytes() == b.filter(o["f"])["out"].tobytes()
    b.close()


# ---------------------------------------------------------------- 2. ranges
def ranges(n):
    """the table's ends, the edges of the judge's 64-record waves, and first records at every phase of the 12-byte entries
    against 16 bytes (record k lies at byte 12 k of the table)"""
    return [(0, 1), (n - 1, n), (63, 64), (64, 129), (1, n), (130, 200), (3, 70), (2, 3)]


@pytest.mark.parametrize("o", [dict(f=FR.flt(min_mean_q=33, max_n=1)), dict(t=R.trm(q_tail=30), f=FR.flt(min_len=60, max_n=2)), FULL, dict()],
                         ids=["a filter alone", "a trim and a filter", "everything", "nothing"])
def test_record_ranges(F, ctx, mode4, o):
    raw, recs = mode4
    n = len(recs)
    assert {(12 * a) % 16 for a, _ in ranges(n)} == {0, 4, 8, 12}
    b = ctx.dblock(raw, recs)
    kept = 0
    for first, end in ranges(n):
        g, want = same(b, raw, recs, first, end, **o)
        kept += int(g["report"][1])
    g, want = same(b, raw, recs, 1, n, **o)
    assert o == {} or 0.2 * n < int(g["report"][1]) < 0.9 * n, "a degenerate draw"
    assert o != {} or (int(g["report"][1]) == n - 1 and g["out"].tobytes() == raw[int(recs["seq_off"][1]) - len(PR.header_lines(raw, recs)[1]):].tobytes())
    for first, end in ((0, 0), (5, 5), (6, 5), (0, n + 1), (n, n + 1)):
        r = b.select_marked(first, end, None, **opts(o))
        assert r["rc"] == E_ARG and r["out_len"] == 0 and not r["report"].any(), (first, end)
    b.close()


def test_record_ranges_of_planted_reads(F, ctx):
    """adapters, poly-G tails and quality drops in the reads of the range"""
    raw, recs = TG.planted(300, 1712)
    b = ctx.dblock(raw, recs)
    o = dict(a=AR.adp(TG.ADAPTER, 5, 10), x=TG.BOTH, t=R.trm(**TG.TT.Q20), f=FR.flt(min_len=25, max_n=0))
    for first, end in ((64, 129), (1, 300), (130, 200)):
        g, want = same(b, raw, recs, first, end, **o)
        assert int(want[1][AR.READS_WITH_ADAPTER]) > 5 and int(want[1][TR.READS_WITH_POLY]) > 5 and int(want[1][TR.READS_WINDOW_CUT]) > 5
    b.close()


@pytest.mark.parametrize("o", [dict(f=FR.flt(min_mean_q=33, max_n=1)), dict(t=R.trm(q_tail=30, cut_front=2), f=FR.flt(min_len=60))], ids=["a filter alone", "a trim"])
def test_record_ranges_with_text_behind_every_plus(F, ctx, mode4, o):
    raw, recs = with_plus_text(*mode4)
    b = ctx.dblock(raw, recs)
    assert np.array_equal(b.records(), recs)
    for first, end in ranges(len(recs)):
        same(b, raw, recs, first, end, what="'+' lines with text", **o)
    rng = np.random.default_rng(8)
    same(b, raw, recs, 3, 203, rng.integers(0, 256, 25, dtype=np.uint8), what="'+' lines with text, marked", **o)
    b.close()


# ---------------------------------------------------------------- 3. marks
def test_marks(F, ctx, mode4):
    raw, recs = mode4
    n = len(recs)
    b = ctx.dblock(raw, recs)
    rng = np.random.default_rng(3)
    for o in (dict(f=FR.flt(min_mean_q=33, max_n=1)), FULL):
        for first, end in ((0, n), (7, 72), (64, 129)):
            m = end - first
            own, _ = same(b, raw, recs, first, end, **o)
            passing = int(own["report"][1])
            assert 0 < passing < m
            # all zero: nothing is written, every read that passes is counted in word 20
            g, _ = same(b, raw, recs, first, end, np.zeros((m + 7) // 8, dtype=np.uint8), "all zero", **o)
            assert g["out_len"] == 0 and int(g["report"][PR.DROPPED_UNMARKED]) == passing and not g["keep"].any()
            assert not g["report"][[1, 3, 4]].any() and g["report"][5:20].tolist() == own["report"][5:20].tolist()
            # all one: the call without a mark
            g, _ = same(b, raw, recs, first, end, np.full((m + 7) // 8, 0xFF, dtype=np.uint8), "all one", **o)
            assert g["out"].tobytes() == own["out"].tobytes() and g["report"].tolist() == own["report"].tolist() and np.array_equal(g["keep"], own["keep"])
            for k in range(3):
                mark = rng.integers(0, 256, (m + 7) // 8, dtype=np.uint8)
                g, want = same(b, raw, recs, first, end, mark, "drawn %d" % k, **o)
                assert 0 < int(g["report"][PR.DROPPED_UNMARKED]) < passing
                assert np.array_equal(g["win"], own["win"]) and np.array_equal(g["places"], own["places"]), "the mark changes no window"
    # 65 records: the second mark word has one live bit; the seven bits behind it in the caller's last byte are not looked at
    first, end, o = 7, 72, dict(f=FR.flt(min_mean_q=30))
    own, _ = same(b, raw, recs, first, end, **o)
    assert PR.bits(own["keep"], 65)[64], "the last record passes"
    for last in (0, 1):
        mark = rng.integers(0, 256, 9, dtype=np.uint8)
        mark[8] = last
        clean, _ = same(b, raw, recs, first, end, mark, "65 records", **o)
        assert bool(PR.bits(clean["keep"], 65)[64]) == bool(last)
        mark[8] = last | 0xFE
        dirty, _ = same(b, raw, recs, first, end, mark, "65 records, padding bits set", **o)
        assert dirty["out"].tobytes() == clean["out"].tobytes() and dirty["report"].tolist() == clean["report"].tolist()
        assert dirty["keep"].tolist() == clean["keep"].tolist() and dirty["keep"][8] <= 1
    b.close()


# ---------------------------------------------------------------- 4. the golden pair
def test_the_golden_pair(F, ctx, golden):
    (raw1, recs1), (raw2, recs2) = golden
    n = len(recs1)
    want1, want2, rep1, rep2, counters = PR.pair_records(raw1, recs1, raw2, recs2, f=Q20)
    assert counters == dict(pairs=1000, kept=619, dropped_mate1_only=80, dropped_mate2_only=84, dropped_both=217)
    b1, b2 = ctx.dblock(raw1, recs1), ctx.dblock(raw2, recs2)
    assert b1.pair_names(0, b2, 0, n) == (0, None)
    k1 = b1.select_marked(0, n, None, flt=Q20, query=True)
    assert k1["rc"] == 0 and k1["out"] is None
    g2 = b2.select_marked(0, n, k1["keep"], flt=Q20)
    g1 = b1.select_marked(0, n, g2["keep"], flt=Q20)
    for g, want, rep in ((g1, want1, rep1), (g2, want2, rep2)):
        assert g["rc"] == 0 and g["out"].tobytes() == want.tobytes() and g["report"].tolist() == rep.tolist()
        counted(g["report"])
    assert np.array_equal(g1["keep"], g2["keep"])
    assert (int(g2["report"][20]), int(g1["report"][20])) == (80, 84)
    out1, out2 = g1["out"], g2["out"]
    t1, t2 = FR.parse(out1), FR.parse(out2)
    assert len(t1) == len(t2) == 619 and PR.read_ids(out1, t1) == PR.read_ids(out2, t2)
    kept = PR.bits(g1["keep"], n)
    assert PR.read_ids(out1, t1) == [i for i, k in zip(PR.read_ids(raw1, recs1), kept) if k], "equal ids in equal order: the input's"
    b1.close()
    b2.close()


# ---------------------------------------------------------------- 5. names
def with_ids(F, raw, recs, change):
    """the chunk with change(r, header line) for every header line -> (raw, recs)"""
    raw = np.asarray(raw, dtype=np.uint8)
    lines, seq = PR.header_lines(raw, recs), recs["seq_off"].astype(np.int64)
    ends = np.concatenate((PR.header_starts(recs)[1:], [int(recs["qual_off"][-1]) + int(recs["len"][-1]) + 1]))
    out = np.frombuffer(b"".join(change(r, line) + raw[seq[r]:ends[r]].tobytes() for r, line in enumerate(lines)), dtype=np.uint8)
    return out, F.parse_fastq(out)


def test_names(F, ctx, golden):
    (raw1, recs1), (raw2, recs2) = golden
    n = len(recs1)
    b1, b2 = ctx.dblock(raw1, recs1), ctx.dblock(raw2, recs2)
    assert PR.first_mismatch(raw1, recs1, 0, raw2, recs2, 0, n) is None
    assert b1.pair_names(0, b2, 0, n) == (0, None) and b1.pair_names(0, b1, 0, n) == (0, None) and b2.pair_names(0, b1, 0, n) == (0, None)
    assert b1.pair_names(990, b2, 990, 10) == (0, None) and b1.pair_names(1, b2, 1, 1) == (0, None)
    id_len = [PR.id_len(line) for line in PR.header_lines(raw2, recs2)]
    for r in (0, 63, 64, n - 1):
        for at in (1, id_len[r]):      # the id's first byte, and its last
            spoilt = raw2.copy()
            where = int(PR.header_starts(recs2)[r]) + at
            spoilt[where] ^= 1
            assert PR.first_mismatch(raw1, recs1, 0, spoilt, recs2, 0, n) == r
            b = ctx.dblock(spoilt, recs2)
            assert b1.pair_names(0, b, 0, n) == (0, r) and b.pair_names(0, b1, 0, n) == (0, r), (r, at)
            assert b1.pair_names(0, b, 0, r) == ((0, None) if r else (E_ARG, None)), "the pairs in front of it agree"
            if r:
                assert b1.pair_names(r - 1, b, r - 1, 2) == (0, 1) and b1.pair_names(r, b, r, n - r) == (0, 0)
            b.close()
        # a byte behind the id may differ
        spoilt = raw2.copy()
        spoilt[int(PR.header_starts(recs2)[r]) + id_len[r] + 2] ^= 1
        b = ctx.dblock(spoilt, recs2)
        assert b1.pair_names(0, b, 0, n) == (0, None)
        b.close()
    # the smallest of several
    spoilt = raw2.copy()
    for r in (700, 131, 999):
        spoilt[int(PR.header_starts(recs2)[r]) + 3] ^= 1
    b = ctx.dblock(spoilt, recs2)
    assert b1.pair_names(0, b, 0, n) == (0, 131) and b1.pair_names(132, b, 132, n - 132) == (0, 700 - 132)
    b.close()
    # "/1" against "/2", against nothing, and ids ended by a tab, by the line's end, longer than 128 bytes
    long_id = b"L" * 300
    forms = [lambda i: i + b"/1 t\n", lambda i: i + b"/2\tt\n", lambda i: i + b"\n", lambda i: i + b"/1\n", lambda i: i + b" /1\n"]
    chunks = []
    for k, form in enumerate(forms):
        raw, recs = with_ids(F, raw1[:int(PR.header_starts(recs1)[200])], recs1[:200],
                             lambda r, line: b"@" + form((long_id if r % 50 == 7 else b"") + line[1:1 + PR.id_len(line)]))
        chunks.append((raw, recs, ctx.dblock(raw, recs)))
    for raw_a, recs_a, a in chunks:
        for raw_b, recs_b, b in chunks:
            assert PR.first_mismatch(raw_a, recs_a, 0, raw_b, recs_b, 0, 200) is None
            assert a.pair_names(0, b, 0, 200) == (0, None)
    # a "/3" is part of the id, and so is a "/1" in its middle
    raw, recs = with_ids(F, chunks[0][0], chunks[0][1], lambda r, line: line.replace(b"/1 ", b"/3 ") if r == 77 else line.replace(b".", b"/1.") if r == 150 else line)
    b = ctx.dblock(raw, recs)
    assert chunks[0][2].pair_names(0, b, 0, 200) == (0, 77) == (0, PR.first_mismatch(chunks[0][0], chunks[0][1], 0, raw, recs, 0, 200))
    assert chunks[0][2].pair_names(78, b, 78, 122) == (0, 150 - 78)
    b.close()
    # an id that is a prefix of its mate's, either way, also behind 128 bytes
    for r in (5, 7, 64):
        raw, recs = with_ids(F, chunks[2][0], chunks[2][1], lambda k, line: line[:-2] + b"\n" if k == r else line)
        b = ctx.dblock(raw, recs)
        assert chunks[2][2].pair_names(0, b, 0, 200) == (0, r) and b.pair_names(0, chunks[2][2], 0, 200) == (0, r)
        assert chunks[0][2].pair_names(0, b, 0, 200) == (0, r)
        b.close()
    for _, _, b in chunks:
        b.close()
    # a file shifted by one record matches at offset 1
    cut = int(PR.header_starts(recs2)[1])
    shifted_raw = raw2[cut:].copy()
    shifted = ctx.dblock(shifted_raw, F.parse_fastq(shifted_raw))
    assert b1.pair_names(1, shifted, 0, n - 1) == (0, None) and shifted.pair_names(0, b1, 1, n - 1) == (0, None)
    assert b1.pair_names(0, shifted, 0, n - 1) == (0, 0) and b1.pair_names(65, shifted, 64, 100) == (0, None)
    # ranges outside either chunk, no pair at all, no block
    for first_a, first_b, count in ((0, 0, 0), (0, 0, n + 1), (1, 0, n), (0, 1, n), (n, 0, 1), (0, n, 1), (0, 0, n)):
        want = (E_ARG, None) if (first_a, first_b, count) != (0, 0, n) else (0, None)
        assert b1.pair_names(first_a, b2, first_b, count) == want, (first_a, first_b, count)
    assert b1.pair_names(0, shifted, 0, n) == (E_ARG, None) and b1.pair_names(0, None, 0, 1) == (E_ARG, None)
    if F.device_count() > 1:     # a block of another device
        other_ctx = F.Context(ctx.seq_ft, ctx.qual_ft, device=1)
        other = other_ctx.dblock(raw2, recs2)
        assert b1.pair_names(0, other, 0, n) == (E_ARG, None)
        other.close()
        other_ctx.close()
    shifted.close()
    b1.close()
    b2.close()


def test_two_handles_with_their_own_tables_on_staged_chunks(F, golden):
    (raw1, recs1), (raw2, recs2) = golden
    n = len(recs1)
    c1, c2 = TS.context_for(F, raw1, recs1), TS.context_for(F, raw2, recs2)
    assert c1.seq_ft.tobytes() != c2.seq_ft.tobytes() or c1.qual_ft.tobytes() != c2.qual_ft.tobytes()
    assert c1.chunk_pair_names(0, c2, 0, n) == (E_ARG, None), "no chunk on either handle"
    g1, g2 = c1.encode_raw(raw1), c2.encode_raw(raw2)
    assert g1["rc"] == 0 == g2["rc"]
    assert c1.chunk_pair_names(0, c2, 0, n) == (0, None) and c2.chunk_pair_names(10, c1, 10, 100) == (0, None)
    assert c1.chunk_pair_names(0, c2, 1, n - 1) == (0, 0) and c1.chunk_pair_names(0, c2, 0, n + 1) == (E_ARG, None)
    assert c1.chunk_pair_names(0, c1, 0, n) == (0, None) and c1.chunk_pair_names(0, None, 0, n) == (E_ARG, None)
    # the three calls of a paired restore, on the staged chunks
    want1, want2, rep1, rep2, counters = PR.pair_records(raw1, recs1, raw2, recs2, t=R.trm(q_tail=20), f=FR.flt(min_len=40, min_mean_q=22))
    sel = dict(trim=R.trm(q_tail=20), flt=FR.flt(min_len=40, min_mean_q=22))
    k1 = c1.chunk_select_marked(0, n, None, query=True, **sel)
    g2 = c2.chunk_select_marked(0, n, k1["keep"], **sel)
    g1 = c1.chunk_select_marked(0, n, g2["keep"], **sel)
    assert g1["rc"] == 0 == g2["rc"] and g1["out"].tobytes() == want1.tobytes() and g2["out"].tobytes() == want2.tobytes()
    assert g1["report"].tolist() == rep1.tolist() and g2["report"].tolist() == rep2.tolist() and 0 < counters["kept"] < n
    assert min(counters.values()) > 0, "every kind of pair"
    # mate 2 in two pieces, as a worker meets a chunk boundary of archive 2
    keep = PR.bits(k1["keep"], n)
    lo = c2.chunk_select_marked(0, 391, np.packbits(keep[:391], bitorder="little"), **sel)
    hi = c2.chunk_select_marked(391, n, np.packbits(keep[391:], bitorder="little"), **sel)
    assert lo["rc"] == 0 == hi["rc"] and lo["out"].tobytes() + hi["out"].tobytes() == want2.tobytes()
    assert (lo["report"] + hi["report"]).tolist() == rep2.tolist()
    assert np.array_equal(np.concatenate((PR.bits(lo["keep"], 391), PR.bits(hi["keep"], n - 391))), PR.bits(g2["keep"], n))
    TG.holds(c1.chunk_tailtrim(n, None, None, sel["trim"], sel["flt"]), TR.tail_records(raw1, recs1.astype(R.REC_DTYPE), None, None, sel["trim"], sel["flt"]),
             "a tail call behind the marked calls: the chunk is as it was")
    c1.close()
    c2.close()


@pytest.mark.parametrize("cut", [None, (574, 572)], ids=["the fixture as it is", "the fixture from pairs 574 and 572 on"])
def test_a_record_range_of_the_staged_chunk_in_every_pair_call(F, ctx, golden, cut):
    """first_a = 3, first_b = 5, count = 64 + 1 of the chunks staged on two handles: a partial last wave, a record in front of
    either range, two different firsts.  Every pair call gives what its block form gives for the same ranges and what its
    reference gives; the correcting calls run on fresh copies.  In the fixture as it is, record 3 of mate 1 and record 5 of
    mate 2 are strangers -- their ids differ at once and nothing overlaps.  Cut in front of pair 574 and of pair 572 the
    chunks' records 3 and 5 are pair 577, whose 65 pairs are the 65 of the fixture with the most overlaps (overlap_ref: 19),
    so that the overlap's own inserts make the correction change both chunks."""
    import correct_ref as CR
    import overlap_ref as OR
    (raw1, recs1), (raw2, recs2) = golden
    if cut:
        raw1, raw2 = raw1[int(PR.header_starts(recs1)[cut[0]]):].copy(), raw2[int(PR.header_starts(recs2)[cut[1]]):].copy()
        recs1, recs2 = F.parse_fastq(raw1), F.parse_fastq(raw2)
    first_a, first_b, count = 3, 5, 64 + 1
    where = (raw1, recs1, first_a, raw2, recs2, first_b, count)

    def fresh():
        c1, c2 = TS.context_for(F, raw1, recs1), TS.context_for(F, raw2, recs2)
        assert c1.encode_raw(raw1)["rc"] == 0 == c2.encode_raw(raw2)["rc"]
        return c1, c2, ctx.dblock(raw1, recs1), ctx.dblock(raw2, recs2)

    c1, c2, b1, b2 = fresh()
    # names
    want = (0, PR.first_mismatch(*where))
    assert want == ((0, None) if cut else (0, 0))
    assert c1.chunk_pair_names(first_a, c2, first_b, count) == want == b1.pair_names(first_a, b2, first_b, count)
    # overlap
    want = OR.overlap_records(*where, OR.spec())
    assert int(want[0][OR.OVERLAPPED]) == (19 if cut else 0)
    for what, g in (("staged", c1.chunk_pair_overlap(first_a, c2, first_b, count, OR.spec())), ("blocks", b1.pair_overlap(first_a, b2, first_b, count, OR.spec()))):
        assert g["rc"] == 0 and g["out"].tolist() == want[0].tolist(), what
        assert [g[k].tolist() for k in ("limit_a", "limit_b", "insert")] == [w.tolist() for w in want[1:]], what
    # correct: with the overlap's inserts, and with an insert of a whole read for every pair, which lays strangers over each other
    changed = False
    for ins in (want[3], np.full(count, 100, dtype=np.uint16)):
        if changed:
            for h in (c1, c2, b1, b2):
                h.close()
            c1, c2, b1, b2 = fresh()
        want_a, want_b, report, fa, fb = CR.correct_records(*where, ins, CR.spec())
        changed = want_a.tobytes() != raw1.tobytes() and want_b.tobytes() != raw2.tobytes()
        assert changed == bool(ins.any()), "a correction that corrects"
        for what, g in (("staged", c1.chunk_pair_correct(first_a, c2, first_b, count, ins, CR.spec())), ("blocks", b1.pair_correct(first_a, b2, first_b, count, ins, CR.spec()))):
            assert g["rc"] == 0 and g["report"].tolist() == report.tolist(), what
            assert g["fixed_a"].tolist() == fa.tolist() and g["fixed_b"].tolist() == fb.tolist(), what
        for c, b, got, recs in ((c1, b1, want_a, recs1), (c2, b2, want_b, recs2)):
            assert b.fetch(raw=True)["raw"].tobytes() == got.tobytes()
            s = c.chunk_select_marked(0, len(recs))
            assert s["rc"] == 0 and s["out"].tobytes() == PR.marked_records(got, recs, 0, len(recs))[0].tobytes()
    for h in (c1, c2, b1, b2):
        h.close()


# ---------------------------------------------------------------- 6. scratch history
def test_results_do_not_depend_on_what_the_scratch_held(F, golden):
    (raw1, recs1), (raw2, recs2) = golden
    n = len(recs1)
    c = TS.context_for(F, raw1, recs1)
    b1, b2 = c.dblock(raw1, recs1), c.dblock(raw2, recs2)
    spoilt = raw2.copy()
    spoilt[int(PR.header_starts(recs2)[321]) + 5] ^= 1
    b3 = c.dblock(spoilt, recs2)
    mark = np.random.default_rng(12).integers(0, 256, (900 + 7) // 8, dtype=np.uint8)

    def calls():
        g = b1.select_marked(37, 937, mark, **opts(FULL))
        assert g["rc"] == 0
        return (g["out"].tobytes(), g["report"].tolist(), g["keep"].tolist(), g["win"].tolist(), g["places"].tolist(),
                b1.pair_names(0, b2, 0, n), b1.pair_names(0, b3, 0, n))

    first = calls()
    assert first[5] == (0, None) and first[6] == (0, 321)
    buffers, filled = c.fill_scratch(0xFF)
    assert buffers > 0 and filled > 0
    assert calls() == first
    c.fill_scratch(0x00)
    assert calls() == first
    want = PR.marked_records(raw1, recs1, 37, 937, mark, FULL["a"], FULL["x"], FULL["t"], FULL["f"])
    assert first[0] == want[0].tobytes() and first[1] == want[1].tolist()
    for b in (b1, b2, b3):
        b.close()
    c.close()


# ---------------------------------------------------------------- 7. arguments
def test_arguments(F, ctx, mode4):
    raw, recs = mode4
    n = len(recs)
    b = ctx.dblock(raw, recs)
    lib = F.binding.lib()
    p = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)  # noqa: E731
    f = FR.flt(min_mean_q=33, max_n=1)
    want = PR.marked_records(raw, recs, 10, 210, None, f=f)

    def call(a, x, t, flt, first, end, out, cap, keep=None):
        size = C.c_size_t(77)
        report = np.full(TR.REPORT_WORDS, 7, dtype=np.uint64)
        rc = lib.fqgpu_dblock_select_marked(ctx.h, b.h, p(a), p(x), p(t), p(flt), first, end, None, p(out), cap, C.byref(size), p(report), p(keep), None, None)
        return rc, size.value, report

    out = np.full(want[0].size + 32, 0x5A, dtype=np.uint8)
    rc, size, report = call(None, None, None, f, 10, 210, out, want[0].size - 1)
    assert rc == -1 and size == want[0].size and report.tolist() == want[1].tolist() and (out == 0x5A).all(), "a buffer one byte short: nothing is written"
    rc, size, report = call(None, None, None, f, 10, 210, out, want[0].size)
    assert rc == 0 and out[:size].tobytes() == want[0].tobytes() and (out[size:] == 0x5A).all(), "exactly *out_len bytes"
    for bad in ((AR.adp(b"ACGT", 5), None, None, f), (None, TR.tl(poly=16), None, f), (None, None, R.trm(crop=0), f), (None, None, None, FR.flt(min_mean_q=64))):
        rc, size, report = call(*bad, 10, 210, out, out.size)
        assert rc == E_ARG and size == 0 and not report.any()
    # a byte that cannot be judged refuses the call only when it lies in the range
    spoilt = raw.copy()
    spoilt[int(recs["qual_off"][5]) + 1] = 32
    b.close()
    b = ctx.dblock(spoilt, recs)
    keep = np.full(25, 0xAA, dtype=np.uint8)
    rc, size, report = call(None, None, None, f, 0, 200, None, 0, keep)
    assert rc == E_ARG and size == 0 and not report.any() and not keep.any()
    rc, size, report = call(None, None, None, f, 10, 210, None, 0)
    assert rc == 0 and size == want[0].size and report.tolist() == want[1].tolist()
    assert np.array_equal(b.fetch_raw(), spoilt), "the chunk is left as it is"
    b.close()
