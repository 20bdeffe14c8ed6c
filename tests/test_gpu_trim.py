"""Read trimming on the device (fqcomp28_amd/csrc/select.hip behind fqgpu_chunk_trim / fqgpu_dblock_trim) against the numpy
restatement in trim_ref.py: the kept bytes, the report, the keep bits and the windows, byte for byte.  Integer arithmetic:
every comparison is exact."""
import ctypes as C
import os
import re
import zlib

import numpy as np
import pytest

import filter_ref as FR
import oracle_lib as O
import stats_ref as SR
import test_gpu_filter as TF
import test_gpu_stats as TS
import test_trim_host as TH
import trim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

E_OVERFLOW, E_ARG = -1, -4
FIXTURES = TH.FIXTURES
Q20 = dict(q_front=20, q_tail=20)


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


def trim_constants():
    """the tiling of select.hip, from its source: its SEL_* constants under the names the tests here use"""
    src = open(os.path.join(ROOT, "fqcomp28_amd", "csrc", "select.hip")).read()
    return {"TRIM_" + k: int(re.search(r"constexpr unsigned SEL_%s = (\d+);" % k, src).group(1))
            for k in ("THREADS", "WAVE_RECORDS", "GROUP_LANES", "UNROLL", "GATHER_THREADS", "GATHER_WORDS")}


def chunk_of(hls, phreds, seed=1, n_rate=0.0, plus_repeats=False, n_at=None):
    """a FASTQ chunk from, per record, the length of the header line with its '@' and the read's Phred values -> (raw, recs):
    the header line is '@' and filler, the bases are drawn, N at rate n_rate and at the places n_at[r]"""
    rng = np.random.default_rng(seed)
    parts, recs, at = [], np.zeros(len(phreds), dtype=R.REC_DTYPE), 0
    for r, (hl, phred) in enumerate(zip(hls, phreds)):
        L = len(phred)
        seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, L)]
        if n_rate:
            seq = np.where(rng.random(L) < n_rate, ord("N"), seq).astype(np.uint8)
        if n_at is not None and n_at[r] is not None:
            seq = seq.copy()
            seq[n_at[r]] = ord("N")
        head = b"@" + b"h" * (int(hl) - 1) + b"\n"
        plus = b"+" + head[1:] if plus_repeats and r % 2 == 0 else b"+\n"
        recs[r] = (at + len(head), at + len(head) + L + len(plus) + 1, L)
        rec = head + seq.tobytes() + b"\n" + plus + (np.asarray(phred) + 33).astype(np.uint8).tobytes() + b"\n"
        parts.append(rec)
        at += len(rec)
    return np.frombuffer(b"".join(parts), dtype=np.uint8), recs


def plateau(rng, L, front=None, back=None):
    """Phred values of a read: a plateau of 30 +- 6 with low ends of 5 +- 4, their lengths drawn when not given"""
    a = int(rng.choice([0, 0, 3, 10, 40])) if front is None else front
    b = int(rng.choice([0, 0, 5, 30, 200])) if back is None else back
    p = 30 + rng.integers(-6, 7, L)
    p[:a] = (5 + rng.integers(-4, 5, L))[:a]
    if b:
        p[-b:] = (5 + rng.integers(-4, 5, L))[-b:]
    return p


def drawn(lens, seed, n_rate=0.01, **kw):
    rng = np.random.default_rng(seed)
    return chunk_of(rng.integers(2, 18, len(lens)), [plateau(rng, int(L)) for L in lens], seed + 1, n_rate, **kw)


def same(ctx, raw, recs, t, f=None, what="", **kw):
    """the device's answer for the block (raw, recs) against the reference's -> (the device's, the reference's)"""
    want = R.trim_records(raw, recs, t, f)
    b = ctx.dblock(raw, recs)
    try:
        g = b.trim(t, f, **kw)
    finally:
        b.close()
    holds(g, want, what)
    return g, want


def holds(g, want, what=""):
    assert g["rc"] == 0, (what, g["rc"])
    assert g["report"].tolist() == want[1].tolist(), what
    assert g["keep"].tolist() == want[2].tolist(), what
    if not np.array_equal(g["win"], want[3]):
        at = int(np.flatnonzero(g["win"] != want[3])[0])
        raise AssertionError("%s: the windows differ, first at record %d: (%d, %d), expected (%d, %d)" % (
            what, at, g["win"][at] & 0xFFFF, g["win"][at] >> 16, want[3][at] & 0xFFFF, want[3][at] >> 16))
    assert g["out_len"] == want[0].size, what
    if g["out"] is not None and not np.array_equal(g["out"], want[0]):
        at = int(np.flatnonzero(g["out"] != want[0])[0])
        raise AssertionError("%s: the kept bytes differ, first at %d of %d" % (what, at, want[0].size))


def shares(want, recs):
    """of a reference result: the shares of reads cut at the front, at the tail, untouched, emptied"""
    start, n, L = (want[3] & 0xFFFF).astype(np.int64), (want[3] >> 16).astype(np.int64), recs["len"].astype(np.int64)
    live = n > 0
    return ((live & (start > 0)).mean() + 0.0, (live & (start + n < L)).mean() + 0.0, (n == L).mean() + 0.0, (n == 0).mean() + 0.0)


# ---------------------------------------------------------------- 1. the fixtures
TRIMS = [dict(), Q20, dict(q_tail=30, crop=100), dict(cut_front=5, cut_tail=5), dict(q_front=25), dict(cut_front=3, q_front=15, q_tail=28, crop=60)]
FILTERS = [None, dict(), dict(min_len=30), dict(max_n=0, min_mean_q=25), dict(min_len=20, max_len=90, low_q=20, max_low_pct=10)]


@pytest.mark.parametrize("name", FIXTURES)
def test_the_fixtures_under_several_trims(F, ctx, golden_dir, name):
    raw, recs = O.load_fastq(os.path.join(golden_dir, name + ".fastq"))
    recs = recs.astype(R.REC_DTYPE)
    for t in TRIMS:
        for f in FILTERS:
            same(ctx, raw, recs, R.trm(**t), None if f is None else FR.flt(**f), "%s %s %s" % (name, t, f))
    if name == "SRR065390_sub_1":   # the input is not vacuous
        want = R.trim_records(raw, recs, R.trm(**Q20))
        trimmed, emptied = int(want[1][R.READS_TRIMMED]) / len(recs), int(want[1][R.READS_EMPTIED]) / len(recs)
        print("SRR065390_sub_1, cutoff 20: %.1f %% of the reads trimmed, %.2f %% emptied" % (100 * trimmed, 100 * emptied))
        assert 0.50 <= trimmed <= 0.90 and 0.001 <= emptied <= 0.10
    b = ctx.dblock(raw)   # with the device parser's record table
    for t, f in ((Q20, None), (dict(q_tail=30, crop=100), dict(max_n=0, min_mean_q=25))):
        g = b.trim(R.trm(**t), None if f is None else FR.flt(**f))
        holds(g, R.trim_chunk(raw, R.trm(**t), None if f is None else FR.flt(**f)), "%s, parsed on the device" % name)
    b.close()


@pytest.mark.parametrize("plus_repeats", [False, True])
def test_the_hand_chunk_of_the_host_test(F, ctx, plus_repeats):
    raw = TH.hand_chunk(plus_repeats)
    for table in (FR.parse(raw), None):
        b = ctx.dblock(raw, table)
        for kw, col in TH.HAND_TRIMS:
            g = b.trim(R.trm(**kw))
            want = TH.hand_expected(col)
            holds(g, want, str(kw))
        holds(b.trim(R.trm(**TH.TRIM_Q), FR.flt(**TH.HAND_FILTER)), TH.hand_expected(3, **TH.HAND_FILTER))
        b.close()


# ---------------------------------------------------------------- 2. synthetic reads
LINE_LENGTHS = [3, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513, 1023, 65535]


def aligned_header(at, L, target, line="seq"):
    """the length of a header line (with its '@') that puts the record's sequence line -- or quality line -- at byte `target`
    of a 16-byte word, for a record that starts at `at` and has bare '+' lines"""
    hl = (target - at - 1 - (L + 3 if line == "qual" else 0)) % 16
    return hl + 16 if hl < 2 else hl


def synthetic_reads():
    """48 reads of every length up to 513, 16 of 1023 and of 65535, shuffled; the header lengths are chosen so that the
    sequence lines of a length start at byte 0, 1, .. 15 of a 16-byte word in turn (the quality lines then do as well)"""
    rng = np.random.default_rng(2)
    lens = np.concatenate([np.full(48 if L <= 513 else 16, L) for L in LINE_LENGTHS])
    rng.shuffle(lens)
    hls, at, seen = [], 0, {}
    for L in lens.tolist():
        target = seen.get(L, 0) % 16
        seen[L] = target + 1
        hls.append(aligned_header(at, L, target))
        at += hls[-1] + 1 + 2 * L + 4
    return chunk_of(hls, [plateau(rng, int(L)) for L in lens], 3, n_rate=0.01)


def test_synthetic_reads_of_every_length_at_every_alignment(F, ctx):
    raw, recs = synthetic_reads()
    for L in LINE_LENGTHS:   # the lines start at all sixteen places of a 16-byte word
        assert len(set((recs["seq_off"][recs["len"] == L] & 15).tolist())) == 16 and len(set((recs["qual_off"][recs["len"] == L] & 15).tolist())) == 16, L
    g, want = same(ctx, raw, recs, R.trm(**Q20), None, "synthetic, cutoff 20")
    front, tail, untouched, emptied = shares(want, recs)
    print("synthetic reads: front cut %.0f %%, tail cut %.0f %%, untouched %.0f %%, emptied %.0f %%" % (100 * front, 100 * tail, 100 * untouched, 100 * emptied))
    assert front >= 0.20 and tail >= 0.20 and untouched >= 0.10 and 0.01 <= emptied <= 0.40
    for t, f in ((dict(q_front=20), None), (dict(q_tail=20), dict(max_n=0)), (dict(cut_front=2, cut_tail=1, q_front=20, q_tail=20, crop=120), dict(min_len=10, min_mean_q=25)),
                 (dict(q_tail=20), dict(low_q=20, max_low_pct=5))):
        same(ctx, raw, recs, R.trm(**t), None if f is None else FR.flt(**f), "synthetic %s %s" % (t, f))


# Where a walk STOPS (the first place with s < 0) and where it CUTS are chosen independently, and both by the byte they have in
# the quality line's 16-byte words: `rel` counts bytes from the aligned word that holds the line's first byte (which sits at
# byte `lead` of it), so byte rel % 16 of word rel // 16, and byte rel % 256 of a request of the record's lanes.
def boundary_rels(L, lead):
    """the bytes to stop at: every byte of the line's first and of its last word, bytes 15 and 0 of inner words, the last and
    the first byte of a request -- those that lie inside the line"""
    last = lead + L - 1
    rels = set(range(lead, 16)) | set(range(last - last % 16, last + 1)) | {31, 32, 47, 48, 255, 256, 511, 512}
    rels |= {last - last % 256 - 1, last - last % 256}
    return sorted(r for r in rels if lead <= r <= last)


def front_read(L, h, x):
    """Phred values: the front walk stops at h; it cuts behind the one low base at x < h (x None: it cuts nothing).  20 adds
    nothing, 2 adds 18, 40 takes 20; 33 behind h stops the tail walk at the line's end -> (values, window)"""
    p = np.full(L, 20)
    p[h], p[h + 1:] = 40, 33
    if x is not None:
        p[x] = 2
    start = 0 if x is None else x + 1
    return p, (start, L - start)


def tail_read(L, h, x):
    """the mirror image: the tail walk stops at h and puts the read's end at the low base at x > h (None: at its end)"""
    p = np.full(L, 20)
    p[h], p[:h] = 40, 33
    if x is not None:
        p[x] = 2
    return p, (0, L if x is None else x)


def boundary_reads(L, pairs, variants):
    """-> [(kind, lead, stop place, Phred values, window)]: for every (lead, rel) a front read and a tail read that stop
    there, for the first `variants` of these cut places: the base beside the stop, none, 17 bases from the
    stop, the line's end"""
    reads = []
    for lead, rel in pairs:
        h = rel - lead
        cuts = [x for x in dict.fromkeys((h - 1, None, h - 17, 0)) if x is None or 0 <= x < h]
        for x in cuts[:variants]:
            reads.append(("front", lead, h) + front_read(L, h, x))
        cuts = [x for x in dict.fromkeys((h + 1, None, h + 17, L - 1)) if x is None or h < x < L]
        for x in cuts[:variants]:
            reads.append(("tail", lead, h) + tail_read(L, h, x))
    return reads


def long_read_pairs(L):
    """(lead, rel) for the longest read: every byte of a first word (byte b at a lead that is at most b), every byte of a
    last word (lead 1 puts the last byte of 65535 at byte 15 of its word; lead 9 at byte 7), and the inner boundaries with
    the leads taking turns"""
    pairs = [((5 * b) % (b + 1), b) for b in range(16)]
    for lead in (1, 9):
        last = lead + L - 1
        pairs += [(lead, r) for r in range(last - last % 16, last + 1)]
    for j, r in enumerate((31, 32, 47, 48, 255, 256, 511, 512)):
        pairs.append(((3 * j + 2) % 16, r))
    for lead in (0, 7, 15):
        last = lead + L - 1
        pairs += [(lead, last - last % 256 - 1), (lead, last - last % 256)]
    return pairs


def stops_of(raw, recs):
    """by the definition: per record (lead of the quality line, rel of the place where the front walk stops, ... the tail walk)"""
    out = []
    for r in recs:
        inc = 20 - (raw[int(r["qual_off"]):int(r["qual_off"]) + int(r["len"])].astype(np.int64) - 33)
        lead, L = int(r["qual_off"]) & 15, int(r["len"])
        f, t = np.flatnonzero(np.cumsum(inc) < 0), np.flatnonzero(np.cumsum(inc[::-1]) < 0)
        out.append((lead, lead + int(f[0]) if f.size else None, lead + L - 1 - int(t[0]) if t.size else None))
    return out


@pytest.mark.parametrize("L", [100, 300, 65535])
def test_walks_that_cut_and_stop_at_every_boundary(F, ctx, L):
    """Below a request of a record's lanes, above one, and the longest read.  For 100 and 300 every lead 0 .. 15 meets every
    byte of boundary_rels with every cut variant.  For 65535 the leads take turns over the bytes and there are two cut variants
    a read: the long-read path differs from the short one only in walking request after request, the words themselves are
    summed up by the code the shorter reads have been through at every lead."""
    every_lead = L <= 300
    pairs = [(lead, rel) for lead in range(16) for rel in boundary_rels(L, lead)] if every_lead else long_read_pairs(L)
    reads = boundary_reads(L, pairs, 4 if every_lead else 2)
    hls, at = [], 0
    for kind, lead, h, p, _ in reads:
        hls.append(aligned_header(at, L, lead, "qual"))
        at += hls[-1] + 1 + 2 * L + 4
    raw, recs = chunk_of(hls, [p for *_, p, _ in reads], L)
    assert (recs["qual_off"] & 15).tolist() == [lead for _, lead, *_ in reads]
    # the reads stop where their construction says, by the definition of the walk
    stops = stops_of(raw, recs)
    for (kind, lead, h, _, _), (_, f, t) in zip(reads, stops):
        assert (f if kind == "front" else t) == lead + h
    last_of = lambda lead: lead + L - 1  # noqa: E731
    for kind, col in (("front", 1), ("tail", 2)):
        met = {(s[0], s[col]) for s, rd in zip(stops, reads) if rd[0] == kind}
        if every_lead:
            for lead in range(16):
                last = last_of(lead)
                want = set(range(lead, 16)) | set(range(last - last % 16, last + 1)) | {31, 32, 47, 48}
                want |= {255, 256} if L > 256 else set()
                assert {(lead, r) for r in want} <= met, (kind, lead)
        else:
            assert {r for _, r in met if r < 16} == set(range(16)), "every byte of a first word"
            assert {r % 16 for lead, r in met if r >= last_of(lead) - last_of(lead) % 16} == set(range(16)), "every byte of a last word"
            assert {r % 256 for _, r in met} >= {255, 0, 15, 31, 32} and {r // 256 for _, r in met} >= {0, 1, 2, 254, 255}
    g, want = same(ctx, raw, recs, R.trm(**Q20), None, "boundaries of %d" % L)
    wins = [(int(w) & 0xFFFF, int(w) >> 16) for w in want[3]]
    assert wins == [w for *_, w in reads], "the reads are cut where their construction says"
    # windows that start, and windows that end, at every byte of a word
    assert {(lead + s) % 16 for (s, n), (_, lead, *_) in zip(wins, reads) if s} == set(range(16))
    assert {(lead + s + n) % 16 for (s, n), (_, lead, *_) in zip(wins, reads) if n < L and not s} == set(range(16))
    same(ctx, raw, recs, R.trm(**Q20), FR.flt(max_n=0, min_mean_q=21, low_q=20, max_low_pct=1), "boundaries of %d, counted" % L)
    if every_lead:   # both walks in one read: a front read's first half, a tail read's second half
        fronts = [p for kind, lead, h, p, _ in reads if kind == "front" and h < L // 2][::7]
        tails = [p for kind, lead, h, p, _ in reads if kind == "tail" and h >= L // 2][::7]
        both = [np.concatenate((a[:L // 2], b[L // 2:])) for a, b in zip(fronts, tails[::-1])]
        assert len(both) > 50
        raw, recs = chunk_of(2 + (np.arange(len(both)) * 3) % 16, both, L + 1)
        g, want = same(ctx, raw, recs, R.trm(**Q20), None, "boundaries of %d, both ends" % L)
        assert int(want[1][R.BASES_CUT_FRONT]) > 0 and int(want[1][R.BASES_CUT_TAIL]) > 0 and int(want[1][R.READS_EMPTIED]) == 0
        same(ctx, raw, recs, R.trm(cut_front=1, cut_tail=2, q_front=20, q_tail=20, crop=L - 20), FR.flt(min_mean_q=20), "boundaries of %d, all" % L)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257])
def test_record_counts(F, ctx, n):
    raw, recs = drawn(np.random.default_rng(n).integers(3, 300, n), 10 + n)
    for t, f in ((Q20, None), (Q20, dict(max_n=0)), (dict(cut_front=4, crop=50), dict(min_len=20)), (dict(), dict(min_mean_q=20))):
        same(ctx, raw, recs, R.trm(**t), None if f is None else FR.flt(**f), "%d records %s %s" % (n, t, f))


# ---------------------------------------------------------------- 3. the gather
@pytest.mark.parametrize("plus_repeats", [False, True])
def test_output_sizes_around_a_word_and_a_tile(F, ctx, plus_repeats):
    k = trim_constants()
    tile = k["TRIM_GATHER_THREADS"] * 16 * k["TRIM_GATHER_WORDS"]
    for cut in (0, 2):
        for edge in (16, tile, 2 * tile):
            for d in (-1, 0, 1):
                total = edge + d
                shape, left = [], total      # records of hl + 2 (L - cut) + 4 output bytes, the last one sized to fit
                while left > 440:
                    shape.append((7, 100 + cut))
                    left -= 7 + 200 + 4
                hl = 6 if left % 2 == 0 else 7
                n = (left - 4 - hl) // 2
                if n + cut < 3:              # (a read has at least three bases)
                    n = 3 - cut
                    hl = left - 4 - 2 * n
                shape.append((hl, n + cut))
                rng = np.random.default_rng(total)
                raw, recs = chunk_of([h - 1 for h, _ in shape], [30 + rng.integers(-6, 7, L) for _, L in shape], total, plus_repeats=plus_repeats)
                g, want = same(ctx, raw, recs, R.trm(cut_front=cut), None, "%d bytes, cut %d" % (total, cut))
                assert g["out_len"] == total


def keep_pattern(which, n, rng):
    keeps = np.zeros(n, bool)
    if which == "first":
        keeps[0] = True
    elif which == "last":
        keeps[-1] = True
    elif which == "alternating":
        keeps[::2] = True
    elif which == "long runs":
        keeps[(np.arange(n) // 700) % 2 == 1] = True
    else:
        keeps[:] = True
    return keeps


@pytest.mark.parametrize("trims", ["all untrimmed", "all trimmed", "trimmed at run ends"])
@pytest.mark.parametrize("which", ["first", "last", "alternating", "long runs", "all"])
def test_keep_patterns_with_trims(F, ctx, which, trims):
    """kept or dropped by an N in the middle of the read (max_n = 0), trimmed or not by low ends: the one-run shortcut of the
    gather, its per-word copies and its seams"""
    n = 3001
    rng = np.random.default_rng(17)
    keeps = keep_pattern(which, n, rng)
    lens = rng.integers(40, 200, n)   # (a plateau long enough to stop either walk in it)
    edge = keeps & (~np.roll(keeps, 1) | ~np.roll(keeps, -1))      # the first and the last record of every run
    edge[0] |= keeps[0]
    edge[-1] |= keeps[-1]
    low = np.ones(n, bool) if trims == "all trimmed" else np.zeros(n, bool) if trims == "all untrimmed" else edge
    phreds = [plateau(rng, int(L), 4 if low[r] else 0, 3 if low[r] else 0) for r, L in enumerate(lens)]
    raw, recs = chunk_of(rng.integers(2, 12, n), phreds, 5, n_at=[None if keeps[r] else int(lens[r]) // 2 for r in range(n)])
    g, want = same(ctx, raw, recs, R.trm(**Q20), FR.flt(max_n=0), "%s, %s" % (which, trims))
    assert np.unpackbits(want[2], bitorder="little")[:n].astype(bool).tolist() == keeps.tolist()
    assert int(want[1][R.READS_TRIMMED]) == int(low.sum())
    if trims == "all untrimmed" and which == "all":
        assert g["out"].tobytes() == raw.tobytes()


def test_fixed_cuts_and_crop_alone(F, ctx):
    L = 50
    rng = np.random.default_rng(4)
    raw, recs = chunk_of(rng.integers(2, 18, 300), [30 + rng.integers(-6, 7, L) for _ in range(300)], 6)
    mixed = drawn(rng.integers(3, 120, 500), 7)
    for t in (dict(cut_front=L - 1), dict(cut_front=L), dict(cut_front=L + 1), dict(cut_front=65535), dict(cut_tail=L - 1), dict(cut_tail=L),
              dict(cut_tail=L + 1), dict(cut_front=20, cut_tail=30), dict(cut_front=20, cut_tail=29), dict(cut_front=49, cut_tail=1),
              dict(crop=1), dict(crop=L - 1), dict(crop=L), dict(crop=L + 1), dict(cut_front=10, crop=L - 10), dict(cut_front=10, crop=L - 11)):
        for f in (None, dict(min_len=2, max_len=48)):
            same(ctx, raw, recs, R.trm(**t), None if f is None else FR.flt(**f), "%s %s" % (t, f))
            same(ctx, *mixed, R.trm(**t), None if f is None else FR.flt(**f), "mixed lengths %s %s" % (t, f))
        g, want = same(ctx, raw, recs, R.trm(**t), None, str(t))
        if t in (dict(cut_front=L), dict(cut_front=L + 1), dict(cut_tail=L), dict(cut_front=20, cut_tail=30), dict(cut_front=49, cut_tail=1)):
            assert int(want[1][R.READS_EMPTIED]) == 300 == int(want[1][R.DROPPED_SHORT]) and g["out_len"] == 0 and not g["win"].any()
        if t in (dict(crop=L), dict(crop=L + 1)):
            assert g["out"].tobytes() == raw.tobytes() and int(want[1][R.READS_TRIMMED]) == 0


def test_a_trim_that_cuts_nothing_is_the_filter(F, ctx):
    raw, recs = TF.drawn(np.random.default_rng(12).integers(3, 300, 4000), 13)
    fat = drawn(np.random.default_rng(14).integers(3, 300, 500), 15, plus_repeats=True)
    for block in ((raw, recs), fat):
        b = ctx.dblock(*block)
        for kw in (dict(), dict(max_n=0), dict(min_mean_q=22), dict(min_len=100, low_q=15, max_low_pct=30)):
            want = b.filter(FR.flt(**kw))
            for t in (dict(), dict(crop=65535), dict(crop=70000)):
                g = b.trim(R.trm(**t), FR.flt(**kw))
                assert g["rc"] == 0 == want["rc"] and g["out"].tobytes() == want["out"].tobytes(), kw
                assert g["report"][:10].tolist() == want["report"][:10].tolist() and not g["report"][10:].any(), kw
                assert g["keep"].tolist() == want["keep"].tolist(), kw
        assert b.trim(R.trm())["out"].tobytes() == b.filter(FR.flt())["out"].tobytes(), "a NULL filter keeps everything"
        b.close()


# ---------------------------------------------------------------- 4. arguments
def raw_call(F, ctx, b, t, f, out, cap, keep=None, win=None):
    n = C.c_size_t(77)
    report = np.full(R.REPORT_WORDS, 7, dtype=np.uint64)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = F.binding.lib().fqgpu_dblock_trim(ctx.h, b.h if b is not None else None, p(t), p(f), p(out), cap, C.byref(n), p(report), p(keep), p(win))
    return rc, n.value, report


def test_size_query_and_a_buffer_one_byte_short(F, ctx):
    raw, recs = drawn(np.random.default_rng(8).integers(3, 200, 900), 9)
    t, f = R.trm(**Q20), FR.flt(min_len=10)
    want = R.trim_records(raw, recs, t, f)
    assert 0 < want[0].size < raw.size
    b = ctx.dblock(raw, recs)
    keep = np.full((len(recs) + 7) // 8, 0xAA, dtype=np.uint8)
    win = np.full(len(recs), 0xAAAAAAAA, dtype=np.uint32)
    rc, n, report = raw_call(F, ctx, b, t, f, None, 0, keep, win)
    assert rc == 0 and n == want[0].size and report.tolist() == want[1].tolist(), "the size query"
    assert keep.tolist() == want[2].tolist() and win.tolist() == want[3].tolist()
    rc, n, report = raw_call(F, ctx, b, t, f, None, 1 << 40)
    assert rc == 0 and n == want[0].size, "out == NULL is a size query whatever out_cap says"
    out = np.full(want[0].size + 32, 0x5A, dtype=np.uint8)
    rc, n, report = raw_call(F, ctx, b, t, f, out, want[0].size - 1)
    assert rc == E_OVERFLOW and n == want[0].size and report.tolist() == want[1].tolist()
    assert (out == 0x5A).all(), "nothing is written"
    rc, n, report = raw_call(F, ctx, b, t, f, out, want[0].size)
    assert rc == 0 and n == want[0].size and out[:n].tobytes() == want[0].tobytes() and (out[n:] == 0x5A).all(), "exactly *out_len bytes"
    rc, n, report = raw_call(F, ctx, b, t, None, None, 0)
    assert rc == 0 and report.tolist() == R.trim_records(raw, recs, t)[1].tolist(), "a NULL filter"
    # a trim or a filter its check refuses, a NULL where data is expected
    for bad in TH.BAD_TRIMS:
        rc, n, report = raw_call(F, ctx, b, R.trm(**bad), f, out, out.size)
        assert rc == E_ARG and n == 0 and not report.any(), bad
    rc, n, report = raw_call(F, ctx, b, t, FR.flt(min_mean_q=64), out, out.size)
    assert rc == E_ARG and n == 0 and not report.any()
    rc, n, report = raw_call(F, ctx, b, None, f, out, out.size)
    assert rc == E_ARG and n == 0 and not report.any()
    rc, n, report = raw_call(F, ctx, None, t, f, out, out.size)
    assert rc == E_ARG and n == 0 and not report.any()
    L = F.binding.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert L.fqgpu_dblock_trim(ctx.h, b.h, p(t), p(f), None, 0, None, p(report), None, None) == E_ARG
    nn = C.c_size_t(5)
    assert L.fqgpu_dblock_trim(ctx.h, b.h, p(t), p(f), None, 0, C.byref(nn), None, None, None) == E_ARG and nn.value == 0
    assert (out[want[0].size:] == 0x5A).all()
    b.close()


@pytest.mark.parametrize("what", ["quality a", "quality space", "quality 200", "base X", "base 0xC1"])
@pytest.mark.parametrize("where", ["cut", "kept"])
def test_bytes_that_cannot_be_judged(F, ctx, what, where):
    """in a line that is read a bad byte refuses the chunk, in the part that is cut as well; in a line that is not read it
    does not"""
    rng = np.random.default_rng(21)
    lens = [40, 150, 90, 17, 300] * 30
    raw, recs = chunk_of(rng.integers(2, 18, len(lens)), [plateau(rng, L, 3, 5) for L in lens], 22)
    raw = raw.copy()
    r = recs[77]
    in_seq = what.startswith("base")
    byte = {"quality a": ord("a"), "quality space": ord(" "), "quality 200": 200, "base X": ord("X"), "base 0xC1": 0xC1}[what]
    raw[int(r["seq_off"] if in_seq else r["qual_off"]) + (int(r["len"]) - 1 if where == "cut" else int(r["len"]) // 2)] = byte
    cuts = dict(cut_front=2, cut_tail=2)   # (the last symbol of the read is cut by it)
    reads_it = [(cuts, dict(max_n=3))] if in_seq else [(Q20, None), (dict(q_front=1), None), (cuts, dict(min_mean_q=1)), (cuts, dict(low_q=1, max_low_pct=100))]
    reads_it_not = [(cuts, None), (dict(crop=10), dict(min_len=5))] + ([(Q20, None), (cuts, dict(min_mean_q=20))] if in_seq else [(cuts, dict(max_n=0))])
    b = ctx.dblock(raw, recs)
    for t, f in reads_it:
        out = np.full(raw.size, 0x5A, dtype=np.uint8)
        keep = np.full((len(recs) + 7) // 8, 0xAA, dtype=np.uint8)
        win = np.full(len(recs), 0xAAAAAAAA, dtype=np.uint32)
        for o in (None, out):
            rc, n, report = raw_call(F, ctx, b, R.trm(**t), None if f is None else FR.flt(**f), o, out.size, keep, win)
            assert rc == E_ARG and n == 0 and not report.any() and not keep.any() and not win.any(), (what, t, f)
        assert (out == 0x5A).all()
        with pytest.raises(R.Refused):
            R.trim_records(raw, recs, R.trm(**t), None if f is None else FR.flt(**f))
    b.close()
    for t, f in reads_it_not:   # nothing reads that line: the byte is not looked at (and, where it is kept, copied)
        same(ctx, raw, recs, R.trm(**t), None if f is None else FR.flt(**f), "%s under %s %s" % (what, t, f))


# ---------------------------------------------------------------- 5. the chunk on the handle's staging block
def test_every_path_to_a_chunk_gives_one_output(F, golden_dir):
    raw, recs = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_1.fastq"))
    t, f = R.trm(cut_front=1, q_front=20, q_tail=20, crop=90), FR.flt(max_n=0, min_len=25)
    want = R.trim_records(raw, recs.astype(R.REC_DTYPE), t, f)
    assert 0 < want[1][R.N_KEPT] < len(recs)
    c = TS.context_for(F, raw, recs)
    fmt = TS.fmt_of(TS.first_header_of(raw))
    for table in (recs, None):
        alive, n = TF.begin(F, c, raw, table)
        holds(c.chunk_trim(t, n, f), want, "in flight")
        assert F.binding.lib().fqgpu_encode_cancel(c.h) == 0
    g = c.encode_raw(raw, flags=F.F_DECODE_INDEX, header_format=fmt)
    assert g["rc"] == 0 and g["headers_rc"] == 0
    holds(c.chunk_trim(t, len(recs), f), want, "behind fqgpu_encode_end")
    args = (fmt, g["header_fields"], g["readlens"], g["seq"], g["qual"], g["n_count"], g["n_pos"], g["used_len"])
    for what, kw in (("indexes", dict(index=g["index"])), ("no indexes", {})):
        d = c.decode_chunk(*args, **kw)
        assert d["rc"] == 0 and np.array_equal(d["raw"], raw)
        holds(c.chunk_trim(t, len(recs), f), want, "decoded, " + what)
    c.set_check_only(True)
    d = c.decode_chunk(*args, want_raw=False, index=g["index"])
    assert d["rc"] == 0 and d["raw"] is None
    holds(c.chunk_trim(t, len(recs), f), want, "check-only")
    c.set_check_only(False)
    b = c.dblock(raw, recs)
    holds(b.trim(t, f), want, "dblock")
    b.close()
    c.close()


def test_states_without_a_chunk(F, golden_dir):
    raw, recs = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_1.fastq"))
    c = TS.context_for(F, raw, recs)
    L = F.binding.lib()
    t = R.trm(**Q20)
    want = R.trim_records(raw, recs.astype(R.REC_DTYPE), t)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def refused(what):
        out = np.full(raw.size, 0x5A, dtype=np.uint8)
        n = C.c_size_t(77)
        report = np.full(R.REPORT_WORDS, 7, dtype=np.uint64)
        rc = L.fqgpu_chunk_trim(c.h, p(t), None, p(out), out.size, C.byref(n), p(report), None, None)
        assert rc == E_ARG and n.value == 0 and not report.any() and (out == 0x5A).all(), what
        assert c.chunk_filter(FR.flt(), len(recs))["rc"] == E_ARG, what + ": exactly where the filter is refused"

    refused("a fresh handle")
    fmt = TS.fmt_of(TS.first_header_of(raw))
    g = c.encode_raw(raw, flags=F.F_DECODE_INDEX, header_format=fmt)
    holds(c.chunk_trim(t, len(recs)), want, "behind an encode")
    args = (fmt, g["header_fields"], g["readlens"], g["seq"], g["qual"], g["n_count"], g["n_pos"], g["used_len"])
    assert c.decode_chunk_range(*args, 3, 40, index=g["index"])["rc"] == 0
    refused("after a range")
    assert c.decode_chunk(*args)["rc"] == 0
    holds(c.chunk_trim(t, len(recs)), want, "after a decode")
    alive, n = TF.begin(F, c, raw)
    holds(c.chunk_trim(t, n), want, "a chunk in flight")
    assert L.fqgpu_encode_cancel(c.h) == 0
    refused("after fqgpu_encode_cancel")
    c.close()


def test_digest_summary_and_filter_are_the_same_before_and_after(F, golden_dir):
    raw, recs = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_1.fastq"))
    t, tf = R.trm(**Q20), FR.flt(min_len=30)
    f = FR.flt(max_n=0, min_mean_q=18)
    want = R.trim_records(raw, recs.astype(R.REC_DTYPE), t, tf)
    want_f = FR.filter_records(raw, recs.astype(R.REC_DTYPE), f)
    crc, stats = (0, zlib.crc32(raw.tobytes()), raw.size), SR.stats_of(raw, recs, 64)
    c = TS.context_for(F, raw, recs)
    alive, n = TF.begin(F, c, raw)
    for s in "tcsftfttcsf":   # t: trim, f: a plain filter (between two trim calls too), c: digest, s: summary
        if s == "t":
            holds(c.chunk_trim(t, n, tf), want, "the trim")
        elif s == "f":
            g = c.chunk_filter(f, n)
            assert g["rc"] == 0 and g["out"].tobytes() == want_f[0].tobytes() and g["report"].tolist() == want_f[1].tolist() and g["keep"].tolist() == want_f[2].tolist()
        elif s == "c":
            assert c.chunk_crc32() == crc
        else:
            rc, got = c.chunk_stats(64)
            assert rc == 0 and np.array_equal(got, stats)
    assert F.binding.lib().fqgpu_encode_cancel(c.h) == 0
    b = c.dblock(raw, recs)
    before = (b.crc32(), b.stats(64), b.filter(f)["out"].tobytes())
    holds(b.trim(t, tf), want)
    assert b.crc32() == before[0] and np.array_equal(b.stats(64), before[1]) and b.filter(f)["out"].tobytes() == before[2]
    assert np.array_equal(b.fetch_raw(), raw)
    holds(b.trim(t, tf), want, "a filter call between two trim calls changes nothing")
    b.close()
    c.close()


def test_the_launches_are_timed_as_trim(F, golden_dir):
    raw, recs = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_1.fastq"))
    c = TS.context_for(F, raw, recs)
    b = c.dblock(raw, recs)
    c.enable_timing(True)
    t = R.trm(**Q20)
    size = b.trim(t, query=True)["out_len"]      # a size query: the judge
    _, groups = c.last_timing()
    assert [(name, calls) for name, _, calls in groups if name == "trim"] == [("trim", 1)], groups
    assert not [name for name, _, _ in groups if name == "filter"]
    assert size > 0 and b.trim(t, out_cap=size)["rc"] == 0      # with a buffer: the judge and the scan, then the gather
    _, groups = c.last_timing()
    assert [calls for name, _, calls in groups if name == "trim"] == [3], groups
    assert all(ms >= 0 for name, ms, _ in groups if name == "trim")
    b.close()
    c.close()


# ---------------------------------------------------------------- 6. filter and trim calls share one scratch on a handle
SHARED_COUNTS = (257, 1, 65)   # records of the chunks, in the order of the calls: the buffers grow, are far too large, then a little
SHARED_FILTER = dict(min_mean_q=25)


def shared_chunks():
    """per count a chunk with bare '+' lines and one whose '+' lines repeat the header, reads of at most 300 bases -> [(what, raw,
    recs, the filter's reference, the trim's reference)].  The inputs are checked here, on the host: the filter alone keeps some
    but not all reads of a chunk, the trim cuts at least one.  A chunk of ONE read cannot keep some and not all: its read is kept
    by the trim call, and by the filter alone in the bare chunk but not in the other (its low ends are cut first there), so
    that both the empty and the one-record output are met."""
    f, t = FR.flt(**SHARED_FILTER), R.trm(**Q20)
    chunks = []
    for n in SHARED_COUNTS:
        for repeats in (False, True):
            if n == 1:   # a clean plateau; a plateau between two low ends that pull the mean of the whole read below the level
                rng = np.random.default_rng(40 + repeats)
                raw, recs = chunk_of([9], [plateau(rng, 300, 100, 60) if repeats else plateau(rng, 299, 0, 5)], 42, plus_repeats=repeats)
            else:
                raw, recs = drawn(np.random.default_rng(30 + n + repeats).integers(3, 301, n), 50 + n + repeats, plus_repeats=repeats)
            what = "%d records, %s" % (n, "'+' lines repeat the header" if repeats else "bare '+' lines")
            want_f, want_t = FR.filter_records(raw, recs, f), R.trim_records(raw, recs, t, f)
            kept_f, kept_t = int(want_f[1][FR.N_KEPT]), int(want_t[1][R.N_KEPT])
            assert int(recs["len"].max()) <= 300 and len(recs) == n, what
            assert int(want_t[1][R.READS_TRIMMED]) >= 1 and 0 < kept_t, what + ": the trim cuts nothing or nothing is left: a vacuous input"
            assert (0 < kept_f < n and kept_t < n) if n > 1 else kept_f == (0 if repeats else 1), what + ": the filter keeps all or nothing: a vacuous input"
            chunks.append((what, raw, recs, want_f, want_t))
    return chunks


def test_filter_and_trim_calls_in_turn_on_one_handle(F, ctx):
    """one SelectScratch and one driver serve both calls: whatever a call leaves behind -- windows, flags of a refused chunk,
    buffers sized for a larger chunk -- the next call's result is the reference's"""
    f, t = FR.flt(**SHARED_FILTER), R.trm(**Q20)

    def filter_holds(g, want, what):
        assert g["rc"] == 0, (what, g["rc"])
        assert g["report"].tolist() == want[1].tolist() and g["keep"].tolist() == want[2].tolist(), what
        assert g["out_len"] == want[0].size and g["out"].tobytes() == want[0].tobytes(), what

    for what, raw, recs, want_f, want_t in shared_chunks():
        spoilt = raw.copy()
        r = recs[len(recs) // 2]
        spoilt[int(r["qual_off"]) + int(r["len"]) // 2] = 200
        b, bad = ctx.dblock(raw, recs), ctx.dblock(spoilt, recs)
        first = b.filter(f)
        filter_holds(first, want_f, what + ": the filter")
        holds(b.trim(t, f), want_t, what + ": the trim behind a filter")
        again = b.filter(f)
        filter_holds(again, want_f, what + ": the filter behind a trim")
        keep = np.full((len(recs) + 7) // 8, 0xAA, dtype=np.uint8)
        win = np.full(len(recs), 0xAAAAAAAA, dtype=np.uint32)
        out = np.full(raw.size, 0x5A, dtype=np.uint8)
        rc, n, report = raw_call(F, ctx, bad, t, f, out, out.size, keep, win)
        assert rc == E_ARG and n == 0 and not report.any() and not keep.any() and not win.any() and (out == 0x5A).all(), what + ": a quality byte of 200"
        last = b.filter(f)
        filter_holds(last, want_f, what + ": the filter behind a refused call")
        for g in (again, last):
            assert all(np.array_equal(g[k], first[k]) for k in ("out", "report", "keep")) and g["out_len"] == first["out_len"], what
        holds(b.trim(t, f), want_t, what + ": the trim behind all of them")
        b.close()
        bad.close()
