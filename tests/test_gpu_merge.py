"""The mate merge on the device (k_merge_size and k_merge_emit in fqcomp28_amd/csrc/pair.hip, behind fqgpu_*_pair_merge) against
the restatement in merge_ref.py: the merged bytes, *out_len, all sixteen report words and the merged bits, for equality; what
is refused leaves `out` untouched and everything else zeroed; both chunks stay as they were.  Integer arithmetic: there is no
tolerance.  Small synthetic chunks: a test takes a few seconds."""
import os
import zlib

import numpy as np
import pytest

import merge_ref as MR
import oracle_lib as O
import overlap_ref as OR
import pair_ref as PR
import test_gpu_stats as TS

pytestmark = pytest.mark.gpu

E_ARG, E_OVERFLOW = -4, -1
# (a line of fewer than 3 bases cannot reach the device -- creating a block refuses it --, so 3 stands for the shortest line;
# test_merge_host.py has shorter ones against the reference)
SIZES = (3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 511, 512)
HEADS = (2, 15, 16, 17, 127, 128, 129, 300)   # bytes of a header line with its '\n'
# Phred values either side of every comparison: equal ones, differences below, at and above a floor of 2, both ends of the range
LEVELS = np.array([0, 1, 2, 3, 20, 21, 22, 23, 40, 62, 63], dtype=np.uint8) + 33
FILL = 0xAB


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
def golden_inserts(golden):
    (raw1, recs1), (raw2, recs2) = golden
    return OR.overlap_records(raw1, recs1, 0, raw2, recs2, 0, len(recs1), OR.spec())[3]


def chunk(seqs, quals, names, plus=None):
    """a FASTQ chunk -> (raw uint8, recs); names: the header lines' text behind the '@'; plus: per record the text behind its
    '+' (None: bare)"""
    parts, recs, at = [], np.zeros(len(seqs), dtype=PR.REC_DTYPE), 0
    for i, (s, q) in enumerate(zip(seqs, quals)):
        head, mid = b"@" + names[i] + b"\n", b"\n+" + (plus[i] if plus else b"") + b"\n"
        assert len(q) == len(s)
        recs[i] = (at + len(head), at + len(head) + len(s) + len(mid), len(s))
        parts += [head, bytes(s), mid, bytes(q), b"\n"]
        at += len(head) + 2 * len(s) + len(mid) + 1
    return np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), recs


def differs(what, name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.size != want.size:
        raise AssertionError("%s: %s has %d entries, expected %d" % (what, name, got.size, want.size))
    if not np.array_equal(got, want):
        at = int(np.flatnonzero(got != want)[0])
        raise AssertionError("%s: %s differs, first at %d: %d, expected %d" % (what, name, at, got[at], want[at]))


def holds(g, want, what):
    out, report, merged = want
    assert g["rc"] == 0, (what, g["rc"])
    differs(what, "the report", g["report"], report)
    assert g["out_len"] == out.size, (what, g["out_len"], out.size)
    if g["merged"] is not None:
        differs(what, "merged_out", g["merged"], merged)
    if g["out"] is not None:
        differs(what, "the merged bytes", g["out"], out)


def same(ctx, raw1, recs1, first_a, raw2, recs2, first_b, count, ins, mark=None, spec=None, what="", blocks=None, **kw):
    """two blocks (fresh ones, or the caller's) merged on the device: everything the call gives back is the reference's -> its
    result"""
    spec = MR.spec() if spec is None else spec
    want = MR.merge_records(raw1, recs1, first_a, raw2, recs2, first_b, count, ins, mark, spec)
    b1, b2 = blocks if blocks else (ctx.dblock(raw1, recs1), ctx.dblock(raw2, recs2))
    g = b1.pair_merge(first_a, b2, first_b, count, ins, mark, spec, **kw)
    if not blocks:
        b1.close()
        b2.close()
    holds(g, want, what)
    return want


def refused(ctx, raw1, recs1, first_a, raw2, recs2, first_b, count, ins, mark, spec, what):
    """the reference refuses it; the call says FQGPU_E_ARG, leaves `out` untouched and zeroes what else it gives back"""
    with pytest.raises(MR.Refused):
        MR.merge_records(raw1, recs1, first_a, raw2, recs2, first_b, count, ins, mark, spec)
    b1, b2 = ctx.dblock(raw1, recs1), ctx.dblock(raw2, recs2)
    out = np.full(raw1.size + raw2.size, FILL, dtype=np.uint8)
    g = b1.pair_merge(first_a, b2, first_b, count, ins, mark, spec, out=out)
    b1.close()
    b2.close()
    assert g["rc"] == E_ARG and g["out_len"] == 0 and not g["report"].any() and not g["merged"].any(), (what, g["rc"], g["out_len"])
    assert (out == FILL).all(), what + ": a refused call wrote to out"


# ---------------------------------------------------------------- 1. the fixture, both call forms
def test_the_fixture_in_both_call_forms(F, ctx, golden, golden_inserts):
    (raw1, recs1), (raw2, recs2) = golden
    n, ins = len(recs1), golden_inserts
    b1, b2 = ctx.dblock(raw1, recs1), ctx.dblock(raw2, recs2)
    blocks = (b1, b2)
    before = [(b.crc32(True), b.select_marked(0, n)["out"].tobytes()) for b in blocks]
    out, report, merged = same(ctx, raw1, recs1, 0, raw2, recs2, 0, n, ins, what="two blocks", blocks=blocks)
    assert report.tolist() == [1000, 111, 111, 12767, 32590, 7011, 159, 10, 1211, 1211, 0, 0, 0, 0, 0, 0] and zlib.crc32(out.tobytes()) == 3403808527
    same(ctx, raw1, recs1, 100, raw2, recs2, 100, 777, ins[100:877], what="a range", blocks=blocks)
    # the mark: none, all ones, all zeros, alternating
    ones, zeros = np.full(125, 0xFF, dtype=np.uint8), np.zeros(125, dtype=np.uint8)
    assert same(ctx, raw1, recs1, 0, raw2, recs2, 0, n, ins, ones, what="all ones", blocks=blocks)[0].tobytes() == out.tobytes()
    none = same(ctx, raw1, recs1, 0, raw2, recs2, 0, n, ins, zeros, what="all zeros", blocks=blocks)
    assert none[0].size == 0 and none[1].tolist() == [1000, 111, 0, 0, 0, 0, 0, 0, 0, 0, 111, 0, 0, 0, 0, 0]
    for byte in (0x55, 0xAA):
        half = same(ctx, raw1, recs1, 0, raw2, recs2, 0, n, ins, np.full(125, byte, dtype=np.uint8), what="alternating", blocks=blocks)
        assert 0 < int(half[1][MR.PAIRS_MERGED]) < 111
    same(ctx, raw1, recs1, 37, raw2, recs2, 37, 900, ins[37:937], np.full(113, 0x6D, dtype=np.uint8), what="a range with a mark", blocks=blocks)
    same(ctx, raw1, recs1, 0, raw2, recs2, 0, n, ins, None, MR.spec(0, 100), what="min_len 100, floor 0", blocks=blocks)
    # merged_out NULL; out NULL; the report and the length left out
    g = b1.pair_merge(0, b2, 0, n, ins, None, MR.spec(), want_merged=False)
    assert g["merged"] is None
    holds(g, (out, report, merged), "merged_out NULL")
    g = b1.pair_merge(0, b2, 0, n, ins, None, MR.spec(), want_out=False)
    assert g["out"] is None
    holds(g, (out, report, merged), "out NULL")
    for kw in (dict(want_report=False), dict(want_len=False)):
        g = b1.pair_merge(0, b2, 0, n, ins, None, MR.spec(), cap=out.size, **kw)
        assert g["rc"] == E_ARG and not g["merged"].any() and not g["out"].any(), kw
    # a byte too little: FQGPU_E_OVERFLOW, nothing written, everything else valid; exactly enough is enough
    small = np.full(out.size, FILL, dtype=np.uint8)
    g = b1.pair_merge(0, b2, 0, n, ins, None, MR.spec(), out=small, cap=out.size - 1)
    assert g["rc"] == E_OVERFLOW and g["out_len"] == out.size and (small == FILL).all()
    differs("out_cap = out_len - 1", "the report", g["report"], report)
    differs("out_cap = out_len - 1", "merged_out", g["merged"], merged)
    holds(b1.pair_merge(0, b2, 0, n, ins, None, MR.spec(), out=small), (out, report, merged), "out_cap = out_len")
    # the same block on both sides is allowed: nothing is patched (mate 1's records 0 .. 499 beside its records 500 .. 999)
    self_ins = np.where(np.arange(500) % 3 == 0, 57, 0).astype(np.uint16)
    same(ctx, raw1, recs1, 0, raw1, recs1, 500, 500, self_ins, what="ba == bb", blocks=(b1, b1))
    # first_a != first_b: mate 2's chunk cut in front of its record 5
    cut = int(PR.header_starts(recs2)[5])
    tail2 = recs2[5:].copy()
    tail2["seq_off"] -= cut
    tail2["qual_off"] -= cut
    part = same(ctx, raw1, recs1, 5, raw2[cut:].copy(), tail2, 0, n - 5, ins[5:], what="first_a 5, first_b 0")
    assert part[0].tobytes() == out.tobytes() or ins[:5].any()
    # both blocks are what they were
    assert [(b.crc32(True), b.select_marked(0, n)["out"].tobytes()) for b in blocks] == before
    assert b1.fetch(raw=True)["raw"].tobytes() == raw1.tobytes() and b2.fetch(raw=True)["raw"].tobytes() == raw2.tobytes()
    b1.close()
    b2.close()
    # the chunks staged on two handles, and on one
    c1, c2 = TS.context_for(F, raw1, recs1), TS.context_for(F, raw2, recs2)
    assert c1.chunk_pair_merge(0, c2, 0, n, ins, None, MR.spec(), cap=out.size)["rc"] == E_ARG, "no chunk on either handle"
    assert c1.encode_raw(raw1)["rc"] == 0 == c2.encode_raw(raw2)["rc"]
    digests = [(c.chunk_crc32(), c.chunk_select_marked(0, n)["out"].tobytes()) for c in (c1, c2)]
    for first_a, first_b, count in ((0, 0, 0), (0, 0, n + 1), (n, 0, 1), (1, 0, n), (0, 1, n)):
        r = c1.chunk_pair_merge(first_a, c2, first_b, count, ins, None, MR.spec(), cap=out.size)
        assert r["rc"] == E_ARG and r["out_len"] == 0 and not r["report"].any() and not r["merged"].any() and not r["out"].any(), (first_a, first_b, count)
    assert c1.chunk_pair_merge(0, None, 0, n, ins, None, MR.spec(), cap=out.size)["rc"] == E_ARG
    holds(c1.chunk_pair_merge(0, c2, 0, n, ins, None, MR.spec()), (out, report, merged), "two staged chunks")
    holds(c1.chunk_pair_merge(100, c2, 100, 777, ins[100:877], None, MR.spec()),
          MR.merge_records(raw1, recs1, 100, raw2, recs2, 100, 777, ins[100:877], None, MR.spec()), "a range of two staged chunks")
    holds(c1.chunk_pair_merge(0, c1, 500, 500, self_ins, None, MR.spec()),
          MR.merge_records(raw1, recs1, 0, raw1, recs1, 500, 500, self_ins, None, MR.spec()), "ctx_a == ctx_b")
    assert [(c.chunk_crc32(), c.chunk_select_marked(0, n)["out"].tobytes()) for c in (c1, c2)] == digests, "digest and selection are what they were"
    c1.close()
    c2.close()


# ---------------------------------------------------------------- 2. synthetic pairs at the edges where the kernel can go wrong
def shapes():
    """Every length of SIZES on either side, each pair with the inserts that put it at an edge: I = 1, I below L2 (d < 0),
    I = L2 (d = 0), I below L1, I = L1, one in between and I = L1 + L2 - 1 (one place of overlap; 1023 from 512 + 512).  The
    inserts are the caller's data, so the lines are random and unrelated -- a place agrees one time in four, and one base in
    thirteen is N -- with qualities either side of every comparison.  The header lines take the lengths of HEADS in turn --
    the first is "@\\n", so mate 2's first line starts two bytes into its chunk --, and mate 2's records have text behind
    their '+' -> (raw1, recs1, raw2, recs2, inserts)"""
    rng = np.random.default_rng(29)
    acgtn = np.frombuffer(b"ACGTACGTACGTN", dtype=np.uint8)
    line = lambda k: acgtn[rng.integers(0, acgtn.size, k)].tobytes()      # noqa: E731
    qual = lambda k: LEVELS[rng.integers(0, LEVELS.size, k)].tobytes()    # noqa: E731
    seqs1, seqs2, q1, q2, ins = [], [], [], [], []
    for L1 in SIZES:
        for L2 in SIZES:
            for I in sorted({1, L2 - 1, L2, L1 - 1, L1, (L1 + L2) // 2, L1 + L2 - 1}):
                if 1 <= I <= L1 + L2 - 1:
                    seqs1.append(line(L1)), q1.append(qual(L1)), seqs2.append(line(L2)), q2.append(qual(L2)), ins.append(I)
    names = [(b"name %d " % i + b"x" * 300)[:HEADS[i % len(HEADS)] - 2] for i in range(len(ins))]
    raw1, recs1 = chunk(seqs1, q1, names)
    raw2, recs2 = chunk(seqs2, q2, names, plus=[n for n in names])
    return raw1, recs1, raw2, recs2, np.array(ins, dtype=np.uint16)


@pytest.fixture(scope="module")
def shaped():
    return shapes()


def test_the_smallest_shapes(F, ctx, shaped):
    raw1, recs1, raw2, recs2, ins = shaped
    n = len(ins)
    assert int(recs1["seq_off"][0]) == 2 == int(recs2["seq_off"][0]) and n > 4 * 64 and int(ins.max()) == 1023
    b1, b2 = ctx.dblock(raw1, recs1), ctx.dblock(raw2, recs2)
    blocks = (b1, b2)
    out, report, merged = same(ctx, raw1, recs1, 0, raw2, recs2, 0, n, ins, what="every shape", blocks=blocks)
    assert int(report[MR.PAIRS_MERGED]) == n and min(int(report[w]) for w in (MR.OVERLAP_BASES, MR.PLACES_DISAGREE, MR.PLACES_N, MR.DROPPED_A, MR.DROPPED_B)) > 100
    assert out.size > 64 * 4096, "many tiles of the emit pass"
    for floor_q in (0, 63):
        same(ctx, raw1, recs1, 0, raw2, recs2, 0, n, ins, None, MR.spec(floor_q), what="floor_q %d" % floor_q, blocks=blocks)
    # ranges of 1, 63, 64, 65 and 129 pairs, the first and the last record of the chunks among them
    for first, count in ((0, 1), (0, 63), (1, 64), (64, 65), (n - 129, 129), (n - 1, 1)):
        same(ctx, raw1, recs1, first, raw2, recs2, first, count, ins[first:first + count], what="[%d, +%d)" % (first, count), blocks=blocks)
    # a mark and a min_len over them: unmerged pairs between the merged ones
    mark = np.random.default_rng(5).integers(0, 256, (n + 7) // 8).astype(np.uint8)
    part = same(ctx, raw1, recs1, 0, raw2, recs2, 0, n, ins, mark, MR.spec(2, 16), what="a mark and min_len 16", blocks=blocks)[1]
    assert min(int(part[w]) for w in (MR.PAIRS_MERGED, MR.PAIRS_UNMARKED, MR.PAIRS_TOO_SHORT)) > 20
    # inserts all zero: nothing is merged and nothing is looked at
    assert same(ctx, raw1, recs1, 0, raw2, recs2, 0, n, np.zeros(n, dtype=np.uint16), what="no inserts", blocks=blocks)[1].tolist() == [n] + [0] * 15
    b1.close()
    b2.close()


def test_the_edges_of_either_mate_on_and_beside_a_word_of_the_output(F, ctx):
    """One pair to a call, so the record starts at byte 0 of the output and place p of the bases is byte hl + p: with a header
    line of 16 bytes mate 1 ends (p = L1) and mate 2 begins (p = I - L2) on and beside the multiples of 16, and the qualities,
    which start at hl + I + 3, meet every alignment as I moves"""
    rng = np.random.default_rng(31)
    acgtn = np.frombuffer(b"ACGTACGTACGTN", dtype=np.uint8)
    seqs1, seqs2, q1, q2, ins = [], [], [], [], []
    for L1 in (15, 16, 17, 31, 32, 33, 48):
        for L2 in (16, 33):
            for d in (0, 1, 15, 16, 17, 31, 32, 33):
                if d + L2 <= L1 + L2 - 1:
                    seqs1.append(acgtn[rng.integers(0, 13, L1)].tobytes()), q1.append(LEVELS[rng.integers(0, LEVELS.size, L1)].tobytes())
                    seqs2.append(acgtn[rng.integers(0, 13, L2)].tobytes()), q2.append(LEVELS[rng.integers(0, LEVELS.size, L2)].tobytes())
                    ins.append(d + L2)
    names = [(b"edge pair %04d......" % i)[:14] for i in range(len(ins))]
    raw1, recs1 = chunk(seqs1, q1, names)
    raw2, recs2 = chunk(seqs2, q2, names)
    assert int(recs1["seq_off"][0]) == 16 and len(ins) > 60
    ins = np.array(ins, dtype=np.uint16)
    blocks = (ctx.dblock(raw1, recs1), ctx.dblock(raw2, recs2))
    for i in range(len(ins)):
        same(ctx, raw1, recs1, i, raw2, recs2, i, 1, ins[i:i + 1], what="pair %d: L1 %d, L2 %d, I %d" % (i, len(seqs1[i]), len(seqs2[i]), ins[i]), blocks=blocks)
    same(ctx, raw1, recs1, 0, raw2, recs2, 0, len(ins), ins, what="all of them", blocks=blocks)
    for b in blocks:
        b.close()


def test_min_len_at_either_side_of_the_insert(F, ctx):
    s = (b"ACGGTCATTGCAGGATCCTAAGCTTGACCGTATGCAATCG" * 2)[:70]
    n = 130
    raw1, recs1 = OR.chunk([s] * n)
    raw2, recs2 = OR.chunk([OR.revcomp(s)] * n)
    ins = np.where(np.arange(n) % 2 == 0, 70, 50).astype(np.uint16)
    blocks = (ctx.dblock(raw1, recs1), ctx.dblock(raw2, recs2))
    for min_len, merged in ((49, n), (50, n), (51, n // 2), (69, n // 2), (70, n // 2), (71, 0), (1023, 0)):
        report = same(ctx, raw1, recs1, 0, raw2, recs2, 0, n, ins, None, MR.spec(2, min_len), what="min_len %d" % min_len, blocks=blocks)[1]
        assert (int(report[MR.PAIRS_MERGED]), int(report[MR.PAIRS_TOO_SHORT])) == (merged, n - merged)
    for b in blocks:
        b.close()


# ---------------------------------------------------------------- 3. what is refused leaves out untouched and the rest zeroed
X, RX, Q = b"ACGTACGTAC", b"GTACGTACGT", b"I" * 10


def put(s, at, c):
    return s[:at] + c + s[at + 1:]


def test_refusals_from_the_last_pair_of_a_call_whose_first_pair_merges(F, ctx):
    long1 = (b"ACGGTCATTGCAGGATCCTAAGCTTGACCGTATGCAATCG" * 13)[:513]
    k = 130   # pairs in front of the one in question: more than two waves, and several words of output

    def chunks(s1, q1, s2, q2):
        raw1, recs1 = OR.chunk([X] * k + [s1], [Q] * k + [q1])
        raw2, recs2 = OR.chunk([RX] * k + [s2], [Q] * k + [q2])
        return raw1, recs1, raw2, recs2

    def inserts(I):
        return np.array([10] * k + [I], dtype=np.uint16)

    n, spec = k + 1, MR.spec()
    last_off = np.zeros((n + 7) // 8, dtype=np.uint8) + 0xFF
    last_off[k // 8] &= ~(1 << (k % 8)) & 0xFF
    raw1, recs1, raw2, recs2 = chunks(X, Q, RX, Q)
    whole = same(ctx, raw1, recs1, 0, raw2, recs2, 0, n, inserts(10), what="the chunks as they are")[1].tolist()
    assert whole[:4] == [n, n, n, 10 * n] and whole[5:8] == [10 * n, 0, 0]
    for I in (20, 21, 600, 65535):
        refused(ctx, raw1, recs1, 0, raw2, recs2, 0, n, inserts(I), None, spec, "I = %d >= L1 + L2" % I)
        refused(ctx, raw1, recs1, 0, raw2, recs2, 0, n, inserts(I), last_off, spec, "I = %d on an unmarked pair" % I)
        refused(ctx, raw1, recs1, 0, raw2, recs2, 0, n, inserts(I), None, MR.spec(2, 1023), "I = %d on a pair too short" % I)
    assert int(same(ctx, raw1, recs1, 0, raw2, recs2, 0, n, inserts(19), what="I = L1 + L2 - 1")[1][MR.OVERLAP_BASES]) == 10 * k + 1
    for what, pair, I in (
        ("513 bases in mate 1", (long1, b"I" * 513, RX, Q), 10), ("513 bases in mate 2", (X, Q, long1, b"I" * 513), 513),
        ("an x in the read region, mate 1", (put(X, 9, b"x"), Q, RX, Q), 10), ("an x in the read region, mate 2", (X, Q, put(RX, 0, b"x"), Q), 10),
        ("an x where mate 1 stands alone", (put(X, 0, b"x"), Q, RX, Q), 14), ("an x where mate 2 stands alone", (X, Q, put(RX, 0, b"x"), Q), 14),
        ("a byte above 127", (X, Q, put(RX, 5, b"\xc1"), Q), 10),
        ("a quality byte 32, mate 1", (X, put(Q, 0, b" "), RX, Q), 10), ("a quality byte 32, mate 2", (X, Q, RX, put(Q, 9, b" ")), 10),
        ("a quality byte 97, mate 1", (X, put(Q, 9, b"a"), RX, Q), 10), ("a quality byte 97, mate 2", (X, Q, RX, put(Q, 0, b"a")), 10),
        ("a quality byte 97 where mate 2 stands alone", (X, Q, RX, put(Q, 1, b"a")), 14), ("a quality byte 255", (X, put(Q, 4, b"\xff"), RX, Q), 10),
    ):
        r1, t1, r2, t2 = chunks(*pair)
        refused(ctx, r1, t1, 0, r2, t2, 0, n, inserts(I), None, spec, what)
        if "513" not in what:   # ... and accepted in a pair that is not merged: without an insert, unmarked, too short
            assert same(ctx, r1, t1, 0, r2, t2, 0, n, inserts(0), what=what + ", no insert")[1].tolist()[:3] == [n, k, k]
            assert same(ctx, r1, t1, 0, r2, t2, 0, n, inserts(I), last_off, what=what + ", unmarked")[1].tolist()[:3] == [n, n, k]
        else:
            assert same(ctx, r1, t1, 0, r2, t2, 0, n, inserts(0), what=what + ", no insert")[1].tolist()[:3] == [n, k, k]
            refused(ctx, r1, t1, 0, r2, t2, 0, n, inserts(I), last_off, spec, what + ": the inserts are judged on an unmarked pair too")
    # the same bad bytes just outside the read region are accepted: behind min(L, I)
    r1, t1, r2, t2 = chunks(b"ACGTACxxxx", b"IIIIII \x7f a", b"GTACGTzzzz", b"IIIIII a\xff ")
    assert same(ctx, r1, t1, 0, r2, t2, 0, n, inserts(6), what="odd bytes behind I")[1].tolist()[:4] == [n, n, n, 10 * k + 6]
    # the arguments
    for first_a, first_b, count in ((0, 0, 0), (0, 0, n + 1), (n, 0, 1), (1, 0, n), (0, 1, n)):
        refused(ctx, raw1, recs1, first_a, raw2, recs2, first_b, count, inserts(10), None, spec, "the range %r" % ((first_a, first_b, count),))
    for bad in (None, MR.spec(64, 1), MR.spec(2, 0), MR.spec(2, 1024), MR.spec(reserved=(1, 0, 0, 0, 0, 0))):
        refused(ctx, raw1, recs1, 0, raw2, recs2, 0, n, inserts(10), None, bad, "the spec %r" % (bad,))
    refused(ctx, raw1, recs1, 0, raw2, recs2, 0, n, None, None, spec, "no inserts")
    b1 = ctx.dblock(raw1, recs1)
    g = b1.pair_merge(0, None, 0, n, inserts(10), None, spec, cap=64)
    assert g["rc"] == E_ARG and not g["report"].any() and not g["merged"].any() and g["out_len"] == 0, "no second block"
    b1.close()


# ---------------------------------------------------------------- 4. nothing depends on what the scratch held
def test_the_same_answer_whatever_the_scratch_held(F, golden, golden_inserts):
    (raw1, recs1), (raw2, recs2) = golden
    n = len(recs1)
    c1, c2 = TS.context_for(F, raw1, recs1), TS.context_for(F, raw2, recs2)
    mark = np.full(113, 0xB7, dtype=np.uint8)

    def calls():
        assert c1.encode_raw(raw1)["rc"] == 0 == c2.encode_raw(raw2)["rc"]   # (staged afresh: filling the scratch ends a staged chunk)
        g = c1.chunk_pair_merge(0, c2, 0, n, golden_inserts, None, MR.spec())
        part = c1.chunk_pair_merge(37, c2, 37, 900, golden_inserts[37:937], mark, MR.spec(0, 60))
        assert g["rc"] == 0 == part["rc"]
        return (g["out"].tobytes(), g["report"].tolist(), g["merged"].tolist(), part["out"].tobytes(), part["report"].tolist(), part["merged"].tolist())

    first = calls()
    assert first[1][:5] == [1000, 111, 111, 12767, 32590] and 0 < first[4][2] < 111
    for c in (c1, c2):
        buffers, filled = c.fill_scratch(0xFF)
        assert buffers > 0 and filled > 0
    assert calls() == first
    for c in (c1, c2):
        c.fill_scratch(0x00)
    assert calls() == first
    c1.close()
    c2.close()
