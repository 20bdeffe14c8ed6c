"""The overlap correction on the device (k_pair_correct in fqcomp28_amd/csrc/pair.hip, behind fqgpu_*_pair_correct) against
the restatement in correct_ref.py: the eight report words, the two per-pair arrays and BOTH chunks' whole raw bytes fetched
back -- header lines, '+' lines and every untouched read included -- for equality; what is refused leaves both chunks as they
were.  Integer arithmetic: there is no tolerance."""
import os
import zlib

import numpy as np
import pytest

import correct_ref as CR
import oracle_lib as O
import overlap_ref as OR
import pair_ref as PR
import test_gpu_overlap as TGO
import test_gpu_stats as TS

pytestmark = pytest.mark.gpu

E_ARG = -4
# (a line of fewer than 3 bases cannot reach the device -- creating a block or staging a chunk refuses it with
# FQGPU_E_SHORT_READ --, so 3 stands for the shortest line; test_correct_host.py has lines of 1 base against the reference)
SIZES = (3, 7, 8, 9, 63, 64, 65, 511, 512)
LEVELS = np.array([0, 14, 15, 29, 30, 41], dtype=np.uint8) + 33   # the Phred values either side of both bounds, as bytes


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


def same(ctx, raw1, recs1, first_a, raw2, recs2, first_b, count, ins, spec=None, what=""):
    """two fresh blocks corrected on the device: the report, both arrays and both whole raws are the reference's -> its result"""
    spec = CR.spec() if spec is None else spec
    want_a, want_b, report, fa, fb = CR.correct_records(raw1, recs1, first_a, raw2, recs2, first_b, count, ins, spec)
    b1, b2 = ctx.dblock(raw1, recs1), ctx.dblock(raw2, recs2)
    g = b1.pair_correct(first_a, b2, first_b, count, ins, spec)
    got_a, got_b = b1.fetch(raw=True)["raw"], b2.fetch(raw=True)["raw"]
    b1.close()
    b2.close()
    assert g["rc"] == 0, (what, g["rc"])
    assert g["report"].tolist() == report.tolist(), what
    for name, got, want in (("fixed_a", g["fixed_a"], fa), ("fixed_b", g["fixed_b"], fb)):
        if not np.array_equal(got, want):
            at = int(np.flatnonzero(got != want)[0])
            raise AssertionError("%s: %s differs, first at pair %d: %d, expected %d" % (what, name, at, got[at], want[at]))
    for name, got, want in (("mate 1", got_a, want_a), ("mate 2", got_b, want_b)):
        if got.tobytes() != want.tobytes():
            raise AssertionError("%s: the raw bytes of %s differ, first at byte %d" % (what, name, int(np.flatnonzero(got != want)[0])))
    return want_a, want_b, report, fa, fb


def refused(ctx, raw1, recs1, first_a, raw2, recs2, first_b, count, ins, spec, what):
    """the reference refuses it; the call says FQGPU_E_ARG, zeroes what it gives back and leaves both blocks' raws as they were"""
    with pytest.raises(CR.Refused):
        CR.correct_records(raw1, recs1, first_a, raw2, recs2, first_b, count, ins, spec)
    b1, b2 = ctx.dblock(raw1, recs1), ctx.dblock(raw2, recs2)
    g = b1.pair_correct(first_a, b2, first_b, count, ins, spec)
    got_a, got_b = b1.fetch(raw=True)["raw"], b2.fetch(raw=True)["raw"]
    b1.close()
    b2.close()
    assert g["rc"] == E_ARG and not g["report"].any() and not g["fixed_a"].any() and not g["fixed_b"].any(), (what, g["rc"])
    assert got_a.tobytes() == np.asarray(raw1).tobytes() and got_b.tobytes() == np.asarray(raw2).tobytes(), what + ": a refused call changed a chunk"


# ---------------------------------------------------------------- 1. the fixture, both call forms
def test_the_fixture_in_both_call_forms(F, ctx, golden, golden_inserts):
    (raw1, recs1), (raw2, recs2) = golden
    n, ins = len(recs1), golden_inserts
    want_a, want_b, report, fa, fb = same(ctx, raw1, recs1, 0, raw2, recs2, 0, n, ins, what="two blocks")
    assert report.tolist()[:5] == [1000, 111, 36, 34, 28] and report.tolist()[6:] == [169, 7011]
    assert int((want_a != raw1).sum()) == 68 and int((want_b != raw2).sum()) == 56
    # first_a != first_b: mate 2's chunk cut in front of its record 5
    cut = int(PR.header_starts(recs2)[5])
    tail2 = recs2[5:].copy()
    tail2["seq_off"] -= cut
    tail2["qual_off"] -= cut
    part = same(ctx, raw1, recs1, 5, raw2[cut:], tail2, 0, n - 5, ins[5:], what="first_a 5, first_b 0")
    assert part[0].tobytes() == want_a.tobytes() or ins[:5].any()
    same(ctx, raw1, recs1, 100, raw2, recs2, 100, 777, ins[100:877], what="a range")
    # the arrays left out
    b1, b2 = ctx.dblock(raw1, recs1), ctx.dblock(raw2, recs2)
    q = b1.pair_correct(0, b2, 0, n, ins, CR.spec(), want_arrays=False)
    assert q["rc"] == 0 and q["report"].tolist() == report.tolist() and q["fixed_a"] is None
    assert b1.fetch(raw=True)["raw"].tobytes() == want_a.tobytes() and b2.fetch(raw=True)["raw"].tobytes() == want_b.tobytes()
    b1.close()
    b2.close()
    # the chunks staged on two handles: every call afterwards sees the corrected bytes
    c1, c2 = TS.context_for(F, raw1, recs1), TS.context_for(F, raw2, recs2)
    assert c1.chunk_pair_correct(0, c2, 0, n, ins, CR.spec())["rc"] == E_ARG, "no chunk on either handle"
    assert c1.encode_raw(raw1)["rc"] == 0 == c2.encode_raw(raw2)["rc"]
    for first_a, first_b, count in ((0, 0, 0), (0, 0, n + 1), (n, 0, 1), (1, 0, n), (0, 1, n)):
        r = c1.chunk_pair_correct(first_a, c2, first_b, count, ins, CR.spec())
        assert r["rc"] == E_ARG and not r["report"].any(), (first_a, first_b, count)
    assert c1.chunk_pair_correct(0, c1, 0, n, ins, CR.spec())["rc"] == E_ARG, "the same handle on both sides"
    assert c1.chunk_pair_correct(0, None, 0, n, ins, CR.spec())["rc"] == E_ARG
    before = [c.chunk_select_marked(0, n) for c in (c1, c2)]
    assert before[0]["out"].tobytes() == PR.marked_records(raw1, recs1, 0, n)[0].tobytes(), "the refused calls changed nothing"
    assert before[1]["out"].tobytes() == PR.marked_records(raw2, recs2, 0, n)[0].tobytes()
    g = c1.chunk_pair_correct(0, c2, 0, n, ins, CR.spec())
    assert g["rc"] == 0 and g["report"].tolist() == report.tolist() and np.array_equal(g["fixed_a"], fa) and np.array_equal(g["fixed_b"], fb)
    for c, want, recs in ((c1, want_a, recs1), (c2, want_b, recs2)):
        canonical = PR.marked_records(want, recs, 0, n)[0].tobytes()
        s = c.chunk_select_marked(0, n)
        assert s["rc"] == 0 and s["out"].tobytes() == canonical
        assert c.chunk_crc32() == (0, zlib.crc32(canonical), len(canonical))
    again = c1.chunk_pair_correct(0, c2, 0, n, ins, CR.spec())
    assert again["rc"] == 0 and again["report"].tolist() == [1000, 111, 0, 0, 0, 0, 169 - 62, 7011]
    c1.close()
    c2.close()


# ---------------------------------------------------------------- 2. synthetic pairs: every length, every kind of fragment
@pytest.fixture(scope="module")
def synth():
    """test_gpu_overlap's synthetic pairs with random qualities over 0 .. 41, mate 2's chunk with three records of its own in
    front, and the reference's inserts"""
    seqs1, seqs2 = TGO.synthetic_pairs()
    seqs2 = [b"ACGT" * 10, b"N" * 31, b"GATTACA" * 9] + seqs2
    rng = np.random.default_rng(19)
    quals = [[(rng.integers(0, 42, len(s)) + 33).astype(np.uint8).tobytes() for s in seqs] for seqs in (seqs1, seqs2)]
    raw1, recs1 = OR.chunk(seqs1, quals[0])
    raw2, recs2 = OR.chunk(seqs2, quals[1])
    ins = OR.overlap_records(raw1, recs1, 0, raw2, recs2, 3, len(seqs1), OR.spec())[3]
    return raw1, recs1, raw2, recs2, ins


def test_synthetic_pairs(F, ctx, synth):
    raw1, recs1, raw2, recs2, ins = synth
    n = len(recs1)
    assert n % 64 != 0 and n > 256, "not a multiple of a wave's pairs, more than one workgroup"
    report = same(ctx, raw1, recs1, 0, raw2, recs2, 3, n, ins, what="first_a 0, first_b 3")[2]
    assert int(report[CR.FIXED_A]) > 0 and int(report[CR.FIXED_B]) > 0 and int(report[CR.N_RESOLVED]) > 0, "a degenerate draw"
    assert 0 < int(report[CR.PAIRS_CORRECTED]) < int(report[CR.WITH_INSERT]) < n and ins[150] == 0 == ins[151], "513 bases: no insert"
    for first, count in ((0, 1), (63, 2), (64, 64), (n - 1, 1), (5, 70)):
        same(ctx, raw1, recs1, first, raw2, recs2, 3 + first, count, ins[first:first + count], what="[%d, +%d)" % (first, count))
    # other levels, the widest and the narrowest among them
    for c in ((63, 62), (1, 0), (20, 19), (41, 2)):
        same(ctx, raw1, recs1, 0, raw2, recs2, 3, n, ins, CR.spec(*c), what=str(c))


def test_a_second_call_corrects_nothing(F, ctx, synth):
    raw1, recs1, raw2, recs2, ins = synth
    n = len(recs1)
    b1, b2 = ctx.dblock(raw1, recs1), ctx.dblock(raw2, recs2)
    one = b1.pair_correct(0, b2, 3, n, ins, CR.spec())
    raws = b1.fetch(raw=True)["raw"].tobytes(), b2.fetch(raw=True)["raw"].tobytes()
    two = b1.pair_correct(0, b2, 3, n, ins, CR.spec())
    assert one["rc"] == 0 == two["rc"] and int(one["report"][3]) + int(one["report"][4]) > 0
    assert two["report"][2:6].tolist() == [0, 0, 0, 0] and not two["fixed_a"].any() and not two["fixed_b"].any()
    assert int(two["report"][6]) == int(one["report"][6]) - int(one["report"][3]) - int(one["report"][4])
    assert [int(two["report"][i]) for i in (0, 1, 7)] == [int(one["report"][i]) for i in (0, 1, 7)]
    assert (b1.fetch(raw=True)["raw"].tobytes(), b2.fetch(raw=True)["raw"].tobytes()) == raws
    b1.close()
    b2.close()


# ---------------------------------------------------------------- 3. the smallest shapes that can go wrong
def shapes():
    """Every length of SIZES on either side, each pair with the inserts that put it at an edge: ov == 1 at both ends (I = 1,
    I = L1 + L2 - 1), d = 0, and one in between.  The inserts are the caller's data, so the lines are random and unrelated --
    three places in four disagree -- with qualities either side of both bounds: corrections everywhere, the first and the
    last place of every overlap included.  The first record of either chunk has the header line "@r", so the reversed
    window of its first places starts in front of the chunk -> (raw1, recs1, raw2, recs2, inserts)"""
    rng = np.random.default_rng(23)
    acgtn = np.frombuffer(b"ACGTACGTACGTN", dtype=np.uint8)
    line = lambda k: acgtn[rng.integers(0, acgtn.size, k)].tobytes()      # noqa: E731
    qual = lambda k: LEVELS[rng.integers(0, LEVELS.size, k)].tobytes()    # noqa: E731
    seqs1, seqs2, q1, q2, ins = [], [], [], [], []
    # the first pair: nine bases on either side at d = 0 -- lane 1's window of mate 2 starts seven bytes in front of place 0,
    # four in front of the chunk -- with mate 1 winning at s2[0] and mate 2 winning at s1[0]
    seqs1.append(b"CACGTACGA"), q1.append(b"!IIIIIIII"), seqs2.append(b"ACGTACGTA"), q2.append(b"!IIIIIIII"), ins.append(9)
    for L1 in SIZES:
        for L2 in SIZES:
            for I in sorted({1, L1 + L2 - 1, L2, (L1 + L2) // 2}):
                seqs1.append(line(L1)), q1.append(qual(L1)), seqs2.append(line(L2)), q2.append(qual(L2)), ins.append(I)
    # the full 512 / 512 overlap with a correction in its first and its last place, in either mate
    s = line(512).replace(b"N", b"A")
    for at in (0, 511):   # s1[0] stands beside s2[511], s1[511] beside s2[0]: a poor N at `at` of either mate loses to the other mate
        a, b = bytearray(s), bytearray(OR.revcomp(s))
        qa, qb = bytearray(b"I" * 512), bytearray(b"I" * 512)
        a[at] = b[at] = ord("N")
        qa[at] = qb[at] = ord("!")
        seqs1.append(bytes(a)), q1.append(bytes(qa)), seqs2.append(bytes(b)), q2.append(bytes(qb)), ins.append(512)
    # the last pair: a correction in the last place of the last record of either chunk
    seqs1.append(b"ACGTACGTN"), q1.append(b"IIIIIIII!"), seqs2.append(b"CCGTACGTN"), q2.append(b"IIIIIIII!"), ins.append(9)
    names = [b"r"] + [b"pair%d" % i for i in range(1, len(ins))]
    raw1, recs1 = OR.chunk(seqs1, q1, names)
    raw2, recs2 = OR.chunk(seqs2, q2, names)
    return raw1, recs1, raw2, recs2, np.array(ins, dtype=np.uint16)


def test_the_smallest_shapes(F, ctx):
    raw1, recs1, raw2, recs2, ins = shapes()
    n = len(ins)
    assert int(recs1["seq_off"][0]) == 3 == int(recs2["seq_off"][0]) and n > 4 * 64
    want_a, want_b, report, fa, fb = same(ctx, raw1, recs1, 0, raw2, recs2, 0, n, ins, what="every shape")
    # the first pair by hand: s1[0] 'C' (Phred 0) beside s2[8] 'A' -> 'T'; s2[0] 'A' (Phred 0) beside s1[8] 'A' -> 'T'
    assert (int(fa[0]), int(fb[0])) == (1, 1)
    assert want_a[3:12].tobytes() == b"TACGTACGA" and want_b[3:12].tobytes() == b"TCGTACGTA" and want_a[15:24].tobytes() == b"I" * 9 == want_b[15:24].tobytes()
    # the 512 / 512 pairs: the first and the last place of each, one in either mate
    assert fa[n - 3:n - 1].tolist() == [1, 1] and fb[n - 3:n - 1].tolist() == [1, 1]
    # the last pair: s1[8] 'N' (Phred 0) beside s2[0] 'C' -> 'G'; s2[8] 'N' (Phred 0) beside s1[0] 'A' -> 'T'; the chunks' last bytes
    assert (int(fa[n - 1]), int(fb[n - 1])) == (1, 1) and want_a[-11:].tobytes() == b"\nIIIIIIIII\n" == want_b[-11:].tobytes()
    assert int(report[CR.FIXED_A]) > 300 and int(report[CR.FIXED_B]) > 300 and int(report[CR.N_RESOLVED]) > 50, "corrections everywhere"
    # pairs with ov == 1 at either end are among the corrected ones
    one = np.flatnonzero((ins == 1) & ((fa > 0) | (fb > 0)))
    far = np.flatnonzero((ins == recs1["len"] + recs2["len"] - 1) & (recs1["len"] + recs2["len"] > 2) & ((fa > 0) | (fb > 0)))
    assert one.size > 0 and far.size > 0
    for first, count in ((0, 1), (0, 63), (1, 64), (64, 65), (n - 129, 129), (n - 1, 1)):
        same(ctx, raw1, recs1, first, raw2, recs2, first, count, ins[first:first + count], what="[%d, +%d)" % (first, count))


def test_inserts_all_zero(F, ctx, synth):
    raw1, recs1, raw2, recs2, _ = synth
    n = len(recs1)
    report = same(ctx, raw1, recs1, 0, raw2, recs2, 3, n, np.zeros(n, dtype=np.uint16), what="no inserts")[2]
    assert report.tolist() == [n, 0, 0, 0, 0, 0, 0, 0]
    # ... whatever the lines hold: bytes that could not be judged
    odd1, odd2 = raw1.copy(), raw2.copy()
    odd1[int(recs1["seq_off"][7])] = ord("x")
    odd2[int(recs2["qual_off"][9])] = 200
    assert same(ctx, odd1, recs1, 0, odd2, recs2, 3, n, np.zeros(n, dtype=np.uint16), what="no inserts, odd lines")[2].tolist() == [n, 0, 0, 0, 0, 0, 0, 0]


# ---------------------------------------------------------------- 4. what is refused leaves both chunks as they were
X, RX, Q = b"ACGTACGTAC", b"GTACGTACGT", b"I" * 10


def put(s, at, c):
    return s[:at] + c + s[at + 1:]


def test_refusals_leave_both_chunks_unchanged(F, ctx):
    """every chunk here has pairs in front of and behind the offending one with something to correct"""
    fixable = (put(X, 3, b"G"), put(Q, 3, b"!"), RX, Q)   # mate 2 wins at s1[3]
    long1 = (b"ACGGTCATTGCAGGATCCTAAGCTTGACCGTATGCAATCG" * 13)[:513]

    def chunks(s1, q1, s2, q2):
        """65 fixable pairs, the pair in question, 65 more: three waves"""
        k = 65
        raw1, recs1 = OR.chunk([fixable[0]] * k + [s1] + [fixable[0]] * k, [fixable[1]] * k + [q1] + [fixable[1]] * k)
        raw2, recs2 = OR.chunk([fixable[2]] * k + [s2] + [fixable[2]] * k, [fixable[3]] * k + [q2] + [fixable[3]] * k)
        return raw1, recs1, raw2, recs2

    def inserts(I):
        return np.array([10] * 65 + [I] + [10] * 65, dtype=np.uint16)

    n, spec = 131, CR.spec()
    raw1, recs1, raw2, recs2 = chunks(X, Q, RX, Q)
    assert same(ctx, raw1, recs1, 0, raw2, recs2, 0, n, inserts(10), what="the chunks as they are")[2].tolist() == [n, n, 130, 130, 0, 0, 130, 1310]
    for I in (20, 21, 600, 65535):
        refused(ctx, raw1, recs1, 0, raw2, recs2, 0, n, inserts(I), spec, "I = %d >= L1 + L2" % I)
    assert same(ctx, raw1, recs1, 0, raw2, recs2, 0, n, inserts(19), what="I = L1 + L2 - 1")[2].tolist() == [n, n, 130, 130, 0, 0, 131, 1301]
    for what, pair, I in (
        ("513 bases in mate 1", (long1, b"I" * 513, RX, Q), 10), ("513 bases in mate 2", (X, Q, long1, b"I" * 513), 513),
        ("an x inside the overlap, mate 1", (put(X, 9, b"x"), Q, RX, Q), 10), ("an x inside the overlap, mate 2", (X, Q, put(RX, 0, b"x"), Q), 10),
        ("a byte above 127 inside the overlap", (X, Q, put(RX, 5, b"\xc1"), Q), 10),
        ("a quality byte 32, mate 1", (X, put(Q, 0, b" "), RX, Q), 10), ("a quality byte 32, mate 2", (X, Q, RX, put(Q, 9, b" ")), 10),
        ("a quality byte 97, mate 1", (X, put(Q, 9, b"a"), RX, Q), 10), ("a quality byte 97, mate 2", (X, Q, RX, put(Q, 0, b"a")), 10),
        ("a quality byte 255", (X, put(Q, 4, b"\xff"), RX, Q), 10),
    ):
        r1, t1, r2, t2 = chunks(*pair)
        refused(ctx, r1, t1, 0, r2, t2, 0, n, inserts(I), spec, what)
        # ... and accepted, the neighbours corrected, when the pair has no insert
        assert same(ctx, r1, t1, 0, r2, t2, 0, n, inserts(0), what=what + ", no insert")[2].tolist() == [n, 130, 130, 130, 0, 0, 130, 1300]
    # the same bytes outside the overlap are not looked at: d = 4 leaves s1[0, 4) and s2[0, 2) out
    r1, t1, r2, t2 = chunks(b"xxxxACGTAC", b" " * 4 + b"I" * 6, b"xxGTACGT", b"aa" + b"I" * 6)
    assert same(ctx, r1, t1, 0, r2, t2, 0, n, inserts(12), what="odd bytes outside the overlap")[2].tolist() == [n, n, 130, 130, 0, 0, 130, 1306]
    # (a record outside its chunk or without bases cannot be put to the device: creating the block refuses its table)
    # the arguments
    for first_a, first_b, count in ((0, 0, 0), (0, 0, n + 1), (n, 0, 1), (1, 0, n), (0, 1, n)):
        refused(ctx, raw1, recs1, first_a, raw2, recs2, first_b, count, inserts(10), spec, "the range %r" % ((first_a, first_b, count),))
    for bad in (None, CR.spec(0, 0), CR.spec(64, 14), CR.spec(30, 30), CR.spec(14, 30), CR.spec(reserved=(1, 0, 0, 0, 0, 0))):
        refused(ctx, raw1, recs1, 0, raw2, recs2, 0, n, inserts(10), bad, "the spec %r" % (bad,))
    refused(ctx, raw1, recs1, 0, raw2, recs2, 0, n, None, spec, "no inserts")
    b1, b2 = ctx.dblock(raw1, recs1), ctx.dblock(raw2, recs2)
    for g in (b1.pair_correct(0, b1, 0, n, inserts(10), spec), b1.pair_correct(0, b1, 66, 65, inserts(10), spec), b1.pair_correct(0, None, 0, n, inserts(10), spec)):
        assert g["rc"] == E_ARG and not g["report"].any() and not g["fixed_a"].any(), "the same block on both sides, or none"
    assert b1.pair_correct(0, b2, 0, n, inserts(10), spec, want_report=False)["rc"] == E_ARG, "no report"
    assert b1.fetch(raw=True)["raw"].tobytes() == raw1.tobytes() and b2.fetch(raw=True)["raw"].tobytes() == raw2.tobytes()
    b1.close()
    b2.close()


# ---------------------------------------------------------------- 5. nothing depends on what the scratch held
def test_the_same_answer_whatever_the_scratch_held(F, golden, golden_inserts):
    (raw1, recs1), (raw2, recs2) = golden
    n = len(recs1)
    c1, c2 = TS.context_for(F, raw1, recs1), TS.context_for(F, raw2, recs2)

    def calls():
        assert c1.encode_raw(raw1)["rc"] == 0 == c2.encode_raw(raw2)["rc"]   # (staged afresh: the call changes the chunks)
        g = c1.chunk_pair_correct(0, c2, 0, n, golden_inserts, CR.spec())
        part = c1.chunk_pair_correct(37, c2, 37, 900, golden_inserts[37:937], CR.spec())
        s1, s2 = c1.chunk_select_marked(0, n), c2.chunk_select_marked(0, n)
        assert g["rc"] == 0 == part["rc"] and s1["rc"] == 0 == s2["rc"]
        return (g["report"].tolist(), g["fixed_a"].tolist(), g["fixed_b"].tolist(), part["report"].tolist(), part["fixed_a"].tolist(),
                s1["out"].tobytes(), s2["out"].tobytes())

    first = calls()
    assert first[0][:5] == [1000, 111, 36, 34, 28]
    for c in (c1, c2):
        buffers, filled = c.fill_scratch(0xFF)
        assert buffers > 0 and filled > 0
    assert calls() == first
    for c in (c1, c2):
        c.fill_scratch(0x00)
    assert calls() == first
    c1.close()
    c2.close()
