"""The mate overlap on the device (k_pair_overlap in fqcomp28_amd/csrc/pair.hip and k_select_limit in select.hip, behind
fqgpu_*_pair_overlap and fqgpu_*_select_limited) against the restatement in overlap_ref.py: all 1040 summary words, the three
per-pair arrays, and -- for a selection with limits -- the kept bytes, all 24 report words, the keep bits, the windows and
the places, for equality.  Integer arithmetic: there is no tolerance."""
import os

import numpy as np
import pytest

import adapter_ref as AR
import filter_ref as FR
import oracle_lib as O
import overlap_ref as OR
import pair_ref as PR
import tail_ref as TR
import test_gpu_stats as TS
import test_gpu_tail as TG
import test_tail_host as HT
import trim_ref as R

pytestmark = pytest.mark.gpu

E_ARG, E_OVERFLOW = -4, -1
TRUSEQ = HT.TRUSEQ
LENGTHS = (29, 30, 31, 32, 33, 63, 64, 65, 127, 128, 129, 300, 511, 512)


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
def golden_want(golden):
    (raw1, recs1), (raw2, recs2) = golden
    return OR.overlap_records(raw1, recs1, 0, raw2, recs2, 0, len(recs1), OR.spec())


def synthetic_pairs(seed=7, n=300):
    """n pairs cut from random fragments: mate 1 the fragment's front, mate 2 the front of its reverse complement, random
    bases behind the fragment's end, a few substitutions and Ns; every length of LENGTHS on either side, fragments from
    shorter than min_overlap to longer than both reads together, and one mate of 513 bases -> (seqs1, seqs2)"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    rnd = lambda k: acgt[rng.integers(0, 4, k)].tobytes()  # noqa: E731
    seqs1, seqs2 = [], []
    for i in range(n):
        L1, L2 = LENGTHS[i % len(LENGTHS)], LENGTHS[(i // len(LENGTHS) + i) % len(LENGTHS)]
        if i == 150:
            L2 = 513
        if i == 151:
            L1, L2 = 513, 100
        kind = i % 5   # 0: shorter than the reads, 1: shorter than min_overlap, 2: between, 3: longer than both together, 4: any
        lo, hi = ((10, min(L1, L2)), (5, 29), (max(L1, L2), L1 + L2), (L1 + L2 + 1, L1 + L2 + 40), (5, L1 + L2 + 40))[kind]
        if i == 152:  # the longest overlap there is: two whole mates of 512 bases
            L1, L2, lo, hi = 512, 512, 512, 512
        frag = rnd(int(rng.integers(lo, max(hi, lo) + 1)))
        s1 = bytearray((frag + rnd(L1))[:L1])
        s2 = bytearray((OR.revcomp(frag) + rnd(L2))[:L2])
        for s in (s1, s2):
            for _ in range(int(rng.integers(0, 4)) if i != 152 else 0):
                s[int(rng.integers(0, len(s)))] = b"ACGTN"[int(rng.integers(0, 5))]
        seqs1.append(bytes(s1))
        seqs2.append(bytes(s2))
    return seqs1, seqs2


@pytest.fixture(scope="module")
def synth():
    """the synthetic pairs as two chunks -- mate 2's with three records of its own in front, so that first_a != first_b --
    and the reference's answer at the defaults"""
    seqs1, seqs2 = synthetic_pairs()
    raw1, recs1 = OR.chunk(seqs1)
    raw2, recs2 = OR.chunk([b"ACGT" * 10, b"N" * 31, b"GATTACA" * 9] + seqs2)
    want = OR.overlap_records(raw1, recs1, 0, raw2, recs2, 3, len(seqs1), OR.spec())
    return raw1, recs1, raw2, recs2, want


def holds(g, want, what=""):
    out, la, lb, ins = want
    assert g["rc"] == 0, (what, g["rc"])
    assert g["out"][:OR.HEAD].tolist() == out[:OR.HEAD].tolist(), what
    assert g["out"].tolist() == out.tolist(), what
    for name, w in (("limit_a", la), ("limit_b", lb), ("insert", ins)):
        if g[name] is not None and not np.array_equal(g[name], w):
            at = int(np.flatnonzero(g[name] != w)[0])
            raise AssertionError("%s: %s differs, first at pair %d: %d, expected %d" % (what, name, at, g[name][at], w[at]))


# ---------------------------------------------------------------- 1. the fixture, both call forms
def test_the_fixture_in_both_call_forms(F, ctx, golden, golden_want):
    (raw1, recs1), (raw2, recs2) = golden
    n = len(recs1)
    assert (int(golden_want[0][OR.OVERLAPPED]), int(golden_want[0][OR.READ_THROUGH])) == (111, 36)
    b1, b2 = ctx.dblock(raw1, recs1), ctx.dblock(raw2, recs2)
    g = b1.pair_overlap(0, b2, 0, n, OR.spec())
    holds(g, golden_want, "two blocks")
    assert int(g["out"][OR.FINGERPRINT]) == OR.fingerprint(OR.spec())
    # a range at another place on either side, and the arrays left out
    want = OR.overlap_records(raw1, recs1, 100, raw2, recs2, 100, 777, OR.spec())
    holds(b1.pair_overlap(100, b2, 100, 777, OR.spec()), want, "a range")
    q = b1.pair_overlap(100, b2, 100, 777, OR.spec(), want_arrays=False)
    assert q["rc"] == 0 and q["out"].tolist() == want[0].tolist() and q["limit_a"] is None
    # what is refused, and what that leaves
    for first_a, first_b, count in ((0, 0, 0), (0, 0, n + 1), (n, 0, 1), (1, 0, n), (0, 1, n)):
        r = b1.pair_overlap(first_a, b2, first_b, count, OR.spec())
        assert r["rc"] == E_ARG and not r["out"].any(), (first_a, first_b, count)
    assert b1.pair_overlap(0, None, 0, n, OR.spec())["rc"] == E_ARG and b1.pair_overlap(0, b2, 0, n, None)["rc"] == E_ARG
    assert b1.pair_overlap(0, b2, 0, n, OR.spec(min_overlap=0))["rc"] == E_ARG
    small = b1.pair_overlap(0, b2, 0, n, OR.spec(), cap_words=OR.WORDS - 1)
    assert small["rc"] == E_OVERFLOW and not small["out"].any()
    b1.close()
    b2.close()
    # the chunks staged on two handles
    c1, c2 = TS.context_for(F, raw1, recs1), TS.context_for(F, raw2, recs2)
    assert c1.chunk_pair_overlap(0, c2, 0, n, OR.spec())["rc"] == E_ARG, "no chunk on either handle"
    assert c1.encode_raw(raw1)["rc"] == 0 == c2.encode_raw(raw2)["rc"]
    holds(c1.chunk_pair_overlap(0, c2, 0, n, OR.spec()), golden_want, "two staged chunks")
    holds(c1.chunk_pair_overlap(100, c2, 100, 777, OR.spec()), want, "a range of two staged chunks")
    assert c1.chunk_pair_overlap(0, c2, 0, n + 1, OR.spec())["rc"] == E_ARG and c1.chunk_pair_overlap(0, None, 0, n, OR.spec())["rc"] == E_ARG
    holds(c1.chunk_pair_overlap(0, c1, 0, n, OR.spec()), OR.overlap_records(raw1, recs1, 0, raw1, recs1, 0, n, OR.spec()), "a staged chunk against itself")
    c1.close()
    c2.close()


# ---------------------------------------------------------------- 2. synthetic pairs: every length, every kind of fragment
def test_synthetic_pairs_at_the_defaults(F, ctx, synth):
    raw1, recs1, raw2, recs2, want = synth
    n = len(recs1)
    assert n % 64 != 0 and n > 256, "not a multiple of a workgroup's pairs, more than one workgroup"
    out = want[0]
    assert int(out[OR.NOT_ANALYSED]) == 2 and 0.15 * n < int(out[OR.OVERLAPPED]) < 0.9 * n, "a degenerate draw"
    assert 0 < int(out[OR.READ_THROUGH]) < int(out[OR.OVERLAPPED]) and int(out[OR.MISMATCHES]) > 0
    b1, b2 = ctx.dblock(raw1, recs1), ctx.dblock(raw2, recs2)
    g = b1.pair_overlap(0, b2, 3, n, OR.spec())
    holds(g, want, "first_a 0, first_b 3")
    assert g["insert"][150] == 0 and g["limit_b"][150] == 513 and g["limit_a"][151] == 513
    # single pairs and short ranges at the workgroup's edges
    for first, count in ((0, 1), (63, 2), (64, 64), (n - 1, 1), (5, 70)):
        holds(b1.pair_overlap(first, b2, 3 + first, count, OR.spec()), OR.overlap_records(raw1, recs1, first, raw2, recs2, 3 + first, count, OR.spec()),
              "[%d, +%d)" % (first, count))
    b1.close()
    b2.close()


@pytest.mark.parametrize("o", [(1, 0, 0), (30, 0, 50), (30, 65535, 50), (12, 2, 10), (512, 5, 20), (100, 5, 20)],
                         ids=["exact, any length", "no mismatch", "percent alone", "short overlaps", "the longest overlap", "long overlaps"])
def test_synthetic_pairs_with_other_limits(F, ctx, synth, o):
    raw1, recs1, raw2, recs2, _ = synth
    n = len(recs1)
    b1, b2 = ctx.dblock(raw1, recs1), ctx.dblock(raw2, recs2)
    want = OR.overlap_records(raw1, recs1, 0, raw2, recs2, 3, n, OR.spec(*o))
    assert int(want[0][OR.OVERLAPPED]) > 0, "a degenerate draw"
    holds(b1.pair_overlap(0, b2, 3, n, OR.spec(*o)), want, str(o))
    b1.close()
    b2.close()


def test_a_chunk_against_itself_and_the_hand_made_pairs(F, ctx, synth):
    raw1, recs1, _, _, _ = synth
    n = len(recs1)
    b = ctx.dblock(raw1, recs1)
    holds(b.pair_overlap(0, b, 0, n, OR.spec()), OR.overlap_records(raw1, recs1, 0, raw1, recs1, 0, n, OR.spec()), "a block against itself")
    holds(b.pair_overlap(1, b, 0, n - 1, OR.spec()), OR.overlap_records(raw1, recs1, 1, raw1, recs1, 0, n - 1, OR.spec()), "... shifted by one")
    b.close()
    import test_overlap_host as HO
    for what, s1, s2, o, hit in HO.HAND:
        ra, ta = OR.chunk([s1])
        rb, tb = OR.chunk([s2])
        ba, bb = ctx.dblock(ra, ta), ctx.dblock(rb, tb)
        g = ba.pair_overlap(0, bb, 0, 1, OR.spec(*o))
        holds(g, OR.overlap_records(ra, ta, 0, rb, tb, 0, 1, OR.spec(*o)), what)
        assert int(g["insert"][0]) == (0 if hit is None else hit[0] + len(s2)), what
        ba.close()
        bb.close()


# ---------------------------------------------------------------- 3. a byte that cannot be judged
def test_a_bad_byte_in_an_analysed_line(F, ctx, synth):
    raw1, recs1, raw2, recs2, want = synth
    n = len(recs1)
    b1, b2 = ctx.dblock(raw1, recs1), ctx.dblock(raw2, recs2)
    # a lower-case base at a line's front, a byte above 127 at a line's end, a dot in the middle; in either mate
    for side, r, at, byte in ((2, 3 + 17, 0, ord("a")), (2, 3 + 299, -1, 0xC1), (1, 64, 5, ord("."))):
        raw, recs = (raw1, recs1) if side == 1 else (raw2, recs2)
        spoilt = raw.copy()
        spoilt[int(recs["seq_off"][r]) + (at if at >= 0 else int(recs["len"][r]) + at)] = byte
        bad = ctx.dblock(spoilt, recs)
        g = bad.pair_overlap(0, b2, 3, n, OR.spec()) if side == 1 else b1.pair_overlap(0, bad, 3, n, OR.spec())
        assert g["rc"] == E_ARG and not g["out"].any() and not g["limit_a"].any() and not g["limit_b"].any() and not g["insert"].any(), (side, r)
        bad.close()
    # the same in a line that is not analysed is not looked at: pair 150's mate 2 has 513 bases
    spoilt = raw2.copy()
    spoilt[int(recs2["seq_off"][3 + 150]) + 7] = ord("x")
    odd = ctx.dblock(spoilt, recs2)
    holds(b1.pair_overlap(0, odd, 3, n, OR.spec()), want, "a line that is not analysed")
    odd.close()
    b1.close()
    b2.close()


# ---------------------------------------------------------------- 4. nothing depends on what the scratch held
def test_the_same_answer_whatever_the_scratch_held(F, golden, golden_want):
    (raw1, recs1), (raw2, recs2) = golden
    n = len(recs1)
    c = TS.context_for(F, raw1, recs1)
    b1, b2 = c.dblock(raw1, recs1), c.dblock(raw2, recs2)
    limit = golden_want[1]

    def calls():
        g = b1.pair_overlap(0, b2, 0, n, OR.spec())
        s = b1.select_limited(37, 937, None, limit[37:937], trim=R.trm(q_tail=20), flt=FR.flt(min_len=40))
        assert g["rc"] == 0 == s["rc"]
        return (g["out"].tolist(), g["limit_a"].tolist(), g["limit_b"].tolist(), g["insert"].tolist(), s["out"].tobytes(), s["report"].tolist(),
                s["keep"].tolist(), s["win"].tolist())

    first = calls()
    assert first[0] == golden_want[0].tolist() and first[3] == golden_want[3].tolist()
    buffers, filled = c.fill_scratch(0xFF)
    assert buffers > 0 and filled > 0
    assert calls() == first
    c.fill_scratch(0x00)
    assert calls() == first
    b1.close()
    b2.close()
    c.close()


# ---------------------------------------------------------------- 5. a selection with limits
FULL = dict(a=AR.adp(TRUSEQ), x=TR.tl("G", window_len=4, window_q=20), t=R.trm(cut_front=1, q_tail=20), f=FR.flt(min_len=30, max_n=1, min_mean_q=18))
SELECTIONS = [dict(), dict(t=R.trm(q_tail=20), f=FR.flt(min_len=40, min_mean_q=22)), dict(a=AR.adp(TRUSEQ)), FULL]
SELECTION_IDS = ["nothing", "a trim and a filter", "an adapter", "everything"]


def opts(o):
    return dict(adapter=o.get("a"), tail=o.get("x"), trim=o.get("t"), flt=o.get("f"))


def same_limited(b, raw, recs, first, end, mark, limit, what="", **o):
    want = OR.limited_records(raw, recs, first, end, mark, limit, o.get("a"), o.get("x"), o.get("t"), o.get("f"))
    g = b.select_limited(first, end, mark, limit, **opts(o))
    TG.holds(g, want, what)
    assert not g["report"][23]
    return g, want


@pytest.mark.parametrize("o", SELECTIONS, ids=SELECTION_IDS)
def test_select_limited_without_limits_and_with_limits_that_cut_nothing(F, ctx, golden, o):
    raw, recs = golden[0]
    n = len(recs)
    b = ctx.dblock(raw, recs)
    mark = np.random.default_rng(3).integers(0, 256, (n + 7) // 8, dtype=np.uint8)
    for first, end, m in ((0, n, None), (37, 937, mark[:(900 + 7) // 8])):
        w = b.select_marked(first, end, m, **opts(o))
        g = b.select_limited(first, end, m, None, **opts(o))
        assert g["rc"] == 0 == w["rc"] and g["out"].tobytes() == w["out"].tobytes() and g["report"].tolist() == w["report"].tolist()
        assert np.array_equal(g["keep"], w["keep"]) and np.array_equal(g["win"], w["win"]) and np.array_equal(g["places"], w["places"])
        L = recs["len"][first:end].astype(np.int64)
        for limit in (L, L + 1, np.full(end - first, 65535)):
            g = b.select_limited(first, end, m, limit.astype(np.uint16), **opts(o))
            assert g["rc"] == 0 and g["out"].tobytes() == w["out"].tobytes() and np.array_equal(g["keep"], w["keep"]) and np.array_equal(g["win"], w["win"])
            assert g["report"][:21].tolist() == w["report"][:21].tolist() and not g["report"][21:].any(), "words 21 / 22 stay zero"
            assert np.array_equal(g["places"], w["places"])
    b.close()


@pytest.mark.parametrize("o", SELECTIONS, ids=SELECTION_IDS)
def test_select_limited_against_the_reference(F, ctx, golden, golden_want, o):
    raw, recs = golden[0]
    n = len(recs)
    b = ctx.dblock(raw, recs)
    rng = np.random.default_rng(11)
    mark = rng.integers(0, 256, (n + 7) // 8, dtype=np.uint8)
    # the overlap's own limits; then random ones, a limit of 0 among them
    g, want = same_limited(b, raw, recs, 0, n, None, golden_want[1], "the overlap's limits", **o)
    assert int(g["report"][OR.READS_CUT_LIMIT]) > 0 and int(g["report"][OR.BASES_CUT_LIMIT]) > 0
    limit = rng.integers(0, 140, n).astype(np.uint16)
    limit[::7] = 0
    g, want = same_limited(b, raw, recs, 0, n, None, limit, "random limits", **o)
    assert int(g["report"][R.READS_EMPTIED]) >= len(limit[::7]) and not (g["win"][::7]).any(), "a limit of 0 empties the read"
    for first, end in ((37, 937), (64, 129), (n - 1, n), (1, 66)):
        same_limited(b, raw, recs, first, end, mark[:(end - first + 7) // 8], limit[first:end], "a range and a mark [%d, %d)" % (first, end), **o)
    if "a" in o:  # a limit below, at and above the adapter's place
        a_adapter = PR.marked_records(raw, recs, 0, n, None, o["a"], o.get("x"), o.get("t"), o.get("f"))[4][:, 0].astype(np.int64)
        hit = np.flatnonzero(a_adapter < recs["len"])
        assert hit.size >= 3
        around = recs["len"].astype(np.int64)
        around[hit[0::3]] = np.maximum(a_adapter[hit[0::3]] - 1, 0)
        around[hit[1::3]] = a_adapter[hit[1::3]]
        around[hit[2::3]] = a_adapter[hit[2::3]] + 1
        g, want = same_limited(b, raw, recs, 0, n, None, around.astype(np.uint16), "limits around the adapter's place", **o)
        assert int(g["report"][OR.READS_CUT_LIMIT]) == int((a_adapter[hit[0::3]] > 0).sum()) == int(g["report"][OR.BASES_CUT_LIMIT])
    r = b.select_limited(5, 5, None, limit[:1], **opts(o))
    assert r["rc"] == E_ARG and not r["report"].any()
    b.close()


def test_the_three_calls_of_a_trimmed_paired_restore(F, golden):
    (raw1, recs1), (raw2, recs2) = golden
    n = len(recs1)
    sel = dict(t=R.trm(q_tail=20), f=FR.flt(min_len=40, min_mean_q=22))
    want1, want2, rep1, rep2, counters, summary = OR.pair_records_trimmed(raw1, recs1, raw2, recs2, OR.spec(), **sel)
    c1, c2 = TS.context_for(F, raw1, recs1), TS.context_for(F, raw2, recs2)
    assert c1.encode_raw(raw1)["rc"] == 0 == c2.encode_raw(raw2)["rc"]
    ov = c1.chunk_pair_overlap(0, c2, 0, n, OR.spec())
    assert ov["rc"] == 0 and ov["out"].tolist() == summary.tolist()
    k1 = c1.chunk_select_limited(0, n, None, ov["limit_a"], query=True, **opts(sel))
    g2 = c2.chunk_select_limited(0, n, k1["keep"], ov["limit_b"], **opts(sel))
    g1 = c1.chunk_select_limited(0, n, g2["keep"], ov["limit_a"], **opts(sel))
    assert g1["rc"] == 0 == g2["rc"] and g1["out"].tobytes() == want1.tobytes() and g2["out"].tobytes() == want2.tobytes()
    assert g1["report"].tolist() == rep1.tolist() and g2["report"].tolist() == rep2.tolist() and 0 < counters["kept"] < n
    c1.close()
    c2.close()
