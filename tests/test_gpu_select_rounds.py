"""The step count of a round (sel_round_steps in fqcomp28_amd/csrc/select.hip): the line readers -- k_adapter_find in both
forms, k_tail_find and the judge -- read eight records a round, and a round takes as many requests as its longest line needs.
One read of 600 bases, three requests of its eight lanes, stands alone among reads of 40 to 150 bases: in every round of a
wave in turn, as the table's last record -- its round then holds four records --, in the first wave and in the second.  What
decides its result -- an adapter, a G tail, a quality drop, three N -- lies behind byte 256 of its lines, so a round that
takes one step too few gives another answer; the short reads of its round carry one of each as well.  Every family is called
once per chunk and compared with its numpy restatement: integer arithmetic, every comparison is exact."""
import os

import numpy as np
import pytest

import adapter_ref as AR
import filter_ref as FR
import oracle_lib as O
import probe_ref as PR
import tail_ref as TR
import test_gpu_adapter as TA
import test_gpu_filter as TF
import test_gpu_probe as TP
import test_gpu_stats as TS
import test_gpu_tail as TL
import test_gpu_trim as TT
import trim_ref as R

pytestmark = pytest.mark.gpu

LONG = 600
NOT_G = np.frombuffer(b"ACT", dtype=np.uint8)
ADAPTER = b"TCAGGACTTGCATCGAAGTCCATGCTAAGTCCA"      # 33 bases; its first five are no run of one base
LEADS = [3, 7, 9, 11, 13, 15, 1, 6]                 # of the long read's sequence line; its quality line's is 11 more: neither is 0
AT_ADAPTER, AT_TAIL, AT_DROP, AT_LOW, AT_N = 400, 570, 300, 520, 350   # the long read's places, all behind byte 256


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


def short_read(rng, r):
    """40 to 150 bases without G, Phred 30 .. 37; by r mod 3 the adapter somewhere, a G tail, or low ends, a quality drop and
    three N"""
    L = int(rng.integers(40, 151))
    s, q = NOT_G[rng.integers(0, 3, L)].copy(), 30 + rng.integers(0, 8, L)
    if r % 3 == 0:
        p = int(rng.integers(5, L - 8))
        k = min(len(ADAPTER), L - p)
        s[p:p + k] = np.frombuffer(ADAPTER[:k], dtype=np.uint8)
    elif r % 3 == 1:
        s[L - int(rng.integers(10, 25)):] = ord("G")
    else:
        p = int(rng.integers(8, L - 12))
        q[:5], q[p:p + 3], q[L - 6:] = 3, 2, 2
        s[p + 4:p + 7] = ord("N")
    return s, q


def long_read(rng):
    s, q = NOT_G[rng.integers(0, 3, LONG)].copy(), 30 + rng.integers(0, 8, LONG)
    s[AT_ADAPTER:AT_ADAPTER + len(ADAPTER)] = np.frombuffer(ADAPTER, dtype=np.uint8)
    s[AT_TAIL:] = ord("G")
    s[AT_N:AT_N + 3] = ord("N")
    q[AT_DROP:AT_DROP + 3] = 2
    q[AT_LOW:] = 5
    return s, q


def chunk(k, front):
    """front + 8 k + 4 records; the long read is the last one, record 8 k + 3 of its wave"""
    rng = np.random.default_rng(100 * k + front)
    n = front + 8 * k + 4
    seqs, phreds, hls, at = [], [], [], 0
    for r in range(n):
        s, q = long_read(rng) if r == n - 1 else short_read(rng, r)
        hls.append(TT.aligned_header(at, len(s), LEADS[k] if r == n - 1 else int(rng.integers(0, 16))))
        seqs.append(s.tobytes())
        phreds.append(q)
        at += hls[-1] + 2 * len(s) + 5
    raw, recs = TA.chunk_with(hls, seqs, phreds)
    assert int(recs["len"][-1]) == LONG and (recs["len"][:-1] <= 150).all() and (recs["len"][:-1] >= 40).all()
    assert int(recs["seq_off"][-1]) & 15 == LEADS[k] and int(recs["qual_off"][-1]) & 15 == (LEADS[k] + 11) % 16 != 0
    return raw, recs


@pytest.fixture(scope="module")
def chunks():
    return [("round %d, %d in front" % (k, front), *chunk(k, front)) for front in (0, 64) for k in range(8)]


def test_filter(F, ctx, chunks):
    f = FR.flt(max_n=2, min_mean_q=20)
    for what, raw, recs in chunks:
        g = TF.same(ctx, raw, recs, f, what)
        n = len(recs)
        assert not g["keep"][(n - 1) // 8] >> ((n - 1) % 8) & 1, "the long read's three N, behind byte 256, drop it"
        kept = np.unpackbits(g["keep"], bitorder="little")[n - 4:n - 1]
        assert kept.tolist() == [(r % 3) != 2 for r in range(n - 4, n - 1)], "the short reads of its round: three N in one of them"


def test_trim(F, ctx, chunks):
    t = R.trm(q_front=20, q_tail=20, crop=550)
    for what, raw, recs in chunks:
        g, want = TT.same(ctx, raw, recs, t, FR.flt(min_mean_q=25), what)
        assert (int(want[3][-1]) & 0xFFFF, int(want[3][-1]) >> 16) == (0, AT_LOW), "the tail walk's cut, in the third request"
        assert int((want[3][-4:-1] >> 16 < recs["len"][-4:-1]).sum()) == 1, "the low ends of a short read of the round"


def test_clip(F, ctx, chunks):
    a = AR.adp(ADAPTER, 5, 10)
    for what, raw, recs in chunks:
        g, want = TA.same(ctx, raw, recs, a, None, None, what)
        assert int(want[3][-1]) >> 16 == AT_ADAPTER, "the adapter in the long read's second request"
        assert int((want[3][-4:-1] >> 16 < recs["len"][-4:-1]).sum()) >= 1, "and in a short read of the round"


def test_tailtrim(F, ctx, chunks):
    x = TR.tl("G", window_len=4, window_q=20)
    for what, raw, recs in chunks:
        g, want = TL.same(ctx, raw, recs, None, x, None, None, what)
        a0, a1, e, e2 = (int(v) for v in want[4][-1])
        assert (a0, a1, e) == (LONG, AT_TAIL, AT_TAIL) and AT_DROP - 3 <= e2 <= AT_DROP, "the G tail in the third request, the drop in the second"
        p = want[4][-4:-1].astype(np.int64)
        assert int((p[:, 1] < p[:, 0]).sum()) == 1 and int((p[:, 3] < p[:, 2]).sum()) == 1, "a tail and a drop in the short reads of the round"


def test_probe(F, ctx, chunks):
    p = PR.prb([AR.adp(ADAPTER, 5, 10), AR.adp(b"G" * 10, 10, 0), AR.adp(TP.TRUSEQ)])
    for what, raw, recs in chunks:
        g, want = TP.same(ctx, raw, recs, p, 512, what)
        assert want[1][-1].tolist() == [AT_ADAPTER, AT_TAIL, LONG], "the long read's places: second request, third request, none"
        assert (want[1][-4:-1, :2] < recs["len"][-4:-1, None]).sum(axis=0).tolist() == [1, 1], "the short reads of the round"
