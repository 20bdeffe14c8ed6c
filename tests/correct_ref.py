"""A pure-Python / numpy restatement of the correction inside the mate overlap (include/fqgpu.h: fqgpu_chunk_pair_correct) from
raw chunks, their record tables and the pairs' insert sizes: the rule for one pair, the patched chunks of a range of pairs with
the eight report words and the two per-pair arrays, and a whole paired restore with the correction behind the overlap and in
front of everything that judges either mate.  Built on overlap_ref.py.  Test code: the product never imports it."""
import numpy as np

import overlap_ref as OR
import pair_ref as PR
import trim_ref as R

REPORT_WORDS = 8
N_PAIRS, WITH_INSERT, PAIRS_CORRECTED, FIXED_A, FIXED_B, N_RESOLVED, MISMATCHES_SEEN, OVERLAP_BASES = range(8)
MAX_LEN = OR.MAX_LEN
Refused = OR.Refused
N = 78


def spec(good_q=30, bad_q=14, reserved=(0, 0, 0, 0, 0, 0)):
    return np.array([good_q, bad_q, *reserved], dtype=np.uint32)


def check(c):
    """fqgpu_correct_check restated -> True iff the spec is accepted"""
    if c is None:
        return False
    c = [int(v) for v in c]
    return len(c) == 8 and 1 <= c[0] <= 63 and 0 <= c[1] < c[0] and not any(c[2:])


def correct_pair(s1, q1, s2, q2, I, c):
    """the rule for one pair with I != 0 (four lines as bytes) -> (s1, q1, s2, q2 patched, fixed_a, fixed_b, n_resolved,
    mismatches_seen, overlap_bases); refuses what cannot be judged"""
    good, bad = int(c[0]), int(c[1])
    L1, L2 = len(s1), len(s2)
    if not (1 <= L1 <= MAX_LEN and 1 <= L2 <= MAX_LEN and 1 <= I <= L1 + L2 - 1):
        raise Refused("an insert the lengths do not allow")
    d = I - L2
    lo, hi = max(0, d), min(L1, I)
    assert hi - lo >= 1
    o1, p1, o2, p2 = bytearray(s1), bytearray(q1), bytearray(s2), bytearray(q2)
    fixed_a = fixed_b = resolved = seen = 0
    for i in range(lo, hi):
        j = I - 1 - i
        assert 0 <= j < L2
        b1, b2, c1, c2 = s1[i], s2[j], q1[i], q2[j]
        if b1 not in b"ACGTN" or b2 not in b"ACGTN":
            raise Refused("a sequence byte outside ACGTN inside an overlap")
        if not (33 <= c1 <= 96 and 33 <= c2 <= 96):
            raise Refused("a quality byte outside 33 .. 96 inside an overlap")
        if not (b1 == N or b2 == N or b1 != OR.COMP[b2]):
            continue
        seen += 1
        if b1 != N and c1 - 33 >= good and c2 - 33 <= bad:    # mate 1 wins
            o2[j], p2[j] = OR.COMP[b1], c1
            fixed_b += 1
            resolved += b2 == N
        elif b2 != N and c2 - 33 >= good and c1 - 33 <= bad:  # mate 2 wins
            o1[i], p1[i] = OR.COMP[b2], c2
            fixed_a += 1
            resolved += b1 == N
    return bytes(o1), bytes(p1), bytes(o2), bytes(p2), fixed_a, fixed_b, resolved, seen, hi - lo


def _lines(raw, rec):
    so, qo, n = int(rec["seq_off"]), int(rec["qual_off"]), int(rec["len"])
    if n == 0 or so + n > len(raw) or qo + n > len(raw):
        raise Refused("a record outside its chunk or of length 0")
    return so, qo, n


def correct_records(raw_a, recs_a, first_a, raw_b, recs_b, first_b, count, inserts, c):
    """-> (patched raw_a, patched raw_b, report uint64[8], fixed_a, fixed_b uint16[count]) of the pairs first_a + i / first_b + i
    with the insert sizes inserts[i], i < count.  The inputs are not changed.  Refuses what the call refuses."""
    raw_a, raw_b = np.asarray(raw_a, dtype=np.uint8), np.asarray(raw_b, dtype=np.uint8)
    if not check(c) or inserts is None:
        raise Refused("a spec the check refuses, or no inserts")
    if count <= 0 or first_a + count > len(recs_a) or first_b + count > len(recs_b):
        raise Refused("not a range of both chunks")
    if raw_a is raw_b or np.shares_memory(raw_a, raw_b):
        raise Refused("the two sides are the same chunk")
    out_a, out_b = raw_a.copy(), raw_b.copy()
    report = np.zeros(REPORT_WORDS, dtype=np.uint64)
    fa, fb = np.zeros(count, dtype=np.uint16), np.zeros(count, dtype=np.uint16)
    for i in range(count):
        I = int(inserts[i])
        if I == 0:
            continue
        so1, qo1, L1 = _lines(raw_a, recs_a[first_a + i])
        so2, qo2, L2 = _lines(raw_b, recs_b[first_b + i])
        s1, q1, s2, q2, a, b, res, seen, ov = correct_pair(raw_a[so1:so1 + L1].tobytes(), raw_a[qo1:qo1 + L1].tobytes(),
                                                           raw_b[so2:so2 + L2].tobytes(), raw_b[qo2:qo2 + L2].tobytes(), I, c)
        out_a[so1:so1 + L1], out_a[qo1:qo1 + L1] = np.frombuffer(s1, dtype=np.uint8), np.frombuffer(q1, dtype=np.uint8)
        out_b[so2:so2 + L2], out_b[qo2:qo2 + L2] = np.frombuffer(s2, dtype=np.uint8), np.frombuffer(q2, dtype=np.uint8)
        fa[i], fb[i] = a, b
        report[WITH_INSERT] += 1
        report[PAIRS_CORRECTED] += int(a + b > 0)
        report[FIXED_A] += a
        report[FIXED_B] += b
        report[N_RESOLVED] += res
        report[MISMATCHES_SEEN] += seen
        report[OVERLAP_BASES] += ov
    report[N_PAIRS] = count
    return out_a, out_b, report, fa, fb


def pair_records_corrected(raw1, recs1, raw2, recs2, o, c, overlap_trim=False, a1=None, a2=None, x=None, t=None, f=None, overlap=None):
    """The whole paired restore with the correction: overlap, then correction, then -- overlap_trim -- the limits, then the
    selection on the patched chunks -> (out1, out2, report1, report2, counters, summary, correct_report).  Every pair is
    handled on its own, so how a farm cuts the files into units does not show.  overlap: overlap_ref.overlap_records of the
    two whole files for o, when the caller has it already."""
    n = len(recs1)
    if n != len(recs2):
        raise ValueError("%d records against %d" % (n, len(recs2)))
    bad = PR.first_mismatch(raw1, recs1, 0, raw2, recs2, 0, n)
    if bad is not None:
        raise ValueError("the ids of record %d differ" % bad)
    summary, la, lb, ins = OR.overlap_records(raw1, recs1, 0, raw2, recs2, 0, n, o) if overlap is None else overlap
    raw1, raw2, correct_report, _, _ = correct_records(raw1, recs1, 0, raw2, recs2, 0, n, ins, c)
    if not overlap_trim:
        la = lb = None
    k1 = OR.limited_records(raw1, recs1, 0, n, None, la, a1, x, t, f)[2]
    out2, report2, k, _, _ = OR.limited_records(raw2, recs2, 0, n, k1, lb, a2, x, t, f)
    out1, report1, k_again, _, _ = OR.limited_records(raw1, recs1, 0, n, k, la, a1, x, t, f)
    assert np.array_equal(k, k_again)
    kept, m1, m2 = int(report1[R.N_KEPT]), int(report2[PR.DROPPED_UNMARKED]), int(report1[PR.DROPPED_UNMARKED])
    counters = dict(pairs=n, kept=kept, dropped_mate1_only=m1, dropped_mate2_only=m2, dropped_both=n - kept - m1 - m2)
    return out1, out2, report1, report2, counters, summary, correct_report
