"""A pure-Python restatement of the mate merge (include/fqgpu.h: fqgpu_chunk_pair_merge) from raw chunks, their record tables,
the pairs' insert sizes and a mark: the rule for one place and one pair, the merged records of a range of pairs with the
sixteen report words and the merged bits, and a whole paired restore with a merged output beside the two mate outputs.
Written place by place: it shares nothing with the device's word logic.  Built on overlap_ref.py and correct_ref.py.  Test
code: the product never imports it."""
import numpy as np

import correct_ref as CR
import overlap_ref as OR
import pair_ref as PR
import trim_ref as R

REPORT_WORDS = 16
(N_PAIRS, WITH_INSERT, PAIRS_MERGED, BASES_MERGED, BYTES_OUT, OVERLAP_BASES, PLACES_DISAGREE, PLACES_N, DROPPED_A, DROPPED_B,
 PAIRS_UNMARKED, PAIRS_TOO_SHORT) = range(12)
MAX_LEN = OR.MAX_LEN
Refused = OR.Refused
N = 78


def spec(floor_q=2, min_len=1, reserved=(0, 0, 0, 0, 0, 0)):
    return np.array([floor_q, min_len, *reserved], dtype=np.uint32)


def check(m):
    """fqgpu_merge_check restated -> True iff the spec is accepted"""
    if m is None:
        return False
    m = [int(v) for v in m]
    return len(m) == 8 and 0 <= m[0] <= 63 and 1 <= m[1] <= 1023 and not any(m[2:])


def merge_place(b1, p1, b2, p2, floor_q):
    """a place both mates cover: mate 1's base and Phred, mate 2's COMPLEMENTED base and Phred -> (base, Phred, disagree, has_n)"""
    if b1 == N and b2 == N:
        return N, min(p1, p2), False, True
    if b1 == N:
        return b2, p2, False, True
    if b2 == N:
        return b1, p1, False, True
    if b1 == b2:
        return b1, max(p1, p2), False, False
    if p1 >= p2:  # mate 1 wins a tie
        return b1, max(p1 - p2, floor_q), True, False
    return b2, max(p2 - p1, floor_q), True, False


def merge_pair(s1, q1, s2, q2, I, floor_q):
    """the rule for one MERGED pair (four lines as bytes, I valid) -> (bases, quals of I bytes each, overlap_bases,
    places_disagree, places_n); refuses what cannot be judged"""
    L1, L2 = len(s1), len(s2)
    assert 1 <= I <= L1 + L2 - 1
    for s, q, L in ((s1, q1, L1), (s2, q2, L2)):
        k = min(L, I)
        if set(s[:k]) - set(b"ACGTN"):
            raise Refused("a base outside ACGTN in a merged pair")
        if any(not 33 <= c <= 96 for c in q[:k]):
            raise Refused("a quality byte outside 33 .. 96 in a merged pair")
    bases, quals = bytearray(), bytearray()
    ov = dis = nn = 0
    for p in range(I):
        j = I - 1 - p
        in1, in2 = p < L1, j < L2
        assert in1 or in2
        if in1 and not in2:
            b, ph = s1[p], q1[p] - 33
        elif in2 and not in1:
            b, ph = OR.COMP[s2[j]], q2[j] - 33
        else:
            b, ph, d, n = merge_place(s1[p], q1[p] - 33, OR.COMP[s2[j]], q2[j] - 33, floor_q)
            ov += 1
            dis += d
            nn += n
        bases.append(b)
        quals.append(ph + 33)
    return bytes(bases), bytes(quals), ov, dis, nn


def merge_records(raw1, recs1, first_a, raw2, recs2, first_b, count, ins, mark, m):
    """-> (out uint8, report uint64[16], merged bits uint8[(count + 7) / 8]) of the pairs first_a + i / first_b + i with the
    insert sizes ins[i] and the mark bits `mark` (None: every pair), i < count.  Refuses what the call refuses."""
    raw1, raw2 = np.asarray(raw1, dtype=np.uint8), np.asarray(raw2, dtype=np.uint8)
    if not check(m) or ins is None:
        raise Refused("a spec the check refuses, or no inserts")
    if count <= 0 or first_a + count > len(recs1) or first_b + count > len(recs2):
        raise Refused("not a range of both chunks")
    floor_q, min_len = int(m[0]), int(m[1])
    marked = np.ones(count, dtype=bool) if mark is None else PR.bits(mark, count)
    h0 = PR.header_starts(recs1)
    report = np.zeros(REPORT_WORDS, dtype=np.uint64)
    merged = np.zeros(count, dtype=bool)
    pieces = []
    for i in range(count):
        I = int(ins[i])
        if I == 0:
            continue
        ra, rb = recs1[first_a + i], recs2[first_b + i]
        L1, L2 = int(ra["len"]), int(rb["len"])
        if not (L1 <= MAX_LEN and L2 <= MAX_LEN and 1 <= I <= L1 + L2 - 1):
            raise Refused("an insert the lengths do not allow")
        report[WITH_INSERT] += 1
        if not marked[i]:
            report[PAIRS_UNMARKED] += 1
            continue
        if I < min_len:
            report[PAIRS_TOO_SHORT] += 1
            continue
        lines = []
        for raw, rec, L in ((raw1, ra, L1), (raw2, rb, L2)):
            so, qo = int(rec["seq_off"]), int(rec["qual_off"])
            if L == 0 or so + L > len(raw) or qo + L > len(raw):
                raise Refused("a merged pair's record outside its chunk or of length 0")
            lines += [raw[so:so + L].tobytes(), raw[qo:qo + L].tobytes()]
        bases, quals, ov, dis, nn = merge_pair(*lines, I, floor_q)
        head = raw1[int(h0[first_a + i]):int(ra["seq_off"])].tobytes()
        assert head[:1] == b"@" and head[-1:] == b"\n"
        pieces += [head, bases, b"\n+\n", quals, b"\n"]
        merged[i] = True
        report[PAIRS_MERGED] += 1
        report[BASES_MERGED] += I
        report[BYTES_OUT] += len(head) + 2 * I + 4   # (the header line with its '\n')
        report[OVERLAP_BASES] += ov
        report[PLACES_DISAGREE] += dis
        report[PLACES_N] += nn
        report[DROPPED_A] += L1 - min(L1, I)
        report[DROPPED_B] += L2 - min(L2, I)
    report[N_PAIRS] = count
    out = np.frombuffer(b"".join(pieces), dtype=np.uint8)
    assert out.size == int(report[BYTES_OUT])
    return out, report, np.packbits(merged, bitorder="little")


def pair_records_merged(raw1, recs1, raw2, recs2, o, m, c=None, overlap_trim=False, a1=None, a2=None, x=None, t=None, f=None,
                        overlap=None):
    """The whole paired restore with a merged output: overlap, then -- c -- the correction, then the selection of both mates
    exactly as without a merge (the pair bits `keep`), the merge of the kept pairs that have an insert (from the untrimmed,
    possibly corrected mates), and the two mate outputs of the kept pairs that were not merged -> (out1, out2, merged_out,
    report1, report2, counters, summary, correct_report, merge_report).  Every pair is handled on its own."""
    n = len(recs1)
    if n != len(recs2):
        raise ValueError("%d records against %d" % (n, len(recs2)))
    bad = PR.first_mismatch(raw1, recs1, 0, raw2, recs2, 0, n)
    if bad is not None:
        raise ValueError("the ids of record %d differ" % bad)
    summary, la, lb, ins = OR.overlap_records(raw1, recs1, 0, raw2, recs2, 0, n, o) if overlap is None else overlap
    correct_report = None
    if c is not None:
        raw1, raw2, correct_report, _, _ = CR.correct_records(raw1, recs1, 0, raw2, recs2, 0, n, ins, c)
    if not overlap_trim:
        la = lb = None
    k1 = OR.limited_records(raw1, recs1, 0, n, None, la, a1, x, t, f)[2]
    keep = OR.limited_records(raw2, recs2, 0, n, k1, lb, a2, x, t, f)[2]
    merged_out, merge_report, mg = merge_records(raw1, recs1, 0, raw2, recs2, 0, n, ins, keep, m)
    rest = keep & ~mg
    out2, report2, k, _, _ = OR.limited_records(raw2, recs2, 0, n, rest, lb, a2, x, t, f)
    out1, report1, k_again, _, _ = OR.limited_records(raw1, recs1, 0, n, k, la, a1, x, t, f)
    assert np.array_equal(k, k_again) and np.array_equal(k, rest)
    kept, merged = int(report1[R.N_KEPT]), int(merge_report[PAIRS_MERGED])
    assert kept + merged == int(PR.bits(keep, n).sum())
    # (a merged pair passes in both mates and is in neither mark: it shows under dropped_unmarked in both reports)
    m1, m2 = int(report2[PR.DROPPED_UNMARKED]) - merged, int(report1[PR.DROPPED_UNMARKED]) - merged
    assert m2 == int((PR.bits(k1, n) & ~PR.bits(keep, n)).sum())
    counters = dict(pairs=n, kept=kept, dropped_mate1_only=m1, dropped_mate2_only=m2, dropped_both=n - kept - merged - m1 - m2, merged=merged)
    return out1, out2, merged_out, report1, report2, counters, summary, correct_report, merge_report
