"""A pure-Python / numpy restatement of the mate overlap (include/fqgpu.h: fqgpu_chunk_pair_overlap, fqgpu_chunk_select_limited)
from raw chunks and their record tables: the rule for one pair, the 1040-word summary of a range of pairs with the three
per-pair arrays, a selection with a per-record limit in front of its steps, and a whole paired restore with the limits
applied.  Built on pair_ref.py.  Test code: the product never imports it.

The limit is restated without touching tail_ref.  The full lines give a_adapter (tail_ref's place a0) and a0 = min(a_adapter,
limit); the records are then laid out again with both lines cut to a0 and judged WITHOUT an adapter -- every step behind step
0 sees the read as if its length were a0 -- and the words that count against the full length (bases_in, bases_cut_tail,
reads_trimmed, the adapter's two words) are restated from their definitions."""
import zlib

import numpy as np

import pair_ref as PR
import tail_ref as TR
import trim_ref as R

MAX_LEN, ROWS, HEAD = 512, 1024, 16
WORDS = HEAD + ROWS
N_PAIRS, OVERLAPPED, READ_THROUGH, BEHIND_A, BEHIND_B, NOT_ANALYSED, MISMATCHES, OVERLAP_BASES, FINGERPRINT = range(9)
READS_CUT_LIMIT, BASES_CUT_LIMIT = 21, 22
Refused = PR.Refused
COMP = {65: 84, 84: 65, 67: 71, 71: 67, 78: 78}  # A<->T, C<->G, N


def spec(min_overlap=30, max_mism=5, max_err_pct=20):
    return np.array([min_overlap, max_mism, max_err_pct, 0, 0, 0, 0, 0], dtype=np.uint32)


def fingerprint(o):
    return zlib.crc32(np.ascontiguousarray(o, dtype="<u4").tobytes())


def revcomp(s):
    return bytes(COMP[c] for c in reversed(bytes(s)))


def pair_overlap(s1, s2, o):
    """the rule for one pair of sequence lines (bytes over ACGTN, neither longer than MAX_LEN) -> (d, mism, ov) of the first
    hit in the order d = 0, 1, 2, ..., -1, -2, ..., or None"""
    min_overlap, max_mism, pct = int(o[0]), int(o[1]), int(o[2])
    L1, L2 = len(s1), len(s2)
    a, r = np.frombuffer(bytes(s1), dtype=np.uint8), np.frombuffer(revcomp(s2), dtype=np.uint8)
    for d in list(range(0, L1)) + list(range(-1, -L2, -1)):
        lo, hi = max(0, d), min(L1, d + L2)
        ov = hi - lo
        if ov < min_overlap:
            continue
        x, y = a[lo:hi], r[lo - d:hi - d]
        mism = int(((x != y) | (x == 78)).sum())  # (an N on either side: N beside N is a mismatch too)
        if mism <= max_mism and 100 * mism <= pct * ov:
            return d, mism, ov
    return None


def pair_limits(s1, s2, o):
    """-> (limit1, limit2, I) of one pair; a pair that is not analysed is one without a hit"""
    L1, L2 = len(s1), len(s2)
    if L1 > MAX_LEN or L2 > MAX_LEN:
        return L1, L2, 0
    hit = pair_overlap(s1, s2, o)
    if hit is None:
        return L1, L2, 0
    ins = hit[0] + L2
    return min(L1, ins), min(L2, ins), ins


def chunk(seqs, quals=None, names=None):
    """a FASTQ chunk with bare '+' lines from sequence lines (bytes) -> (raw uint8, recs); quals: per record the quality
    line (default: all 'I'); names: the header lines' text behind the '@' (default r<i>)"""
    parts, recs, at = [], np.zeros(len(seqs), dtype=PR.REC_DTYPE), 0
    for i, s in enumerate(seqs):
        s = bytes(s)
        head = b"@" + (names[i] if names else b"r%d" % i) + b"\n"
        q = bytes(quals[i]) if quals else b"I" * len(s)
        assert len(q) == len(s)
        recs[i] = (at + len(head), at + len(head) + len(s) + 3, len(s))
        parts += [head, s, b"\n+\n", q, b"\n"]
        at += len(head) + 2 * len(s) + 4
    return np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), recs


def seq_line(raw, rec):
    off, n = int(rec["seq_off"]), int(rec["len"])
    if n == 0 or off + n > len(raw):
        raise Refused("a record outside its chunk or of length 0")
    return raw[off:off + n].tobytes()


def overlap_records(raw_a, recs_a, first_a, raw_b, recs_b, first_b, count, o):
    """-> (out uint64[WORDS], limit_a, limit_b, insert uint16[count]) of the pairs first_a + i / first_b + i, i < count"""
    raw_a, raw_b = np.asarray(raw_a, dtype=np.uint8), np.asarray(raw_b, dtype=np.uint8)
    if count <= 0 or first_a + count > len(recs_a) or first_b + count > len(recs_b):
        raise Refused("not a range of both chunks")
    out = np.zeros(WORDS, dtype=np.uint64)
    la, lb, ins = (np.zeros(count, dtype=np.uint16) for _ in range(3))
    for i in range(count):
        s1, s2 = seq_line(raw_a, recs_a[first_a + i]), seq_line(raw_b, recs_b[first_b + i])
        L1, L2 = len(s1), len(s2)
        la[i], lb[i] = L1, L2
        if L1 > MAX_LEN or L2 > MAX_LEN:
            out[NOT_ANALYSED] += 1
            continue
        if set(s1 + s2) - set(b"ACGTN"):
            raise Refused("a byte outside ACGTN")
        hit = pair_overlap(s1, s2, o)
        if hit is None:
            continue
        d, mism, ov = hit
        I = d + L2
        assert 1 <= ov <= I < ROWS
        la[i], lb[i], ins[i] = min(L1, I), min(L2, I), I
        out[OVERLAPPED] += 1
        out[READ_THROUGH] += int(la[i] < L1 or lb[i] < L2)
        out[BEHIND_A] += L1 - int(la[i])
        out[BEHIND_B] += L2 - int(lb[i])
        out[MISMATCHES] += mism
        out[OVERLAP_BASES] += ov
        out[HEAD + I] += 1
    out[N_PAIRS] = count
    out[FINGERPRINT] = fingerprint(o)
    assert int(out[HEAD:].sum()) == int(out[OVERLAPPED])
    return out, la, lb, ins


def merge(dst, src):
    """fqgpu_overlap_merge restated -> the sum (dst is not changed)"""
    if int(dst[N_PAIRS]) == 0 and int(dst[FINGERPRINT]) == 0:
        return src.copy()
    if int(dst[FINGERPRINT]) != int(src[FINGERPRINT]):
        raise Refused("different specs")
    if int(dst[N_PAIRS]) == 0:
        return src.copy()
    out = dst + src
    out[FINGERPRINT] = dst[FINGERPRINT]
    return out


# ---------------------------------------------------------------- a selection with limits
def limited_records(raw, recs, first, end, mark=None, limit=None, a=None, x=None, t=None, f=None):
    """-> (out, report, keep, win, places) of the records [first, end) with limit[i] in front of record first + i's steps;
    limit None: pair_ref.marked_records"""
    if limit is None:
        return PR.marked_records(raw, recs, first, end, mark, a, x, t, f)
    raw = np.asarray(raw, dtype=np.uint8)
    n = end - first
    limit = np.asarray(limit, dtype=np.int64)
    assert limit.size == n
    sub, table, full = PR.judged(raw, recs, first, end, a, x, t, f)  # (refuses what the call refuses; its places give a_adapter)
    L = table["len"].astype(np.int64)
    a_adapter = full[4][:, 0].astype(np.int64) if a is not None else L
    a0 = np.minimum(a_adapter, limit)
    # the LIVE records (a0 > 0) with their lines cut to a0 -- header line, s[0, a0), "\n+\n", q[0, a0), '\n' -- as a chunk of
    # their own, judged without an adapter: steps 0b to 5 see the read as if its length were a0.  An emptied read (a0 == 0)
    # is no record of tail_ref's: dropped_short, reads_emptied, window (0, 0), places all zero
    h0 = PR.header_starts(table)
    live = np.flatnonzero(a0 > 0)
    parts, cut, pos = [], np.zeros(live.size, dtype=PR.REC_DTYPE), 0
    for j, r in enumerate(live):
        k, so, qo = int(a0[r]), int(table["seq_off"][r]), int(table["qual_off"][r])
        head = sub[h0[r]:so].tobytes()
        parts += [head, sub[so:so + k].tobytes(), b"\n+\n", sub[qo:qo + k].tobytes(), b"\n"]
        cut[j] = (pos + len(head), pos + len(head) + k + 3, k)
        pos += len(head) + 2 * k + 4
    chunk = np.frombuffer(b"".join(parts), dtype=np.uint8)
    _, cut_report, cut_keep, cut_win, cut_places = TR.tail_records(chunk, cut, None, x, R.trm() if t is None else t, f)
    kept = np.zeros(n, dtype=bool)
    kept[live] = PR.bits(cut_keep, live.size)
    win = np.zeros(n, dtype=np.uint32)
    win[live] = cut_win
    places = np.zeros((n, 4), dtype=np.uint16)
    places[live] = cut_places
    marked = np.ones(n, dtype=bool) if mark is None else PR.bits(mark, n)
    final = kept & marked
    start, kept_n = (win & 0xFFFF).astype(np.int64), (win >> 16).astype(np.int64)
    pieces = []
    for r in np.flatnonzero(final):
        s, k = int(start[r]), int(kept_n[r])
        so, qo = int(table["seq_off"][r]), int(table["qual_off"][r])
        pieces += [sub[h0[r]:so].tobytes(), sub[so + s:so + s + k].tobytes(), b"\n+\n", sub[qo + s:qo + s + k].tobytes(), b"\n"]
    out = np.frombuffer(b"".join(pieces), dtype=np.uint8)
    # the report: the verdicts and the tail trims' words are the cut chunk's, the words that count against the full length
    # are restated from their definitions
    gone = n - live.size
    rep = np.zeros(PR.REPORT_WORDS, dtype=np.uint64)
    rep[R.DROPPED_SHORT:R.DROPPED_SHORT + 5] = cut_report[R.DROPPED_SHORT:R.DROPPED_SHORT + 5]
    rep[R.DROPPED_SHORT] += gone
    rep[R.READS_EMPTIED] = int(cut_report[R.READS_EMPTIED]) + gone
    rep[16:20] = cut_report[16:20]
    rep[R.N_RECORDS] = n
    rep[R.N_KEPT] = int(final.sum())
    rep[R.BASES_IN] = int(L.sum())
    rep[R.BASES_KEPT] = int(kept_n[final].sum())
    rep[R.BYTES_KEPT] = out.size
    rep[R.READS_TRIMMED] = int((kept_n != L).sum())
    rep[R.BASES_CUT_FRONT] = int(start.sum())
    rep[R.BASES_CUT_TAIL] = int((L - start - kept_n).sum())
    rep[14] = int((a0 < L).sum())
    rep[15] = int((L - a0).sum())
    rep[PR.DROPPED_UNMARKED] = int((kept & ~marked).sum())
    rep[READS_CUT_LIMIT] = int((limit < a_adapter).sum())
    rep[BASES_CUT_LIMIT] = int((a_adapter - a0).sum())
    assert n == int(rep[R.N_KEPT]) + int(rep[R.DROPPED_SHORT:R.DROPPED_SHORT + 5].sum()) + int(rep[PR.DROPPED_UNMARKED])
    return out, rep, np.packbits(final, bitorder="little"), win, places


# ---------------------------------------------------------------- a paired restore with the limits applied
def pair_records_trimmed(raw1, recs1, raw2, recs2, o, a1=None, a2=None, x=None, t=None, f=None):
    """pair_ref.pair_records with the mates' overlap limits in front of each mate's steps -> (out1, out2, report1, report2,
    counters, summary)"""
    n = len(recs1)
    if n != len(recs2):
        raise ValueError("%d records against %d" % (n, len(recs2)))
    bad = PR.first_mismatch(raw1, recs1, 0, raw2, recs2, 0, n)
    if bad is not None:
        raise ValueError("the ids of record %d differ" % bad)
    summary, la, lb, _ = overlap_records(raw1, recs1, 0, raw2, recs2, 0, n, o)
    k1 = limited_records(raw1, recs1, 0, n, None, la, a1, x, t, f)[2]
    out2, report2, k, _, _ = limited_records(raw2, recs2, 0, n, k1, lb, a2, x, t, f)
    out1, report1, k_again, _, _ = limited_records(raw1, recs1, 0, n, k, la, a1, x, t, f)
    assert np.array_equal(k, k_again)
    kept, m1, m2 = int(report1[R.N_KEPT]), int(report2[PR.DROPPED_UNMARKED]), int(report1[PR.DROPPED_UNMARKED])
    counters = dict(pairs=n, kept=kept, dropped_mate1_only=m1, dropped_mate2_only=m2, dropped_both=n - kept - m1 - m2)
    return out1, out2, report1, report2, counters, summary
