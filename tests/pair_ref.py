"""A numpy / pure-Python restatement of the paired calls (include/fqgpu.h: fqgpu_chunk_select_marked, fqgpu_chunk_pair_names)
from raw chunks and their record tables: a selection over a record range against a mark -- the kept bytes, the 24-word
report with word 20, the final keep bits, the windows and the places, all relative to the range's first record --, the read
id rule, and a whole paired restore out of the three calls.  Test code: the product never imports it.

A range is restated by cutting the chunk in front of the header line of the range's first record and handing what is left,
with the range's records, to tail_ref.tail_records: a record's verdict depends on its own lines alone."""
import numpy as np

import tail_ref as TR
import trim_ref as R

REC_DTYPE = TR.REC_DTYPE
Refused = TR.Refused
REPORT_WORDS = TR.REPORT_WORDS
DROPPED_UNMARKED = 20


# ---------------------------------------------------------------- the id rule
def id_len(line):
    """the length of the read id of a header line (bytes that start with the '@'): up to the first ' ', '\\t' or '\\n' or the
    line's end, without a "/1" or "/2" at the end"""
    line = bytes(line)
    body = line[1:]
    n = len(body)
    for i, c in enumerate(body):
        if c in b" \t\n":
            n = i
            break
    if n >= 2 and body[n - 2:n] in (b"/1", b"/2"):
        n -= 2
    return n


def header_starts(recs):
    """where the header line of every record starts: behind the record in front"""
    ends = recs["qual_off"].astype(np.int64) + recs["len"].astype(np.int64) + 1
    return np.concatenate(([0], ends[:-1]))


def header_lines(raw, recs):
    """the header line of every record, with its '\\n'"""
    raw = np.asarray(raw, dtype=np.uint8)
    h0 = header_starts(recs)
    return [raw[int(a):int(b)].tobytes() for a, b in zip(h0, recs["seq_off"].astype(np.int64))]


def read_ids(raw, recs):
    return [line[1:1 + id_len(line)] for line in header_lines(raw, recs)]


def first_mismatch(raw_a, recs_a, first_a, raw_b, recs_b, first_b, count):
    """-> the smallest i < count at which the ids of record first_a + i and record first_b + i differ, or None"""
    ia, ib = read_ids(raw_a, recs_a), read_ids(raw_b, recs_b)
    for i in range(count):
        if ia[first_a + i] != ib[first_b + i]:
            return i
    return None


# ---------------------------------------------------------------- a range and a mark
def bits(packed, n):
    return np.unpackbits(np.asarray(packed, dtype=np.uint8), bitorder="little")[:n].astype(bool)


def judged(raw, recs, first, end, a=None, x=None, t=None, f=None):
    """the records [first, end) judged on their own -> what with_mark needs: the range as a chunk of its own (cut in front of
    the header line of its first record), its table, and tail_ref's results for it"""
    raw = np.asarray(raw, dtype=np.uint8)
    if not 0 <= first < end <= len(recs):
        raise Refused("not a range of the chunk")
    cut = int(header_starts(recs)[first])
    sub = raw[cut:]
    table = recs[first:end].astype(REC_DTYPE).copy()
    table["seq_off"] -= cut
    table["qual_off"] -= cut
    return sub, table, TR.tail_records(sub, table, a, x, R.trm() if t is None else t, f)


def with_mark(own, mark=None):
    """-> (out, report, keep, win, places) of a judged range under `mark`: None, or the packed bits of the range (bits behind
    the range are not looked at)"""
    sub, table, (out, report, keep, win, places) = own
    n = len(table)
    kept = bits(keep, n)
    marked = np.ones(n, dtype=bool) if mark is None else bits(mark, n)
    final = kept & marked
    if mark is not None:
        h0 = header_starts(table)
        so, qo = table["seq_off"].astype(np.int64), table["qual_off"].astype(np.int64)
        start, kept_n = (win & 0xFFFF).astype(np.int64), (win >> 16).astype(np.int64)
        parts = []
        for r in np.flatnonzero(final):
            s, k = int(start[r]), int(kept_n[r])
            parts += [sub[h0[r]:so[r]].tobytes(), sub[so[r] + s:so[r] + s + k].tobytes(), b"\n+\n", sub[qo[r] + s:qo[r] + s + k].tobytes(), b"\n"]
        out = np.frombuffer(b"".join(parts), dtype=np.uint8)
        report = report.copy()
        report[R.N_KEPT] = int(final.sum())
        report[R.BASES_KEPT] = int(kept_n[final].sum())
        report[R.BYTES_KEPT] = out.size
        report[DROPPED_UNMARKED] = int((kept & ~marked).sum())
    assert int(report[R.N_RECORDS]) == n == int(report[R.N_KEPT]) + int(report[R.DROPPED_SHORT:R.DROPPED_SHORT + 5].sum()) + int(report[DROPPED_UNMARKED])
    return out, report, np.packbits(final, bitorder="little"), win, places


def marked_records(raw, recs, first, end, mark=None, a=None, x=None, t=None, f=None):
    """-> (out, report, keep, win, places) of the records [first, end), everything relative to `first`.  mark: None, or the
    packed bits of the range; a, x, t, f None: off."""
    return with_mark(judged(raw, recs, first, end, a, x, t, f), mark)


# ---------------------------------------------------------------- a paired restore
def pair_records(raw1, recs1, raw2, recs2, a1=None, a2=None, x=None, t=None, f=None):
    """Two files whose records are mates, a pair kept only if both mates pass -> (out1, out2, report1, report2, counters):
    the three calls of a paired restore on whole files; counters: dict(pairs, kept, dropped_mate1_only, dropped_mate2_only,
    dropped_both).  ValueError: the files have different record counts, or a pair's ids differ."""
    n = len(recs1)
    if n != len(recs2):
        raise ValueError("%d records against %d" % (n, len(recs2)))
    bad = first_mismatch(raw1, recs1, 0, raw2, recs2, 0, n)
    if bad is not None:
        raise ValueError("the ids of record %d differ" % bad)
    own1, own2 = judged(raw1, recs1, 0, n, a1, x, t, f), judged(raw2, recs2, 0, n, a2, x, t, f)
    k1 = with_mark(own1)[2]
    out2, report2, k, _, _ = with_mark(own2, k1)
    out1, report1, k_again, _, _ = with_mark(own1, k)
    assert np.array_equal(k, k_again)
    kept, m1, m2 = int(report1[R.N_KEPT]), int(report2[DROPPED_UNMARKED]), int(report1[DROPPED_UNMARKED])
    assert kept == int(report2[R.N_KEPT])
    return out1, out2, report1, report2, dict(pairs=n, kept=kept, dropped_mate1_only=m1, dropped_mate2_only=m2, dropped_both=n - kept - m1 - m2)
