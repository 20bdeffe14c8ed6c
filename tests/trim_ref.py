"""A numpy / pure-Python restatement of read trimming (include/fqgpu.h: fqgpu_chunk_trim) from a raw chunk and its record table:
the trimmed canonical bytes of the kept records, the 16-word report, the keep bits and the windows.  Test code: the product
never imports it.

The running-sum walk is here in three forms that are asserted equal: `walk_serial`, the definition, word for word;
`walk_pieces`, the form the device computes (pieces summarised by total, smallest prefix, largest prefix and its first place;
entering sums by a prefix sum; only the piece the walk stops in is walked byte by byte); `walk`, the same by cumulative sums
in numpy, which `trim_records` uses so that a read of 65535 symbols costs nothing."""
import numpy as np

import filter_ref as FR

NONE = FR.NONE
Refused = FR.Refused
REC_DTYPE = FR.REC_DTYPE
REPORT_WORDS = 16
N_RECORDS, N_KEPT, BASES_IN, BASES_KEPT, BYTES_KEPT, DROPPED_SHORT, DROPPED_LONG, DROPPED_N, DROPPED_MEAN_Q, DROPPED_LOW_Q = range(10)
READS_TRIMMED, BASES_CUT_FRONT, BASES_CUT_TAIL, READS_EMPTIED = 10, 11, 12, 13


def trm(cut_front=0, cut_tail=0, q_front=0, q_tail=0, crop=NONE, reserved=(0, 0, 0)):
    """an fqgpu_trim as its eight uint32 words; the defaults cut nothing"""
    return np.array([cut_front, cut_tail, q_front, q_tail, crop, reserved[0], reserved[1], reserved[2]], dtype=np.uint32)


def check(t):
    """what fqgpu_trim_check accepts"""
    cut_front, cut_tail, q_front, q_tail, crop, r0, r1, r2 = (int(x) for x in t)
    return cut_front <= 65535 and cut_tail <= 65535 and q_front <= 64 and q_tail <= 64 and crop != 0 and r0 == 0 and r1 == 0 and r2 == 0


# ---------------------------------------------------------------- the walk: increments in walk order -> symbols cut
def walk_serial(inc):
    """the definition: s = 0, best = 0; s += inc; s < 0: stop; s > best (strictly): best = s, cut up to and with this one"""
    s = best = cut = 0
    for j, x in enumerate(inc):
        s += int(x)
        if s < 0:
            break
        if s > best:
            best, cut = s, j + 1
    return cut


def walk_pieces(inc, bounds):
    """the same from pieces inc[bounds[k]:bounds[k + 1]] (bounds[0] == 0, bounds[-1] == len(inc), empty pieces allowed)"""
    inc = [int(x) for x in inc]
    pieces = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        s = mn = mx = 0     # (the empty prefix counts: a piece whose prefixes never rise above 0 offers no candidate)
        place = None
        for j in range(lo, hi):
            s += inc[j]
            mn = min(mn, s)
            if s > mx:
                mx, place = s, j + 1
        pieces.append((s, mn, mx, place))
    entering = np.concatenate(([0], np.cumsum([p[0] for p in pieces]))).tolist()
    stops = [k for k, p in enumerate(pieces) if entering[k] + p[1] < 0]
    stop_at = stops[0] if stops else len(pieces)
    best = cut = 0
    for k in range(stop_at):            # valid as a whole; equal candidates: the earlier piece
        if pieces[k][3] is not None and entering[k] + pieces[k][2] > best:
            best, cut = entering[k] + pieces[k][2], pieces[k][3]
    if stop_at < len(pieces):           # the piece the walk stops in: byte by byte
        s = entering[stop_at]
        for j in range(bounds[stop_at], bounds[stop_at + 1]):
            s += inc[j]
            if s < 0:
                break
            if s > best:
                best, cut = s, j + 1
    return cut


def walk(inc):
    """the same by cumulative sums: among the prefixes in front of the first negative one, the first largest, if above 0"""
    inc = np.asarray(inc, dtype=np.int64)
    if inc.size == 0:
        return 0
    s = np.cumsum(inc)
    neg = np.flatnonzero(s < 0)
    s = s[:neg[0]] if neg.size else s
    if s.size == 0 or s.max() <= 0:
        return 0
    return int(np.argmax(s)) + 1


def window(phred, t):
    """steps 1 .. 4 for one read: its Phred values (None when no walk is on) and an fqgpu_trim -> (start, n)"""
    cut_front, cut_tail, q_front, q_tail, crop = (int(x) for x in t[:5])
    L = len(phred)
    f = min(cut_front, L)
    tl = min(cut_tail, L - f)
    start, stop = f, L - tl
    if q_front:
        start = f + walk(q_front - phred[f:L - tl])
    if q_tail:
        stop = L - tl - walk(q_tail - phred[f:L - tl][::-1])
    if start >= stop:
        return 0, 0
    return start, min(stop - start, crop)


def trim_records(raw, recs, t, f=None):
    """-> (out, report, keep, win): the trimmed canonical bytes of the records of `recs` that pass `f` after the trim `t`
    (uint8 array), the report (uint64[16]), the keep bits (uint8[(n + 7) // 8]) and the windows start | n << 16 (uint32[n]).
    f None: every read that is not emptied is kept.  Refused: what the device refuses."""
    raw = np.asarray(raw, dtype=np.uint8)
    f = FR.flt() if f is None else f
    if not check(t) or not FR.check(f):
        raise Refused("a trim fqgpu_trim_check refuses, or a filter fqgpu_filter_check refuses")
    q_front, q_tail = int(t[2]), int(t[3])
    min_len, max_len, max_n, min_mean_q, low_q, pct = (int(x) for x in f[:6])
    n = len(recs)
    report = np.zeros(REPORT_WORDS, dtype=np.uint64)
    if n == 0:
        return np.zeros(0, dtype=np.uint8), report, np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint32)
    lens = recs["len"].astype(np.int64)
    so, qo = recs["seq_off"].astype(np.int64), recs["qual_off"].astype(np.int64)
    if (lens == 0).any() or (lens > 65535).any() or (so + lens > raw.size).any() or (qo + lens > raw.size).any():
        raise Refused("a record outside the chunk, or without symbols")
    need_seq, need_qual = max_n != NONE, bool(q_front or q_tail or min_mean_q or low_q)
    # a line that is read is judged over all its bytes, the cut ones too; a line that is not read is not looked at
    if need_seq or need_qual:
        seq, qual, _ = FR.per_record(raw, recs)
        if need_seq and not np.isin(seq, np.frombuffer(b"ACGTN", dtype=np.uint8)).all():
            raise Refused("a sequence byte outside ACGTN")
        if need_qual and (qual.min() < 33 or qual.max() > 96):
            raise Refused("a quality byte outside 33 .. 96")
    start = np.zeros(n, dtype=np.int64)
    kept_n = np.zeros(n, dtype=np.int64)
    n_per = np.zeros(n, dtype=np.int64)
    q_per = np.zeros(n, dtype=np.int64)
    low_per = np.zeros(n, dtype=np.int64)
    for r in range(n):
        L = int(lens[r])
        phred = raw[qo[r]:qo[r] + L].astype(np.int64) - 33 if need_qual else np.zeros(L, dtype=np.int64)
        s, m = window(phred, t)
        start[r], kept_n[r] = s, m
        if need_seq:
            n_per[r] = int((raw[so[r] + s:so[r] + s + m] == ord("N")).sum())
        if need_qual:
            q_per[r] = int(phred[s:s + m].sum())
            low_per[r] = int((phred[s:s + m] < low_q).sum())
    emptied = kept_n == 0
    # the first failing criterion, in the report's order, judged on what is left; an emptied read is "short"
    verdict = np.zeros(n, dtype=np.int64)
    fails = [(kept_n < min_len) | emptied, kept_n > max_len, (n_per > max_n) if need_seq else np.zeros(n, bool),
             (q_per < min_mean_q * kept_n) if min_mean_q else np.zeros(n, bool),
             (100 * low_per > pct * kept_n) if low_q else np.zeros(n, bool)]
    for code in (5, 4, 3, 2, 1):
        verdict[fails[code - 1]] = code
    kept = verdict == 0
    h0 = np.concatenate(([0], (qo + lens + 1)[:-1]))
    hl = np.maximum(so - h0, 0)
    size = hl + 2 * kept_n + 4
    parts = []
    for r in np.flatnonzero(kept):
        s, m = int(start[r]), int(kept_n[r])
        parts += [raw[h0[r]:h0[r] + hl[r]].tobytes(), raw[so[r] + s:so[r] + s + m].tobytes(), b"\n+\n", raw[qo[r] + s:qo[r] + s + m].tobytes(), b"\n"]
    out = np.frombuffer(b"".join(parts), dtype=np.uint8)
    report[N_RECORDS], report[N_KEPT] = n, int(kept.sum())
    report[BASES_IN], report[BASES_KEPT] = int(lens.sum()), int(kept_n[kept].sum())
    report[BYTES_KEPT] = int(size[kept].sum())
    for code in range(1, 6):
        report[DROPPED_SHORT + code - 1] = int((verdict == code).sum())
    report[READS_TRIMMED] = int((kept_n != lens).sum())
    report[BASES_CUT_FRONT] = int(start.sum())
    report[BASES_CUT_TAIL] = int((lens - start - kept_n).sum())
    report[READS_EMPTIED] = int(emptied.sum())
    assert out.size == int(report[BYTES_KEPT])
    assert int(report[BASES_IN]) == int(report[BASES_CUT_FRONT]) + int(report[BASES_CUT_TAIL]) + int(kept_n.sum())
    return out, report, np.packbits(kept, bitorder="little"), (start | kept_n << 16).astype(np.uint32)


def trim_chunk(raw, t, f=None):
    """the same for a FASTQ chunk, parsed here"""
    raw = np.asarray(raw, dtype=np.uint8)
    return trim_records(raw, FR.parse(raw), t, f)
