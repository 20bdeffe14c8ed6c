"""A numpy / pure-Python restatement of the tail trims (include/fqgpu.h: fqgpu_chunk_tailtrim) from a raw chunk and its record
table: the poly-X tail (step 0b) and the sliding-window quality cut (step 1b) between the adapter clip and the trim's steps --
the kept bytes, the 24-word report, the keep bits, the windows and the places a0, a1, e, e2.  Test code: the product never
imports it.

Both rules are here in two forms that are asserted equal: `poly_serial` / `window_serial`, the definition, place by place, and
`poly_all` / `window_all`, the same over all the records of a chunk at once by cumulative sums, which `tail_records` uses so
that a read of 65535 symbols, or a file of some MiB, costs nothing.  Step 0 is adapter_ref's, the walks and the crop are
trim_ref's, the checks and the parsing filter_ref's."""
import numpy as np

import adapter_ref as AR
import filter_ref as FR
import trim_ref as R

NONE = FR.NONE
Refused = FR.Refused
REC_DTYPE = FR.REC_DTYPE
REPORT_WORDS = 24
READS_WITH_POLY, BASES_CUT_POLY, READS_WINDOW_CUT, BASES_CUT_WINDOW = 16, 17, 18, 19
BASE_BITS = {"A": 1, "C": 2, "G": 4, "T": 8}
ALL = 15


def tl(poly=0, poly_min_len=None, poly_every=None, poly_max_mism=None, window_len=0, window_q=0, reserved=(0, 0)):
    """an fqgpu_tail as its eight uint32 words.  poly: the set, a string over ACGT or the bit mask; with a set the other three
    default to 10, 8 and 5, without one to zero.  The defaults cut nothing."""
    bases = sum(BASE_BITS[c] for c in set(poly)) if isinstance(poly, str) else int(poly)
    pick = lambda v, d: (d if bases else 0) if v is None else v  # noqa: E731
    return np.array([bases, pick(poly_min_len, 10), pick(poly_every, 8), pick(poly_max_mism, 5), window_len, window_q, reserved[0], reserved[1]],
                    dtype=np.uint32)


def check(x):
    """what fqgpu_tail_check accepts"""
    bases, min_len, every, max_mism, W, Q, r0, r1 = (int(v) for v in x)
    if bases > 15 or max_mism > 255 or W > 32 or r0 or r1:
        return False
    if bases:
        if not 1 <= min_len <= 65535 or not 2 <= every <= 255:
            return False
    elif min_len or every:
        return False
    return 1 <= Q <= 64 if W else Q == 0


def is_on(x):
    return x is not None and bool(int(x[0]) or int(x[4]))


# ---------------------------------------------------------------- step 0b: a sequence line and a0 -> the length of the tail
def poly_serial_base(s, a0, X, min_len, every, max_mism):
    """the definition for one base X (a byte value): t_X"""
    mism = 0
    t = 0
    for i in range(1, a0 + 1):
        b = s[a0 - i]
        mism += b != X
        if mism > min(i // every, max_mism):
            break               # the FIRST violation: nothing behind it counts
        if b == X:
            t = i               # (the largest i in front of the violation at which X stands)
    return t if t >= min_len else 0


def poly_serial(s, a0, x):
    """-> t, the largest t_X over the set of the tail x"""
    bases, min_len, every, max_mism = (int(v) for v in x[:4])
    s = bytes(s)
    return max([poly_serial_base(s, a0, ord(c), min_len, every, max_mism) for c, bit in BASE_BITS.items() if bases & bit] + [0])


def poly_all(raw, so, a0, x):
    """`poly_serial` for every record of a chunk at once (sequence lines from raw[so[r]], clip places a0[r]) -> t (int64[n])"""
    bases, min_len, every, max_mism = (int(v) for v in x[:4])
    n = a0.size
    t = np.zeros(n, dtype=np.int64)
    live = np.flatnonzero(a0 > 0)
    if not bases or not live.size:
        return t
    cnt = a0[live]
    first = np.cumsum(cnt) - cnt                    # where a record's tail places begin in the flat arrays
    rec = np.repeat(np.arange(live.size), cnt)
    i = np.arange(int(cnt.sum())) - first[rec] + 1    # the tail place, 1 .. a0
    b = np.asarray(raw, dtype=np.uint8)[so[live][rec] + cnt[rec] - i]
    allowed = np.minimum(i // every, max_mism)
    for c, bit in BASE_BITS.items():
        if not bases & bit:
            continue
        miss = (b != ord(c)).astype(np.int64)
        cum = np.cumsum(miss)
        cum -= (cum[first] - miss[first])[rec]      # mism_X(i) of the place's own record
        v = np.minimum.reduceat(np.where(cum > allowed, i, 1 << 30), first)
        tx = np.maximum.reduceat(np.where((b == ord(c)) & (i < v[rec]), i, 0), first)
        tx[tx < min_len] = 0
        t[live] = np.maximum(t[live], tx)
    return t


# ---------------------------------------------------------------- step 1b: Phred values and [f, e) -> e2
def window_serial(phred, f, e, W, Q):
    """the definition"""
    p = f
    while p + W <= e:
        if sum(int(v) for v in phred[p:p + W]) < Q * W:
            i = p
            while phred[i] >= Q:      # (it exists inside the window: a window of bases >= Q sums to at least Q * W)
                i += 1
            assert i < p + W
            return i
        p += 1
    return e


def window_all(raw, qo, f, e, W, Q):
    """`window_serial` for every record of a chunk at once (quality lines from raw[qo[r]]) -> e2 (int64[n])"""
    raw = np.asarray(raw, dtype=np.uint8)
    e2 = e.copy()
    cnt = np.maximum(e - f - W + 1, 0)          # the windows of a record
    live = np.flatnonzero(cnt > 0)
    if not W or not live.size:
        return e2
    prefix = np.concatenate(([0], np.cumsum(raw.astype(np.int64) - 33)))
    c = cnt[live]
    first = np.cumsum(c) - c
    rec = np.repeat(np.arange(live.size), c)
    p = np.arange(int(c.sum())) - first[rec] + f[live][rec]
    at = qo[live][rec] + p
    fails = prefix[at + W] - prefix[at] < Q * W
    where = np.minimum.reduceat(np.where(fails, p, 1 << 30), first)
    hit = where < (1 << 30)
    rows, p0 = live[hit], where[hit]
    got = np.full(rows.size, -1, dtype=np.int64)
    for i in range(W - 1, -1, -1):              # (downwards: the smallest i is written last)
        low = raw[qo[rows] + p0 + i].astype(np.int64) - 33 < Q
        got[low] = p0[low] + i
    assert (got >= 0).all()
    e2[rows] = got
    return e2


# ---------------------------------------------------------------- the whole call
def tail_records(raw, recs, a=None, x=None, t=None, f=None):
    """-> (out, report, keep, win, places): the forms of adapter_ref.clip_records with a report of 24 words and the places
    a0, a1, e, e2 (uint16[n, 4]).  a None: no adapter; x None, or both rules off: adapter_ref.clip_records with the same a, t,
    f; t None: no fixed cuts, no walks, no crop; f None: every read that is not emptied is kept.  Refused: what the device
    refuses."""
    raw = np.asarray(raw, dtype=np.uint8)
    if x is not None and not check(x):
        raise Refused("a tail fqgpu_tail_check refuses")
    n = len(recs)
    if not is_on(x):
        out, report, keep, win, clip = AR.clip_records(raw, recs, a, t, f)
        tt = R.trm() if t is None else t
        f0 = np.minimum(int(tt[0]), clip)
        e0 = clip - np.minimum(int(tt[1]), clip - f0)
        places = np.stack([clip, clip, e0, e0], axis=1).astype(np.uint16) if n else np.zeros((0, 4), dtype=np.uint16)
        return out, np.concatenate((report, np.zeros(REPORT_WORDS - len(report), dtype=np.uint64))), keep, win, places
    t = R.trm() if t is None else t
    f = FR.flt() if f is None else f
    if (a is not None and not AR.check(a)) or not R.check(t) or not FR.check(f):
        raise Refused("an adapter, a trim or a filter its check refuses")
    bases, W, Q = int(x[0]), int(x[4]), int(x[5])
    cut_front, cut_tail, q_front, q_tail = (int(v) for v in t[:4])
    min_len, max_len, max_n, min_mean_q, low_q, low_pct = (int(v) for v in f[:6])
    report = np.zeros(REPORT_WORDS, dtype=np.uint64)
    if n == 0:
        return np.zeros(0, dtype=np.uint8), report, np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint32), np.zeros((0, 4), dtype=np.uint16)
    lens = recs["len"].astype(np.int64)
    so, qo = recs["seq_off"].astype(np.int64), recs["qual_off"].astype(np.int64)
    if (lens == 0).any() or (lens > 65535).any() or (so + lens > raw.size).any() or (qo + lens > raw.size).any():
        raise Refused("a record outside the chunk, or without symbols")
    need_seq = max_n != NONE or a is not None or bases != 0
    need_qual = bool(q_front or q_tail or min_mean_q or low_q or W)
    seq, qual, _ = FR.per_record(raw, recs)
    if need_seq and not np.isin(seq, np.frombuffer(b"ACGTN", dtype=np.uint8)).all():
        raise Refused("a sequence byte outside ACGTN")
    if need_qual and (qual.min() < 33 or qual.max() > 96):
        raise Refused("a quality byte outside 33 .. 96")
    # step 0: the clip places, by adapter_ref
    a0 = lens.copy() if a is None else AR.clip_records(raw, recs, a)[4].astype(np.int64)
    a1 = a0 - poly_all(raw, so, a0, x)                          # step 0b
    fcut = np.minimum(cut_front, a1)                           # step 1
    e = a1 - np.minimum(cut_tail, a1 - fcut)
    e2 = window_all(raw, qo, fcut, e, W, Q)                    # step 1b
    assert (fcut <= e2).all() and (e2 <= e).all()
    walks = R.trm(cut_front, 0, q_front, q_tail, int(t[4]))    # steps 2 .. 4 over [f, e2): cut_tail is in e already
    start = np.zeros(n, dtype=np.int64)
    kept_n = np.zeros(n, dtype=np.int64)
    n_per = np.zeros(n, dtype=np.int64)
    q_per = np.zeros(n, dtype=np.int64)
    low_per = np.zeros(n, dtype=np.int64)
    for r in range(n):
        at = int(e2[r])
        phred = raw[qo[r]:qo[r] + at].astype(np.int64) - 33 if need_qual else np.zeros(at, dtype=np.int64)
        s, k = R.window(phred, walks)
        start[r], kept_n[r] = s, k
        n_per[r] = int((raw[so[r] + s:so[r] + s + k] == ord("N")).sum())
        if need_qual:
            q_per[r] = int(phred[s:s + k].sum())
            low_per[r] = int((phred[s:s + k] < low_q).sum())
    emptied = kept_n == 0
    verdict = np.zeros(n, dtype=np.int64)
    fails = [(kept_n < min_len) | emptied, kept_n > max_len, (n_per > max_n) if max_n != NONE else np.zeros(n, bool),
             (q_per < min_mean_q * kept_n) if min_mean_q else np.zeros(n, bool),
             (100 * low_per > low_pct * kept_n) if low_q else np.zeros(n, bool)]
    for code in (5, 4, 3, 2, 1):
        verdict[fails[code - 1]] = code
    kept = verdict == 0
    h0 = np.concatenate(([0], (qo + lens + 1)[:-1]))
    hl = np.maximum(so - h0, 0)
    size = hl + 2 * kept_n + 4
    parts = []
    for r in np.flatnonzero(kept):
        s, k = int(start[r]), int(kept_n[r])
        parts += [raw[h0[r]:h0[r] + hl[r]].tobytes(), raw[so[r] + s:so[r] + s + k].tobytes(), b"\n+\n", raw[qo[r] + s:qo[r] + s + k].tobytes(), b"\n"]
    out = np.frombuffer(b"".join(parts), dtype=np.uint8)
    report[R.N_RECORDS], report[R.N_KEPT] = n, int(kept.sum())
    report[R.BASES_IN], report[R.BASES_KEPT] = int(lens.sum()), int(kept_n[kept].sum())
    report[R.BYTES_KEPT] = int(size[kept].sum())
    for code in range(1, 6):
        report[R.DROPPED_SHORT + code - 1] = int((verdict == code).sum())
    report[R.READS_TRIMMED] = int((kept_n != lens).sum())
    report[R.BASES_CUT_FRONT] = int(start.sum())
    report[R.BASES_CUT_TAIL] = int((lens - start - kept_n).sum())
    report[R.READS_EMPTIED] = int(emptied.sum())
    report[AR.READS_WITH_ADAPTER] = int((a0 < lens).sum())
    report[AR.BASES_CUT_ADAPTER] = int((lens - a0).sum())
    report[READS_WITH_POLY] = int((a1 < a0).sum())
    report[BASES_CUT_POLY] = int((a0 - a1).sum())
    report[READS_WINDOW_CUT] = int((e2 < e).sum())
    report[BASES_CUT_WINDOW] = int((e - e2).sum())
    assert out.size == int(report[R.BYTES_KEPT])
    assert int(report[R.BASES_IN]) == int(report[R.BASES_CUT_FRONT]) + int(report[R.BASES_CUT_TAIL]) + int(kept_n.sum())
    places = np.stack([a0, a1, e, e2], axis=1).astype(np.uint16)
    return out, report, np.packbits(kept, bitorder="little"), (start | kept_n << 16).astype(np.uint32), places


def tail_chunk(raw, a=None, x=None, t=None, f=None):
    """the same for a FASTQ chunk, parsed here"""
    raw = np.asarray(raw, dtype=np.uint8)
    return tail_records(raw, FR.parse(raw), a, x, t, f)
