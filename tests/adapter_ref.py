"""A numpy / pure-Python restatement of adapter clipping (include/fqgpu.h: fqgpu_chunk_clip) from a raw chunk and its record
table: the clipped, trimmed canonical bytes of the kept records, the 16-word report, the keep bits, the windows and the clip
places.  Test code: the product never imports it.

The search is here in four forms that are asserted equal: `find_serial`, the definition, place by place; `find_planes`, the
form the device computes (the line and the adapter as four bit planes, the MATCHES at a place a population count, the planes
zero outside the line and behind the adapter's end); `find`, the same by one vector comparison per adapter base, and
`find_all`, that over all the records of a chunk at once, which `clip_records` uses so that a read of 65535 symbols, or a
file of some MiB, costs nothing."""
import numpy as np

import filter_ref as FR
import trim_ref as R

NONE = FR.NONE
Refused = FR.Refused
REC_DTYPE = FR.REC_DTYPE
REPORT_WORDS = R.REPORT_WORDS
READS_WITH_ADAPTER, BASES_CUT_ADAPTER = 14, 15
ADAPTER_MAX = 64
ADAPTER_WORDS = ADAPTER_MAX // 4 + 4


def adp(seq, min_overlap=5, max_err_pct=10, reserved=0, length=None):
    """an fqgpu_adapter as its twenty uint32 words: seq in sixty-four bytes, zero behind it, then len (length when it is not
    len(seq)), min_overlap, max_err_pct, reserved"""
    seq = seq.encode() if isinstance(seq, str) else bytes(seq)
    a = np.zeros(ADAPTER_WORDS, dtype=np.uint32)
    a[:ADAPTER_MAX // 4].view(np.uint8)[:min(len(seq), ADAPTER_MAX)] = np.frombuffer(seq[:ADAPTER_MAX], dtype=np.uint8)
    a[ADAPTER_MAX // 4:] = (len(seq) if length is None else length, min_overlap, max_err_pct, reserved)
    return a


def fields(a):
    """-> (the sixty-four bytes, len, min_overlap, max_err_pct, reserved)"""
    a = np.ascontiguousarray(a, dtype=np.uint32)
    return (a[:ADAPTER_MAX // 4].view(np.uint8),) + tuple(int(x) for x in a[ADAPTER_MAX // 4:])


def check(a):
    """what fqgpu_adapter_check accepts"""
    seq, m, min_overlap, pct, reserved = fields(a)
    if not 1 <= m <= ADAPTER_MAX or not 1 <= min_overlap <= m or pct > 50 or reserved:
        return False
    return bool(np.isin(seq[:m], np.frombuffer(b"ACGT", dtype=np.uint8)).all()) and not seq[m:].any()


# ---------------------------------------------------------------- the search: a sequence line -> the clip place
def find_serial(s, A, min_overlap, pct):
    """the definition: the smallest p with ov = min(m, L - p) >= min_overlap and 100 * mism(p) <= pct * ov, or L"""
    s, A = bytes(s), bytes(A)
    L, m = len(s), len(A)
    for p in range(L):
        ov = min(m, L - p)
        mism = sum(1 for j in range(ov) if s[p + j] != A[j])
        if ov >= min_overlap and 100 * mism <= pct * ov:
            return p
    return L


def planes_of(s):
    """four integers: bit i of plane b is set iff s[i] is base b of ACGT (an N, like everything outside s, is in none)"""
    s = np.frombuffer(bytes(s), dtype=np.uint8)
    return [int.from_bytes(np.packbits(s == c, bitorder="little").tobytes(), "little") for c in b"ACGT"]


def find_planes(s, A, min_overlap, pct, lead=0):
    """the device's form: the line sits `lead` bytes into its first 16-byte word and is looked at word by word, sixteen places
    a word; a place sees the 64 bases from it as bits, the matches are the population count of the planes ANDed with the
    adapter's, and a hit is ov >= min_overlap and 100 * matches >= (100 - pct) * ov"""
    L, m = len(s), len(A)
    read = [p << lead for p in planes_of(s)]
    adapter = planes_of(A)
    best = None
    for word in range((lead + L + 15) // 16):
        hits = 0
        for j in range(16):
            p = 16 * word + j - lead
            matches = bin(sum(((read[b] >> (16 * word + j)) & (2 ** 64 - 1) & adapter[b]) for b in range(4))).count("1")
            ov = min(m, L - p)
            if p >= 0 and ov >= min_overlap and 100 * matches >= (100 - pct) * ov:
                hits |= 1 << j
        if hits and best is None:
            best = 16 * word - lead + (hits & -hits).bit_length() - 1
    return L if best is None else best


def find(s, A, min_overlap, pct):
    """the same by one comparison per adapter base over all places at once"""
    s = np.asarray(s, dtype=np.uint8)
    L, m = s.size, len(A)
    mism = np.zeros(L, dtype=np.int64)
    for j in range(min(m, L)):
        mism[:L - j] += s[j:] != A[j]
    ov = np.minimum(m, L - np.arange(L))
    hit = np.flatnonzero((ov >= min_overlap) & (100 * mism <= pct * ov))
    return int(hit[0]) if hit.size else L


def find_all(raw, so, lens, A, min_overlap, pct):
    """`find` for every record of a chunk at once (sequence lines at raw[so[r], so[r] + lens[r])) -> the clip places"""
    A = bytes(A)
    m, total = len(A), int(lens.sum())
    rec = np.repeat(np.arange(lens.size), lens)
    p = np.arange(total) - np.repeat(np.cumsum(lens) - lens, lens)
    pos, rem = so[rec] + p, lens[rec] - p          # where the place lies in the chunk; the bases from it to the line's end
    padded = np.concatenate((np.asarray(raw, dtype=np.uint8), np.zeros(m, dtype=np.uint8)))
    mism = np.zeros(total, dtype=np.int64)
    for j in range(m):
        mism += (j < rem) & (padded[pos + j] != A[j])
    ov = np.minimum(m, rem)
    hit = np.flatnonzero((ov >= min_overlap) & (100 * mism <= pct * ov))[::-1]
    clip = lens.copy()
    clip[rec[hit]] = p[hit]          # (in falling order of the places: the smallest one of a record is written last)
    return clip


def clip_records(raw, recs, a, t=None, f=None):
    """-> (out, report, keep, win, clip): what trim_ref.trim_records returns, for the records clipped at the adapter `a` first
    (step 0), and the clip places (int64[n]).  a None: exactly the trim (t is then needed); t None: nothing is cut beyond the
    clip; f None: every read that is not emptied is kept.  Refused: what the device refuses."""
    raw = np.asarray(raw, dtype=np.uint8)
    if a is None:
        if t is None:
            raise Refused("no adapter and no trim")
        return R.trim_records(raw, recs, t, f) + (recs["len"].astype(np.int64),)
    t = R.trm() if t is None else t
    f = FR.flt() if f is None else f
    if not check(a) or not R.check(t) or not FR.check(f):
        raise Refused("an adapter, a trim or a filter its check refuses")
    seq64, m, min_overlap, pct, _ = fields(a)
    A = seq64[:m].tobytes()
    q_front, q_tail = int(t[2]), int(t[3])
    min_len, max_len, max_n, min_mean_q, low_q, low_pct = (int(x) for x in f[:6])
    n = len(recs)
    report = np.zeros(REPORT_WORDS, dtype=np.uint64)
    if n == 0:
        return np.zeros(0, dtype=np.uint8), report, np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.int64)
    lens = recs["len"].astype(np.int64)
    so, qo = recs["seq_off"].astype(np.int64), recs["qual_off"].astype(np.int64)
    if (lens == 0).any() or (lens > 65535).any() or (so + lens > raw.size).any() or (qo + lens > raw.size).any():
        raise Refused("a record outside the chunk, or without symbols")
    need_qual = bool(q_front or q_tail or min_mean_q or low_q)
    # the sequence line is always read here, and judged over all its bytes; the quality line by the trim's rule
    seq, qual, _ = FR.per_record(raw, recs)
    if not np.isin(seq, np.frombuffer(b"ACGTN", dtype=np.uint8)).all():
        raise Refused("a sequence byte outside ACGTN")
    if need_qual and (qual.min() < 33 or qual.max() > 96):
        raise Refused("a quality byte outside 33 .. 96")
    clip = find_all(raw, so, lens, A, min_overlap, pct)
    start = np.zeros(n, dtype=np.int64)
    kept_n = np.zeros(n, dtype=np.int64)
    n_per = np.zeros(n, dtype=np.int64)
    q_per = np.zeros(n, dtype=np.int64)
    low_per = np.zeros(n, dtype=np.int64)
    for r in range(n):
        L = int(lens[r])
        at = int(clip[r])
        phred = raw[qo[r]:qo[r] + at].astype(np.int64) - 33 if need_qual else np.zeros(at, dtype=np.int64)
        s, k = R.window(phred, t)     # steps 1 .. 4 on the read as if its length were the clip place
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
    report[READS_WITH_ADAPTER] = int((clip < lens).sum())
    report[BASES_CUT_ADAPTER] = int((lens - clip).sum())
    assert out.size == int(report[R.BYTES_KEPT])
    assert int(report[R.BASES_IN]) == int(report[R.BASES_CUT_FRONT]) + int(report[R.BASES_CUT_TAIL]) + int(kept_n.sum())
    return out, report, np.packbits(kept, bitorder="little"), (start | kept_n << 16).astype(np.uint32), clip


def clip_chunk(raw, a, t=None, f=None):
    """the same for a FASTQ chunk, parsed here"""
    raw = np.asarray(raw, dtype=np.uint8)
    return clip_records(raw, FR.parse(raw), a, t, f)
