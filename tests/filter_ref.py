"""A numpy / pure-Python restatement of the read filter (include/fqgpu.h: fqgpu_chunk_filter) from a raw chunk: the canonical
bytes of the kept records, the 16-word report and the keep bits.  Test code: the product never imports it."""
import numpy as np

NONE = 0xFFFFFFFF
REPORT_WORDS = 16
N_RECORDS, N_KEPT, BASES_IN, BASES_KEPT, BYTES_KEPT, DROPPED_SHORT, DROPPED_LONG, DROPPED_N, DROPPED_MEAN_Q, DROPPED_LOW_Q = range(10)
REC_DTYPE = np.dtype([("seq_off", "<u4"), ("qual_off", "<u4"), ("len", "<u4")])


class Refused(ValueError):
    """what the device answers with FQGPU_E_ARG"""


def flt(min_len=0, max_len=NONE, max_n=NONE, min_mean_q=0, low_q=0, max_low_pct=0, reserved=(0, 0)):
    """an fqgpu_filter as its eight uint32 words; the defaults keep every read"""
    return np.array([min_len, max_len, max_n, min_mean_q, low_q, max_low_pct, reserved[0], reserved[1]], dtype=np.uint32)


def check(f):
    """what fqgpu_filter_check accepts"""
    min_len, max_len, _, min_mean_q, low_q, pct, r0, r1 = (int(x) for x in f)
    return min_len <= max_len and min_mean_q <= 63 and low_q <= 64 and pct <= 100 and r0 == 0 and r1 == 0


def parse(raw):
    """the record table of a chunk with the semantics of fqgpu_parse_fastq: four lines per record, '@' and '+' in front of
    the first and third, sequence and quality of one length; a partial record at the end is ignored"""
    raw = np.asarray(raw, dtype=np.uint8)
    nl = np.flatnonzero(raw == 10)
    n = nl.size // 4
    nl = nl[:4 * n].reshape(n, 4).astype(np.int64)
    start = np.empty_like(nl)
    start[:, 1:] = nl[:, :3] + 1
    start[1:, 0] = nl[:-1, 3] + 1
    if n:
        start[0, 0] = 0
    if n and not ((raw[start[:, 0]] == ord("@")).all() and (raw[start[:, 2]] == ord("+")).all()):
        raise Refused("malformed FASTQ")
    recs = np.zeros(n, dtype=REC_DTYPE)
    recs["seq_off"], recs["qual_off"], recs["len"] = start[:, 1], start[:, 3], nl[:, 1] - start[:, 1]
    if n and ((nl[:, 3] - start[:, 3] != recs["len"]).any() or recs["len"].max() > 65535):
        raise Refused("malformed FASTQ")
    return recs


def per_record(raw, recs):
    """-> (sequence byte, quality byte, record) of every symbol of the records"""
    lens = recs["len"].astype(np.int64)
    starts = np.concatenate(([0], np.cumsum(lens)))
    rec_of = np.repeat(np.arange(len(recs)), lens)
    pos = np.arange(int(starts[-1]), dtype=np.int64) - starts[:-1][rec_of]
    seq = raw[recs["seq_off"].astype(np.int64)[rec_of] + pos]
    qual = raw[recs["qual_off"].astype(np.int64)[rec_of] + pos]
    return seq, qual, rec_of


def filter_records(raw, recs, f):
    """-> (out, report, keep): the canonical bytes of the records of `recs` that pass `f` (uint8 array), the report
    (uint64[16]) and the keep bits (uint8[(n + 7) // 8]).  Refused: what the device refuses."""
    raw = np.asarray(raw, dtype=np.uint8)
    if not check(f):
        raise Refused("a filter fqgpu_filter_check refuses")
    min_len, max_len, max_n, min_mean_q, low_q, pct = (int(x) for x in f[:6])
    n = len(recs)
    report = np.zeros(REPORT_WORDS, dtype=np.uint64)
    keep_bits = np.zeros((n + 7) // 8, dtype=np.uint8)
    if n == 0:
        return np.zeros(0, dtype=np.uint8), report, keep_bits
    lens = recs["len"].astype(np.int64)
    so, qo = recs["seq_off"].astype(np.int64), recs["qual_off"].astype(np.int64)
    if (lens == 0).any() or (lens > 65535).any() or (so + lens > raw.size).any() or (qo + lens > raw.size).any():
        raise Refused("a record outside the chunk, or without symbols")
    need_seq, need_qual = max_n != NONE, min_mean_q != 0 or low_q != 0
    seq, qual, rec_of = per_record(raw, recs)
    n_per = np.zeros(n, dtype=np.int64)
    q_per = np.zeros(n, dtype=np.int64)
    low_per = np.zeros(n, dtype=np.int64)
    if need_seq:   # only the lines a criterion reads are judged
        if not np.isin(seq, np.frombuffer(b"ACGTN", dtype=np.uint8)).all():
            raise Refused("a sequence byte outside ACGTN")
        n_per = np.bincount(rec_of, weights=(seq == ord("N")), minlength=n).astype(np.int64)
    if need_qual:
        phred = qual.astype(np.int64) - 33
        if phred.min() < 0 or phred.max() > 63:
            raise Refused("a quality byte outside 33 .. 96")
        q_per = np.bincount(rec_of, weights=phred, minlength=n).astype(np.int64)
        low_per = np.bincount(rec_of, weights=(phred < low_q), minlength=n).astype(np.int64)
    # the first failing criterion, in the report's order
    verdict = np.zeros(n, dtype=np.int64)
    fails = [lens < min_len, lens > max_len, (n_per > max_n) if need_seq else np.zeros(n, bool),
             (q_per < min_mean_q * lens) if min_mean_q else np.zeros(n, bool),
             (100 * low_per > pct * lens) if low_q else np.zeros(n, bool)]
    for code in (5, 4, 3, 2, 1):
        verdict[fails[code - 1]] = code
    kept = verdict == 0
    keep_bits = np.packbits(kept, bitorder="little")
    h0 = np.concatenate(([0], (qo + lens + 1)[:-1]))
    hl = np.maximum(so - h0, 0)
    size = hl + 2 * lens + 4
    bare = bool((qo == so + lens + 3).all() and (so >= h0).all() and qo[-1] + lens[-1] + 1 <= raw.size)
    if bare:   # a kept record is the span [h0, h0 + size) of the chunk
        marks = np.zeros(raw.size + 1, dtype=np.int64)
        np.add.at(marks, h0[kept], 1)
        np.add.at(marks, (h0 + size)[kept], -1)
        out = raw[np.cumsum(marks[:-1]) > 0]
    else:
        parts = []
        for r in np.flatnonzero(kept):
            parts += [raw[h0[r]:h0[r] + hl[r]].tobytes(), raw[so[r]:so[r] + lens[r]].tobytes(), b"\n+\n", raw[qo[r]:qo[r] + lens[r]].tobytes(), b"\n"]
        out = np.frombuffer(b"".join(parts), dtype=np.uint8)
    report[N_RECORDS], report[N_KEPT] = n, int(kept.sum())
    report[BASES_IN], report[BASES_KEPT] = int(lens.sum()), int(lens[kept].sum())
    report[BYTES_KEPT] = int(size[kept].sum())
    for code in range(1, 6):
        report[DROPPED_SHORT + code - 1] = int((verdict == code).sum())
    assert out.size == int(report[BYTES_KEPT])
    return out, report, keep_bits


def filter_chunk(raw, f):
    """the same for a FASTQ chunk, parsed here"""
    raw = np.asarray(raw, dtype=np.uint8)
    return filter_records(raw, parse(raw), f)
