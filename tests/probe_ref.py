"""A numpy restatement of adapter content (include/fqgpu.h: fqgpu_chunk_probe) from a raw chunk and its record table: per
probe the clip places of adapter_ref.find_all, then the tables, the merge, and the lines `fqc_tool s --adapters` appends
to its report.  Test code: the product never imports it."""
import zlib

import numpy as np

import adapter_ref as AR

HEAD, TABLE_HEAD, PROBES_MAX = 8, 8, 16
WINDOW_ROWS = 320    # the rows the device sums on chip: the tests' shapes stand on both sides of it
Refused = AR.Refused

# the tool's built-in probes, in the order `all` expands to
BUILTIN = [("truseq", b"AGATCGGAAGAGC"), ("truseq-r1", b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"), ("truseq-r2", b"AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"),
           ("nextera", b"CTGTCTCTTATACACATCT"), ("smallrna-3p", b"TGGAATTCTCGG"), ("smallrna-5p", b"GATCGTCGGACT"), ("solid", b"CGCCTTGGCCGT"),
           ("poly-a", b"A" * 20), ("poly-g", b"G" * 20)]


def words(n, P):
    return HEAD + (n + 1) * (TABLE_HEAD + P + 1) if 1 <= n <= PROBES_MAX and 1 <= P <= 65535 else 0


def prb(adapters, n=None, reserved=(0, 0, 0)):
    """an fqgpu_probes as its 4 + 16 * 20 uint32 words, from a list of adapter_ref.adp arrays"""
    p = np.zeros(4 + PROBES_MAX * AR.ADAPTER_WORDS, dtype=np.uint32)
    p[0] = len(adapters) if n is None else n
    p[1:4] = reserved
    for k, a in enumerate(adapters[:PROBES_MAX]):
        p[4 + k * AR.ADAPTER_WORDS:4 + (k + 1) * AR.ADAPTER_WORDS] = a
    return p


def probe(p, k):
    return p[4 + k * AR.ADAPTER_WORDS:4 + (k + 1) * AR.ADAPTER_WORDS]


def check(p):
    """what fqgpu_probes_check accepts"""
    n = int(p[0])
    if not 1 <= n <= PROBES_MAX or p[1:4].any():
        return False
    return all(AR.check(probe(p, k)) for k in range(n)) and not p[4 + n * AR.ADAPTER_WORDS:].any()


def fingerprint(p):
    n = int(p[0])
    return zlib.crc32(p[4:4 + n * AR.ADAPTER_WORDS].tobytes())


def places_of(raw, recs, p):
    """-> int64[n_recs, n]: a_k of every record.  Refused: what the device refuses."""
    raw = np.asarray(raw, dtype=np.uint8)
    n = int(p[0])
    lens = recs["len"].astype(np.int64)
    so = recs["seq_off"].astype(np.int64)
    if (lens == 0).any() or (lens > 65535).any() or (so + lens > raw.size).any():
        raise Refused("a record outside the chunk, or without symbols")
    if len(recs):
        rec_of = np.repeat(np.arange(len(recs)), lens)
        pos = np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens)
        if not np.isin(raw[so[rec_of] + pos], np.frombuffer(b"ACGTN", dtype=np.uint8)).all():
            raise Refused("a sequence byte outside ACGTN")
    out = np.zeros((len(recs), n), dtype=np.int64)
    for k in range(n):
        seq64, m, mo, pct, _ = AR.fields(probe(p, k))
        out[:, k] = AR.find_all(raw, so, lens, seq64[:m].tobytes(), mo, pct) if len(recs) else 0
    return out


def tables_of(places, lens, p, P):
    """the result words from the places"""
    n = int(p[0])
    assert check(p) and words(n, P)
    lens = np.asarray(lens, dtype=np.int64)
    w = np.zeros(words(n, P), dtype=np.uint64)
    w[0], w[1], w[2], w[3], w[4] = len(lens), int(lens.sum()), n, P, fingerprint(p)
    stride = TABLE_HEAD + P + 1
    for t in range(n + 1):
        a = places[:, t] if t < n else places.min(axis=1) if len(lens) else np.zeros(0, dtype=np.int64)
        m = AR.fields(probe(p, t))[1] if t < n else None
        hit = a < lens
        at = HEAD + t * stride
        w[at + 0] = int(hit.sum())
        w[at + 1] = int((lens - a).sum())
        w[at + 2] = int((a + m <= lens).sum()) if m is not None else 0
        w[at + 3] = int((a == 0).sum())
        w[at + TABLE_HEAD:at + stride] = np.bincount(np.minimum(a[hit], P), minlength=P + 1)
    return w


def probe_of(raw, recs, p, P):
    """-> (words, places)"""
    places = places_of(raw, recs, p)
    return tables_of(places, recs["len"], p, P), places


def view(w):
    n, P = int(w[2]), int(w[3])
    assert w.size == words(n, P)
    body = w[HEAD:].reshape(n + 1, TABLE_HEAD + P + 1)
    return dict(n_records=int(w[0]), n_bases=int(w[1]), n=n, positions=P, fingerprint=int(w[4]), tables=body[:, :TABLE_HEAD],
                rows=body[:, TABLE_HEAD:])


def merge(a, b):
    """what fqgpu_probe_merge makes of two results of one probe set and one P"""
    assert a.size == b.size and (a[2:5] == b[2:5]).all()
    if a[0] == 0:
        return b.copy()
    if b[0] == 0:
        return a.copy()
    out = a + b
    out[2:8] = a[2:8]
    return out


def render(w, p, names):
    """the lines the tool appends to its report, as bytes"""
    v = view(w)
    n = v["n"]
    lines = []
    for t in range(n + 1):
        c = [int(x) for x in v["tables"][t, :4]]
        if t < n:
            seq64, m, mo, pct, _ = AR.fields(probe(p, t))
            lines.append("probe\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d" % (t, names[t], seq64[:m].tobytes().decode(), mo, pct, *c))
        else:
            lines.append("probe\tany\t-\t-\t-\t-\t%d\t%d\t%d\t%d" % tuple(c))
    for t in range(n + 1):
        lines += ["probepos\t%s\t%d\t%d" % (t if t < n else "any", i, int(v["rows"][t, i])) for i in np.flatnonzero(v["rows"][t])]
    return ("\n".join(lines) + "\n").encode()
