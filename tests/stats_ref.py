"""A numpy restatement of the read summary (include/fqgpu.h: fqgpu_chunk_stats) from a raw chunk and its record table, and
the renderer / parser of the report `fqc_tool s` writes.  Test code: the product never imports it."""
import numpy as np

HEAD = 176
BASES = b"ACGTN"


def words(P):
    return HEAD + 70 * (P + 1)


def stats_of(raw, recs, P):
    """-> uint64 array of words(P): the summary of the records `recs` (seq_off, qual_off, len) of `raw`"""
    assert 1 <= P <= 65535
    raw = np.asarray(raw, dtype=np.uint8)
    out = np.zeros(words(P), dtype=np.uint64)
    rows = P + 1
    n = len(recs)
    out[5] = P
    if n == 0:
        return out
    lens = recs["len"].astype(np.int64)
    starts = np.concatenate(([0], np.cumsum(lens)))
    total = int(starts[-1])
    rec_of = np.repeat(np.arange(n), lens)
    pos = np.arange(total, dtype=np.int64) - starts[:-1][rec_of]
    seq = raw[recs["seq_off"].astype(np.int64)[rec_of] + pos]
    phred = raw[recs["qual_off"].astype(np.int64)[rec_of] + pos].astype(np.int64) - 33
    code = np.full(256, -1, dtype=np.int64)
    for i, c in enumerate(BASES):
        code[c] = i
    base = code[seq]
    assert base.min() >= 0 and phred.min() >= 0 and phred.max() <= 63, "a byte the summary refuses"
    row = np.minimum(pos, P)
    out[0], out[1], out[2], out[3] = n, total, lens.min(), lens.max()
    n_per = np.bincount(rec_of, weights=(base == 4), minlength=n).astype(np.int64)
    gc_per = np.bincount(rec_of, weights=(base == 1) | (base == 2), minlength=n).astype(np.int64)
    q_per = np.bincount(rec_of, weights=phred, minlength=n).astype(np.int64)
    out[4] = int((n_per > 0).sum())
    out[8:72] = np.bincount(q_per // lens, minlength=64)
    out[72:173] = np.bincount(100 * gc_per // lens, minlength=101)
    at = HEAD
    out[at:at + rows] = np.bincount(np.minimum(lens, P), minlength=rows)
    out[at + rows:at + 6 * rows] = np.bincount(row * 5 + base, minlength=5 * rows)
    out[at + 6 * rows:at + 70 * rows] = np.bincount(row * 64 + phred, minlength=64 * rows)
    return out


def view(w):
    P = int(w[5])
    rows = P + 1
    assert w.size == words(P)
    return dict(n_records=int(w[0]), n_bases=int(w[1]), min_len=int(w[2]), max_len=int(w[3]), reads_with_n=int(w[4]), positions=P,
                meanq_hist=w[8:72], gc_hist=w[72:173], len_hist=w[HEAD:HEAD + rows],
                base_pos=w[HEAD + rows:HEAD + 6 * rows].reshape(rows, 5), qual_pos=w[HEAD + 6 * rows:].reshape(rows, 64))


def merge(a, b):
    """what fqgpu_stats_merge makes of two summaries of one P"""
    assert a[5] == b[5] and a.size == b.size
    if a[0] == 0:
        return b.copy()
    if b[0] == 0:
        return a.copy()
    out = a + b
    out[2], out[3], out[5] = min(a[2], b[2]), max(a[3], b[3]), a[5]
    return out


def render(w):
    """the report file of a summary, as bytes"""
    v = view(w)
    lines = ["#fqgpu-stats 1"]
    for key, name in (("n_records", "records"), ("n_bases", "bases"), ("min_len", "min_len"), ("max_len", "max_len"),
                      ("reads_with_n", "reads_with_n"), ("positions", "positions")):
        lines.append("%s\t%d" % (name, v[key]))
    for tag, hist in (("len", v["len_hist"]), ("mq", v["meanq_hist"]), ("gc", v["gc_hist"])):
        lines += ["%s\t%d\t%d" % (tag, i, int(hist[i])) for i in np.flatnonzero(hist)]
    used = np.flatnonzero(v["base_pos"].sum(axis=1) + v["qual_pos"].sum(axis=1))
    last = int(used[-1]) if used.size else -1
    for tag, table in (("base", v["base_pos"]), ("qual", v["qual_pos"])):
        lines += ["%s\t%d\t%s" % (tag, r, "\t".join(str(int(x)) for x in table[r])) for r in range(last + 1)]
    return ("\n".join(lines) + "\n").encode()


def parse(text):
    """a report back into the summary's words"""
    lines = text.decode().split("\n")
    assert lines[0] == "#fqgpu-stats 1" and lines[-1] == ""
    rows = [ln.split("\t") for ln in lines[1:-1]]
    scalars = {r[0]: int(r[1]) for r in rows if len(r) == 2}
    P = scalars["positions"]
    w = np.zeros(words(P), dtype=np.uint64)
    for i, name in enumerate(("records", "bases", "min_len", "max_len", "reads_with_n", "positions")):
        w[i] = scalars[name]
    n = P + 1
    for r in rows:
        if len(r) == 2:
            continue
        tag, i, vals = r[0], int(r[1]), [int(x) for x in r[2:]]
        if tag == "len":
            w[HEAD + i] = vals[0]
        elif tag == "mq":
            w[8 + i] = vals[0]
        elif tag == "gc":
            w[72 + i] = vals[0]
        elif tag == "base":
            assert len(vals) == 5
            w[HEAD + n + 5 * i:HEAD + n + 5 * i + 5] = vals
        else:
            assert tag == "qual" and len(vals) == 64
            w[HEAD + 6 * n + 64 * i:HEAD + 6 * n + 64 * i + 64] = vals
    return w
