"""A plain line-by-line restatement of the FASTQ record parser (FastqReader::parseRecords, reference src/fastq_io.cpp:67-125)
and the inputs that pin the device parser (fqcomp28_amd/csrc/parse.hip) to it.  Test code: it imports nothing from the
library, and the product never imports it.

`parse` walks the block one line at a time, as the reference does, and judges every whole record; where the reference
asserts, it says "format".  The one rule that is the library's own (include/fqgpu.h, FQGPU_E_SHORT_READ) is the verdict
"short".  `cases` builds the inputs, by family; each case is named for the property it has, and the generator asserts
that it has it.  The kernels' geometry the families aim at: 16 bytes per lane, 1 KiB per wave, 4 KiB (PCHUNK) per
workgroup in k_nl_count / k_nl_write; one thread per record, 256 per workgroup, in k_records; one wave per record, 64
bases per step, a grid-stride loop above 32768 records in k_count_n; chunks of 2048 items in the scan of the chunk counts.
"""
import functools

import numpy as np

REC_DTYPE = np.dtype([("seq_off", "<u4"), ("qual_off", "<u4"), ("len", "<u4")])
MAX_READ = 65535   # readlen_t
MIN_READ = 3       # below it: FQGPU_E_SHORT_READ
LANE, WAVE, PCHUNK = 16, 1024, 4096
LINE_KINDS = ("header", "sequence", "plus", "quality")

# the library's codes for the verdicts (include/fqgpu.h): FQGPU_E_ARG, FQGPU_E_SHORT_READ
CODE = {"ok": 0, "format": -4, "empty": -4, "short": -2}


def parse(raw):
    """-> (verdict, recs, used_len, n_bases, n_n).  recs holds every whole record (four lines, each ended by a newline);
    whatever lies behind the last of them -- a cut line, or one to three whole lines -- is ignored.  used_len: the bytes up
    to the end of the last whole record.  n_n: 'N' bytes of the sequence lines."""
    b = bytes(raw) if not isinstance(raw, np.ndarray) else raw.tobytes()
    size = len(b)
    recs = []
    fmt = short = False
    used = n_bases = n_n = 0
    line_start = 0
    ln = 0
    seq_start = seq_len = 0
    first_byte = -1
    while line_start < size:
        line_end = b.find(b"\n", line_start)
        if line_end < 0:
            break  # a cut line: it and the lines of its record before it are carried over
        line_length = line_end - line_start
        if ln == 0:
            first_byte = b[line_start]   # (of an empty line: its newline)
        elif ln == 1:
            seq_start, seq_len = line_start, line_length
        elif ln == 2:
            if b[line_start] != 0x2B:
                fmt = True
        else:
            if first_byte != 0x40 or line_length != seq_len or seq_len > MAX_READ:
                fmt = True
            if seq_len < MIN_READ:
                short = True
            recs.append((seq_start, line_start, seq_len))
            n_bases += seq_len
            n_n += b.count(b"N", seq_start, seq_start + seq_len)
            used = line_end + 1
            ln = -1
        ln += 1
        line_start = line_end + 1
    table = np.array(recs, dtype=REC_DTYPE) if recs else np.zeros(0, dtype=REC_DTYPE)
    verdict = "empty" if not recs else "format" if fmt else "short" if short else "ok"
    return verdict, table, used, n_bases, n_n


# ------------------------------------------------------------------------------------------------------------ records
QUALS = b"#+05:<@ABDGI"   # a dozen values


class _Gen:
    """seeded reads"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)

    def seq(self, n, p_n=0.02):
        s = np.frombuffer(b"ACGT", dtype=np.uint8)[self.rng.integers(0, 4, size=n)].copy()
        s[self.rng.random(n) < p_n] = ord("N")
        return s.tobytes()

    def qual(self, n):
        return np.frombuffer(QUALS, dtype=np.uint8)[self.rng.integers(0, len(QUALS), size=n)].tobytes()


def record(hdr_len, seq, qual, plus=b"+"):
    """one record whose header line holds hdr_len bytes ('@' included)"""
    assert hdr_len >= 1
    return b"@" + (b"read" * (hdr_len // 4 + 1))[: hdr_len - 1] + b"\n" + seq + b"\n" + plus + b"\n" + qual + b"\n"


STD_HDR, STD_LEN = 8, 21
STD_SIZE = STD_HDR + 5 + 2 * STD_LEN   # 55 bytes: four newlines and the plus


def std_record(g, hdr_len=STD_HDR, n=STD_LEN):
    return record(hdr_len, g.seq(n), g.qual(n))


def newlines(b):
    return np.flatnonzero(np.frombuffer(b, dtype=np.uint8) == 10)


def _well_formed(b):
    v, recs, used, _, _ = parse(b)
    return v == "ok" and used == len(b)


# ----------------------------------------------------------------------------------------------------------- families
def _newline_on_a_boundary(out):
    """the newline that ends a line of each kind exactly at offset T: the last byte of a lane word, wave or workgroup
    (T + 1 a multiple of 16, 1024, 4096) or the first byte of the next; whole, and cut directly behind the record"""
    g = _Gen(1)
    for T in (LANE - 1, LANE, WAVE - 1, WAVE, PCHUNK - 1, PCHUNK, 2 * PCHUNK - 1, 2 * PCHUNK):
        for k, kind in enumerate(LINE_KINDS):
            n = 3 if T < 64 else STD_LEN
            behind_header = (0, 1 + n, 3 + n, 4 + 2 * n)[k]   # from the header's newline to the newline of line k
            parts, at = [], 0
            while T - at - behind_header > 120:
                parts.append(std_record(g))
                at += STD_SIZE
            hdr_len = T - at - behind_header
            assert 1 <= hdr_len <= 120, (T, kind)
            parts.append(record(hdr_len, g.seq(n, 0), g.qual(n)))
            cut = at + hdr_len + 5 + 2 * n
            parts += [std_record(g) for _ in range(3)]
            b = b"".join(parts)
            nl = newlines(b)
            i = int(np.searchsorted(nl, T))
            assert b[T] == 10 and nl[i] == T and i % 4 == k, (T, kind)
            assert _well_formed(b) and _well_formed(b[:cut]) and nl[i - k + 3] == cut - 1
            out["boundary:newline-of-%s-line-at-%d" % (kind, T)] = b
            out["boundary:newline-of-%s-line-at-%d-cut-behind-its-record" % (kind, T)] = b[:cut]


def block_of_size(g, size):
    """a well-formed block of exactly `size` bytes: standard records and a last one whose header is padded"""
    parts, at = [], 0
    while size - at - STD_SIZE >= STD_SIZE:
        parts.append(std_record(g))
        at += STD_SIZE
    parts.append(std_record(g, hdr_len=size - at - 5 - 2 * STD_LEN))
    b = b"".join(parts)
    assert len(b) == size and _well_formed(b)
    return b


END_SIZES = (4096, 4097, 8191, 8192, 2720, 2721, 2735, 5008, 5009, 5007)


def _block_ends_on_a_boundary(out):
    g = _Gen(2)
    for size in END_SIZES:
        b = block_of_size(g, size)
        assert b[-1] == 10
        out["ends:block-of-%d-bytes" % size] = b
    for res in (0, 1, 15):
        assert any(s % 16 == res and s % PCHUNK for s in END_SIZES)


def _densest(out):
    """about five newlines per lane word, more than 256 records per workgroup of the newline kernels"""
    b = b"@\nACG\n+\nIII\n" * 4000
    nl = newlines(b)
    assert len(nl) == 16000 and np.bincount(nl // LANE).max() >= 5
    assert np.bincount(nl // PCHUNK)[:-1].min() // 4 > 256
    out["dense:4000-records-of-12-bytes"] = b
    b = b"".join(record(1 + i % 17, b"ACG", b"III") for i in range(4000))
    nl = newlines(b)
    for k in range(4):   # the newline of every line kind meets every residue
        assert len(set((nl[k::4] % LANE).tolist())) == LANE
    assert _well_formed(b)
    out["dense:4000-records-headers-of-1-to-17-bytes"] = b


def long_read(g, n):
    """few quality levels and skewed bases: both streams stay far inside the capacity rule"""
    s = np.frombuffer(b"AAAAACGT", dtype=np.uint8)[g.rng.integers(0, 8, size=n)].copy()
    s[[0, 63, 64, n - 1]] = ord("N")
    q = np.frombuffer(b"IIIB", dtype=np.uint8)[g.rng.integers(0, 4, size=n)]
    return s.tobytes(), q.tobytes()


def _sparsest(out):
    g = _Gen(3)
    s, q = long_read(g, MAX_READ)
    alone = record(3, s, q)
    around = [std_record(g) for _ in range(40)]
    between = b"".join(around[:25]) + alone + b"".join(around[25:])
    assert (25 * STD_SIZE) % PCHUNK not in (0, PCHUNK - 1)   # the read starts in the middle of a chunk
    for name, b in (("sparse:one-read-of-65535-bases-alone", alone), ("sparse:one-read-of-65535-bases-between-short-records", between)):
        v, recs, used, _, _ = parse(b)
        assert v == "ok" and used == len(b) and int(recs["len"].max()) == MAX_READ
        n_chunks = (len(b) + PCHUNK - 1) // PCHUNK
        empty = n_chunks - len(set((newlines(b) // PCHUNK).tolist()))
        assert empty >= 28, empty   # some thirty workgroups count no newline
        out[name] = b
    s, q = long_read(g, MAX_READ + 1)
    b = b"".join(around[:25]) + record(3, s, q) + b"".join(around[25:])
    assert parse(b)[0] == "format"
    out["sparse:one-read-of-65536-bases-between-short-records"] = b


def _every_cut(out):
    """a block of three chunks, cut at every byte inside its last two records; then with one, two and three whole lines
    behind it that look like the start of a record"""
    g = _Gen(4)
    parts = [std_record(g, hdr_len=6 + i % 11) for i in range(180)]
    b = b"".join(parts)
    assert 2 * PCHUNK < len(b) <= 3 * PCHUNK and _well_formed(b)
    n = len(parts)
    start = len(b) - len(parts[-1]) - len(parts[-2])
    for cut in range(start, len(b)):
        v, recs, used, _, _ = parse(b[:cut])
        assert v == "ok" and len(recs) == (n - 2 if cut < len(b) - len(parts[-1]) else n - 1) and used <= cut
        out["cuts:cut-at-%d" % cut] = b[:cut]
    extra = (b"@read 181\n", b"ACGTNACGTACGT\n", b"+\n")
    for k in (1, 2, 3):
        c = b + b"".join(extra[:k])
        v, recs, used, _, _ = parse(c)
        assert v == "ok" and len(recs) == n and used == len(b) and len(newlines(c)) % 4 == k
        out["cuts:%d-whole-lines-of-the-next-record-behind" % k] = c


def _reference_pin(out):
    """the '+' lines repeat the header; qualities begin with '@' or '+' (restated from tests/test_reference_pin.py)"""
    plus = b"".join(b"@r%d x\nACGTN\n+r%d x\n%s\n" % (i, i, q)
                    for i, q in enumerate([b"IIIII", b"@IIII", b"+IIII", b"@@@@@", b"+++++", b"I@+@I"]))
    v, recs, used, n_bases, n_n = parse(plus)
    assert (v, len(recs), used, n_bases, n_n) == ("ok", 6, len(plus), 30, 6)
    out["pin:plus-lines-repeat-the-header-qualities-start-with-at-or-plus"] = plus
    assert plus[:-4].endswith(b"\nI@") and len(parse(plus[:-4])[1]) == 5
    out["pin:same-cut-four-bytes-short"] = plus[:-4]


DEFECT_PLACES = (0, 63, 64, 255, 256, 599)
DEFECTS = {   # name -> (verdict, record maker from (sequence, quality))
    "first-byte-not-at": ("format", lambda s, q: b"r" + record(STD_HDR, s, q)[1:]),
    "third-line-not-plus": ("format", lambda s, q: record(STD_HDR, s, q, plus=b"-")),
    "quality-one-byte-short": ("format", lambda s, q: record(STD_HDR, s, q[:-1])),
    "quality-one-byte-long": ("format", lambda s, q: record(STD_HDR, s, q + b"I")),
    "read-of-length-2": ("short", lambda s, q: record(STD_HDR, s[:2], q[:2])),
    "read-of-length-0": ("short", lambda s, q: record(STD_HDR, b"", b"")),
}


def _defect_by_place(out):
    """one defect in a block of 600 records: at the first and last thread of a wave and of a workgroup of k_records, and
    in the block's first and last record"""
    g = _Gen(5)
    reads = [(g.seq(STD_LEN), g.qual(STD_LEN)) for _ in range(600)]
    good = [record(STD_HDR, s, q) for s, q in reads]
    assert _well_formed(b"".join(good))
    for name, (verdict, make) in DEFECTS.items():
        for place in DEFECT_PLACES:
            parts = list(good)
            parts[place] = make(*reads[place])
            b = b"".join(parts)
            v, recs, _, _, _ = parse(b)
            assert v == verdict and len(recs) == 600, (name, place, v)
            assert parse(b"".join(parts[:place] + parts[place + 1:]))[0] == "ok"   # the defect is that record's alone
            out["defect:%s-in-record-%d" % (name, place)] = b
    parts = list(good)
    parts[100] = DEFECTS["read-of-length-2"][1](*reads[100])
    parts[400] = DEFECTS["quality-one-byte-short"][1](*reads[400])
    b = b"".join(parts)
    assert parse(b)[0] == "format" and parse(b"".join(parts[:400]))[0] == "short"
    out["defect:short-read-in-record-100-and-short-quality-in-record-400"] = b


def _crlf(out):
    g = _Gen(6)
    b = b"".join(b"@r%d\r\n%s\r\n+\r\n%s\r\n" % (i, g.seq(30, 0), g.qual(30)) for i in range(20))
    v, recs, used, n_bases, _ = parse(b)
    assert v == "ok" and used == len(b) and n_bases == 20 * 31   # the length counts the carriage return
    assert all(b[int(r["seq_off"]) + 30] == 13 and b[int(r["qual_off"]) + 30] == 13 for r in recs)
    out["crlf:20-records-with-carriage-returns"] = b


MANY_RECORDS, MANY_LEN = 60500, 70
MANY_N_AT = (0, 63, 64, 69)


def _many_records(out):
    """more than 2048 chunks of the newline kernels (the scan of their counts leaves its first chunk of items) and more
    than 32768 records (k_count_n strides over the grid); N at 0, 63, 64 and 69 by the bits of a pattern that changes
    with the record: behind position 63 a wave takes its second step"""
    g = _Gen(7)
    n, L = MANY_RECORDS, MANY_LEN
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[g.rng.integers(0, 4, size=(n, L))].copy()
    qual = np.frombuffer(QUALS, dtype=np.uint8)[g.rng.integers(0, len(QUALS), size=(n, L))]
    pattern = (np.arange(n) * 7 + np.arange(n) // 16) % 16
    for bit, pos in enumerate(MANY_N_AT):
        seq[(pattern >> bit) & 1 == 1, pos] = ord("N")
    rows_s, rows_q = seq.tobytes(), qual.tobytes()
    b = b"".join(b"@m%d\n%s\n+\n%s\n" % (i, rows_s[i * L: (i + 1) * L], rows_q[i * L: (i + 1) * L]) for i in range(n))
    assert len(b) > 2049 * PCHUNK - PCHUNK and (len(b) + PCHUNK - 1) // PCHUNK >= 2049 and n > 32768
    assert len(b) < 10 << 20
    per_record = (seq == ord("N")).sum(axis=1)
    assert per_record.min() == 0 and per_record.max() == 4 and set(pattern.tolist()) == set(range(16))
    assert int((seq[:, 64:] == ord("N")).sum()) > 0
    out["many:60500-records-of-70-bases"] = b


FAMILIES = {
    "boundary": _newline_on_a_boundary,
    "ends": _block_ends_on_a_boundary,
    "dense": _densest,
    "sparse": _sparsest,
    "cuts": _every_cut,
    "pin": _reference_pin,
    "defect": _defect_by_place,
    "crlf": _crlf,
    "many": _many_records,
}
MANY = "many:60500-records-of-70-bases"
# cases whose reads no table codes: they are parsed, and the encode's own verdict is checked apart (include/fqgpu.h:
# a sequence byte that is neither A, C, G, T nor N is FQGPU_E_ARG)
PARSE_ONLY = {"crlf:20-records-with-carriage-returns": -4}


def cases():
    """-> {name: bytes}; a name is "family:property" """
    out = {}
    for family, make in FAMILIES.items():
        before = len(out)
        make(out)
        assert len(out) > before and all(k.startswith(family + ":") for k in list(out)[before:])
    return out


def family(name):
    return name.split(":")[0]


@functools.lru_cache(maxsize=None)
def shared_cases():
    """cases(), made once for all the tests of a run"""
    return cases()


def names_of(fam):
    return [k for k in shared_cases() if family(k) == fam]


@functools.lru_cache(maxsize=None)
def reference(name):
    """parse() of a case, computed once and shared: (verdict, recs, used_len, n_bases, n_n); the table is read-only"""
    got = parse(shared_cases()[name])
    got[1].setflags(write=False)
    return got
