"""The reference and the inputs of the header families (tests/test_headers_families_host.py on the CPU,
tests/test_gpu_headers_families.py on the device).

`restate` is the host's decodeChunk layout (workspace.hpp decodeChunk over headers.hpp decodeHeader) as one sequential
loop over Python ints on top of oracle/headers_oracle.py; it raises Refused(record) where the host throws out_of_range.
`families()` is a deterministic generator of header lists, each aimed at one edge of the prefix sums in
fqcomp28_amd/csrc/headers.hip and decode_headers.hip (workgroups of 256 records, rounds of 64 and 256 workgroups, groups
of 256 contentLength entries, CL_STAGE_BYTES) and each carrying an `assert` of the property it is named for.

TEST INFRASTRUCTURE ONLY: nothing under fqcomp28_amd/ imports it.
"""
import os
import struct
import sys
from collections import namedtuple

import ref_pin as R

sys.path.insert(0, os.path.join(R.ROOT, "oracle"))
import headers_oracle as HO  # noqa: E402

WG = 256            # records of a workgroup in both files (HDR_THREADS, CL_THREADS)
STAGE_BYTES = 32768  # CL_STAGE_BYTES: a workgroup's headers up to here are staged in LDS, more are written directly


class Refused(Exception):
    def __init__(self, record):
        super().__init__(record)
        self.record = record


class Layout(namedtuple("Layout", "raw recs starts headers reads")):
    """raw: the chunk's bytes, zero-filled to raw_len; recs: [(seq_off, qual_off, len)]; starts: every record's start
    offset and, last, the end of the last record; headers: the decoded header lines"""

    def window(self, a, b):
        """records [a, b) as fqgpu_decode_chunk_range documents them: exactly their bytes, and the record table of the
        chunk's records a .. b - 1 with offsets relative to the window's first byte"""
        out, recs = bytearray(), []
        for r in range(a, b):
            seq, qual = self.reads[r]
            out += self.headers[r] + b"\n"
            s_off = len(out)
            out += seq + b"\n+\n"
            q_off = len(out)
            out += qual + b"\n"
            recs.append((s_off, q_off, len(seq)))
        assert len(out) == self.starts[b] - self.starts[a]
        return bytes(out), recs

    def fasta(self, a, b):
        """records [a, b) as fqgpu_decode_chunk_fasta documents them (">hdr\\nSEQ\\n", qual_off 0).  The chunk was judged
        on the FASTQ layout: a chunk that `restate` refuses has no FASTA form either."""
        out, recs = bytearray(), []
        for r in range(a, b):
            seq = self.reads[r][0]
            out += b">" + self.headers[r][1:] + b"\n"
            recs.append((len(out), 0, len(seq)))
            out += seq + b"\n"
        return bytes(out), recs


def restate(first_header, fields, reads, raw_len):
    """the host's decodeChunk layout: -> Layout or Refused(first failing record).
    fields = [(flags, content, lengths)], reads = [(sequence, quality)]"""
    types, seps = HO.format_from_header(first_header)
    prev = [HO.parse_numeric(f) if t == HO.NUMERIC else f for f, t in zip(HO.split_header(first_header, seps), types)]
    fields = [tuple(bytes(x) for x in f) for f in fields]
    cur = [[0, 0, 0] for _ in types]
    out, recs, starts, headers = bytearray(), [], [], []
    for r, (seq, qual) in enumerate(reads):
        h = bytearray(b"@")
        for i, t in enumerate(types):
            flags, content, lengths = fields[i]
            c = cur[i]
            if t == HO.NUMERIC:
                if c[1] + 4 > len(content):
                    raise Refused(r)
                (d,) = struct.unpack_from("<I", content, c[1]); c[1] += 4
                v = (prev[i] + d) & 0xFFFFFFFF
                prev[i] = v - (1 << 32) if v >= 1 << 31 else v
                h += str(prev[i]).encode()
            else:
                if c[0] >= len(flags):
                    raise Refused(r)
                flag = flags[c[0]]; c[0] += 1
                if flag:
                    if c[2] >= len(lengths):
                        raise Refused(r)
                    ln = lengths[c[2]]; c[2] += 1
                    if c[1] + ln > len(content):
                        raise Refused(r)
                    prev[i] = content[c[1]: c[1] + ln]; c[1] += ln
                h += prev[i]
            if i + 1 < len(types):
                h.append(seps[i])
        if len(out) + len(h) + 2 * len(seq) + 5 > raw_len:
            raise Refused(r)
        starts.append(len(out))
        headers.append(bytes(h))
        out += h + b"\n"
        s_off = len(out)
        out += seq + b"\n+\n"
        q_off = len(out)
        out += qual + b"\n"
        recs.append((s_off, q_off, len(seq)))
    starts.append(len(out))
    return Layout(bytes(out) + bytes(raw_len - len(out)), recs, starts, headers, list(reads))


def first_uncodable(headers, first_header):
    """the record at which headers_oracle's field coder raises (the reference's asserts), or None"""
    types, seps = HO.format_from_header(first_header)
    try:
        prev = [HO.parse_numeric(f) if t == HO.NUMERIC else f for f, t in zip(HO.split_header(first_header, seps), types)]
    except ValueError:
        return 0
    streams = [HO.FieldStreams() for _ in types]
    for r, h in enumerate(headers):
        try:
            for i, (f, t) in enumerate(zip(HO.split_header(h, seps), types)):
                prev[i] = streams[i].store_numeric(f, prev[i]) if t == HO.NUMERIC else streams[i].store_string(f, prev[i])
        except ValueError:
            return r
    return None


def fmt_of(first_header):
    types, seps = HO.format_from_header(first_header)
    return ([0 if t == HO.NUMERIC else 1 for t in types], bytes(seps), first_header)


_READS = []


def reads(n):
    """the (sequence, quality) pairs ref_pin.fastq_of_headers puts under n headers: SRR065390_sub_1's, in turn"""
    if not _READS:
        R.fastq_of_headers([b"@x"])
        for x in R._READS:
            _, seq, plus, qual, _ = x.split(b"\n")
            assert plus == b"+" and len(seq) == len(qual)
            _READS.append((seq, qual))
    return [_READS[i % len(_READS)] for i in range(n)]


def chunk_table(headers, rds):
    """the record table of the chunk ref_pin.fastq_of_headers(headers) is"""
    recs, at = [], 0
    for h, (seq, _) in zip(headers, rds):
        s_off = at + len(h) + 1
        q_off = s_off + len(seq) + 3
        recs.append((s_off, q_off, len(seq)))
        at = q_off + len(seq) + 1
    return recs, at


# ---------------------------------------------------------------------------------------------------------------------
# Cases.  kind: "ok" (coded and restored; extra["lossless"] False where a numeric text does not come back),
# "uncodable" (extra["bad"]: the record both coders refuse), "windows" (extra["bounds"]: the a and b to pair up),
# "refusals" (extra["damage"]: [(name, fields -> (fields, raw_len delta), refused record or None)]).
Case = namedtuple("Case", "family name first headers kind extra")

_oracle = {}


def oracle_fields(case):
    """headers_oracle.encode_headers of a codable case as [(flags, content, lengths)], made once"""
    key = (case.family, case.name)
    if key not in _oracle:
        _oracle[key] = R.oracle_fields(case.headers, case.first)[2]
    return _oracle[key]


def new_flags(headers, first, field):
    """the flags of STRING field `field`, straight from the texts: 1 where the field differs from the record in front"""
    seps = HO.format_from_header(first)[1]
    prev, out = HO.split_header(first, seps)[field], []
    for h in headers:
        v = HO.split_header(h, seps)[field]
        out.append(int(v != prev))
        prev = v
    return out


def _val(r, length=None):
    """a value that names its record; lengths 6 .. 245, never the same for two records less than 240 apart"""
    length = 6 + (r * 7) % 240 if length is None else length
    return (b"v%d" % r).ljust(length, b"abcdefg"[r % 7: r % 7 + 1])[:length]


FIRST = b"@1 x"  # NUMERIC, ' ', STRING: the string is the last field, so it may be empty


def _ns(nums_vals):
    return [b"@%d %s" % (n, v) for n, v in nums_vals]


def _edge_new():
    edges = (63, 64, 65, 127, 128, 255, 256, 257, 511, 512)
    n = 768
    for name, at in (("only-at-edges", set(edges)), ("everywhere-but-edges", set(range(n)) - set(edges))):
        v, hdrs, k = b"x", [], 0
        for r in range(n):
            if r in at:
                k += 1
                v = _val(r, 3 + (k * 11) % 250 if name == "only-at-edges" else None)
            hdrs.append((r + 2, v))
        hdrs = _ns(hdrs)
        fl = new_flags(hdrs, FIRST, 1)
        assert [r for r in range(n) if fl[r]] == sorted(at), "string values change exactly at the named records"
        news = [h.split(b" ")[1] for r, h in enumerate(hdrs) if fl[r]]
        if name == "only-at-edges":
            assert len(set(map(len, news))) == len(news) == 10, "every value has a length of its own"
        else:
            assert all(len(a) != len(b) for a, b in zip(news, news[1:])), "neighbouring values differ in length"
        yield Case("edge-new", name, FIRST, hdrs, "ok", {})


def _carried_value():
    w0, n = 3 * WG, 4 * WG + 40  # record 0 of workgroup 3 is "same"
    for dist, length in ((1, 5), (256, 0), (257, 254), (600, 3), (600, 0), (256, 254), (1, 254)):
        at = w0 - dist
        hdrs = []
        for r in range(n):
            if r < at:
                v = _val(r)
            elif r < w0 + 5:
                v = _val(at, length)
            else:
                v = _val(r)
            hdrs.append((7 - r, v))
        hdrs = _ns(hdrs)
        fl = new_flags(hdrs, FIRST, 1)
        assert fl[at] == 1 and not any(fl[at + 1: w0 + 5]) and fl[w0 + 5] == 1, "the value at workgroup 3's record 0 was set %d records earlier" % dist
        assert len(hdrs[w0].split(b" ", 1)[1]) == length and sum(fl[:w0]) == at + 1
        whole = [w for w in range(3) if at < w * WG and not any(fl[w * WG: (w + 1) * WG])]
        assert len(whole) == {1: 0, 256: 0, 257: 1, 600: 2}[dist], "whole workgroups without a new value in between"
        yield Case("carried-value", "set-%d-earlier-len-%d" % (dist, length), FIRST, hdrs, "ok", {})
    # nothing new in front of workgroup 1's record 0 at all: the dataset's first header's field
    first = b"@1 firstvalue"
    hdrs = _ns([(r, b"firstvalue" if r < WG + 9 else _val(r)) for r in range(2 * WG + 3)])
    fl = new_flags(hdrs, first, 1)
    assert not any(fl[: WG + 9]) and fl[WG + 9], "no new value in front of workgroup 1: the first header's field is used"
    yield Case("carried-value", "first-header-field", first, hdrs, "ok", {})


def _group_of_256():
    for k in (255, 256, 257, 511, 512, 513):
        w = (k + WG - 1) // WG  # the first workgroup with k new values in front of it
        n = (w + 2) * WG + 1
        sparse = {w * WG + 3, w * WG + 100, w * WG + 255, (w + 1) * WG, (w + 1) * WG + 200, n - 1}
        v, hdrs = b"x", []
        for r in range(n):
            if r < k or r in sparse:
                v = _val(r)
            hdrs.append((3 * r - 500, v))
        hdrs = _ns(hdrs)
        fl = new_flags(hdrs, FIRST, 1)
        assert sum(fl[: w * WG]) == k, "exactly %d new values lie in front of workgroup %d" % (k, w)
        assert all(fl[:k]) and sum(fl[: (w + 1) * WG]) == k + 3 and sum(fl) == k + 6
        yield Case("group-of-256", "%d-in-front-of-workgroup-%d" % (k, w), FIRST, hdrs, "ok", {})


def _encode_rounds():
    for n in (16383, 16384, 16385, 32769):
        v, hdrs = b"x", []
        for r in range(n):
            if r % WG in (0, WG - 1) or r == n - 1:
                v = _val(r)
            hdrs.append((r, v))
        hdrs = _ns(hdrs)
        fl = new_flags(hdrs, FIRST, 1)
        n_wg = (n + WG - 1) // WG
        assert n_wg == {16383: 64, 16384: 64, 16385: 65, 32769: 129}[n], "workgroups against k_hdr_layout's rounds of 64"
        assert all(fl[w * WG] for w in range(n_wg)) and all(fl[w * WG - 1] for w in range(1, n_wg)) and fl[n - 1]
        yield Case("encode-rounds", "%d-records" % n, FIRST, hdrs, "ok", {})


def _wrap32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= 1 << 31 else v


def _decode_rounds():
    first = b"@0:0 x"  # NUMERIC ':' NUMERIC ' ' STRING
    for n in (65536, 65537):
        news = {3, 255 * WG + 7} | ({256 * WG} if n > 256 * WG else set())
        v, hdrs = b"x", []
        for r in range(n):
            if r in news:
                v = _val(r)
            hdrs.append(b"@%d:%d %s" % (_wrap32(r * 32768), _wrap32(r * 65536), v))
        n_tiles = (n + WG - 1) // WG
        assert n_tiles == {65536: 256, 65537: 257}[n], "tiles against k_chunk_scan's rounds of 256"
        fl = new_flags(hdrs, first, 2)
        assert sorted(r // WG for r in range(n) if fl[r]) == [0, 255, 256][: len(news)], "new string values in tiles 0, 255, 256"
        # the running sums of the deltas, as the unsigned numbers the stream holds
        nums = [[int(v) for v in h[1:].split(b" ")[0].split(b":")] for h in hdrs]
        x = [(a[0] - b[0]) & 0xFFFFFFFF for a, b in zip(nums, [[0, 0]] + nums)]
        y = [(a[1] - b[1]) & 0xFFFFFFFF for a, b in zip(nums, [[0, 0]] + nums)]
        assert all(d != 0 for d in x[1:]) and all(d != 0 for d in y[1:]), "every record has a numeric delta"
        assert (1 << 31) - 32768 == sum(x[: 256 * WG]) and (1 << 32) - 65536 == sum(y[: 256 * WG])
        if n > 256 * WG:  # what the first record of tile 256 adds takes field 0's sum to 2^31 and field 1's to 2^32
            assert sum(x[: 256 * WG + 1]) == 1 << 31 and sum(y[: 256 * WG + 1]) == 1 << 32
            assert hdrs[256 * WG].startswith(b"@-2147483648:0 ")
        yield Case("decode-rounds", "%d-records" % n, first, hdrs, "ok", {})


def _stage_threshold():
    for total in (STAGE_BYTES - 1, STAGE_BYTES, STAGE_BYTES + 1):
        hdrs = []
        for r in range(3 * WG):
            if WG <= r < 2 * WG:  # '@', three digits, ' ', 123 bytes: 128 a header
                hdrs.append((r, _val(r, 123 + (total - STAGE_BYTES if r == WG + 77 else 0))))
            else:
                hdrs.append((100 + r % 7, _val(r, 6)))
        hdrs = _ns(hdrs)
        assert sum(len(h) for h in hdrs[WG: 2 * WG]) == total, "workgroup 1's header bytes total %d" % total
        assert all(sum(len(h) for h in hdrs[w * WG: (w + 1) * WG]) < 4096 for w in (0, 2)), "short headers on either side"
        yield Case("stage-threshold", "%d-bytes" % total, FIRST, hdrs, "ok", {})
    first = b"@a 1 x"  # STRING ' ' NUMERIC ' ' STRING: every field at the longest text it can have
    hdrs = [b"@%s %d %s" % (_val(r, 254), -2147483648 + r % 2, _val(r + 1, 254)) for r in range(WG)]
    assert all(len(h) == 1 + 254 + 1 + 11 + 1 + 254 for h in hdrs) and all(new_flags(hdrs, first, 0)) and all(new_flags(hdrs, first, 2))
    yield Case("stage-threshold", "greatest-length", first, hdrs, "ok", {})


def _numeric_text():
    targets = [0]
    for k in range(1, 10):
        targets += [10 ** k - 1, -(10 ** k - 1), 10 ** k, -(10 ** k)]
    targets += [2147483647, -2147483648]
    vals, how = [], []
    for t in targets:
        near = t - 1 if t > -2147483648 else t + 1
        far = -2147483648 if t >= 0 else 2147483647
        vals += [near, t, far, t]
        how += [None, "small", None, "wrap"]
    hdrs = _ns([(v, b"x") for v in vals])
    prev = 1
    seen = {}
    for v, h in zip(vals, how):
        if h == "small":
            assert abs(v - prev) == 1
            seen.setdefault(v, set()).add(h)
        elif h == "wrap":
            assert abs(v - prev) >= 1 << 31, "the int32 difference wraps"
            seen.setdefault(v, set()).add(h)
        prev = v
    assert all(seen[t] == {"small", "wrap"} for t in targets) and len(targets) == 39
    yield Case("numeric-text", "every-digit-count", FIRST, hdrs, "ok", {})
    # texts std::from_chars reads but std::to_chars does not write: the streams still agree, the headers do not come back
    odd = [b"-0", b"007", b"0" * 21 + b"5", b"12ab"]
    hdrs = [b"@%s x" % odd[r % 4] if r % 3 == 0 else b"@%d x" % (r * 1000003 % 4001 - 2000) for r in range(WG + 45)]
    assert all(len(odd[2]) == 22 and HO.parse_numeric(t) == w for t, w in zip(odd, (0, 7, 5, 12)))
    assert {h[1:].split(b" ")[0] for h in hdrs} >= set(odd)
    yield Case("numeric-text", "texts-that-do-not-come-back", FIRST, hdrs, "ok", {"lossless": False})


def _uncodable():
    first = b"@r.1 x"  # STRING '.' NUMERIC ' ' STRING
    n = 4 * WG
    good = [b"@r.%d %s" % (r + 1, _val(r // 5, 9)) for r in range(n)]
    texts = (("plus-sign", b"@r.+5 x"), ("lone-minus", b"@r.- x"), ("empty-field", b"@r."), ("int32-max-plus-1", b"@r.2147483648 x"),
             ("int32-min-minus-1", b"@r.-2147483649 x"), ("23-digits", b"@r.%d x" % (1000 * 2 ** 64 + 7)),
             ("new-string-of-255", b"@r.7 " + b"z" * 255))
    assert HO.split_header(b"@r.", [46, 32])[1:] == [b"", b""], "an empty numeric field"
    t23 = HO.split_header(dict(texts)["23-digits"], [46, 32])[1]
    assert len(t23) == 23 and int(t23) % 2 ** 64 == 7, "a sum of digits that wraps 64 bits without saturating would be a 7"
    for name, bad in texts:
        for at in (0, WG - 1, WG, 2 * WG - 1, n - WG, n - 1):
            hdrs = list(good)
            hdrs[at] = bad
            later = at + 300
            if later < n:
                hdrs[later] = b"@r.x x"  # a later one, in another workgroup, must not win
                assert later // WG != at // WG
            assert at % WG in (0, WG - 1) and at // WG in (0, 1, 3)
            assert first_uncodable(hdrs, first) == at and first_uncodable(hdrs[:at], first) is None
            yield Case("uncodable", "%s-at-%d" % (name, at), first, hdrs, "uncodable", {"bad": at})
    hdrs = list(good)
    hdrs[WG + 1] = b"@r.2147483648 " + b"z" * 255  # a numeric and a length defect in one record
    assert first_uncodable(hdrs, first) == WG + 1
    yield Case("uncodable", "two-defects-in-one-record", first, hdrs, "uncodable", {"bad": WG + 1})
    out = b"@r.2147483648 x"  # the dataset's first header itself: refused at record 0
    assert HO.format_from_header(out) == HO.format_from_header(first) and first_uncodable(good, out) == 0
    yield Case("uncodable", "first-header-outside-int32", out, good, "uncodable", {"bad": 0})
    # what is still coded: 254 new bytes, and 255 bytes that do not differ
    hdrs = [b"@r.%d %s" % (r + 1, bytes([97 + r % 26]) * 254) for r in range(WG + 44)]
    assert first_uncodable(hdrs, first) is None and all(new_flags(hdrs, first, 2))
    yield Case("uncodable", "new-strings-of-254-are-coded", first, hdrs, "ok", {})
    long_first = b"@r.1 " + b"z" * 255
    hdrs = [b"@r.%d %s" % (r + 1, b"z" * 255) for r in range(WG + 44)]
    assert first_uncodable(hdrs, long_first) is None and not any(new_flags(hdrs, long_first, 2))
    yield Case("uncodable", "a-same-string-of-255-is-coded", long_first, hdrs, "ok", {})


def _separator_first():
    """a field ends at the first separator from its SECOND byte on: fields that begin with their own separator"""
    n = 2 * WG + 10
    first = b"@a b c"  # STRING ' ' STRING ' ' STRING
    hdrs = [b"@ p%d  q%d c%d" % (r, r // 2, r // 7) if r % 5 == 0 or r % WG in (0, WG - 1) else b"@p%d q%d c%d" % (r, r // 2, r // 7)
            for r in range(n)]
    for r in (0, WG - 1, WG, 2 * WG - 1, 2 * WG, 5):
        f = HO.split_header(hdrs[r], [32, 32])
        assert f[0][:1] == b" " and f[1][:1] == b" " and len(f[0]) > 1 and len(f[1]) > 1, "fields 0 and 1 begin with their separator"
    yield Case("separator-first", "strings-that-begin-with-a-space", first, hdrs, "ok", {})
    first = b"@1-2 x"  # NUMERIC '-' NUMERIC ' ' STRING: negative numbers in front of and behind a '-'
    hdrs = [b"@%d-%d %s" % (5 - r, 300 - 3 * r, _val(r // 3, 7)) for r in range(n)]
    for r in (WG - 1, WG, 2 * WG - 1, 2 * WG, n - 1):
        f = HO.split_header(hdrs[r], [45, 32])
        assert f[0][:1] == b"-" and f[1][:1] == b"-" and HO.parse_numeric(f[0]) == 5 - r and HO.parse_numeric(f[1]) == 300 - 3 * r
    assert HO.split_header(hdrs[2], [45, 32])[:2] == [b"3", b"294"]
    yield Case("separator-first", "negative-numbers-beside-a-minus", first, hdrs, "ok", {})


def _mixed(n):
    """sparse new strings of changing length, a number that goes up and down"""
    v, hdrs = b"x", []
    for r in range(n):
        if r % 3 == 0 or r % WG in (0, WG - 1):
            v = _val(r, 1 + (r * 5) % 60)
        hdrs.append((r * 37 % 1000 - 500, v))
    return _ns(hdrs)


def _windows():
    for n in (256, 512, 513):
        hdrs = _mixed(n)
        bounds = sorted({0, 1, 255, 256, 257, 511, 512, n - 1, n, n + 1})
        assert n in bounds and n + 1 in bounds, "bounds the call takes and bounds behind the chunk"
        yield Case("windows", "%d-records" % n, FIRST, hdrs, "windows", {"bounds": bounds})


def _cut(fields, i, k, size):
    out = [list(f) for f in fields]
    assert 0 <= size <= len(out[i][k])
    out[i][k] = out[i][k][:size]
    return [tuple(f) for f in out]


def _refusals():
    n = 4 * WG
    hdrs = _mixed(n)
    fl = new_flags(hdrs, FIRST, 1)
    at = (0, WG - 1, WG, 2 * WG - 1, n - WG, n - 1)
    assert all(fl[r] for r in at), "the records the streams are cut at have new values"
    lens = [len(h.split(b" ", 1)[1]) for h in hdrs]
    assert all(lens[r] >= 1 for r in at)
    rds = reads(n)
    ends, e = [], 0
    for h, (s, _) in zip(hdrs, rds):
        e += len(h) + 2 * len(s) + 5
        ends.append(e)

    def news_before(r):
        return sum(fl[:r])

    def content_before(r):
        return sum(lens[k] for k in range(r) if fl[k])

    damage = []
    for r in at:
        damage += [("flags-cut-to-%d" % r, lambda f, r=r: (_cut(f, 1, 0, r), 0), r),
                   ("lengths-cut-in-front-of-%d" % r, lambda f, r=r: (_cut(f, 1, 2, news_before(r)), 0), r),
                   ("content-one-byte-short-of-%d" % r, lambda f, r=r: (_cut(f, 1, 1, content_before(r) + lens[r] - 1), 0), r),
                   ("numeric-content-of-4x%d+3-bytes" % r, lambda f, r=r: (_cut(f, 0, 1, 4 * r + 3), 0), r),
                   ("raw-len-one-byte-short-of-%d" % r, lambda f, r=r: (f, ends[r] - 1 - ends[-1]), r)]
    damage.append(("two-defects-the-lower-record-wins", lambda f: (_cut(_cut(f, 1, 0, 600), 0, 1, 4 * 300 + 3), 0), 300))
    damage.append(("two-defects-the-lower-record-wins-other-order", lambda f: (_cut(_cut(f, 0, 1, 4 * 900 + 3), 1, 2, news_before(WG)), 0), WG))

    def longer(f):
        return [(f[0][0], f[0][1] + b"\1\2\3\4\5\6\7", f[0][2]), (f[1][0] + b"\1\1\0", f[1][1] + b"tail", f[1][2] + b"\4\xFF")]
    damage.append(("streams-longer-than-needed", lambda f: (longer(f), 0), None))
    damage.append(("raw-len-longer-than-needed", lambda f: (f, 1000), None))
    yield Case("refusals", "%d-records" % n, FIRST, hdrs, "refusals", {"damage": damage})


FAMILIES = (_edge_new, _carried_value, _group_of_256, _encode_rounds, _decode_rounds, _stage_threshold, _numeric_text,
            _uncodable, _separator_first, _windows, _refusals)

_cases = []


def families():
    """every case of every family, in a fixed order, made once; each family's generator asserts its own property"""
    if not _cases:
        for fam in FAMILIES:
            _cases.extend(fam())
        assert len({(c.family, c.name) for c in _cases}) == len(_cases)
    return list(_cases)


def case_id(c):
    return "%s/%s" % (c.family, c.name)


def by_kind(*kinds):
    return [c for c in families() if c.kind in kinds]
