"""The inputs of the block-decoder families (tests/test_decode_families_host.py on the CPU,
tests/test_gpu_decode_families.py on the device).

`families()` is a deterministic generator of small FASTQ blocks plus the tables they are coded with, each aimed at one
edge of the chain walk of fqcomp28_amd/csrc/decode.hip -- walk_positions with its plain and RUN step forms and its stores,
LdsBits, decode_chunk / seed_history / decode_stream<SNAP>, k_gather_ncount and k_npatch -- and each carrying an `assert`
of the property it is named for.  The coded streams are always the oracle's (O.OracleCtx.encode); bit lengths come from
the oracle's streams and the table logs, nbBits from the DTable fo_build_dtable gives.

The generator restates two functions of the reference model on Python ints (calcContext of the quality model and
addSymUpper of the sequence model, as CtxHist in decode.hip restates them): `contexts` gives the context of every position
of a read in decode order, `self_following` says at which steps the next context is the current one, and `step_forms`
replays the switch between the two step forms that walk_positions makes between groups of four.

TEST INFRASTRUCTURE ONLY: nothing under fqcomp28_amd/ imports it.
"""
from collections import namedtuple

import numpy as np

import oracle_lib as O
import ref_pin as R

STRIDE = 65536            # fqgpu_ctx_set_index_stride rounds up to whole multiples of this
BITBUF_DW = 512           # FQ_BITBUF_DW: dwords of LdsBits' LDS buffer
SEQ_INIT = 0xD7           # FSE_Sequence::INITIAL_CONTEXT
LEVELS = (0, 2, 20, 30, 40, 41, 62, 63)  # the Phred values every table set here can code in every context
RARE = (62, 63)           # ... these two with one cell a context in the log-12 tables
BASE_CODE = {65: 0, 67: 1, 71: 2, 84: 3, 78: 0}  # N is coded as A


# ---------------------------------------------------------------------------------------------------------------------
# the model, restated
def contexts(symbols, stream):
    """the context of every position of a read in decode order (position 0 first) and, last, the context behind the last
    symbol; symbols: base codes 0..3 (stream 0) or Phred values (stream 1)"""
    out = []
    if stream == 0:
        c = SEQ_INIT
        for s in symbols:
            out.append(c)
            c = (c >> 2) + (s << 6)  # addSymUpper
        out.append(c)
        return out
    q1 = q2 = 0

    def ctx(q, q1, q2):  # calcContext
        return (((max(q1, q2) << 6) + q) & 0xFFF) + (int(q1 == q2) << 12)
    c = ctx(0, 0, 0)
    for q in symbols:
        out.append(c)
        c = ctx(q, q1, q2)
        q2, q1 = q1, q
    out.append(c)
    return out


def self_following(symbols, stream):
    """per step: the context behind the symbol is the context the symbol was decoded in"""
    c = contexts(symbols, stream)
    return [c[i + 1] == c[i] for i in range(len(symbols))]


def step_forms(selfs):
    """walk_positions over one whole read: [(form, self-following steps)] for every whole group of four, form "plain" or
    "run": the plain form hands over to the RUN form behind a group with two or more self-following steps, the RUN form
    hands back behind a group with none; -> (groups, switches) with switches a list of "up" / "down" """
    form, groups, switches = "plain", [], []
    for g in range(len(selfs) // 4):
        n = sum(selfs[4 * g: 4 * g + 4])
        groups.append((form, n))
        if form == "plain" and n >= 2:
            form = "run"; switches.append("up")
        elif form == "run" and n == 0:
            form = "plain"; switches.append("down")
    return groups, switches


def symbols_of(seq, qual):
    return [BASE_CODE[b] for b in seq], [q - 33 for q in qual]


# ---------------------------------------------------------------------------------------------------------------------
# blocks and tables
def _rng(seed):
    return np.random.default_rng(seed)


def rand_bases(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].tobytes()


def rand_quals(rng, n, levels=LEVELS[:6]):
    return (np.array(levels, dtype=np.uint8)[rng.integers(0, len(levels), size=n)] + 33).astype(np.uint8).tobytes()


def quiet_bases(n, at=0):
    """bases without a self-following step: ACGT in turn"""
    return bytes(b"ACGT"[(at + i) % 4] for i in range(n))


def quiet_quals(n, at=0):
    """qualities without a self-following step: three levels in turn, no two neighbours equal"""
    return bytes((20, 30, 41)[(at + i) % 3] + 33 for i in range(n))


def block(reads, align=None):
    """[(seq, qual)] -> (raw, recs).  align: per read the wanted seq_off mod 4 (None: a header of two bytes); the header's
    length is chosen for it"""
    out = bytearray()
    for k, (seq, qual) in enumerate(reads):
        assert len(seq) == len(qual) >= 3
        h = 2
        if align is not None and align[k] is not None:
            h = 2 + (align[k] - (len(out) + 3)) % 4
        out += b"@" + b"h" * (h - 1) + b"\n" + seq + b"\n+\n" + qual + b"\n"
    raw = np.frombuffer(bytes(out), dtype=np.uint8).copy()
    recs = O.parse_fastq(raw)
    assert len(recs) == len(reads)
    return raw, recs


_tables = {}


def _sample():
    rng = _rng(2801)
    reads = [(rand_bases(rng, 100), rand_quals(rng, 100)) for _ in range(400)]
    return block(reads)


def _ft_from_counts(sc, qc):
    L = O.lib()
    sft, qft = np.zeros(1, dtype=O.SEQ_FT_DTYPE), np.zeros(1, dtype=O.QUAL_FT_DTYPE)
    assert L.fqo_seq_ft_from_counts(O.ptr(np.ascontiguousarray(sc)), O.ptr(sft)) == 0
    assert L.fqo_qual_ft_from_counts(O.ptr(np.ascontiguousarray(qc)), O.ptr(qft)) == 0
    return sft, qft


def tables(key):
    """the named table sets, made once.  "sample": of an unrelated sample (400 random reads over six of the LEVELS; the
    reference's count pass starts every count at one, so every symbol can be coded in every context); "log12": the same
    sample with the common levels counted thousands of times more in every context and the two RARE ones never, every
    context renormalised to 2^12 (ref_pin.rescale_tables) and the RARE symbols left one DTable cell, nbBits 12; "flat": every
    base and every level of LEVELS equally often in every context -- every cell of a context has the same nbBits, so a
    changed payload bit changes symbols and never the bit count"""
    if key not in _tables:
        raw, recs = _sample()
        sc, qc, _, _ = O.freq_tables(raw, recs)
        if key == "sample":
            sc, qc = sc + 1, qc.copy()
            qc[:, list(LEVELS)] += 1
            _tables[key] = _ft_from_counts(sc, qc)
        elif key == "log12":
            sc, qc = sc + 1, qc.copy()
            common = [v for v in LEVELS if v not in RARE]
            assert (qc[:, list(RARE)] == 1).all(), "the sample holds neither: the one count every symbol starts with"
            qc[:, common] += 3000
            sft, qft = _ft_from_counts(sc, qc)
            qft = R.rescale_tables(qft, 12)
            # (a symbol with one cell at log 11 or below comes out of the rescaling with two, nbBits 11: the RARE ones are
            # given one cell, what they lose goes to the context's most frequent symbol)
            norm = qft["norm"][0]
            for r in RARE:
                top = np.argmax(norm, axis=1)
                assert (np.abs(norm[:, r]) <= 2).all() and (top != r).all()
                norm[np.arange(norm.shape[0]), top] += np.abs(norm[:, r]) - 1
                norm[:, r] = 1
            assert (np.abs(norm.astype(np.int64)).sum(axis=1) == 4096).all()
            _tables[key] = (sft, qft)
        elif key == "flat":
            sc, qc = np.full_like(sc, 512), np.zeros_like(qc)
            qc[:, list(LEVELS)] = 512
            _tables[key] = _ft_from_counts(sc, qc)
        else:
            raise KeyError(key)
    return _tables[key]


def dtable(ft, c):
    """fo_build_dtable of context c -> the cells (without the header word)"""
    L = O.lib()
    log = int(ft["logs"][0][c])
    norm = np.ascontiguousarray(ft["norm"][0][c])
    dt = np.zeros(L.fo_dtable_words(log), dtype=np.uint32)
    assert L.fo_build_dtable(O.ptr(dt), O.ptr(norm), len(norm) - 1, log) == 0
    return dt[1: 1 + (1 << log)]


def nb_bits(ft, c, sym):
    """the set of nbBits of the cells of context c that hold symbol sym"""
    cells = dtable(ft, c)
    return set(int(x) >> 24 for x in cells[((cells >> 16) & 0xFF) == sym])


# Cases.  kind: "ok" (coded, restored byte for byte) or "damage" (extra["base"]: the case whose streams are damaged,
# extra["damage"]: (stream, name, bytes -> bytes)).  tables: a key of tables() or "own" (the block's own tables).
# extra["n_pos_front"]: entries put in front of the oracle's n_pos (an N buffer longer than the block's total).
Case = namedtuple("Case", "family name raw recs tables kind extra")


def case_tables(case):
    if case.tables == "own":
        _, _, sft, qft = O.freq_tables(case.raw, case.recs)
        return sft, qft
    return tables(case.tables)


_octx = {}


def oracle_ctx(case):
    """the oracle's coder for the case's tables (the named sets: made once)"""
    if case.tables == "own":
        return O.OracleCtx(*case_tables(case))
    if case.tables not in _octx:
        _octx[case.tables] = O.OracleCtx(*tables(case.tables))
    return _octx[case.tables]


_coded = {}


def coded(case):
    """the oracle's streams of a case, made once: dict(seq, qual, n_count, n_pos, readlens, rc); a "damage" case: its
    base's streams with the damage applied"""
    key = case_id(case)
    if key not in _coded:
        if case.kind == "damage":
            e = dict(coded(case.extra["base"]))
            stream, _, fn = case.extra["damage"]
            k = ("seq", "qual")[stream]
            e[k] = np.frombuffer(fn(e[k].tobytes()), dtype=np.uint8).copy()
        else:
            e = oracle_ctx(case).encode(case.raw, case.recs)
            e.pop("raw_after")
            front = case.extra.get("n_pos_front", 0)
            if front:
                e["n_pos"] = np.concatenate([np.full(front, 0x7777, dtype=np.uint16), e["n_pos"]])
        _coded[key] = e
    return _coded[key]


def oracle_decode(case):
    """-> (rc, bytes): the oracle's decoder over the case's streams into the blanked block"""
    e = coded(case)
    return oracle_ctx(case).decode(e["seq"], e["qual"], e["n_count"], e["n_pos"], case.recs, O.blank_skeleton(case.raw, case.recs))


def sum_logs(ft):
    return int(ft["logs"][0].astype(np.int64).sum())


def payload_bits(stream_bytes, ft):
    """where the walk starts: the bits below the state flush = the position of the end mark less the table logs"""
    b = bytes(stream_bytes)
    assert b and b[-1]
    return (len(b) - 1) * 8 + b[-1].bit_length() - 1 - sum_logs(ft)


# ---------------------------------------------------------------------------------------------------------------------
# lengths: the store path of walk_positions
LENGTHS = tuple(range(3, 21)) + tuple(range(251, 262)) + tuple(range(507, 518)) + tuple(range(1019, 1030))
LONGEST = 65535


def _read(rng, n):
    s, q = bytearray(rand_bases(rng, n)), bytearray(rand_quals(rng, n))
    if n >= 16:  # a homopolymer and a constant-quality stretch on the way: both step forms store
        s[n // 2: n // 2 + 7] = b"G" * len(s[n // 2: n // 2 + 7])
        q[n // 3: n // 3 + 6] = b"I" * len(q[n // 3: n // 3 + 6])
    return bytes(s), bytes(q)


def _lengths():
    rng = _rng(11)
    seen = {}

    def note(n, recs, k, where):
        seen.setdefault(n, set()).add((where, int(recs[k]["seq_off"]) % 4, int(recs[k]["qual_off"]) % 4))

    for n in LENGTHS + (LONGEST,):
        raw, recs = block([_read(rng, n)], align=[n % 4])
        note(n, recs, 0, "alone")
        yield Case("lengths", "alone-%d" % n, raw, recs, "sample", "ok", {})
    groups = [LENGTHS[i: i + 6] for i in range(0, len(LENGTHS), 6)]
    for group in groups:
        reads, align, which = [_read(rng, 37)], [None], [None]
        for n in group:
            for a in range(4):
                reads += [_read(rng, n), _read(rng, 5 + a)]
                align += [a, None]
                which += [n, None]
        raw, recs = block(reads, align)
        for k, n in enumerate(which):
            if n is not None:
                assert which[k - 1] is None and which[k + 1] is None, "a read on either side"
                note(n, recs, k, "between")
        yield Case("lengths", "between-%d-to-%d" % (group[0], group[-1]), raw, recs, "sample", "ok", {})
    raw, recs = block([_read(rng, 9), _read(rng, LONGEST), _read(rng, 10)], align=[None, 3, None])
    note(LONGEST, recs, 1, "between")
    yield Case("lengths", "between-%d" % LONGEST, raw, recs, "sample", "ok", {})
    for n in LENGTHS:
        assert {(w, a) for w, a, _ in seen[n] if w == "between"} == {("between", a) for a in range(4)}, "sequence lines at all four alignments"
        assert {b for w, _, b in seen[n] if w == "between"} == {0, 1, 2, 3}, "quality lines at all four alignments"
        assert any(w == "alone" for w, _, _ in seen[n])
    assert {w for w, _, _ in seen[LONGEST]} == {"alone", "between"}
    # what the lengths are chosen for: r = n mod 4 tail bytes 0..3, `full` = whole dwords behind the last 256-byte store
    # 0, 1, 2, 62, 63, and one, two, four and 255 stores of 256 bytes
    assert {n % 4 for n in LENGTHS} == {0, 1, 2, 3}
    assert {0, 1, 2, 62, 63} <= {((n & ~3) >> 2) & 63 for n in LENGTHS}
    assert {1, 2, 4, 255} <= {n // 256 for n in LENGTHS + (LONGEST,)}


# ---------------------------------------------------------------------------------------------------------------------
# runs: the plain and the RUN form of step() and the switch between groups of four
def _with_runs(n_steps, at, total):
    """a read of `total` symbols whose self-following steps are exactly [at, at + n_steps), in both streams: a homopolymer
    of n_steps + 4 bases and a constant quality of n_steps + 3 values that end at position at + n_steps"""
    end = at + n_steps
    s, q = bytearray(quiet_bases(total)), bytearray(quiet_quals(total))
    assert end - (n_steps + 4) >= 0 and end < total
    s[end - (n_steps + 4): end] = b"T" * (n_steps + 4)
    s[end] = ord("A")  # (whatever base follows a run of T: not T)
    if end - (n_steps + 4) > 0 and s[end - (n_steps + 5)] == ord("T"):
        s[end - (n_steps + 5)] = ord("C")
    # (a value above its neighbours': with a lower one max(q1, q2) can make a context follow itself one step early)
    q[end - (n_steps + 3): end] = bytes([63 + 33]) * (n_steps + 3)
    return bytes(s), bytes(q)


def _runs_blocks():
    """(name, reads)"""
    reads = []
    for n in range(1, 13):
        for start in range(4):
            at = 8 + start
            read = _with_runs(n, at, at + n + 9)
            for stream, syms in enumerate(symbols_of(*read)):
                sf = self_following(syms, stream)
                assert [i for i, x in enumerate(sf) if x] == list(range(at, at + n)), (n, start, stream)
            reads.append(read)
    yield "inserted-1-to-12-at-0-to-3", reads
    # both switch directions in one read, twice; a run across position 256
    a, b, c = _with_runs(6, 9, 40), _with_runs(9, 10, 40), _with_runs(30, 240, 300)
    reads = [(a[0] + b[0], a[1] + b[1]), c]
    sw = step_forms(self_following(symbols_of(*reads[0])[0], 0))[1]
    assert sw == ["up", "down", "up", "down"], sw
    sf = self_following(symbols_of(*c)[1], 1)
    assert all(sf[240:270]) and not sf[239] and not sf[270], "a run across position 256"
    yield "both-switches-and-position-256", reads
    # whole reads of one value, lengths 0..3 mod 4: the tail in RUN form has 0, 1, 2, 3 symbols; Phred 0 self-follows
    # from the first symbol
    reads = []
    for n in (5, 6, 7, 8, 9, 10, 11, 12, 33):
        for base, q in ((b"A", 40), (b"T", 0), (b"C", 63), (b"G", 0)):
            reads.append((base * n, bytes([q + 33]) * n))
        reads.append((quiet_bases(n), quiet_quals(n)))
    sf = self_following([0] * 9, 1)
    assert all(sf), "a Phred-0 read follows itself from the first symbol (CtxHist<QualModel>::start)"
    sf = self_following([40] * 9, 1)
    assert sf == [False] * 3 + [True] * 6
    assert self_following([0] * 9, 0) == [False] * 4 + [True] * 5
    assert self_following([3] * 9, 0) == [False] * 3 + [True] * 6, "the base in front of a read counts as T (INITIAL_CONTEXT)"
    assert {n % 4 for n in (5, 6, 7, 8)} == {0, 1, 2, 3}
    yield "one-value-reads", reads
    # a run that ends with the read, its context entered again by a read decoded later (= earlier in the block): the
    # slot the run left stale is what the later read finds
    late = (quiet_bases(9) + b"G" * 9, quiet_quals(9) + bytes([30 + 33]) * 9)     # decoded first
    early = (quiet_bases(5) + b"G" * 7 + b"ACA", quiet_quals(5) + bytes([30 + 33]) * 6 + quiet_quals(4))
    for stream in (0, 1):
        l, e = symbols_of(*late)[stream], symbols_of(*early)[stream]
        cl, ce = contexts(l, stream), contexts(e, stream)
        assert self_following(l, stream)[-1] and self_following(l, stream)[-2], "the run ends with the read"
        assert cl[-1] in ce[:-1], "the same context is entered again by the read decoded next"
    yield "stale-slot", [early, late, early, late]


def _runs():
    groups = {0: set(), 1: set()}
    both = {0: False, 1: False}
    for name, reads in _runs_blocks():
        raw, recs = block(reads)
        for read in reads:
            for stream, syms in enumerate(symbols_of(*read)):
                g, sw = step_forms(self_following(syms, stream))
                groups[stream] |= set(g)
                both[stream] |= "up" in sw and "down" in sw
        for t in ("own", "sample"):
            yield Case("runs", "%s-%s-tables" % (name, t), raw, recs, t, "ok", {})
    for stream in (0, 1):
        assert groups[stream] == {(f, n) for f in ("plain", "run") for n in range(5)}, ("groups of four with 0..4 self-following steps, in either form", stream, sorted(groups[stream]))
        assert both[stream], "both switch directions in one read"


# ---------------------------------------------------------------------------------------------------------------------
# window: LdsBits
WINDOW_K = (1, 510, 511, 512, 1022, 1023, 1024)


class _Grower:
    """blocks of the first n symbols of one fixed random read stream (reads of 100, the last one 3..102), under the "sample"
    tables; hit(stream, wanted): grows n a base at a time through the neighbourhood of the wanted payload bit counts"""

    def __init__(self, seed):
        rng = _rng(seed)
        self.bases, self.quals = rand_bases(rng, 40000), rand_quals(rng, 40000)
        self.fts = tables("sample")
        self.octx = O.OracleCtx(*self.fts)
        self.memo = {}

    def block(self, n):
        cuts = list(range(0, n, 100)) + [n]
        if len(cuts) > 2 and cuts[-1] - cuts[-2] < 3:
            del cuts[-2]
        return block([(self.bases[a:b], self.quals[a:b]) for a, b in zip(cuts, cuts[1:])])

    def bits(self, n):
        if n not in self.memo:
            raw, recs = self.block(n)
            e = self.octx.encode(raw, recs)
            assert e["rc"] == 0
            self.memo[n] = (payload_bits(e["seq"], self.fts[0]), payload_bits(e["qual"], self.fts[1]), len(e["seq"]), len(e["qual"]))
        return self.memo[n]

    def near(self, stream, target):
        """an n whose payload bit count lies just below target"""
        n = 3
        per = self.bits(4000)[stream] / 4000.0
        for _ in range(8):
            n = max(3, min(39000, n + int((target - 24 - self.bits(n)[stream]) / per)))
        while self.bits(n)[stream] >= target - 1 and n > 3:
            n -= 1
        return n


def _window_search(wanted, key_of, seeds=range(40, 80)):
    """-> {key: (seed, n)} for every key of `wanted`; key_of(stream, bits tuple) -> key or None"""
    found = {}
    for seed in seeds:
        g = _Grower(seed)
        for stream, target in sorted({(k[0], k[1]) for k in wanted if k not in found}):
            n = g.near(stream, target)
            for n in range(n, min(n + 40, 39900)):
                key = key_of(stream, g.bits(n))
                if key in wanted and key not in found:
                    found[key] = (seed, n)
                if g.bits(n)[stream] > target + 8:
                    break
        if len(found) == len(wanted):
            return found
    raise AssertionError("payload bit counts not reached: %r" % sorted(set(wanted) - set(found)))


def _window():
    wanted = {(stream, 32 * k, d) for stream in (0, 1) for k in WINDOW_K for d in (-1, 0, 1)}

    def key_of(stream, bits):
        for d in (-1, 0, 1):
            if (bits[stream] - d) % 32 == 0 and (bits[stream] - d) // 32 in WINDOW_K:
                return (stream, bits[stream] - d, d)
        return None
    found = _window_search(wanted, key_of)
    growers, mod4 = {}, {0: set(), 1: set()}
    for (stream, target, d), (seed, n) in sorted(found.items()):
        g = growers.setdefault(seed, _Grower(seed))
        raw, recs = g.block(n)
        c = Case("window", "%s-walk-starts-at-32x%d%+d" % (("seq", "qual")[stream], target // 32, d), raw, recs, "sample", "ok", {})
        e = coded(c)
        got = payload_bits(e[("seq", "qual")[stream]], tables("sample")[stream])
        assert got == target + d, "the %s walk starts at payload bit %d" % (("seq", "qual")[stream], target + d)
        mod4[0].add(len(e["seq"]) % 4); mod4[1].add(len(e["qual"]) % 4)
        yield c
    # place() fills the buffer up to dword (pos0 >> 5) + 1: on either side of the buf_lo rule's bound, twice as far (the first
    # refill of dword() then has the bottom of the stream on either side of a whole buffer), and with d_lo == -1 at once
    tops = {((32 * k + d) >> 5) + 1 for k in WINDOW_K for d in (-1, 0, 1)}
    assert tops >= {1, BITBUF_DW - 2, BITBUF_DW - 1, BITBUF_DW, BITBUF_DW + 1, 2 * BITBUF_DW - 1, 2 * BITBUF_DW, 2 * BITBUF_DW + 1}
    # stream byte lengths 0..3 mod 4 in both streams: what the targets above leave out is grown for
    g = _Grower(39)
    for stream in (0, 1):
        n = 150
        while mod4[stream] != {0, 1, 2, 3}:
            m = g.bits(n)[2 + stream] % 4
            if m not in mod4[stream]:
                mod4[stream].add(m)
                raw, recs = g.block(n)
                yield Case("window", "%s-stream-of-4k+%d-bytes" % (("seq", "qual")[stream], m), raw, recs, "sample", "ok", {})
            n += 1
            assert n < 1000
    raw, recs = block([(b"GAT", b"I5!")])
    yield Case("window", "one-read-of-3-bases", raw, recs, "sample", "ok", {})
    # log-12 tables, quality reads of symbols with nbBits 12, many in a row: two reads of 12 bits between two looks at the
    # window take rel from 32 down to 8, the bound of `look_after`
    sft, qft = tables("log12")
    a, b = RARE
    rare_reads = [[a] * 40, [a, b] * 20, [b, b, a] * 13, [a] * 3 + [b] * 37, [b] * 41]
    reads = []
    for k, qs in enumerate(rare_reads):
        ctxs = contexts(qs, 1)
        for c, q in zip(ctxs, qs):
            assert nb_bits(qft, c, q) == {12}, "every cell of symbol %d in context %d has nbBits 12" % (q, c)
        reads.append((quiet_bases(len(qs), k), bytes(q + 33 for q in qs)))
        reads.append((quiet_bases(7, k), quiet_quals(7, k)))
    assert int(qft["logs"][0].min()) == int(qft["logs"][0].max()) == 12
    raw, recs = block(reads)
    c = Case("window", "log12-runs-of-12-bit-symbols", raw, recs, "log12", "ok", {})
    assert payload_bits(coded(c)["qual"], qft) >= 12 * sum(len(q) for q in rare_reads)
    yield c


# ---------------------------------------------------------------------------------------------------------------------
# n: k_gather_ncount, the scan, k_npatch
def _n():
    rng = _rng(13)

    def with_n(n, where):
        s, q = bytearray(rand_bases(rng, n)), rand_quals(rng, n)
        for p in where:
            s[p] = ord("N")
        return bytes(s), q

    def plain(n):
        return rand_bases(rng, n), rand_quals(rng, n)

    reads = [with_n(40, [0]), plain(9), with_n(40, [39]), plain(3), with_n(40, range(40)), with_n(40, range(0, 40, 2)), plain(50),
             with_n(40, range(1, 40, 2)), with_n(60, list(range(5, 12)) + list(range(30, 33)) + [59]), with_n(3, [0]), plain(3),
             with_n(3, [2]), with_n(3, [0, 1, 2]), plain(20), with_n(3, [1]), with_n(300, [0, 255, 256, 299])]
    raw, recs = block(reads)
    counts = [s.count(b"N") for s, _ in reads]
    assert counts == [1, 0, 1, 0, 40, 20, 0, 20, 11, 1, 0, 1, 3, 0, 1, 4], "N first, last, everywhere, every other, in runs; reads without N between"
    yield Case("n", "short-reads", raw, recs, "sample", "ok", {})
    # an N buffer longer than the block's own total: the counts and deltas are taken from the END (k_npatch's `shift`)
    c = Case("n", "short-reads-n-buffer-longer-than-the-total", raw, recs, "sample", "ok", {"n_pos_front": 37})
    assert len(coded(c)["n_pos"]) == sum(counts) + 37 and int(coded(c)["n_count"].sum()) == sum(counts)
    yield c
    long_n = [0] + list(range(1000, 1010)) + list(range(30000, 30600, 2)) + [LONGEST - 1]
    reads = [plain(5), with_n(3, [1]), plain(4), with_n(LONGEST, long_n), plain(6), with_n(3, [0, 2]), plain(3)]
    raw, recs = block(reads)
    assert [len(s) for s, _ in reads] == [5, 3, 4, LONGEST, 6, 3, 3] and reads[3][0][0] == reads[3][0][-1] == ord("N")
    yield Case("n", "reads-of-3-and-65535", raw, recs, "sample", "ok", {})
    raw, recs = block([plain(30), plain(3), plain(17)])
    yield Case("n", "no-n-at-all", raw, recs, "sample", "ok", {"n_pos_front": 5})


# ---------------------------------------------------------------------------------------------------------------------
# strides: decode_chunk, seed_history, the pieces of decode_stream<SNAP>
def rec_starts(recs):
    """encode index of the first symbol of every record, and the total"""
    return np.concatenate([[0], np.cumsum(recs["len"].astype(np.int64))])


def boundary_places(recs, stride=STRIDE):
    """per snapshot k = 1 ..: (record, i1) with i1 = one past the position of symbol k * stride in its record: the record is
    walked as [0, i1) and [i1, len)"""
    rs = rec_starts(recs)
    out = []
    for k in range(1, (int(rs[-1]) - 1) // stride + 1):
        r = int(np.searchsorted(rs, k * stride, side="right")) - 1
        out.append((r, int(rs[r] + recs["len"][r]) - k * stride))
    return out


def _strides_block(rng, specials, tail):
    """reads of 100 with, for every (read, i1) of `specials` in turn, the read placed so that the next stride boundary
    falls i1 positions into it; `tail` symbols behind the last boundary"""
    reads, total = [], 0
    for k, (read, i1) in enumerate(specials, 1):
        want = k * STRIDE + i1 - len(read[0])  # the special read's first encode index
        fill = want - total
        assert fill >= 3
        sizes = [100] * (fill // 100)
        rest = fill - 100 * len(sizes)
        if rest:
            if rest < 3:
                sizes[-1] -= 3 - rest
                rest = 3
            sizes.append(rest)
        reads += [(rand_bases(rng, n), rand_quals(rng, n)) for n in sizes] + [read]
        total = want + len(read[0])
    sizes = [100] * (tail // 100) + ([tail % 100] if tail % 100 >= 3 else [])
    reads += [(rand_bases(rng, n), rand_quals(rng, n)) for n in sizes]
    return reads


def _strides():
    rng = _rng(17)
    run = (quiet_bases(30) + b"C" * 40 + quiet_bases(30), quiet_quals(30) + bytes([41 + 33]) * 40 + quiet_quals(30))
    ordinary = (rand_bases(rng, 100), rand_quals(rng, 100))
    three = (b"TGC", bytes([63, 33, 74]))
    shapes = (("inside-a-run", [(run, 50)], 300), ("first-position-of-a-read", [(ordinary, 1)], 7),
              ("last-position-of-a-read", [(ordinary, 99)], 203), ("between-two-reads", [(ordinary, 100)], 150),
              ("inside-a-read-of-3-after-1", [(three, 1)], 41), ("inside-a-read-of-3-after-2", [(three, 2)], 3),
              ("three-strides", [(run, 35), (three, 2)], 77))
    for name, specials, tail in shapes:
        reads = _strides_block(rng, specials, tail)
        raw, recs = block(reads)
        n_sym = int(recs["len"].sum())
        places = boundary_places(recs)
        assert len(places) == len(specials) and (n_sym - 1) // STRIDE == len(specials), "%d strides" % (len(specials) + 1)
        assert n_sym > len(specials) * STRIDE, "symbols behind the last boundary"
        for (read, i1), (r, got) in zip(specials, places):
            assert got == i1 and reads[r] == read, "the boundary falls %d positions into the read meant" % i1
            assert 1 <= i1 <= len(read[0])
        if name == "inside-a-run":
            r, i1 = places[0]
            for stream, syms in enumerate(symbols_of(*reads[r])):
                sf = self_following(syms, stream)
                assert all(sf[i1 - 4: i1 + 4]), "self-following steps on both sides of the boundary"
        if name == "between-two-reads":
            assert places[0][1] == len(reads[places[0][0]][0])
        yield Case("strides", name, raw, recs, "sample", "ok", {"n_strides": len(specials) + 1})


# ---------------------------------------------------------------------------------------------------------------------
# damage
def _mark(b):
    return b[-1].bit_length() - 1


def _mark_up(b):
    hb = _mark(b)
    if hb == 7:
        return b[:-1] + bytes([b[-1] & 0x7F, 1])
    return b[:-1] + bytes([(b[-1] & ~(1 << hb)) | (2 << hb)])


def _mark_down(b):
    hb = _mark(b)
    if hb == 0:
        return b[:-2] + bytes([b[-2] | 0x80])
    return b[:-1] + bytes([(b[-1] & ~(1 << hb)) | (1 << (hb - 1))])


def _flip(at_of):
    return lambda b: b[: at_of(b)] + bytes([b[at_of(b)] ^ 0x10]) + b[at_of(b) + 1:]


DAMAGE = tuple([("cut-by-%d" % k, lambda b, k=k: b[:-k]) for k in (1, 2, 3, 4)] +
               # (the states of contexts a block never enters are flushed as zeros, so a short cut often ends in a zero byte;
               # this one ends in a set bit: in a small block the mark then lies below what the state flush takes)
               [("cut-to-a-quarter", lambda b: b[: len(b) // 4].rstrip(b"\0") or b[:1]),
                ("end-mark-up-one-bit", _mark_up), ("end-mark-down-one-bit", _mark_down),
                ("last-byte-zero", lambda b: b[:-1] + b"\0"),
                ("bit-flipped-in-the-first-payload-byte", _flip(lambda b: 0)),
                ("bit-flipped-in-a-middle-payload-byte", _flip(lambda b: len(b) // 3))])
DAMAGE_BASES = (("lengths", "between-3-to-8", None), ("runs", "both-switches-and-position-256-sample-tables", None),
                ("runs", "one-value-reads-sample-tables", "flat"), ("window", "seq-walk-starts-at-32x511+0", None),
                ("window", "one-read-of-3-bases", None),  # (a cut leaves fewer bits than the state flush takes)
                ("n", "short-reads", None), ("strides", "inside-a-run", None), ("strides", "inside-a-run", "flat"))


def _damage(cases):
    by_id = {(c.family, c.name): c for c in cases}
    for family, name, other_tables in DAMAGE_BASES:
        base = by_id[(family, name)]
        if other_tables:
            base = base._replace(name="%s-%s-tables" % (base.name, other_tables), tables=other_tables)
        for stream in (0, 1):
            for what, fn in DAMAGE:
                yield Case("damage", "%s/%s/%s-%s" % (family, base.name, ("seq", "qual")[stream], what), base.raw, base.recs,
                           base.tables, "damage", {"base": base, "damage": (stream, what, fn)})


FAMILIES = (_lengths, _runs, _window, _n, _strides)

_cases = []


def families():
    """every case of every family, in a fixed order, made once; each family's generator asserts its own property"""
    if not _cases:
        for fam in FAMILIES:
            _cases.extend(fam())
        _cases.extend(_damage(list(_cases)))
        assert len({(c.family, c.name) for c in _cases}) == len(_cases)
    return list(_cases)


def case_id(c):
    return "%s/%s" % (c.family, c.name)


def of_family(*names):
    return [c for c in families() if c.family in names]
