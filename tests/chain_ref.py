"""The quality chain stage of the encoder (fqcomp28_amd/csrc/enc_chains_generic.h: k_seg_scan, k_seg_stage1 with its walk,
candidate and set-function roles, k_seg_heads, k_seg_compose, k_seg_resolve2/3, k_seg_walk<2>), restated, and the inputs of
its families (tests/test_chain_families_host.py on the CPU, tests/test_gpu_chain_families.py on the device).

Restated on Python ints and numpy, from the tables and the block alone:
  runs        the symbols of every quality context in encode order (records forward, positions backward; calcContext)
  cells       what k_seg_scan puts in s_cells
  classify    (class, anchor) of every segment of a run, by k_seg_scan's rules -- a LIST of allowed outcomes, because the
              power table of a context goes to the first uniform symbol to ask, and that is a race on the device
  route       who computes a segment's function (seg_wants_setfunc / seg_fslot / seg_entry_known) and which items of 64
              segments own a composed function
  set_sizes   how many distinct states are carried behind 4, 16, 48, 128, 512 and 2048 symbols of a segment: the merge
              points of seg_setfunc_role

`families()` is a deterministic generator of small blocks, each aimed at one branch, and each family asserts the property it
is named for.  How a case steers one context: a read of four qualities `a a a x` puts x into context T(a) = calcContext(a, a,
a) and a into contexts 4096, calcContext(a, 0, 0) and calcContext(a, a, 0); n such reads give T(a) any chosen run of n
symbols.  The quality tables are crafted: every context but the targets gives each of the 64 symbols one cell (log 6: every
symbol a reset symbol), the target contexts get the rows of ROWS.

TEST INFRASTRUCTURE ONLY: nothing under fqcomp28_amd/ imports it.
"""
import numpy as np

import decode_ref as D
import oracle_lib as O
from decode_ref import Case, contexts  # noqa: F401  (the cases have decode_ref's shape)

SEG_NONE = 0xFFFFFFFF
MAX_CAND = 64             # SEG_MAX_CAND
OPAQUE, UNIFORM = 0, 0xFF
SEG_SLOT = 16             # lanes of one candidate walk: 64 / SEG_SLOT segments share a wave
ITEM = 64                 # segments per item of the resolve
STOPS = (4, 16, 48, 128, 512, 2048)  # symbols behind which seg_setfunc_role counts its states
SETS_MAX_CLASSES = 512
MAX_FASTQ = 5 << 19       # 2.5 MiB: no case is larger


# ---------------------------------------------------------------------------------------------------------------------
# the model, restated
def calc_context(q, q1, q2):
    return (((max(q1, q2) << 6) + q) & 0xFFF) + (int(q1 == q2) << 12)


def target(a):
    """the context of x in a read `a a a x`"""
    return calc_context(a, a, a)


def runs(raw, recs):
    """{context: uint8 array}: the symbols of every non-empty quality context in encode order"""
    lens = recs["len"].astype(np.int64)
    total = int(lens.sum())
    first = np.concatenate([[0], np.cumsum(lens)[:-1]])
    rid = np.repeat(np.arange(len(recs)), lens)
    p = lens[rid] - 1 - (np.arange(total) - first[rid])  # position inside the record: the last one first
    base = recs["qual_off"].astype(np.int64)[rid]
    raw = np.asarray(raw)

    def at(k):  # the quality k positions in front, 0 in front of the read
        ok = p - k >= 0
        return np.where(ok, raw[np.where(ok, base + p - k, 0)].astype(np.int64) - 33, 0)
    sym, d1, d2, d3 = at(0), at(1), at(2), at(3)
    ctx = (((np.maximum(d2, d3) << 6) + d1) & 0xFFF) + ((d2 == d3).astype(np.int64) << 12)
    order = np.argsort(ctx, kind="stable")
    ctx_sorted, sym_sorted = ctx[order], sym[order].astype(np.uint8)
    cuts = np.flatnonzero(np.diff(ctx_sorted)) + 1
    return {int(ctx_sorted[a]): sym_sorted[a:b] for a, b in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [total]]))}


def cells(qft, c):
    """per symbol: 1 for a normalised count of 1 or -1, the count for 2 .. 64, 255 otherwise"""
    v = qft["norm"][0][c].astype(np.int64)
    return np.where(v == -1, 1, np.where((v >= 1) & (v <= MAX_CAND), v, 255)).astype(np.int64)


def classify(run, cell, S):
    """-> the list of allowed outcomes, each a list of (class, anchor) per segment of S symbols"""
    assert S <= 1 << 20, "anchors are looked for in the first 2^20 symbols of a segment"
    run = np.asarray(run)
    fixed, asking = [], {}
    for k in range(0, len(run), S):
        seg = run[k: k + S]
        c = cell[seg]
        resets = np.flatnonzero(c == 1)
        if resets.size:
            fixed.append((1, int(resets[0])))
        elif int(c.min()) <= MAX_CAND:
            fixed.append((int(c.min()), int(np.argmin(c))))  # (argmin: the lowest offset of the smallest)
        elif len(seg) == S and (seg == seg[0]).all():
            asking.setdefault(int(seg[0]), []).append(len(fixed))
            fixed.append(None)
        else:
            fixed.append((OPAQUE, SEG_NONE))
    if not asking:
        return [fixed]
    out = []
    for winner in sorted(asking):
        o = list(fixed)
        for s, where in asking.items():
            for i in where:
                o[i] = (UNIFORM, s) if s == winner else (OPAQUE, SEG_NONE)
        out.append(o)
    return out


def kind_of(cls):
    """T transparent, A anchored, U uniform, O opaque"""
    return "T" if cls == 1 else "U" if cls == UNIFORM else "O" if cls == OPAQUE else "A"


def route(classes):
    """classes of one chain -> (per segment "none" / "setfunc" / "cand" / "pow", per item of 64 segments has_g)"""
    n = len(classes)
    out = []
    for k, cls in enumerate(classes):
        if k + 1 >= n or cls == 1:
            out.append("none")     # nothing follows, or k_seg_walk<1> knows the exit state
        elif cls == UNIFORM:
            out.append("pow")
        elif cls == OPAQUE:
            out.append("setfunc")
        else:
            pred = classes[k - 1] if k else 1
            known = k == 0 or pred == 1 or 2 <= pred <= MAX_CAND
            out.append("cand" if known else "setfunc")
    has_g = [any(r != "none" for r in out[i: i + ITEM]) for i in range(0, n, ITEM)]
    return out, has_g


def ctable(qft, c):
    """fo_build_ctable of context c -> (log, stateTable as int64, deltaFindState per symbol, deltaNbBits per symbol)"""
    L = O.lib()
    log = int(qft["logs"][0][c])
    norm = np.ascontiguousarray(qft["norm"][0][c])
    ct = np.zeros(int(L.fo_ctable_words(log, len(norm) - 1)) + 4, dtype=np.uint32)
    assert L.fo_build_ctable(O.ptr(ct), O.ptr(norm), len(norm) - 1, log) == 0
    size = 1 << log
    st = ct.view(np.uint16)[2: 2 + size].astype(np.int64)
    tt = ct[1 + (size >> 1): 1 + (size >> 1) + 2 * len(norm)]
    return log, st, tt[0::2].astype(np.int32).astype(np.int64), tt[1::2].astype(np.int64)


def step_all(ct, x, s):
    """FSE_encodeSymbol's state change for an array of states"""
    _, st, dfs, dnb = ct
    nb = (x + dnb[s]) >> 16
    return st[(x >> nb) + dfs[s]]


def set_sizes(ct, symbols, stops=STOPS):
    """distinct states carried behind stops[i] symbols, from all 2^log states; -> list (as far as the symbols reach)"""
    size = 1 << ct[0]
    x = np.arange(size, 2 * size, dtype=np.int64)
    out = []
    for i, s in enumerate(symbols):
        x = step_all(ct, x, int(s))
        if i + 1 in stops:
            x = np.unique(x)
            out.append(len(x))
    return out


def setfunc_walks(sizes, S):
    """seg_setfunc_role over one segment of S symbols whose set_sizes are `sizes` -> (stop at which level 1 starts or None,
    [(n + 63) / 64 of every seg_sets_walk call])"""
    stops = [t for t in STOPS if t < S]  # (no merge at the segment's end)
    level1, n, cases = None, None, []
    for i, t in enumerate(stops):
        if level1 is None:
            if sizes[i] <= SETS_MAX_CLASSES:
                level1, n = i, sizes[i]
        elif n > 64:
            n = sizes[i]
        if level1 is not None:
            cases.append(min((n + 63) // 64, 8))
    return level1, cases


def walk_ints(ct, symbols, x=None):
    """one state through the symbols, on Python ints -> the final state"""
    log, st, dfs, dnb = ct
    st, dfs, dnb = st.tolist(), dfs.tolist(), dnb.tolist()
    x = (1 << log) if x is None else x  # FSE_initCState
    for s in symbols.tolist() if hasattr(symbols, "tolist") else symbols:
        x = st[(x >> ((x + dnb[s]) >> 16)) + dfs[s]]
    return x


def flushed_states(stream, qft, wanted):
    """the state flush at the end of a quality stream -> {context: state} for the wanted contexts"""
    logs = qft["logs"][0].astype(np.int64)
    offs = D.payload_bits(stream, qft) + np.concatenate([[0], np.cumsum(logs)[:-1]])
    big = int.from_bytes(bytes(stream), "little")
    return {c: (1 << int(logs[c])) + ((big >> int(offs[c])) & ((1 << int(logs[c])) - 1)) for c in wanted}


# ---------------------------------------------------------------------------------------------------------------------
# tables
R0, R1, C2, C16, C17, C63, C64, C65, BIG8, BIG9, C33, C16B = range(12)
BIG = (C65, BIG8, BIG9)
# the row of most target contexts, log 10: two reset symbols (counts 1 and -1), anchors of 2, 16, 16, 17, 33, 63 and 64
# cells, and three symbols too large to be one
ROW10 = (10, {R0: 1, R1: -1, C2: 2, C16: 16, C17: 17, C63: 63, C64: 64, C65: 65, BIG8: 300, BIG9: 446, C33: 33, C16B: 16})
ROWS = {a: ROW10 for a in range(1, 41)}
ROWS[41] = (5, {R0: 1, C2: 2, C16: 16, 12: 13})                       # no symbol of 32 cells can be above 64
ROWS[42] = (6, {C2: 2, C16: 16, C17: 17, 12: 29})
ROWS[43] = (7, {R0: 1, C2: 2, C65: 65, BIG8: 60})                     # (BIG8 is an anchor here)
ROWS[44] = (11, {R0: 1, R1: -1, C2: 2, C16: 16, C65: 65, BIG8: 1000, BIG9: 963})
ROWS[45] = (12, {R0: 1, C2: 2, C64: 64, C65: 1500, BIG8: 1500, BIG9: 1029})
ROWS[46] = (12, {BIG8: 2048, BIG9: 2048})
ROWS[47] = (12, {C65: 1024, BIG8: 1024, BIG9: 1024, C33: 1024})
ROWS[49] = (12, {BIG8: 4000, BIG9: 96})                               # BIG8 merges few states a step, BIG9 leaves 96
ROWS[48] = (7, {C65: 128})                                            # one symbol owns the table: every state stays apart

_tables, _octx, _coded, _segs = {}, {}, {}, {}


def _seq_row(sft, log, counts):
    assert sum(abs(v) for v in counts) == 1 << log
    sft["norm"][0][:] = np.array(counts, dtype=np.int16)
    sft["logs"][0][:] = log
    sft["max_log"][0] = log


def tables(key):
    """"main": the crafted quality tables above, flat sequence tables.  "seq-1-8": sequence tables in which A has one cell
    and C eight in every context; "seq-big": T has 200 of 256 cells; both with decode_ref's "sample" quality tables"""
    if key not in _tables:
        if key == "main":
            sft, qft = D.tables("flat")
            qft = qft.copy()
            qft["norm"][0][:] = 1
            qft["logs"][0][:] = 6
            for a, (log, row) in ROWS.items():
                c = target(a)
                qft["norm"][0][c] = 0
                for s, v in row.items():
                    qft["norm"][0][c][s] = v
                qft["logs"][0][c] = log
            qft["max_log"][0] = int(qft["logs"][0].max())
        else:
            sft, qft = D.tables("sample")
            sft = sft.copy()
            if key == "seq-1-8":
                _seq_row(sft, 6, [1, 8, 27, 28])
            elif key == "seq-big":
                _seq_row(sft, 8, [-1, 8, 47, 200])
            else:
                raise KeyError(key)
        for ft in (sft, qft):  # what upload_tables checks
            norm, logs = ft["norm"][0].astype(np.int64), ft["logs"][0].astype(np.int64)
            assert ((logs >= 5) & (logs <= 12)).all() and (norm >= -1).all() and int(ft["max_log"][0]) == logs.max()
            assert (np.abs(norm).sum(axis=1) == (1 << logs)).all(), "every row sums to 2^log, -1 counted as 1"
        _tables[key] = (sft, qft)
    return _tables[key]


def oracle_ctx(case):
    if case.tables not in _octx:
        _octx[case.tables] = O.OracleCtx(*tables(case.tables))
    return _octx[case.tables]


def coded(case):
    """the oracle's streams of a case, made once"""
    key = case_id(case)
    if key not in _coded:
        e = oracle_ctx(case).encode(case.raw, case.recs)
        e.pop("raw_after")
        _coded[key] = e
    return _coded[key]


def oracle_decode(case):
    e = coded(case)
    return oracle_ctx(case).decode(e["seq"], e["qual"], e["n_count"], e["n_pos"], case.recs, O.blank_skeleton(case.raw, case.recs))


def segments(case):
    """the restatement over a whole block -> (ctx per segment, [outcome], {context: (first segment, run)}): an outcome is
    (cls array, anchor array) over the block's segments in the kernels' numbering (contexts ascending)"""
    key = case_id(case)
    if key not in _segs:
        qft, S = tables(case.tables)[1], case.extra["S"]
        ctx, outcomes, where = [], [([], [])], {}
        for c, run in sorted(runs(case.raw, case.recs).items()):
            assert (qft["norm"][0][c][run] != 0).all(), "every (context, symbol) pair of the block has a count"
            alts = classify(run, cells(qft, c), S)
            where[c] = (len(ctx), run)
            ctx += [c] * len(alts[0])
            outcomes = [(cl + [s[0] for s in alt], an + [s[1] for s in alt]) for cl, an in outcomes for alt in alts]
        assert len(outcomes) <= 8
        _segs[key] = (np.array(ctx, dtype=np.uint32), [(np.array(cl, dtype=np.uint8), np.array(an, dtype=np.uint32)) for cl, an in outcomes],
                      where)
    return _segs[key]


def chain_classes(case, a, outcome=0):
    """the classes of the segments of target context T(a)"""
    ctx, outcomes, _ = segments(case)
    return [int(v) for v in outcomes[outcome][0][ctx == target(a)]]


def chain_segments(case, a, outcome=0):
    ctx, outcomes, _ = segments(case)
    m = ctx == target(a)
    return [(int(c), int(an)) for c, an in zip(outcomes[outcome][0][m], outcomes[outcome][1][m])]


# ---------------------------------------------------------------------------------------------------------------------
# blocks
_TEMPLATE = np.frombuffer(b"@h\nACGT\n+\n!!!!\n", dtype=np.uint8)


def block_of(chains):
    """{a: run} -> (raw, recs): per symbol x of a's run one read `a a a x`, the chains one behind the other"""
    a_all = np.concatenate([np.full(len(r), a, dtype=np.uint8) for a, r in chains.items()])
    x_all = np.concatenate([np.asarray(r, dtype=np.uint8) for r in chains.values()])
    assert a_all.size and 1 <= int(a_all.min()) and int(a_all.max()) <= 63 and int(x_all.max()) <= 63
    rows = np.tile(_TEMPLATE, (a_all.size, 1))
    rows[:, 10:13] = (a_all + 33)[:, None]
    rows[:, 13] = x_all + 33
    raw = rows.reshape(-1).copy()
    assert raw.size <= MAX_FASTQ, "a case is at most 2.5 MiB of FASTQ"
    recs = O.parse_fastq(raw)
    assert len(recs) == a_all.size
    return raw, recs


def make(family, name, chains, S=1024, tables_key="main", **extra):
    chains = {a: np.asarray(r, dtype=np.uint8) for a, r in chains.items()}
    raw, recs = block_of(chains)
    case = Case(family, name, raw, recs, tables_key, "ok", dict(extra, S=S, chains=chains))
    got = runs(raw, recs)
    for a, r in chains.items():  # the steering works: T(a) holds exactly the run meant
        assert np.array_equal(got[target(a)], r), (name, a)
    segments(case)
    return case


def _rng(seed):
    return np.random.default_rng(seed)


def opaque_seg(rng, n, big=BIG):
    """n symbols with too many cells for an anchor, not all the same"""
    seg = np.array(big, dtype=np.uint8)[rng.integers(0, len(big), size=n)]
    if n > 1 and (seg == seg[0]).all():
        seg[n // 2] = big[1] if seg[0] == big[0] else big[0]
    return seg


def with_syms(seg, places):
    seg = seg.copy()
    for off, s in places.items():
        seg[off] = s
    return seg


def cat(*parts):
    return np.concatenate([np.asarray(p, dtype=np.uint8) for p in parts])


# ---------------------------------------------------------------------------------------------------------------------
def _scan_offsets():
    """the `hit` loop (j from 15 down to 0), __ffsll of the ballot, the break behind the first batch, `p + j < end`"""
    rng = _rng(101)
    S = 1024
    offs = (0, 15, 16, 17, 1007, 1008, 1023)
    chains = {1: cat(*[with_syms(opaque_seg(rng, S), {o: R0}) for o in offs])}
    want = {1: [(1, o) for o in offs]}
    # two reset symbols in one 16-byte group (in either order of the two symbols), two in different lanes, a reset symbol
    # behind an earlier anchor candidate and in front of one; the count -1 acts as the count 1
    spots = [({35: R0, 40: R1}, 35), ({35: R1, 40: R0}, 35), ({47: R0, 32: R1}, 32), ({100: R0, 900: R0}, 100),
             ({10: C2, 500: R0}, 500), ({10: R1, 500: C2}, 10), ({1023: R1}, 1023), ({0: R1}, 0), ({15: R1, 16: R0}, 15)]
    chains[2] = cat(*[with_syms(opaque_seg(rng, S), p) for p, _ in spots])
    want[2] = [(1, o) for _, o in spots]
    # a short last segment whose LAST symbol is the reset symbol
    for a, n in zip(range(3, 8), (1, 15, 16, 17, 1023)):
        chains[a] = cat(opaque_seg(rng, S), with_syms(opaque_seg(rng, n), {n - 1: R0}))
        want[a] = [(OPAQUE, SEG_NONE), (1, n - 1)]
    # a short last segment behind whose end the run of the next non-empty context begins with a reset symbol
    chains[20] = cat(opaque_seg(rng, S), opaque_seg(rng, 5))
    chains[21] = cat([R0], opaque_seg(rng, 40))
    want[20], want[21] = [(OPAQUE, SEG_NONE)] * 2, [(1, 0)]
    case = make("scan-offsets", "s1024", chains, S)
    for a, w in want.items():
        assert chain_segments(case, a) == w, (a, chain_segments(case, a), w)
    nonempty = sorted(segments(case)[2])
    assert nonempty[nonempty.index(target(20)) + 1] == target(21) and segments(case)[2][target(21)][1][0] == R0
    yield case
    S = 2048
    offs = (0, 1023, 1024, 1025, 2047)
    chains = {1: cat(*[with_syms(opaque_seg(rng, S), {o: R0}) for o in offs], with_syms(opaque_seg(rng, S), {1030: R1, 1040: R0}),
                     with_syms(opaque_seg(rng, 1025), {1024: R0}))}
    case = make("scan-offsets", "s2048", chains, S)
    assert chain_segments(case, 1) == [(1, o) for o in offs] + [(1, 1030), (1, 1024)]
    yield case


def _anchor_choice():
    """the min over cells << 20 | offset"""
    rng = _rng(102)
    S = 1024
    segs, want = [], []

    def add(places, cls, off):
        segs.append(with_syms(opaque_seg(rng, S), places)); want.append((cls, off))
    for sym, n in ((C2, 2), (C16, 16), (C17, 17), (C63, 63), (C64, 64)):  # the smallest count present
        add({100: sym}, n, 100)
    segs.append(with_syms(opaque_seg(rng, S, (BIG8, BIG9)), {100: C65})); want.append((OPAQUE, SEG_NONE))  # 65 cells: no anchor
    add({10: C16, 500: C2}, 2, 500)        # the fewest cells stand BEHIND more
    add({10: C2, 500: C16}, 2, 10)
    add({300: C16B, 700: C16}, 16, 300)    # equal cell counts: the lower offset
    add({300: C16, 700: C16B}, 16, 300)
    add({16: C16, 15: C16B, 31: C17}, 16, 15)
    add({5: C2, 1000: C2}, 2, 5)
    for off in (0, 15, 16, 17, 1022, 1023):  # (offset 0: the head walk is empty; 1023: the tail walk)
        add({off: C2}, 2, off)
        add({off: C64}, 64, off)
    segs.append(np.full(S, C64, dtype=np.uint8)); want.append((64, 0))   # one symbol of <= 64 cells: anchored, not uniform
    segs.append(np.full(S, C2, dtype=np.uint8)); want.append((2, 0))
    segs.append(with_syms(opaque_seg(rng, 17), {16: C17})); want.append((17, 16))  # (a short last segment has its anchor too)
    case = make("anchor-choice", "s1024", {1: cat(*segs)}, S)
    assert chain_segments(case, 1) == want
    yield case
    S = 2048
    case = make("anchor-choice", "s2048", {1: cat(with_syms(opaque_seg(rng, S), {1500: C16, 1024: C17}), with_syms(opaque_seg(rng, S), {2047: C2, 3: C16}),
                                                with_syms(opaque_seg(rng, S), {1023: C33, 1024: C33}), opaque_seg(rng, 3))}, S)
    assert chain_segments(case, 1) == [(16, 1500), (2, 2047), (33, 1023), (OPAQUE, SEG_NONE)]
    yield case


def _uniform():
    rng = _rng(103)
    for S, others in ((1024, (0, 1, 1023)), (2048, (0, 1, 1023, 1024, 2047)), (3072, (0, 2048, 3071)), (5120, (0, 4096, 5119))):
        U = np.full(S, BIG8, dtype=np.uint8)
        # a full segment of one symbol; the same with ONE other symbol (also above 64 cells); a short last one: opaque
        chains = {1: cat(U, *[with_syms(U, {o: BIG9}) for o in others], U, U, np.full(S - 1 if S == 1024 else 7, BIG8, dtype=np.uint8))}
        want = {1: [(UNIFORM, BIG8)] + [(OPAQUE, SEG_NONE)] * len(others) + [(UNIFORM, BIG8)] * 2 + [(OPAQUE, SEG_NONE)]}
        # segments of symbol a then of symbol b in one context: whoever asks first owns the power table
        V = np.full(S, BIG9, dtype=np.uint8)
        chains[2] = cat(U, V, U, V, V, opaque_seg(rng, 9))
        # other logs of the uniform context: per = max(size >> 6, 1); (no symbol of a log-5 or log-6 table has more than 64
        # cells, so log 7 is the smallest table with a uniform segment)
        for a in (43, 44, 45, 48):
            W = np.full(S, C65, dtype=np.uint8)
            chains[a] = cat(W, W, W, np.full(5, C65, dtype=np.uint8))
            want[a] = [(UNIFORM, C65)] * 3 + [(OPAQUE, SEG_NONE)]
        case = make("uniform", "s%d" % S, chains, S)
        for a, w in want.items():
            assert chain_segments(case, a) == w, (S, a)
        alts = [chain_segments(case, 2, i) for i in range(len(segments(case)[1]))]
        u, v, o = (UNIFORM, BIG8), (UNIFORM, BIG9), (OPAQUE, SEG_NONE)
        assert sorted(alts) == sorted([[u, o, u, o, o, o], [o, v, o, v, v, o]]), "two outcomes: either symbol owns the power table"
        assert route(chain_classes(case, 1))[0].count("pow") == 3 and route(chain_classes(case, 48))[0] == ["pow", "pow", "pow", "none"]
        yield case
    # 130 uniform segments: the power-table slot goes through k_seg_compose across three items
    case = make("uniform", "chain-of-130", {3: np.full(130 * 1024, BIG8, dtype=np.uint8)}, 1024)
    r, has_g = route(chain_classes(case, 3))
    assert r == ["pow"] * 129 + ["none"] and has_g == [True, True, True]
    yield case


def _euler_pairs():
    """a walk over T, A, U, O that takes every ordered pair once: 17 segments"""
    kinds = "TAUO"
    left = {k: list(kinds) for k in kinds}
    stack, walk = ["T"], []
    while stack:  # Hierholzer
        v = stack[-1]
        if left[v]:
            stack.append(left[v].pop())
        else:
            walk.append(stack.pop())
    walk.reverse()
    assert len(walk) == 17 and {(a, b) for a, b in zip(walk, walk[1:])} == {(a, b) for a in kinds for b in kinds}
    return walk


def _kind_seg(rng, kind, S, anchor_sym, i):
    if kind == "T":
        return with_syms(opaque_seg(rng, S), {(37 * i + 5) % S: R0})
    if kind == "A":
        return with_syms(opaque_seg(rng, S), {(53 * i + 11) % S: anchor_sym})
    if kind == "U":
        return np.full(S, BIG8, dtype=np.uint8)
    return opaque_seg(rng, S)


def _pairs():
    rng = _rng(104)
    S = 1024
    walk = _euler_pairs()
    for sym, n in ((C2, 2), (C64, 64)):
        chains = {1: cat(*[_kind_seg(rng, k, S, sym, i) for i, k in enumerate(walk)])}
        ends = (("T", "A"), ("A", "U"), ("U", "O"), ("O", "T"))  # every class first in a chain and last in one
        for a, (k0, k1) in zip(range(2, 6), ends):
            chains[a] = cat(_kind_seg(rng, k0, S, sym, a), _kind_seg(rng, k1, S, sym, a + 1))
        case = make("pairs", "anchors-of-%d" % n, chains, S)
        cls = chain_classes(case, 1)
        assert [kind_of(c) for c in cls] == walk and all(c == n for c in cls if kind_of(c) == "A")
        for a, e in zip(range(2, 6), ends):
            assert tuple(kind_of(c) for c in chain_classes(case, a)) == e
        r = route(cls)[0]
        for k in range(len(walk)):
            pred = walk[k - 1] if k else None
            if k == len(walk) - 1 or walk[k] == "T":
                assert r[k] == "none"
            elif walk[k] == "A":
                assert r[k] == ("setfunc" if pred in ("O", "U") else "cand"), (k, pred, r[k])
            else:
                assert r[k] == {"U": "pow", "O": "setfunc"}[walk[k]]
        assert route(chain_classes(case, 3))[0] == ["cand", "none"], "anchored first in the chain"
        yield case


def _heads():
    rng = _rng(105)
    S = 1024
    by_n = {2: C2, 16: C16, 17: C17, 33: C33, 64: C64}
    head_lens = (0, 1, 15, 16, 17, 33)
    segs, want, i = [], [], 0
    for p in (2, 16, 17, 33, 64):        # the predecessor's candidates: the walks of a head, sixteen a round
        for q in (2, 17, 64):            # ... against the segment's own
            for n, off in ((p, 700 + i), (q, head_lens[i % 6])):
                segs.append(with_syms(opaque_seg(rng, S), {off: by_n[n]})); want.append((n, off))
            i += 1
    segs.append(opaque_seg(rng, 30)); want.append((OPAQUE, SEG_NONE))
    chains = {1: cat(*segs)}
    # small tables: the function slots and k_seg_compose at 32 and 64 states
    chains[41] = cat(*[with_syms(np.full(S, 12, dtype=np.uint8), {off: C2}) for off in (0, 1, 15, 16, 17, 33, 1023)], [12] * 3)
    chains[42] = cat(*[with_syms(np.full(S, 12, dtype=np.uint8), {off: s}) for off, s in ((0, C2), (17, C16), (33, C17), (1000, C2))], [12] * 3)
    case = make("heads", "anchored-behind-anchored", chains, S)
    assert chain_segments(case, 1) == want
    pairs = {(a[0], b[0]) for a, b in zip(want, want[1:])}
    assert pairs >= {(p, q) for p in (2, 16, 17, 33, 64) for q in (2, 17, 64)}
    assert {b[1] for a, b in zip(want, want[1:]) if b[0] in (2, 17, 64)} >= set(head_lens)
    assert set(route(chain_classes(case, 1))[0][:-2]) == {"cand"}
    assert chain_classes(case, 41) == [2] * 7 + [13] and chain_classes(case, 42)[:4] == [2, 16, 17, 2]
    yield case
    # six target contexts of two or three anchored segments and two of one: a wave's four slots hold segments of two, three
    # and four contexts, and wanted ones of two (a context's last segment is never wanted, so two is the most)
    lens = {1: 2, 2: 3, 3: 1, 4: 1, 5: 2, 6: 3, 7: 2, 8: 3}
    chains = {a: cat(*[with_syms(opaque_seg(rng, S), {(97 * a + 13 * k) % S: (C2, C17, C64)[(a + k) % 3]}) for k in range(n - 1)],
                     with_syms(opaque_seg(rng, 50), {a: C16})) for a, n in lens.items()}
    case = make("heads", "cand-mixed-contexts", chains, S)
    ctx, outcomes, _ = segments(case)
    cls = outcomes[0][0]
    held, wanted = set(), set()
    for w in range(0, len(ctx), 64 // SEG_SLOT):
        slots = range(w, min(w + 64 // SEG_SLOT, len(ctx)))
        held.add(len({int(ctx[s]) for s in slots}))
        wanted.add(len({int(ctx[s]) for s in slots if 2 <= cls[s] <= MAX_CAND and s + 1 < len(ctx) and ctx[s + 1] == ctx[s]}))
    assert held >= {2, 3, 4} and wanted >= {0, 1, 2}, (held, wanted)
    yield case


OPAQUE_SEARCH = 400  # seeded runs looked at, at most
OPAQUE_UNREACHED = set()  # what the search does not reach: nothing


def _opaque():
    """seg_setfunc_role by set_sizes: a bounded search over seeded symbol runs for the level at which the state sets start
    and the widths they are walked with"""
    qft = tables("main")[1]
    S = 1024
    wanted = {"level1-at-stop-0", "above-512-through-3-stops", "never-512", "walk-1", "walk-2", "walk-8"}
    found = {}
    # (context, symbols to draw from, how: "rand" or a period)
    recipes = [(1, BIG, "rand"), (1, (BIG8, BIG9), "rand"), (45, (C65, BIG8, BIG9), "rand"), (46, (BIG8, BIG9), "rand"),
               (47, (C65, BIG8, BIG9, C33), "rand"), (46, (BIG8, BIG9), 2), (47, (C65, BIG8, BIG9, C33), 4), (46, (BIG8, BIG9), 3),
               (44, (BIG8, BIG9), "rand"), (49, (BIG8, BIG9), ("spot", 1023)), (49, (BIG8, BIG9), ("spot", 60))]
    cts = {a: ctable(qft, target(a)) for a, _, _ in recipes}
    tried = 0
    for seed in range(OPAQUE_SEARCH // len(recipes)):
        for a, big, how in recipes:
            tried += 1
            rng = _rng(1000 * a + seed)
            if how == "rand":
                seg = opaque_seg(rng, S, big)
            elif isinstance(how, tuple):  # the first symbol throughout, the second one once
                seg = with_syms(np.full(S, big[0], dtype=np.uint8), {how[1]: big[1]})
            else:
                unit = opaque_seg(rng, how, big)
                seg = np.tile(unit, S // how + 1)[:S]
            if int(cells(qft, target(a))[seg].min()) <= MAX_CAND:
                continue
            sizes = set_sizes(cts[a], seg)
            level1, widths = setfunc_walks(sizes, S)
            keys = set()
            if level1 == 0:
                keys.add("level1-at-stop-0")
            if level1 is None:
                keys.add("never-512")
            elif level1 >= 3:
                keys.add("above-512-through-3-stops")
            keys |= {"walk-%d" % w for w in widths}
            for k in keys & wanted:
                if k not in found:
                    found[k] = (a, seed, how, big, seg, sizes)
        if set(found) == wanted:
            break
    _opaque.found, _opaque.tried = sorted(found), tried
    assert set(found) >= wanted - OPAQUE_UNREACHED, sorted(wanted - set(found))
    assert not set(found) & OPAQUE_UNREACHED, "reached after all: take it off the list"
    rng = _rng(9)
    by_ctx, names = {}, []
    for k, (a, seed, how, big, seg, sizes) in sorted(found.items()):
        segs = by_ctx.setdefault(a, [])
        if not any(seg is s for s in segs):
            segs.append(seg)
        names.append("%s-ctx%d-seed%d" % (k, a, seed))
        if k == "never-512":
            assert min(sizes) > SETS_MAX_CLASSES
        if k == "above-512-through-3-stops":
            assert min(sizes[:3]) > SETS_MAX_CLASSES >= sizes[3]
    # (behind the segments found a short last one of the same symbols: every segment found has a successor)
    chains = {a: cat(*segs, opaque_seg(rng, 11, tuple(int(v) for v in np.unique(segs[0])))) for a, segs in by_ctx.items()}
    case = make("opaque", "+".join(names), chains, S)
    for a in chains:
        assert set(route(chain_classes(case, a))[0][:-1]) == {"setfunc"} and set(chain_classes(case, a)) == {OPAQUE}
    yield case
    # S = 2048: two blocks of 1024 symbols per segment (nblk = 2, the `nxt` prefetch), one more stop
    chains = {1: cat(opaque_seg(rng, 2048), opaque_seg(rng, 2048), opaque_seg(rng, 2048, (BIG8, BIG9)), opaque_seg(rng, 100)),
              46: cat(opaque_seg(rng, 2048, (BIG8, BIG9)), opaque_seg(rng, 2048, (BIG8, BIG9)), [BIG8])}
    case = make("opaque", "s2048", chains, 2048)
    assert chain_classes(case, 1) == [OPAQUE] * 4 and route(chain_classes(case, 46))[0] == ["setfunc", "setfunc", "none"]
    yield case


def _mixed_chain(rng, kinds, S=1024):
    """a chain of the kinds given (T, O, A, or a for an anchor of 64)"""
    return cat(*[_kind_seg(rng, "A" if k == "a" else k, S, C64 if k == "a" else C2, i) for i, k in enumerate(kinds)])


def _items():
    rng = _rng(107)

    def check(case, a, kinds):
        assert [kind_of(c) for c in chain_classes(case, a)] == [k.upper() for k in kinds], a
        return route(chain_classes(case, a))
    # 129 segments: an all-transparent item in front of one with functions; a transparent segment as segment 63 of an item
    # and as segment 0 of the next; the successor of a transparent segment opaque across an item edge; the chain's last
    # segment as segment 0 of an item (n_here == 1)
    kinds = "T" * 64 + "OAaTOOTA" * 7 + "OAOaOAOT" + "T"
    assert len(kinds) == 129 and kinds[63] == "T" and kinds[64] == "O" and kinds[127] == "T" and kinds[128] == "T"
    case = make("items", "129-transparent-item-first", {1: _mixed_chain(rng, kinds)})
    assert check(case, 1, kinds)[1] == [False, True, False]
    yield case
    # ... and behind one: items with, without, with
    kinds = "OAaTOOTA" * 8 + "T" * 64 + "O"
    case = make("items", "129-transparent-item-in-the-middle", {1: _mixed_chain(rng, kinds)})
    r, has_g = check(case, 1, kinds)
    assert has_g == [True, False, False] and kinds[63] == "A" and kinds[64] == "T"
    yield case
    kinds = "OAaO" * 16 + "T" * 64 + "A"
    case = make("items", "129-no-transparent-segment-in-item-0", {1: _mixed_chain(rng, kinds)})
    assert check(case, 1, kinds)[1] == [True, False, False]
    yield case
    # one and two items without any transparent segment; 127 and 128: the last item one short of full and full
    lengths = {129}
    for n, more in ((128, {2: "O", 3: "aO"}), (127, {2: "A", 3: "TO"}), (65, {2: "OaAO" * 15 + "OaA"}), (64, {2: "AOTa" * 16})):
        lengths |= {n} | {len(k) for k in more.values()}
        kinds = ("OaAO" * 33)[:n]
        chains = {1: _mixed_chain(rng, kinds)}
        chains.update({a: _mixed_chain(rng, k) for a, k in more.items()})
        case = make("items", "%d-without-a-transparent-segment" % n, chains)
        assert check(case, 1, kinds)[1] == ([True, False] if n == 65 else [True] * ((n + 63) // 64))  # (segment 64 of 65 is the last)
        for a, k in more.items():
            check(case, a, k)
        yield case
    assert lengths == {1, 2, 63, 64, 65, 127, 128, 129}


def _walk_ends():
    """seg_walk_range in both passes"""
    rng = _rng(108)
    S = 1024
    lens = (0, 1, 15, 16, 17, 31, 32, 33)
    chains, want, a = {}, {}, 1
    # pass 1: the piece behind the reset symbol is `n` long and starts at 0, 1, 15 mod 16 (a short only segment)
    for start in (16, 17, 31):
        for n in lens:
            chains[a] = with_syms(opaque_seg(rng, start + n), {start - 1: R0})
            want[a] = [(1, start - 1)]
            a += 1
    # ... the same behind a full opaque segment, so that the head in pass 2 starts from a resolved state
    for n in lens:
        chains[a] = cat(opaque_seg(rng, S), with_syms(opaque_seg(rng, 31 + n), {30: R1}))
        want[a] = [(OPAQUE, SEG_NONE), (1, 30)]
        a += 1
    # pass 2: heads of these lengths (full segments: the piece behind ends at a multiple of 16)
    heads = (1, 15, 16, 17, 31, 32, 33)
    chains[a] = cat(*[with_syms(opaque_seg(rng, S), {h - 1: R0}) for h in heads], *[with_syms(opaque_seg(rng, S), {S - 1 - n: R0}) for n in lens])
    want[a] = [(1, h - 1) for h in heads] + [(1, S - 1 - n) for n in lens]
    a += 1
    # contexts of 1, 2, 15, 16, 17 symbols in all; final_state written by pass 2 (no reset symbol) ...
    for n in (1, 2, 15, 16, 17):
        chains[a] = opaque_seg(rng, n) if n > 1 else np.array([BIG8], dtype=np.uint8)
        want[a] = [(OPAQUE, SEG_NONE)]
        a += 1
    chains[a] = np.array([R0], dtype=np.uint8); want[a] = [(1, 0)]  # ... and by pass 1
    assert a <= 40
    case = make("walk-ends", "pieces", chains, S)
    for k, w in want.items():
        assert chain_segments(case, k) == w, k
    yield case


def _bases(rng, n, probs):
    """random bases, A C G T as often as `probs` says (a stream above two bits a base does not fit the capacity rule)"""
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.choice(4, size=n, p=probs)].tobytes()


def _seq_generic():
    """the sequence stream through the same kernels (FQGPU_CHAIN_SEQ_GENERIC): A = 4, B = 256"""
    rng = _rng(109)
    for key, probs in (("seq-1-8", (0.04, 0.16, 0.4, 0.4)), ("seq-big", (0.03, 0.07, 0.2, 0.7))):
        raw, recs = D.block([(_bases(rng, 100, probs), D.rand_quals(rng, 100)) for _ in range(6000)])
        assert 2 <= int(recs["len"].sum()) // 256 // 1024 <= 3, "contexts of two or three segments on average"
        yield Case("seq-generic", "random-bases-%s" % key, raw, recs, key, "ok", {"S": 1024, "seq_generic": True})
    raw, recs = D.block([(b"T" * 100, D.rand_quals(rng, 100)) for _ in range(300)])
    assert tables("seq-big")[0]["norm"][0][:, 3].min() > MAX_CAND
    yield Case("seq-generic", "one-base-above-64-cells", raw, recs, "seq-big", "ok", {"S": 1024, "seq_generic": True})


FAMILIES = (_scan_offsets, _anchor_choice, _uniform, _pairs, _heads, _opaque, _items, _walk_ends, _seq_generic)
QUAL_FAMILIES = ("scan-offsets", "anchor-choice", "uniform", "pairs", "heads", "opaque", "items", "walk-ends")

_cases = []


def families():
    """every case of every family, in a fixed order, made once; each family's generator asserts its own property"""
    if not _cases:
        for fam in FAMILIES:
            _cases.extend(fam())
        assert len({(c.family, c.name) for c in _cases}) == len(_cases)
        for c in _cases:
            assert c.raw.size <= MAX_FASTQ
    return list(_cases)


def case_id(c):
    return "%s/%s" % (c.family, c.name)


def of_family(*names):
    return [c for c in families() if c.family in names]


def reached(cases):
    """over the quality cases -> (set of (predecessor kind or None, kind), set of (route, kind, predecessor kind or None),
    set of has_g patterns of neighbouring items)"""
    pairs, routes, items = set(), set(), set()
    for case in cases:
        ctx, outcomes, _ = segments(case)
        for cls, _ in outcomes:
            for c in np.unique(ctx):
                chain = [int(v) for v in cls[ctx == c]]
                kinds = [kind_of(v) for v in chain]
                r, has_g = route(chain)
                for k in range(len(chain)):
                    pairs.add((kinds[k - 1] if k else None, kinds[k]))
                    routes.add((r[k], kinds[k], kinds[k - 1] if k else None, k + 1 == len(chain)))
                items |= set(zip(has_g, has_g[1:]))
    return pairs, routes, items
